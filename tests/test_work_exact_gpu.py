"""Every entry point with a multi-piece workspace stays inside what its *_work_bytes promises (csrc: one layout function per entry
point on the shared Carver serves both the size query and the consumer).

(a) The workspace is the front of ONE allocation of work_bytes + 4096 bytes whose tail is filled with 0xA5: the call gets exactly
    work_bytes, its result equals the reference (the ops wrapper where there is one, NumPy otherwise), and the tail is unchanged.
    The canary lies inside the test's own allocation, so an overrun is a failed assertion, not a fault.
(b) With work_bytes - 1 the call returns AVL_ERR_INVALID before any device work: the outputs keep their fill pattern.
(c) The entry points that align the base themselves (their totals carry 256 or 512 bytes of slack for it) run (a) once more from
    an odd address, base + 1 of a 256-aligned allocation: the alignment then eats 255 bytes of the slack, and with 256 bytes of
    slack the last piece ends one byte before the canary (with 512, 257 bytes before it: no address uses more than 255)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AVL_ERR_INVALID = 1
CANARY = 4096
FILL = 0x77


@pytest.fixture(scope="module")
def env():
    from avlmaps_amd import _lib, ops
    from avlmaps_amd.device import DeviceArray
    lib = _lib.load()
    _lib.require_gpu()
    return _lib, lib, ops, DeviceArray


def dev(DeviceArray, a):
    return DeviceArray.from_numpy(np.ascontiguousarray(a))


def filled(DeviceArray, shape, dtype):
    """an output buffer whose every byte is FILL"""
    a = np.empty(shape, dtype)
    a.view(np.uint8).fill(FILL)
    return DeviceArray.from_numpy(a)


def untouched(d):
    return bool((d.numpy().view(np.uint8) == FILL).all())


def exact_and_short(env, query, qargs, call, outputs, check, aligns_base=False):
    """call(ws_ptr, ws_bytes, outs) -> status, with fresh FILL-ed outputs() each time: (a), (b) and, for an entry point that aligns
    the base itself, (c) of the module docstring"""
    _lib, lib, ops, DeviceArray = env
    nb = C.c_size_t(0)
    _lib.check(query(*qargs, C.byref(nb)), query.__name__)
    n = nb.value
    assert n >= 1
    host = np.full(n + CANARY, 0x5A, np.uint8)                 # the workspace starts as garbage: nothing may rely on zeros
    host[n:] = 0xA5
    buf = DeviceArray.from_numpy(host)
    outs = outputs()
    _lib.check(call(buf.ptr, n, outs), "exact-size call")
    check(outs)
    assert (buf.numpy()[n:] == 0xA5).all(), "the call wrote past work_bytes"
    outs = outputs()
    assert call(buf.ptr, n - 1, outs) == AVL_ERR_INVALID
    assert all(untouched(o) for o in outs), "a refused call wrote to an output"
    if aligns_base:
        host = np.full(1 + n + CANARY, 0x5A, np.uint8)
        host[1 + n:] = 0xA5
        buf = DeviceArray.from_numpy(host)
        assert buf.ptr % 256 == 0
        outs = outputs()
        _lib.check(call(buf.ptr + 1, n, outs), "exact-size call from an odd address")
        check(outs)
        got = buf.numpy()
        assert got[0] == 0x5A and (got[1 + n:] == 0xA5).all(), "the call wrote outside [base + 1, base + 1 + work_bytes)"


@pytest.mark.parametrize("dilate_iter", [0, 2])
def test_dilate_map(env, dilate_iter):
    _lib, lib, ops, DeviceArray = env
    H, W = 5, 7
    mask = (np.random.default_rng(5).random((H, W)) < 0.4).astype(np.uint8)
    want_v, want_z = ops.dilate_map(mask, dilate_iter, 1.0)
    d_mask = dev(DeviceArray, mask)

    def check(outs):
        assert np.array_equal(outs[0].numpy(), want_v) and np.array_equal(outs[1].numpy().astype(bool), want_z)

    exact_and_short(env, lib.avl_dilate_map_work_bytes, (H, W),
                    lambda ws, n, o: lib.avl_dilate_map(d_mask.ptr, H, W, dilate_iter, 1.0, o[0].ptr, o[1].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W), np.float64), filled(DeviceArray, (H, W), np.uint8)], check)


def test_mask_foreground(env):
    _lib, lib, ops, DeviceArray = env
    H, W = 5, 7
    mask = (np.random.default_rng(6).random((H, W)) < 0.5).astype(np.uint8)
    want = ops.mask_foreground(mask)
    d_mask = dev(DeviceArray, mask)
    exact_and_short(env, lib.avl_mask_foreground_work_bytes, (H, W),
                    lambda ws, n, o: lib.avl_mask_foreground(d_mask.ptr, W, 0, H, 0, W, o[0].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W), np.uint8)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy().astype(bool), want))


@pytest.mark.parametrize("shape", [(3, 130), (1, 1025)])            # (1, 1025): two scan blocks
def test_label_islands(env, shape):
    _lib, lib, ops, DeviceArray = env
    H, W = shape
    mask = (np.random.default_rng(H * W).random(shape) < 0.45).astype(np.uint8)
    with ops.label_islands(mask) as isl:
        want_n, want = isl.n, np.array(isl.labels)
    d_mask = dev(DeviceArray, mask)

    def check(outs):
        assert int(outs[1].numpy()[0]) == want_n and np.array_equal(outs[0].numpy(), want)

    exact_and_short(env, lib.avl_label_islands_work_bytes, (H, W),
                    lambda ws, n, o: lib.avl_label_islands(d_mask.ptr, W, H, W, o[0].ptr, o[1].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W), np.int32), filled(DeviceArray, (1,), np.int32)], check)


def test_audio_segment(env):
    _lib, lib, ops, DeviceArray = env
    n, gap = 4096 + 1, 50                                             # T + 1 samples: two tiles, the second holds one sample
    audio = np.zeros(n, np.float32)
    audio[[3, 100, 101, 900, 4095, 4096]] = 1.0
    want = ops.segment_audio(audio, 50, 1.0, 0.0).segments_host
    assert len(want) == 4
    d_audio = dev(DeviceArray, audio)
    cap = len(want)

    def check(outs):
        assert int(outs[1].numpy()[0]) == len(want) and np.array_equal(outs[0].numpy(), want)

    exact_and_short(env, lib.avl_audio_segment_work_bytes, (n,),
                    lambda ws, nb, o: lib.avl_audio_segment(d_audio.ptr, n, 0.0, gap, o[0].ptr, cap, o[1].ptr, ws, nb, None),
                    lambda: [filled(DeviceArray, (cap, 2), np.int64), filled(DeviceArray, (1,), np.int64)], check)


@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("dtype,bits", [(np.int64, 40), (np.int32, 5)])
def test_argsort_bits(env, n, dtype, bits):
    _lib, lib, ops, DeviceArray = env
    keys = np.random.default_rng(n + bits).integers(0, 1 << bits, n).astype(dtype)
    d_keys = dev(DeviceArray, keys)
    kb = keys.dtype.itemsize
    exact_and_short(env, lib.avl_argsort_bits_work_bytes, (n, kb, bits),
                    lambda ws, nb, o: lib.avl_argsort_bits(n, d_keys.ptr, kb, bits, o[0].ptr, ws, nb, None),
                    lambda: [filled(DeviceArray, (n,), np.int64)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy(), np.argsort(keys, kind="stable")), aligns_base=True)


@pytest.mark.parametrize("n", [1, 300])
def test_merge_partition(env, n):
    """avl_merge_partition: the work buffer of avl_merge_work_bytes"""
    _lib, lib, ops, DeviceArray = env
    ws = 3
    rng = np.random.default_rng(n)
    cell = rng.permutation(4 * n + 8)[:n].astype(np.int32)
    key = ((rng.integers(0, 50, n) << 32) | rng.permutation(n)).astype(np.int64)
    dest = (((cell.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(12)) % np.uint64(ws)
    order = np.argsort(dest, kind="stable")
    head = np.concatenate([np.bincount(dest.astype(np.int64), minlength=ws), [n, key.min(), key.max()]]).astype(np.int64)
    d_cell, d_key = dev(DeviceArray, cell), dev(DeviceArray, key)

    def check(outs):
        assert np.array_equal(outs[0].numpy(), order) and np.array_equal(outs[1].numpy(), cell[order])
        assert np.array_equal(outs[2].numpy(), head)

    exact_and_short(env, lib.avl_merge_work_bytes, (n,),
                    lambda w, nb, o: lib.avl_merge_partition(n, d_cell.ptr, d_key.ptr, ws, o[0].ptr, o[1].ptr, o[2].ptr, w, nb, None),
                    lambda: [filled(DeviceArray, (n,), np.int64), filled(DeviceArray, (n,), np.int32), filled(DeviceArray, (ws + 3,), np.int64)],
                    check, aligns_base=True)


@pytest.mark.parametrize("n", [1, 300])
def test_merge_rows_other(env, n):
    """avl_merge_rows_other: the work buffer of avl_merge_rows_work_bytes"""
    _lib, lib, ops, DeviceArray = env
    rng = np.random.default_rng(7 * n)
    m4 = (rng.random(n) < 0.5).astype(np.uint8)
    m4[0] = 1
    n4 = int(m4.sum())
    ordd = rng.permutation(n).astype(np.int64)
    recv4 = rng.integers(0, 1 << 40, n4).astype(np.int64)
    want = np.empty(n, np.int64)
    want.view(np.uint8).fill(FILL)
    want[ordd[m4 != 0]] = recv4
    d_m4, d_ordd, d_recv4 = dev(DeviceArray, m4), dev(DeviceArray, ordd), dev(DeviceArray, recv4)
    exact_and_short(env, lib.avl_merge_rows_work_bytes, (n,),
                    lambda w, nb, o: lib.avl_merge_rows_other(n, d_m4.ptr, d_ordd.ptr, d_recv4.ptr, n4, o[0].ptr, w, nb, None),
                    lambda: [filled(DeviceArray, (n,), np.int64)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy(), want), aligns_base=True)


def test_merge2_prepare(env):
    _lib, lib, ops, DeviceArray = env
    n, key_bits, flags = 300, 40, 5
    rng = np.random.default_rng(300)
    key = ((rng.integers(0, 50, n) << 32) | rng.permutation(n)).astype(np.int64)
    cell = rng.permutation(4 * n)[:n].astype(np.int32)
    perm = np.argsort(key, kind="stable")
    d_key, d_cell = dev(DeviceArray, key), dev(DeviceArray, cell)

    def check(outs):
        assert np.array_equal(outs[0].numpy(), key[perm]) and np.array_equal(outs[1].numpy(), cell[perm])
        assert np.array_equal(outs[2].numpy(), perm) and np.array_equal(outs[3].numpy(), [n, key.min(), key.max(), flags])

    exact_and_short(env, lib.avl_merge2_prepare_work_bytes, (n,),
                    lambda w, nb, o: lib.avl_merge2_prepare(n, d_key.ptr, d_cell.ptr, key_bits, flags, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr,
                                                            w, nb, None),
                    lambda: [filled(DeviceArray, (n,), np.int64), filled(DeviceArray, (n,), np.int32), filled(DeviceArray, (n,), np.int32),
                             filled(DeviceArray, (4,), np.int64)], check, aligns_base=True)


def test_merge2_fold(env):
    """n_own = 5 rows from ws = 3 peers, every row with two or three contributors: the sums in rank order, finalize's expressions"""
    _lib, lib, ops, DeviceArray = env
    n_own, ws, D, gs, vh, r0 = 5, 3, 6, 10, 4, 2
    rng = np.random.default_rng(53)
    rows_of = [np.array([0, 1, 2, 3, 4]), np.array([0, 2, 4]), np.array([1, 2, 3])]          # peer p's records, rows ascending
    side, part = [], []
    for p in range(ws):
        k = len(rows_of[p])
        src = rng.permutation(k)                                                              # the record's row in the peer's partial rows
        rec = np.zeros((k, 8), np.int64)
        rec[:, 0] = rows_of[p] | (src << 32)
        w4 = np.concatenate([rng.uniform(0.5, 2.0, (k, 1)), rng.uniform(0.0, 300.0, (k, 3))], axis=1)
        rec[:, 1:5] = w4.view(np.int64)
        side.append(rec)
        part.append(rng.standard_normal((k, D)))
    rowcell = rng.integers(0, gs * gs * vh, r0 + n_own).astype(np.int32)
    w4 = np.zeros((n_own, 4))
    feat = np.zeros((n_own, D))
    for p in range(ws):                                                                       # rank order
        w4[rows_of[p]] += side[p][:, 1:5].view(np.float64)
        feat[rows_of[p]] += part[p][side[p][:, 0] >> 32]
    cl = rowcell[r0:]
    want = [(feat / w4[:, :1]).astype(np.float32), np.stack([cl // (gs * vh), (cl // vh) % gs, cl % vh], axis=1).astype(np.int32),
            w4[:, 0].astype(np.float32), np.clip(w4[:, 1:] / w4[:, :1] + 1e-9, 0.0, 255.0).astype(np.uint8), cl]
    d_side, d_part = [dev(DeviceArray, s) for s in side], [dev(DeviceArray, q) for q in part]
    d_done = filled(DeviceArray, (1,), np.float32)                                           # no single-contributor row reads it
    d_rowcell, d_err = dev(DeviceArray, rowcell), dev(DeviceArray, np.zeros(1, np.int32))
    vps = lambda a: (C.c_void_p * len(a))(*a)
    h_side, h_part, h_done = vps([d.ptr for d in d_side]), vps([d.ptr for d in d_part]), vps([d_done.ptr] * ws)
    h_count = (C.c_int64 * ws)(*[len(r) for r in rows_of])

    def check(outs):
        assert int(d_err.numpy()[0]) == 0
        for got, ref in zip(outs, want):
            assert np.array_equal(got.numpy(), ref)

    exact_and_short(env, lib.avl_merge2_fold_work_bytes, (n_own, ws),
                    lambda w, nb, o: lib.avl_merge2_fold(n_own, r0, ws, D, gs, vh, h_side, h_done, h_part, h_count, d_rowcell.ptr, 0, o[0].ptr,
                                                         o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr, w, nb, d_err.ptr, None),
                    lambda: [filled(DeviceArray, (n_own, D), np.float32), filled(DeviceArray, (n_own, 3), np.int32),
                             filled(DeviceArray, (n_own,), np.float32), filled(DeviceArray, (n_own, 3), np.uint8),
                             filled(DeviceArray, (n_own,), np.int32)], check)
