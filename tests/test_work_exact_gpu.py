"""Every entry point that works in a caller's buffer stays inside what its size query promises (csrc: one layout function per entry
point on the shared Carver serves both the size query and the consumer).  The module imports without a GPU: REGISTRY below names,
for every size query the library exports, the tests here that hold its consumers to it (tests/test_work_bytes_host.py checks that
none is missing).

(a) The workspace is the front of ONE allocation of work_bytes + 4096 bytes whose tail is filled with 0xA5: the call gets exactly
    work_bytes, its result equals a reference that does not go through the ops wrapper alone (the family's restatement under
    tests/_*_ref.py, NumPy or SciPy), and the tail is unchanged.  The canary lies inside the test's own allocation, so an overrun
    is a failed assertion, not a fault.  Every OUTPUT has a tail of its own, 4096 bytes of 0x77 inside its allocation, which is
    checked after every call: a table with room for `cap` rows never gets row `cap`.
(b) With work_bytes - 1 the call returns AVL_ERR_INVALID before any device work: the outputs keep their fill pattern.
(c) The entry points that align the base themselves (their totals carry 256 or 512 bytes of slack for it) run (a) once more from
    an odd address, base + 1 of a 256-aligned allocation: the alignment then eats 255 bytes of the slack, and with 256 bytes of
    slack the last piece ends one byte before the canary (with 512, 257 bytes before it: no address uses more than 255).

The entry points held here.  "aligns": the source calls align256_ptr on the caller's base, so (c) runs; the others get aligned
bases only (their 8-byte atomics would be misaligned from an odd one).  "tight": the case whose last piece that holds data is a
whole multiple of 256 bytes (or whose layout has no rounding), so the first byte past it is the canary and not padding.

  avl_dilate_map, avl_mask_foreground, avl_label_islands, avl_audio_segment, avl_merge2_fold      as before; no (c)
  avl_argsort_bits, avl_merge_partition, avl_merge_rows_other, avl_merge2_prepare                   as before; align
  avl_merge_dir_scan (avl_merge_work_bytes), avl_merge_rows_new, avl_merge_dir_rows (avl_merge_rows_work_bytes)     align
  avl_merge_classify      takes no work buffer: only its outputs' tails are held
  avl_edt2d, avl_mask_decay_2d      tight at (8, 8): the column distances g are 8 * 8 * 4 = 256 bytes
  avl_nearest_pair_i32
  avl_render_topdown, avl_render_view      tight always: H * W * 16 and H * W * 8 bytes, no rounding
  avl_pnp_ransac      tight always: n_hyp * 96 bytes, no rounding
  avl_resize_u8, avl_clip_preprocess      align; tight at B = 2, H = 8, out_w = 4, C = 4: the horizontal pass's bytes are 2 * 8 * 16 = 256.
                          A call without a vertical pass does not use the workspace and, as the header says, does not ask for it
  avl_label_voxels, avl_label_classes      (the last piece is one count per 1024 voxels: never a whole 256 bytes at a test's size)
  avl_pool_rows      tight at N = n = 32, C = 32: max_chunks = n, every chunk is used, the partial sums are 32 * 32 * 8 = 8192 bytes
  avl_object_relations      the table of max_pairs rows is the caller-capacity case of the output tails
  avl_cell_index_build + avl_cell_index_lookup      align (both)
  avl_match_frames      aligns
  avl_travel2d      aligns
  avl_travel_decay_2d      aligns; no size query, the figure of its AVL_REQUIRE: 256 + 16 bytes, tight from base + 1
  avl_grow_labels      aligns; embeds avl_travel2d's workspace
  avl_room_seeds      aligns; embeds avl_label_islands' workspace
  avl_room_doors + avl_room_door_table      align; tight at K = 2: the sorted slots are 64 * 4 = 256 bytes
  avl_colselect_f32      aligns; tight always: the last piece, next_key, is 64 * 4 = 256 bytes
  avl_merge2_plan      aligns; its results live in the work buffer at the offsets it reports
  avl_sim_scores_ws, avl_sim_scores_blocks      another contract, see test_sim_workspace"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

AVL_OK = 0
AVL_ERR_INVALID = 1
CANARY = 4096
FILL = 0x77

# size query -> the tests of this module that run its consumers at exactly that size
REGISTRY = {
    "avl_dilate_map_work_bytes": ["test_dilate_map"],
    "avl_mask_foreground_work_bytes": ["test_mask_foreground"],
    "avl_label_islands_work_bytes": ["test_label_islands"],
    "avl_audio_segment_work_bytes": ["test_audio_segment"],
    "avl_argsort_bits_work_bytes": ["test_argsort_bits"],
    "avl_merge_work_bytes": ["test_merge_partition", "test_merge_dir_scan"],
    "avl_merge_rows_work_bytes": ["test_merge_rows_other", "test_merge_rows_new", "test_merge_dir_rows"],
    "avl_merge2_prepare_work_bytes": ["test_merge2_prepare"],
    "avl_merge2_fold_work_bytes": ["test_merge2_fold"],
    "avl_merge2_work_bytes": ["test_merge2_plan"],
    "avl_edt2d_work_bytes": ["test_edt2d", "test_mask_decay_2d"],
    "avl_nearest_pair_work_bytes": ["test_nearest_pair"],
    "avl_render_topdown_work_bytes": ["test_render_topdown"],
    "avl_render_view_work_bytes": ["test_render_view"],
    "avl_pnp_ransac_work_bytes": ["test_pnp_ransac"],
    "avl_resize_work_bytes": ["test_resize_u8", "test_clip_preprocess"],
    "avl_label_voxels_work_bytes": ["test_label_voxels"],
    "avl_label_classes_work_bytes": ["test_label_classes"],
    "avl_pool_rows_work_bytes": ["test_pool_rows"],
    "avl_object_relations_work_bytes": ["test_object_relations", "test_object_relations_overflow"],
    "avl_cell_index_work_bytes": ["test_cell_index"],
    "avl_match_ws_bytes": ["test_match_frames"],
    "avl_travel2d_workspace_bytes": ["test_travel2d"],
    "avl_grow_labels_workspace_bytes": ["test_grow_labels"],
    "avl_room_seeds_workspace_bytes": ["test_room_seeds"],
    "avl_room_doors_workspace_bytes": ["test_room_doors"],
    "avl_colselect_workspace_bytes": ["test_colselect"],
    "avl_sim_workspace_bytes_n": ["test_sim_workspace", "test_sim_exact_matrix_core_sweep"],
}
# size queries that have no case of their own, each with its reason
EXEMPT = {
    "avl_sim_workspace_bytes": "the figure without N; avl_sim_workspace_bytes_n adds the guard words to it and is the one callers allocate by",
}


@pytest.fixture(scope="module")
def env():
    from avlmaps_amd import _lib, ops
    from avlmaps_amd.device import DeviceArray
    lib = _lib.load()
    _lib.require_gpu()
    return _lib, lib, ops, DeviceArray


def dev(DeviceArray, a):
    return DeviceArray.from_numpy(np.ascontiguousarray(a))


class Out:
    """an output buffer of `shape` whose every byte is FILL, followed inside the same allocation by CANARY bytes of FILL"""

    def __init__(self, DeviceArray, shape, dtype):
        self.shape, self.dtype = tuple(int(s) for s in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.buf = DeviceArray.from_numpy(np.full(self.nbytes + CANARY, FILL, np.uint8))
        self.ptr = self.buf.ptr

    def numpy(self):
        return self.buf.numpy()[:self.nbytes].copy().view(self.dtype).reshape(self.shape)

    def tail_intact(self):
        return bool((self.buf.numpy()[self.nbytes:] == FILL).all())


def filled(DeviceArray, shape, dtype):
    return Out(DeviceArray, shape, dtype)


def untouched(d):
    return bool((d.buf.numpy() == FILL).all())


def tails_intact(outs):
    return all(o.tail_intact() for o in outs)


def exact_and_short(env, query, qargs, call, outputs, check, aligns_base=False, check_work=None, refuses_short=True):
    """call(ws_ptr, ws_bytes, outs) -> status, with fresh FILL-ed outputs() each time: (a), (b) and, for an entry point that aligns
    the base itself, (c) of the module docstring.  query: the size query, or the number of bytes itself where the entry point has
    none.  check_work(outs, work): for an entry point that leaves results in the workspace, `work` its work_bytes bytes after the
    call.  refuses_short=False: the call does not use the workspace and, by its documentation, does not ask for it either: (b) is
    then that the short call gives the same result."""
    _lib, lib, ops, DeviceArray = env
    if isinstance(query, int):
        n = query
    else:
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
    got = buf.numpy()
    assert (got[n:] == 0xA5).all(), "the call wrote past work_bytes"
    assert tails_intact(outs), "the call wrote past the end of an output"
    if check_work is not None:
        check_work(outs, got[:n])
    outs = outputs()
    if refuses_short:
        assert call(buf.ptr, n - 1, outs) == AVL_ERR_INVALID
        assert all(untouched(o) for o in outs), "a refused call wrote to an output"
    else:
        _lib.check(call(buf.ptr, n - 1, outs), "a call that does not use its workspace")
        check(outs)
        assert tails_intact(outs)
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
        assert tails_intact(outs), "the call wrote past the end of an output"
        if check_work is not None:
            check_work(outs, got[1:1 + n])


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


def dir_owner(cell, ws):
    """the directory rank of a cell (csrc/avl_merge.hip)"""
    return ((((np.asarray(cell).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(12)) % np.uint64(ws)).astype(np.int64)


@pytest.mark.parametrize("n", [1, 300])
def test_merge_partition(env, n):
    """avl_merge_partition: the work buffer of avl_merge_work_bytes"""
    _lib, lib, ops, DeviceArray = env
    ws = 3
    rng = np.random.default_rng(n)
    cell = rng.permutation(4 * n + 8)[:n].astype(np.int32)
    key = ((rng.integers(0, 50, n) << 32) | rng.permutation(n)).astype(np.int64)
    dest = dir_owner(cell, ws)
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


def directory_world(R, ws, seed):
    """What a directory rank holds after the first exchange of the directory merge plan: R cells that arrived from ws source ranks,
    grouped by source (rc of them from each), every cell at most once per source and many held by two or three sources -- and
    NumPy's restatement of avl_merge_dir_scan on them (the tensor code of parallel.plan_merge_directory)."""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(1 << 20)[:max(R // 2, 1) + 2].astype(np.int32)
    rc = np.full(ws, R // ws, np.int64)
    rc[0] += R - rc.sum()
    recv = np.concatenate([rng.permutation(pool)[:k] for k in rc]).astype(np.int32)
    assert len(recv) == R and all(k <= len(pool) for k in rc)
    src = np.repeat(np.arange(ws), rc)
    perm = np.argsort(recv, kind="stable").astype(np.int64)          # arrivals are grouped by source: stable = (cell, source) order
    cs, ss = recv[perm], src[perm]
    first = np.ones(R, bool)
    first[1:] = cs[1:] != cs[:-1]
    last = np.ones(R, bool)
    last[:-1] = first[1:]
    prev_r, next_r = np.empty(R, np.int64), np.empty(R, np.int64)
    prev_r[perm] = np.where(first, -1, np.roll(ss, 1))
    next_r[perm] = np.where(last, -1, np.roll(ss, -1))
    m3r, m4r = (prev_r < 0) & (next_r >= 0), prev_r >= 0
    cnt = np.concatenate([np.bincount(src[m3r], minlength=ws), np.bincount(src[m4r], minlength=ws), [first.sum()]]).astype(np.int64)
    reply = ((prev_r + 1) | ((next_r + 1) << 16)).astype(np.int32)
    return dict(recv=recv, rc=rc, perm=perm, first=first.astype(np.uint8), prev_r=prev_r, next_r=next_r, reply=reply,
                m3r=m3r.astype(np.uint8), m4r=m4r.astype(np.uint8), cnt=cnt)


@pytest.mark.parametrize("R", [1, 300])
def test_merge_dir_scan(env, R):
    """avl_merge_dir_scan: the second consumer of avl_merge_work_bytes"""
    _lib, lib, ops, DeviceArray = env
    ws = 3
    w = directory_world(R, ws, R)
    if R > 1:
        assert w["m3r"].any() and w["m4r"].any() and not w["first"].all()
    d_recv, d_rc = dev(DeviceArray, w["recv"]), dev(DeviceArray, w["rc"])
    names = ("perm", "first", "prev_r", "next_r", "reply", "m3r", "m4r", "cnt")

    def check(outs):
        for o, k in zip(outs, names):
            assert np.array_equal(o.numpy(), w[k]), k

    exact_and_short(env, lib.avl_merge_work_bytes, (R,),
                    lambda wk, nb, o: lib.avl_merge_dir_scan(R, d_recv.ptr, d_rc.ptr, ws, 31, *[x.ptr for x in o], wk, nb, None),
                    lambda: [filled(DeviceArray, w[k].shape, w[k].dtype) for k in names], check, aligns_base=True)


def home_world(n, ws, seed):
    """What a rank holds when the directory's replies are back: n slots in sending order ordd, their cells in that order, the packed
    (prev + 1) | (next + 1) << 16 of every entry -- and NumPy's restatement of avl_merge_classify and avl_merge_rows_new"""
    rng = np.random.default_rng(seed)
    cell = rng.permutation(1 << 20)[:n].astype(np.int32)
    dest = dir_owner(cell, ws)
    ordd = np.argsort(dest, kind="stable").astype(np.int64)
    cell_sorted = cell[ordd]
    pv, nx = rng.integers(-1, ws, n), rng.integers(-1, ws, n)
    pv[0] = -1                                                         # at least one new voxel
    back = ((pv + 1) | ((nx + 1) << 16)).astype(np.int32)              # in sending order
    prev, nxt = np.empty(n, np.int64), np.empty(n, np.int64)
    prev[ordd], nxt[ordd] = pv, nx
    is_new = prev < 0
    m3, m4 = (is_new & (nxt >= 0))[ordd], (~is_new)[ordd]
    d_o = dest[ordd]
    cnt = np.concatenate([[is_new.sum()], np.bincount(d_o[m3], minlength=ws), np.bincount(d_o[m4], minlength=ws),
                          np.bincount(prev[prev >= 0], minlength=ws), np.bincount(nxt[nxt >= 0], minlength=ws)]).astype(np.int64)
    key = ((rng.integers(0, 50, n) << 32) | rng.permutation(n)).astype(np.int64)
    return dict(cell_sorted=cell_sorted, ordd=ordd, back=back, prev=prev, nxt=nxt, is_new=is_new.astype(np.uint8), m3=m3.astype(np.uint8),
                m4=m4.astype(np.uint8), cnt=cnt, key=key)


@pytest.mark.parametrize("n", [1, 300])
def test_merge_classify(env, n):
    """avl_merge_classify takes no work buffer (its `ws` is the number of ranks): every output keeps its tail"""
    _lib, lib, ops, DeviceArray = env
    ws = 3
    w = home_world(n, ws, 5 * n)
    d_back, d_ordd, d_cs = dev(DeviceArray, w["back"]), dev(DeviceArray, w["ordd"]), dev(DeviceArray, w["cell_sorted"])
    names = ("prev", "nxt", "is_new", "m3", "m4", "cnt")
    outs = [filled(DeviceArray, w[k].shape, w[k].dtype) for k in names]
    _lib.check(lib.avl_merge_classify(n, d_back.ptr, d_ordd.ptr, d_cs.ptr, ws, *[o.ptr for o in outs], None), "avl_merge_classify")
    for o, k in zip(outs, names):
        assert np.array_equal(o.numpy(), w[k]), k
    assert tails_intact(outs)


@pytest.mark.parametrize("n", [1, 300])
def test_merge_rows_new(env, n):
    """avl_merge_rows_new: the work buffer of avl_merge_rows_work_bytes, all three of its passes (the compaction, the sort of the
    new voxels by key, the list of rows it reports)"""
    _lib, lib, ops, DeviceArray = env
    ws, base = 3, 1000
    w = home_world(n, ws, 5 * n)
    is_new, key, ordd, m3 = w["is_new"] != 0, w["key"], w["ordd"], w["m3"] != 0
    idx_new = np.flatnonzero(is_new)
    idx_new = idx_new[np.argsort(key[idx_new], kind="stable")].astype(np.int64)
    c, n3 = len(idx_new), int(m3.sum())
    row = np.full(n, -1, np.int64)
    row[idx_new] = base + np.arange(c)
    send3 = row[ordd[m3]]
    assert c >= 1 and (n == 1 or (n3 >= 1 and c < n))
    d_new, d_key, d_ordd, d_m3 = dev(DeviceArray, w["is_new"]), dev(DeviceArray, key), dev(DeviceArray, ordd), dev(DeviceArray, w["m3"])

    def check(outs):
        assert np.array_equal(outs[0].numpy(), row) and np.array_equal(outs[1].numpy(), idx_new) and np.array_equal(outs[2].numpy(), send3)

    exact_and_short(env, lib.avl_merge_rows_work_bytes, (n,),
                    lambda wk, nb, o: lib.avl_merge_rows_new(n, c, d_new.ptr, d_key.ptr, 40, base, d_ordd.ptr, d_m3.ptr, n3, o[0].ptr, o[1].ptr,
                                                             o[2].ptr, wk, nb, None),
                    lambda: [filled(DeviceArray, (n,), np.int64), filled(DeviceArray, (c,), np.int64), filled(DeviceArray, (n3,), np.int64)],
                    check, aligns_base=True)


def test_merge_dir_rows(env):
    """avl_merge_dir_rows: the work buffer of avl_merge_rows_work_bytes with all five of its vectors in use"""
    _lib, lib, ops, DeviceArray = env
    R, ws = 300, 3
    w = directory_world(R, ws, R)
    m3r, m4r, first, perm = w["m3r"] != 0, w["m4r"] != 0, w["first"] != 0, w["perm"]
    n3r, n4 = int(m3r.sum()), int(m4r.sum())
    recv3 = np.random.default_rng(8).integers(0, 1 << 40, n3r).astype(np.int64)
    rowfirst_r = np.full(R, -1, np.int64)
    rowfirst_r[m3r] = recv3
    seg = np.cumsum(first) - 1
    row_r = np.empty(R, np.int64)
    row_r[perm] = rowfirst_r[perm[first]][seg]
    send4 = row_r[m4r]
    assert n3r >= 1 and n4 >= 1 and (send4 >= 0).all()
    d_recv3, d_m3r, d_first, d_perm, d_m4r = (dev(DeviceArray, a) for a in (recv3, w["m3r"], w["first"], perm, w["m4r"]))
    exact_and_short(env, lib.avl_merge_rows_work_bytes, (R,),
                    lambda wk, nb, o: lib.avl_merge_dir_rows(R, d_recv3.ptr, d_m3r.ptr, d_first.ptr, d_perm.ptr, d_m4r.ptr, n4, o[0].ptr, wk, nb, None),
                    lambda: [filled(DeviceArray, (n4,), np.int64)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy(), send4), aligns_base=True)


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


# ---------------------------------------------------------------------------------------------------------------- the merge2 plan
@pytest.mark.parametrize("rank", [0, 1])
def test_merge2_plan(env, rank):
    """avl_merge2_plan on a world of 2 peers with 300 and 200 voxels, 41 cells held by both: the results in the work buffer (at the
    offsets the call reports) and the host tables against the NumPy twin of the kernels (merge2.HostKernels)"""
    _lib, lib, ops, DeviceArray = env
    from avlmaps_amd import merge2
    import merge_worlds
    import torch
    sizes, ws, grow_row = [300, 200], 2, 3
    cells, keys = merge_worlds.plan_world(sizes, 17)
    share = [c for c in cells[0].tolist() if c != 0 and c not in set(cells[1].tolist())][:40]
    private = [i for i, c in enumerate(cells[1].tolist()) if c != 0][:40]
    cells[1][private] = share                                          # cell 0 and these 40: held by both peers
    assert all(len(set(c.tolist())) == len(c) for c in cells)
    twins = [merge2.HostKernels(dict(cell=cells[r], first_key=keys[r], sum_feat=np.zeros((sizes[r], 1)))) for r in range(ws)]
    nmax = max(sizes)
    stride = nmax + (nmax + 1) // 2
    gathered = torch.zeros(ws * stride, dtype=torch.int64)
    for r in range(ws):
        twins[r].fill_chunk(gathered[r * stride:(r + 1) * stride], nmax)
    twin = twins[rank]
    res = twin.plan(gathered, sizes, nmax, rank, ws, 31, grow_row, True)
    M, n, E = int(res[0]), sizes[rank], sum(sizes)
    assert M == E - 41 and res[1] >= 0
    want = [("row", twin.row, np.int32), ("prev", twin.prev, np.int32), ("next", twin.next, np.int32), ("order", twin.order, np.int32),
            ("sidx", twin.sidx, np.int32), ("selA", twin.selA, np.int64), ("selB", twin.selB, np.int64), ("idx_prev", twin.idx_prev, np.int32),
            ("idx_next", twin.idx_next, np.int32), ("rowcell", twin.rowcell, np.int32), ("res", res, np.int64)]
    d_gathered, d_perm = dev(DeviceArray, gathered.numpy()), dev(DeviceArray, twin.perm.astype(np.int32))
    h_n = (C.c_int64 * ws)(*sizes)
    nres = len(res)
    host = {}

    def call(wk, nb, o):
        host["off"], host["res"] = (C.c_int64 * 11)(*([-7] * 11)), (C.c_int64 * nres)(*([-7] * nres))
        rc = lib.avl_merge2_plan(ws, rank, h_n, nmax, d_gathered.ptr, d_perm.ptr, 31, grow_row, 1, 0, 0, wk, nb, host["off"], host["res"], None)
        if rc != AVL_OK:                                               # a refused call leaves the host tables alone as well
            assert list(host["off"]) == [-7] * 11 and list(host["res"]) == [-7] * nres
        return rc

    def check(outs):
        assert np.array_equal(np.frombuffer(host["res"], np.int64, nres), res)

    def check_work(outs, work):
        off = list(host["off"])
        for (name, ref, dt), o in zip(want, off):
            got = work[o:o + ref.size * np.dtype(dt).itemsize].copy().view(dt)
            assert np.array_equal(got, np.asarray(ref).astype(dt)), name

    exact_and_short(env, lib.avl_merge2_work_bytes, (E, n, ws, 0), call, lambda: [], check, aligns_base=True, check_work=check_work)


# ---------------------------------------------------------------------------------------------------------------- 2-D images
@pytest.mark.parametrize("shape", [(8, 8), (1, 65)])                  # (8, 8): g is 256 bytes exactly; (1, 65): a second workgroup and tile
def test_edt2d(env, shape):
    from scipy import ndimage
    _lib, lib, ops, DeviceArray = env
    H, W = shape
    img = (np.random.default_rng(H + W).random(shape) < 0.8).astype(np.uint8)
    img.flat[3] = 0
    want = ndimage.distance_transform_edt(img)
    assert want.max() > 1.0
    d_img = dev(DeviceArray, img)

    def check(outs):
        assert np.array_equal(outs[0].numpy(), want) and int(outs[1].numpy()[0]) == 1

    exact_and_short(env, lib.avl_edt2d_work_bytes, (H, W),
                    lambda ws, n, o: lib.avl_edt2d(d_img.ptr, W, H, W, 0, o[0].ptr, o[1].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W), np.float64), filled(DeviceArray, (1,), np.int32)], check)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("shape", [(8, 8), (1, 65)])
def test_mask_decay_2d(env, shape, normalize):
    from scipy import ndimage
    _lib, lib, ops, DeviceArray = env
    H, W = shape
    cs, decay = 0.5, 0.03
    mask = (np.random.default_rng(H * W).random(shape) < 0.1).astype(np.uint8)
    mask.flat[5] = 1
    d = ndimage.distance_transform_edt(mask == 0)
    t = 1 - (d / cs) * decay
    t[t < 0] = 0
    lo, hi = t.min(), t.max()
    assert hi > lo
    want = (t - lo) / (hi - lo) if normalize else t
    d_mask = dev(DeviceArray, mask)

    def check(outs):
        assert np.array_equal(outs[0].numpy(), want) and int(outs[2].numpy()[0]) == 1
        assert np.array_equal(outs[1].numpy(), [lo, hi])

    exact_and_short(env, lib.avl_edt2d_work_bytes, (H, W),
                    lambda ws, n, o: lib.avl_mask_decay_2d(d_mask.ptr, W, H, W, cs, decay, normalize, o[0].ptr, o[1].ptr, o[2].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W), np.float64), filled(DeviceArray, (2,), np.float64), filled(DeviceArray, (1,), np.int32)],
                    check)


@pytest.mark.parametrize("na,nb", [(1, 1), (257, 1025)])              # (257, 1025): a second block along each grid axis
def test_nearest_pair(env, na, nb):
    """ties (coordinates from a small range: many pairs at distance 0, in every block) go to the smallest i * nb + j"""
    _lib, lib, ops, DeviceArray = env
    rng = np.random.default_rng(na + nb)
    a, b = rng.integers(-20, 21, (na, 2)).astype(np.int32), rng.integers(-20, 21, (nb, 2)).astype(np.int32)
    a[-1] = b[-1]                                                      # distance 0 in the last block of either axis as well
    d2 = ((a[:, None].astype(np.int64) - b[None].astype(np.int64)) ** 2).sum(axis=2)
    i, j = np.unravel_index(np.argmin(d2), d2.shape)
    if na > 1:
        assert (d2 == 0).sum() > 10 and (i, j) != (na - 1, nb - 1)
    d_a, d_b = dev(DeviceArray, a), dev(DeviceArray, b)
    exact_and_short(env, lib.avl_nearest_pair_work_bytes, (na, nb),
                    lambda ws, n, o: lib.avl_nearest_pair_i32(d_a.ptr, na, d_b.ptr, nb, o[0].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (3,), np.int64)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy(), [i, j, d2[i, j]]))


# ---------------------------------------------------------------------------------------------------------------- rendering
@pytest.mark.parametrize("window", [(2, 6, 3, 9), (4, 4, 0, 16)])     # 5 x 7 and 1 x 17 cells; the workspace has no rounding
def test_render_topdown(env, window):
    from test_render_gpu import ref_topdown
    _lib, lib, ops, DeviceArray = env
    gs, vh, N, t, bg = 17, 5, 200, 0.3, np.array([9, 200, 31], np.uint8)
    rng = np.random.default_rng(17)
    flat = rng.permutation(9 * 9 * vh)[:N]                             # 200 of the 405 cells of rows and columns 2 .. 10: several per column
    pos = np.stack([flat // (9 * vh) + 2, (flat // vh) % 9 + 2, flat % vh], axis=1).astype(np.int32)
    heat, rgb = rng.random(N).astype(np.float32), rng.integers(0, 256, (N, 3)).astype(np.uint8)
    table = ops.jet_table()
    rmin, rmax, cmin, cmax = window
    H, W = rmax - rmin + 1, cmax - cmin + 1
    want = ref_topdown(pos, heat, rgb, gs, window, t, table, bg)
    assert np.unique(pos[:, 0].astype(np.int64) * gs + pos[:, 1], return_counts=True)[1].max() >= 3
    assert np.any(np.any(want != bg, axis=2))
    d_pos, d_heat, d_rgb, d_table = dev(DeviceArray, pos), dev(DeviceArray, heat), dev(DeviceArray, rgb), dev(DeviceArray, table)
    exact_and_short(env, lib.avl_render_topdown_work_bytes, (H, W),
                    lambda ws, n, o: lib.avl_render_topdown(d_pos.ptr, d_heat.ptr, 0, d_rgb.ptr, d_table.ptr, N, gs, rmin, rmax, cmin, cmax, t,
                                                            bg.ctypes.data, o[0].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W, 3), np.uint8)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy(), want))


@pytest.mark.parametrize("size", [(7, 5), (33, 1)])                   # (W, H); the workspace has no rounding
def test_render_view(env, size):
    from test_render_gpu import ref_view, view_scene
    _lib, lib, ops, DeviceArray = env
    W, H = size
    pos, color, T, (fx, fy, cx, cy) = view_scene(size, W, n_random=200)
    T = np.ascontiguousarray(T, dtype=np.float64)
    znear, smax, bg = 2.0, 4.0, np.array([17, 0, 99], np.uint8)
    want = ref_view(pos, color, T, fx, fy, cx, cy, size, znear, smax, bg)
    assert np.any(np.any(want != bg, axis=2))
    d_pos, d_color = dev(DeviceArray, pos), dev(DeviceArray, color)
    N = len(pos)
    exact_and_short(env, lib.avl_render_view_work_bytes, (W, H),
                    lambda ws, n, o: lib.avl_render_view(d_pos.ptr, d_color.ptr, N, T.ctypes.data, fx, fy, cx, cy, W, H, znear, smax,
                                                         bg.ctypes.data, o[0].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W, 3), np.uint8)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy(), want))


# ---------------------------------------------------------------------------------------------------------------- localization
@pytest.mark.parametrize("n_hyp", [1, 5, 9])                          # a block scores 4 hypotheses: 9 = two whole blocks and one more
def test_pnp_ransac(env, n_hyp):
    """the buffer is n_hyp * 96 bytes with no rounding.  Counts, pose and triples are bit-equal to a second run (through the ops
    wrapper, with its own buffer); the inlier count of the returned pose, and of every hypothesis's pose in the workspace, is
    _loc_synth.inlier_mask's"""
    import _loc_synth as L
    _lib, lib, ops, DeviceArray = env
    sc = L.make_scene(60, 0.6, 11)
    pts, pix, K = sc["points"], sc["pixels"], sc["K"]
    M = len(pts)
    # the first seed whose hypothesis 0 has a solution (three outliers seldom have one): the pose of every case is then a real one
    seed = next(s for s in range(1, 200) if ops.pnp_ransac(pts, pix, K, max_error=L.MAX_ERROR, n_hyp=1, seed=s).hyp_counts[0] > 0)
    again = ops.pnp_ransac(pts, pix, K, max_error=L.MAX_ERROR, n_hyp=n_hyp, seed=seed, want_triples=True, want_poses=True)
    d_pts, d_pix = dev(DeviceArray, pts), dev(DeviceArray, pix)

    def check(outs):
        triples, counts, pose, count = (o.numpy() for o in outs)
        assert np.array_equal(triples, again.triples) and np.array_equal(counts, again.hyp_counts)
        assert np.array_equal(pose.view(np.uint64), np.ascontiguousarray(again.pose).view(np.uint64)) and int(count[0]) == again.count
        assert counts[0] > 0 and int(count[0]) == counts.max() == int(L.inlier_mask(pose, pts, pix, K).sum())

    def check_work(outs, work):
        poses = work.copy().view(np.float64).reshape(n_hyp, 3, 4)
        counts = outs[1].numpy()
        assert np.array_equal(poses.view(np.uint64), np.ascontiguousarray(again.hyp_poses).view(np.uint64))
        for h in range(n_hyp):
            if counts[h] > 0:
                assert int(L.inlier_mask(poses[h], pts, pix, K).sum()) == counts[h], h

    exact_and_short(env, lib.avl_pnp_ransac_work_bytes, (n_hyp,),
                    lambda ws, n, o: lib.avl_pnp_ransac(d_pts.ptr, d_pix.ptr, M, K[0, 0], K[0, 2], K[1, 2], L.MAX_ERROR, seed, n_hyp, o[0].ptr,
                                                        o[1].ptr, o[2].ptr, o[3].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (n_hyp, 3), np.int32), filled(DeviceArray, (n_hyp,), np.int32),
                             filled(DeviceArray, (3, 4), np.float64), filled(DeviceArray, (1,), np.int32)], check, check_work=check_work)


# ---------------------------------------------------------------------------------------------------------------- resize / CLIP
def resize_tables(DeviceArray, R, in_size, out_size):
    """(k pointer, bounds pointer, ksize, keepalive) of one pass from the restatement's tables; nulls where the axis keeps its size"""
    if in_size == out_size:
        return None, None, 0, None
    k, b = R.coeffs_ref(in_size, out_size, "bicubic")
    dk, db = dev(DeviceArray, k), dev(DeviceArray, b)
    return dk.ptr, db.ptr, k.shape[1], (dk, db)


# B = 2 throughout.  (5, 7, 3) -> (3, 4): both passes; -> (5, 4): horizontal only, the workspace is not used; C = 1; and
# (8, 7, 4) -> (3, 4): the horizontal pass's bytes, 2 * 8 * 16 = 256, fill their piece exactly
@pytest.mark.parametrize("H,W,Cn,oh,ow", [(5, 7, 3, 3, 4), (5, 7, 3, 5, 4), (5, 7, 1, 3, 4), (8, 7, 4, 3, 4)])
def test_resize_u8(env, H, W, Cn, oh, ow):
    import _resize_ref as R
    _lib, lib, ops, DeviceArray = env
    B = 2
    imgs = np.stack(R.make_images(H * W + Cn, (H, W, Cn)))
    want = np.stack([R.resize_ref(im, (oh, ow), "bicubic") for im in imgs])
    kh, bh, ksh, keep_h = resize_tables(DeviceArray, R, W, ow)
    kv, bv, ksv, keep_v = resize_tables(DeviceArray, R, H, oh)
    d_in = dev(DeviceArray, imgs)
    exact_and_short(env, lib.avl_resize_work_bytes, (B, H, Cn, ow, int(oh != H)),
                    lambda ws, n, o: lib.avl_resize_u8(d_in.ptr, B, H, W, Cn, kh, bh, ksh, ow, kv, bv, ksv, oh, 0, 0, oh, ow, o[0].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (B, oh, ow, Cn), np.uint8)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy(), want), aligns_base=True, refuses_short=oh != H)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_clip_preprocess(env, dtype):
    import _resize_ref as R
    _lib, lib, ops, DeviceArray = env
    B, H, W, oh, ow, top, left, h, w = 2, 5, 7, 3, 4, 0, 1, 3, 3
    imgs = np.stack(R.make_images(35, (H, W, 3)))
    table = R.table_ref(dtype=dtype)
    want = []
    for im in imgs:
        u8 = R.resize_ref(im, (oh, ow), "bicubic", (top, left, h, w))
        want.append(np.stack([table[u8[:, :, c], c] for c in range(3)]))
    want = np.stack(want)
    kh, bh, ksh, keep_h = resize_tables(DeviceArray, R, W, ow)
    kv, bv, ksv, keep_v = resize_tables(DeviceArray, R, H, oh)
    d_in, d_table = dev(DeviceArray, imgs), dev(DeviceArray, table)
    bits = np.uint32 if dtype == np.float32 else np.uint16
    exact_and_short(env, lib.avl_resize_work_bytes, (B, H, 3, w, 1),
                    lambda ws, n, o: lib.avl_clip_preprocess(d_in.ptr, B, H, W, kh, bh, ksh, ow, kv, bv, ksv, oh, top, left, h, w, d_table.ptr,
                                                             int(dtype == np.float16), o[0].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (B, 3, h, w), dtype)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy().view(bits), want.view(bits)), aligns_base=True)


# ---------------------------------------------------------------------------------------------------------------- sparse voxels
def label_ref(pos, classes, connectivity):
    """scipy.ndimage.label once per class on the class's dense array, all components then numbered by (first cell, class); a voxel
    with a negative class takes part in nothing -> (labels (N,) int32, n)"""
    from scipy import ndimage
    pos, classes = np.asarray(pos, np.int64), np.asarray(classes, np.int64)
    labels = np.zeros(len(pos), np.int32)
    part = classes >= 0
    if not part.any():
        return labels, 0
    mn = pos[part].min(axis=0)
    shape = tuple(pos[part].max(axis=0) - mn + 1)
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    comps = []
    for cls in np.unique(classes[part]).tolist():
        ids = np.flatnonzero(classes == cls)
        q = pos[ids] - mn
        dense = np.zeros(shape, bool)
        dense[q[:, 0], q[:, 1], q[:, 2]] = True
        lab, k = ndimage.label(dense, structure)
        of = lab[q[:, 0], q[:, 1], q[:, 2]]
        for j in range(1, k + 1):
            members = ids[of == j]
            comps.append((min(map(tuple, pos[members].tolist())), cls, members))
    comps.sort(key=lambda c: (c[0], c[1]))
    for j, (_, _, members) in enumerate(comps):
        labels[members] = j + 1
    return labels, len(comps)


def voxel_cloud(N, seed):
    """N cells, some of them twice, in a box of which they fill about 15 %, at negative and positive coordinates"""
    rng = np.random.default_rng(seed)
    side = max(2, int(round((2 * N / 0.15) ** (1 / 3))))
    return (np.stack([rng.integers(0, side, N), rng.integers(0, side, N), rng.integers(0, max(side // 2, 1), N)], axis=1) - 3).astype(np.int32)


# N = 1; N = 300 with half masked; N = 1025 with all masked: two scan blocks, and M = N
@pytest.mark.parametrize("N,share,connectivity", [(1, 1.0, 26), (300, 0.5, 6), (300, 0.5, 26), (1025, 1.0, 18)])
def test_label_voxels(env, N, share, connectivity):
    _lib, lib, ops, DeviceArray = env
    pos = voxel_cloud(N, N)
    mask = np.ones(N, np.uint8) if share == 1.0 else (np.random.default_rng(N + 1).random(N) < share).astype(np.uint8)
    want, want_n = label_ref(pos, np.where(mask != 0, 0, -1), connectivity)
    assert want_n >= 1 and (N == 1 or want_n < int(mask.sum()))
    d_pos, d_mask = dev(DeviceArray, pos), dev(DeviceArray, mask)

    def check(outs):
        assert int(outs[1].numpy()[0]) == want_n and np.array_equal(outs[0].numpy(), want)

    exact_and_short(env, lib.avl_label_voxels_work_bytes, (N,),
                    lambda ws, n, o: lib.avl_label_voxels(d_pos.ptr, d_mask.ptr, N, connectivity, o[0].ptr, o[1].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (N,), np.int32), filled(DeviceArray, (1,), np.int32)], check)


# every voxel takes part.  Three classes: the class keys of sort 1 and their sorted copy fill both halves of the sorted cell keys'
# piece (M = N).  One class: there is no sort 1
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("n_classes", [3, 1])
def test_label_classes(env, n_classes, connectivity):
    _lib, lib, ops, DeviceArray = env
    N = 1025
    pos = voxel_cloud(N, 7)
    classes = (np.random.default_rng(3).integers(0, n_classes, N) * 5 + 2).astype(np.int32)
    want, want_n = label_ref(pos, classes, connectivity)
    assert 1 < want_n < N
    if n_classes == 1:                                                 # avl_label_voxels on the mask classes >= 0, byte for byte
        assert np.array_equal(want, label_ref(pos, np.zeros(N), connectivity)[0])
    d_pos, d_cls = dev(DeviceArray, pos), dev(DeviceArray, classes)

    def check(outs):
        assert int(outs[1].numpy()[0]) == want_n and np.array_equal(outs[0].numpy(), want)

    exact_and_short(env, lib.avl_label_classes_work_bytes, (N,),
                    lambda ws, n, o: lib.avl_label_classes(d_pos.ptr, d_cls.ptr, N, connectivity, o[0].ptr, o[1].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (N,), np.int32), filled(DeviceArray, (1,), np.int32)], check)


def pool_ref(rows, labels, n):
    """the float64 sum of every object's rows in member order: chunks of 256 consecutive members summed one after the other from
    0.0, then the chunks' partial sums one after the other from 0.0 (the order the header pins)"""
    out = np.zeros((n, rows.shape[1]))
    for k in range(1, n + 1):
        members = np.flatnonzero(labels == k)
        total = np.zeros(rows.shape[1])
        for c0 in range(0, len(members), 256):
            part = np.zeros(rows.shape[1])
            for i in members[c0:c0 + 256]:
                part = part + rows[i].astype(np.float64)
            total = total + part
        out[k - 1] = total
    return out


# "full": N = n = 32, C = 32, one member each: max_chunks = N / 256 + n = n and every chunk is used, the partial sums are
#         32 * 32 * 8 = 8192 bytes, a whole multiple of 256: the byte after them is the canary.
# "bound": N = 513, n = 3 with 256, 257 and 0 members: 1 + 2 + 0 chunks of the 5 the bound allows.
# "foreign": the same plus rows labelled 0, -1, n + 1 and 2^31 - 1, which take part in nothing
@pytest.mark.parametrize("case", ["full", "bound", "foreign"])
def test_pool_rows(env, case):
    _lib, lib, ops, DeviceArray = env
    rng = np.random.default_rng(len(case))
    if case == "full":
        N, n, Cn = 32, 32, 32
        labels = (rng.permutation(n) + 1).astype(np.int32)
    else:
        n, Cn = 3, 7
        labels = np.concatenate([np.full(256, 1), np.full(257, 2), [0, -1, n + 1, 2**31 - 1, 0, n + 1, -5] if case == "foreign" else []]).astype(np.int32)
        labels = labels[rng.permutation(len(labels))]
        N = len(labels)
        assert N == (513 if case == "bound" else 520)
    rows = (rng.standard_normal((N, Cn)) * np.exp(rng.uniform(-8, 8, (N, 1)))).astype(np.float32)
    want = pool_ref(rows, labels, n)
    d_rows, d_labels = dev(DeviceArray, rows), dev(DeviceArray, labels)
    exact_and_short(env, lib.avl_pool_rows_work_bytes, (N, Cn, n),
                    lambda ws, nb, o: lib.avl_pool_rows(d_rows.ptr, N, Cn, Cn, d_labels.ptr, n, o[0].ptr, ws, nb, None),
                    lambda: [filled(DeviceArray, (n, Cn), np.float64)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy().view(np.uint64), want.view(np.uint64)))


# ---------------------------------------------------------------------------------------------------------------- the cell index
def build_index(env, pos, gs, vh):
    """the cell index of pos in a buffer of exactly avl_cell_index_work_bytes -> (DeviceArray, its size)"""
    _lib, lib, ops, DeviceArray = env
    nb = C.c_size_t(0)
    _lib.check(lib.avl_cell_index_work_bytes(len(pos), gs, vh, C.byref(nb)), "avl_cell_index_work_bytes")
    index = DeviceArray((nb.value,), np.uint8)
    d_pos = dev(DeviceArray, pos)
    _lib.check(lib.avl_cell_index_build(d_pos.ptr, len(pos), gs, vh, index.ptr, nb.value, None), "avl_cell_index_build")
    _lib.check(lib.avl_device_sync(), "avl_device_sync")
    return index, nb.value


# (300, 8, 7): duplicates (448 cells, 300 rows drawn with replacement); (300, 33, 31): 33 * 33 * 31 = 33759 cells, 1055 words: two
# prefix blocks
@pytest.mark.parametrize("N,gs,vh", [(1, 2, 1), (300, 8, 7), (300, 33, 31)])
def test_cell_index(env, N, gs, vh):
    """avl_cell_index_build, then avl_cell_index_lookup of every cell of the grid (and of some outside it) on the same buffer"""
    import _audit_ref as A
    _lib, lib, ops, DeviceArray = env
    rng = np.random.default_rng(N + gs)
    pos = np.stack([rng.integers(0, gs, N), rng.integers(0, gs, N), rng.integers(0, vh, N)], axis=1).astype(np.int32)
    if N > 1:
        pos[:4] = [[-1, 0, 0], [gs, 0, 0], [0, 0, vh], [0, -1, 0]]    # rows outside the grid are ignored
        assert len(np.unique(pos, axis=0)) < N
    cells = np.concatenate([np.argwhere(np.ones((gs, gs, vh), bool)), [[-1, 0, 0], [0, gs, 0], [0, 0, vh]]]).astype(np.int32)
    Mc = len(cells)
    want = A.lookup_ref(pos, gs, vh, cells)
    assert (want >= 0).any() and (want < 0).any() if N > 1 else True
    d_pos, d_cells = dev(DeviceArray, pos), dev(DeviceArray, cells)

    def call(ws, n, o):
        rc = lib.avl_cell_index_build(d_pos.ptr, N, gs, vh, ws, n, None)
        return rc if rc != AVL_OK else lib.avl_cell_index_lookup(ws, n, N, gs, vh, d_cells.ptr, Mc, o[0].ptr, None)

    exact_and_short(env, lib.avl_cell_index_work_bytes, (N, gs, vh), call, lambda: [filled(DeviceArray, (Mc,), np.int32)],
                    lambda outs: np.testing.assert_array_equal(outs[0].numpy(), want), aligns_base=True)


# ---------------------------------------------------------------------------------------------------------------- object relations
def relations_scene():
    """about 200 voxels of an 8 x 8 x 4 grid, some cells twice, four objects that touch: the quadrants of the map"""
    rng = np.random.default_rng(24)
    gs, vh = 8, 4
    flat = np.concatenate([rng.permutation(gs * gs * vh)[:190], rng.integers(0, gs * gs * vh, 12)])
    pos = np.stack([flat // (gs * vh), (flat // vh) % gs, flat % vh], axis=1).astype(np.int32)
    labels = (1 + 2 * (pos[:, 0] >= 4) + (pos[:, 1] >= 4)).astype(np.int32)
    labels[:5] = [0, 5, -1, 0, 7]                                     # take part in nothing
    return pos, labels, gs, vh, 4


# max_pairs = the number of pairs that exist: rows 0 .. P - 1 are written and nothing after them; 513: a pair table of 2048 slots,
# two scan blocks
@pytest.mark.parametrize("max_pairs", ["P", 513])
def test_object_relations(env, max_pairs):
    import _scene_graph_ref as G
    _lib, lib, ops, DeviceArray = env
    pos, labels, gs, vh, n = relations_scene()
    N, R = len(pos), 1
    want, P = G.reference_relations(pos, labels, n, R, gs, vh)
    assert P == 4 and (want[:, 7] > 0).all()
    cap = P if max_pairs == "P" else max_pairs
    index, index_bytes = build_index(env, pos, gs, vh)
    d_pos, d_labels = dev(DeviceArray, pos), dev(DeviceArray, labels)

    def check(outs):
        table = outs[0].numpy()
        assert int(outs[1].numpy()[0]) == P and np.array_equal(table[:P], want)
        assert (table[P:].view(np.uint8) == FILL).all(), "rows P .. max_pairs - 1 are not written"

    exact_and_short(env, lib.avl_object_relations_work_bytes, (cap,),
                    lambda ws, nb, o: lib.avl_object_relations(index.ptr, index_bytes, N, gs, vh, d_pos.ptr, d_labels.ptr, n, R, cap, o[0].ptr,
                                                               o[1].ptr, ws, nb, None),
                    lambda: [filled(DeviceArray, (cap, 8), np.int64), filled(DeviceArray, (1,), np.int64)], check)


def test_object_relations_overflow(env):
    """max_pairs = 1 with 4 pairs present: the count reports it (some value above max_pairs, the table is then unspecified), and the
    tails of the pair table's workspace and of the one-row output table hold"""
    import _scene_graph_ref as G
    _lib, lib, ops, DeviceArray = env
    pos, labels, gs, vh, n = relations_scene()
    assert G.reference_relations(pos, labels, n, 1, gs, vh)[1] == 4
    index, index_bytes = build_index(env, pos, gs, vh)
    d_pos, d_labels = dev(DeviceArray, pos), dev(DeviceArray, labels)
    exact_and_short(env, lib.avl_object_relations_work_bytes, (1,),
                    lambda ws, nb, o: lib.avl_object_relations(index.ptr, index_bytes, len(pos), gs, vh, d_pos.ptr, d_labels.ptr, n, 1, 1, o[0].ptr,
                                                               o[1].ptr, ws, nb, None),
                    lambda: [filled(DeviceArray, (1, 8), np.int64), filled(DeviceArray, (1,), np.int64)],
                    lambda outs: int(outs[1].numpy()[0]) > 1 or pytest.fail("the count does not report the overflow"))


# ---------------------------------------------------------------------------------------------------------------- the pose search
_MATCH = {}


def match_world():
    """_match_ref's scene of 17 frames, rendered once for both cases"""
    import _match_ref as M
    if not _MATCH:
        _MATCH["scene"] = M.scene(17)
    return M, _MATCH["scene"]


# per frame with R = 1 (3 x 3 shifts, plain stores) and two angles; joint with R = 5 and split = 4 (atomics, blocks past a list's end);
# 17 frames: a second launch of frames
@pytest.mark.parametrize("vh,R,K,joint,split", [(7, 1, 2, 0, 0), (8, 5, 1, 1, 4)])
def test_match_frames(env, vh, R, K, joint, split):
    _lib, lib, ops, DeviceArray = env
    M, (depth, Ts) = match_world()
    F, stride = 17, 3
    H, W = depth.shape[1:]
    pos = M.voxels(vh)
    angles = np.ascontiguousarray([(1.0, 0.0), (np.cos(np.radians(3.0)), np.sin(np.radians(3.0)))][:K], dtype=np.float64)
    want = M.match_ref(pos, M.GS, vh, depth, M.K, Ts, M.CS, angles, R, stride=stride, joint=bool(joint), k0=0, **M.DEPTHS)
    assert want[2].max() > 0 and want[1][:, 3].max() > 0
    V, S = (1 if joint else F), 2 * R + 1
    index, index_bytes = build_index(env, pos, M.GS, vh)
    Kinv = np.ascontiguousarray(np.linalg.inv(M.K))
    T = np.ascontiguousarray(Ts, dtype=np.float64)
    px, py = float(T[0, 0, 3]), float(T[0, 1, 3])
    d_depth = dev(DeviceArray, depth)

    def check(outs):
        for o, ref, what in zip(outs, want, ("scores", "best", "valid")):
            assert np.array_equal(o.numpy(), ref), what

    exact_and_short(env, lib.avl_match_ws_bytes, (F, H, W, stride, K, R, joint),
                    lambda ws, n, o: lib.avl_match_frames(index.ptr, index_bytes, len(pos), M.GS, vh, d_depth.ptr, 0, 1000.0, F, H, W,
                                                          Kinv.ctypes.data, T.ctypes.data, M.CS, stride, M.DEPTHS["min_depth"], M.DEPTHS["max_depth"],
                                                          angles.ctypes.data, K, R, 2, vh - 1, joint, px, py, 0, split, o[0].ptr, o[1].ptr, o[2].ptr,
                                                          ws, n, None),
                    lambda: [filled(DeviceArray, (V, K, S, S), np.uint32), filled(DeviceArray, (V, 4), np.int32), filled(DeviceArray, (V,), np.uint32)],
                    check, aligns_base=True)


# ---------------------------------------------------------------------------------------------------------------- travel and rooms
def travel_map(H, W):
    """free space with a wall that has a door, and two sources, one on each side"""
    free = np.ones((H, W), np.uint8)
    sources = np.zeros((H, W), np.uint8)
    if H > 1:
        free[:, W // 2] = 0
        free[H // 2:H // 2 + 2, W // 2] = 1
        free[3, 5:9] = 0
        sources[1, 2] = sources[H - 2, W - 3] = 1
    else:
        sources[0, 0] = 1
    return free, sources


@pytest.mark.parametrize("shape", [(1, 1), (33, 65)])                 # (33, 65): 2 x 3 tiles
def test_travel2d(env, shape):
    import _travel_ref as TR
    _lib, lib, ops, DeviceArray = env
    H, W = shape
    free, sources = travel_map(H, W)
    A, B = TR.travel_ref(free, sources)
    d_free, d_src = dev(DeviceArray, free), dev(DeviceArray, sources)

    def check(outs):
        stats = outs[2].numpy()
        assert np.array_equal(outs[0].numpy(), A) and np.array_equal(outs[1].numpy(), B)
        assert stats[2] == (A >= 0).sum() and stats[3] == 1 and stats[0] >= 0 and stats[1] >= 0

    exact_and_short(env, lib.avl_travel2d_workspace_bytes, (H, W),
                    lambda ws, n, o: lib.avl_travel2d(d_free.ptr, W, d_src.ptr, W, H, W, o[0].ptr, o[1].ptr, o[2].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W), np.int32), filled(DeviceArray, (H, W), np.int32), filled(DeviceArray, (4,), np.int64)],
                    check, aligns_base=True)


@pytest.mark.parametrize("normalize", [0, 1])
def test_travel_decay_2d(env, normalize):
    """no size query: the figure in its AVL_REQUIRE, 256 bytes of slack and two float64.  From base + 1 the pair ends at the canary"""
    import _travel_ref as TR
    _lib, lib, ops, DeviceArray = env
    H, W = 33, 65
    free, sources = travel_map(H, W)
    free[20:, :3] = 0
    free[19, :4] = 0                                                   # a pocket no walk reaches
    free[25, 1] = 1
    A, B = TR.travel_ref(free, sources)
    assert (A < 0).any() and (A > 0).any()
    want = TR.decay_ref(A, B, 0.02, 0.5, bool(normalize))
    d_a, d_b = dev(DeviceArray, A), dev(DeviceArray, B)

    def check(outs):
        assert np.array_equal(outs[0].numpy(), want) and int(outs[1].numpy()[0]) == 0

    exact_and_short(env, 256 + 16, (),
                    lambda ws, n, o: lib.avl_travel_decay_2d(d_a.ptr, d_b.ptr, H, W, 0.5, 0.02, normalize, o[0].ptr, o[1].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W), np.float64), filled(DeviceArray, (1,), np.int32)], check, aligns_base=True)


def test_grow_labels(env):
    """(33, 65), two seeds, one wall with a door: the workspace embeds avl_travel2d's, which aligns its base again"""
    import _rooms_ref as RR
    _lib, lib, ops, DeviceArray = env
    H, W = 33, 65
    free, sources = travel_map(H, W)
    seeds = np.zeros((H, W), np.int32)
    seeds[1, 2], seeds[H - 2, W - 3] = 2, 1
    owner, A, B = RR.grow_ref(free, seeds)
    assert set(np.unique(owner).tolist()) == {0, 1, 2}
    d_free, d_seeds = dev(DeviceArray, free), dev(DeviceArray, seeds)

    def check(outs):
        stats = outs[3].numpy()
        assert np.array_equal(outs[0].numpy(), A) and np.array_equal(outs[1].numpy(), B) and np.array_equal(outs[2].numpy(), owner)
        assert stats[2] == (A >= 0).sum() and stats[3] == 1 and stats[6] == 0 and stats[7] == 0

    exact_and_short(env, lib.avl_grow_labels_workspace_bytes, (H, W),
                    lambda ws, n, o: lib.avl_grow_labels(d_free.ptr, W, d_seeds.ptr, W, H, W, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W), np.int32) for _ in range(3)] + [filled(DeviceArray, (8,), np.int64)],
                    check, aligns_base=True)


# (1, 2049) with clearance above the radius at every even column: 1025 islands of one cell, two count blocks, and the bound on the
# island count, ceil(H / 2) * ceil(W / 2) = 1025, reached exactly
@pytest.mark.parametrize("shape", [(5, 7), (1, 2049)])
def test_room_seeds(env, shape):
    from scipy import ndimage
    _lib, lib, ops, DeviceArray = env
    H, W = shape
    radius = 1.5
    if H == 1:
        E = np.where(np.arange(W) % 2 == 0, 2.0, 1.0).reshape(1, W)
        least = 1
    else:
        E = np.array([[3, 3, 0, 0, 2, 0, 2], [3, 3, 0, 0, 0, 0, 0], [0, 0, 0, 2, 2, 0, 0], [0, 0, 0, 2, 0, 0, 2], [2, 0, 0, 0, 0, 0, 2]], np.float64)
        least = 2
    lab, n_isl = ndimage.label(E > radius, structure=np.ones((3, 3)))
    want, k = np.zeros((H, W), np.int32), 0
    for old in range(1, n_isl + 1):
        if (lab == old).sum() >= least:
            k += 1
            want[lab == old] = k
    assert (n_isl, k) == ((1025, 1025) if H == 1 else (6, 3))       # (5, 7): three islands of one cell are dropped
    d_E = dev(DeviceArray, E)

    def check(outs):
        assert int(outs[1].numpy()[0]) == k and np.array_equal(outs[0].numpy(), want)

    exact_and_short(env, lib.avl_room_seeds_workspace_bytes, (H, W),
                    lambda ws, n, o: lib.avl_room_seeds(d_E.ptr, H, W, radius, least, o[0].ptr, o[1].ptr, ws, n, None),
                    lambda: [filled(DeviceArray, (H, W), np.int32), filled(DeviceArray, (1,), np.int32)], check, aligns_base=True)


# K = 2: a pair table of 64 slots, the sorted slots are 256 bytes.  K = 40 on a random label image, where hundreds of pairs touch:
# 1024 slots
@pytest.mark.parametrize("K", [2, 40])
def test_room_doors(env, K):
    """avl_room_doors, then avl_room_door_table on the same buffer with D = the number of pairs: a table of exactly D rows"""
    import _rooms_ref as RR
    _lib, lib, ops, DeviceArray = env
    rng = np.random.default_rng(K)
    H, W = (5, 7) if K == 2 else (24, 24)
    labels = rng.integers(0, K + 1, (H, W)).astype(np.int32)
    E = rng.integers(1, 6, (H, W)).astype(np.float64) / 2                 # many equal clearances: the smallest raster index wins
    want = RR.door_table_ref(labels, E)
    D = len(want)
    assert D == 1 if K == 2 else D > 300
    d_labels, d_E = dev(DeviceArray, labels), dev(DeviceArray, E)

    def call(ws, n, o):
        rc = lib.avl_room_doors(d_labels.ptr, d_E.ptr, H, W, K, o[0].ptr, ws, n, None)
        return rc if rc != AVL_OK else lib.avl_room_door_table(ws, n, K, W, D, o[1].ptr, None)

    def check(outs):
        assert outs[0].numpy().tolist() == [D, 0] and np.array_equal(outs[1].numpy(), want)

    exact_and_short(env, lib.avl_room_doors_workspace_bytes, (K,), call,
                    lambda: [filled(DeviceArray, (2,), np.int64), filled(DeviceArray, (D, 10), np.int64)], check, aligns_base=True)


# ---------------------------------------------------------------------------------------------------------------- column selection
# 65 slots: two groups of at most 64 share the one workspace, one after the other
@pytest.mark.parametrize("S", [1, 65])
def test_colselect(env, S):
    """N = 300 rows with NaNs, infinities, zeros of both signs and ties, against np.sort (NaN last, -0 = +0)"""
    _lib, lib, ops, DeviceArray = env
    N, Q = 300, 9
    rng = np.random.default_rng(S)
    scores = rng.integers(-4, 5, (N, Q)).astype(np.float32) / 2
    scores[rng.random((N, Q)) < 0.05] = np.nan
    scores[rng.random((N, Q)) < 0.02] = np.inf
    scores[rng.random((N, Q)) < 0.02] = -np.inf
    scores[rng.random((N, Q)) < 0.05] = -0.0
    scores[:, 4] = np.nan
    scores[:3, 4] = [1.0, -0.0, 1.0]
    cols = rng.integers(0, Q, S).astype(np.int32)
    ks = rng.integers(0, N, S).astype(np.int64)
    cols[0], ks[0] = 4, N - 1
    if S > 1:
        cols[1:5], ks[1:5] = [4, 4, 0, 0], [0, 2, 0, N - 1]
    want = [np.zeros(S, np.float32), np.zeros(S, np.float32), np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int64)]
    for s in range(S):
        col = np.sort(scores[:, cols[s]])
        k = int(ks[s])
        v = col[k]
        want[0][s], want[1][s] = v + np.float32(0), col[min(k + 1, N - 1)] + np.float32(0)
        nan = int(np.isnan(col).sum())
        want[2][s] = N - nan if np.isnan(v) else int((col < v).sum())
        want[3][s] = N if np.isnan(v) else int((col <= v).sum())
        want[4][s] = nan
    d_scores = dev(DeviceArray, scores)

    def check(outs):
        for o, ref in zip(outs, want):
            got = o.numpy()
            assert np.array_equal(got, ref, equal_nan=ref.dtype == np.float32)
            if ref.dtype == np.float32:
                assert not np.signbit(got[got == 0]).any()

    exact_and_short(env, lib.avl_colselect_workspace_bytes, (S,),
                    lambda ws, n, o: lib.avl_colselect_f32(d_scores.ptr, N, Q, Q, cols.ctypes.data, ks.ctypes.data, S, *[x.ptr for x in o], ws, n, None),
                    lambda: [filled(DeviceArray, (S,), np.float32), filled(DeviceArray, (S,), np.float32)] +
                            [filled(DeviceArray, (S,), np.int64) for _ in range(3)], check, aligns_base=True)


# ---------------------------------------------------------------------------------------------------------------- similarity
def sim_inputs(N, D, Q, seed):
    """rows of norm 0.5 .. 2 and unit queries (scores of order 1, as in tests/test_sim_gpu.py), and their float64 product"""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((N, D)).astype(np.float32)
    feat *= (rng.uniform(0.5, 2.0, (N, 1)) / np.linalg.norm(feat, axis=1, keepdims=True)).astype(np.float32)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return feat, q, feat.astype(np.float64) @ q.astype(np.float64).T


# every precision the ops layer can select, and "blocks": one column-block call (one query has one column window: no such call)
SIM_CASES = [(p, Q) for p in ("auto", "exact", "split_f16", "exact_valu", "prepared") for Q in (1, 64, 65)] + [("blocks", 64), ("blocks", 65)]


@pytest.mark.parametrize("precision,Q", SIM_CASES)
def test_sim_workspace(env, precision, Q):
    """avl_sim_scores_ws does not refuse a short buffer, it allocates its own.  So: with exactly avl_sim_workspace_bytes_n bytes the
    tail is untouched; with a buffer one byte short of what the call needs (the end of what the exact-size call wrote, rounded up
    to the layout's 256 bytes, less one), with 255 bytes and with none, scores, argmax and best are bit-identical to the
    exact-size call's and the caller's short buffer keeps its pattern in every byte.  The _n figure is an upper bound by design
    (it still carries the guard words and the gathered queries of an earlier layout), so the tail check catches only gross
    overruns; the tight check of the exact matrix-core path is the condition run_mfma_f32 tests on the host before it launches
    (test_sim_exact_matrix_core_sweep).  "blocks": one column-block call, avl_sim_scores_blocks, queries of two column windows."""
    _lib, lib, ops, DeviceArray = env
    N, D = 257, 512
    feat, q, ref = sim_inputs(N, D, Q, Q)
    blocks = precision == "blocks"
    if blocks:
        q[::2, 256:] = 0.0
        q[1::2, :256] = 0.0
        ref = feat.astype(np.float64) @ q.astype(np.float64).T
        cb, ce = np.where(np.arange(Q) % 2 == 0, 0, 256).astype(np.int32), np.where(np.arange(Q) % 2 == 0, 256, 512).astype(np.int32)
    d_feat, d_q = dev(DeviceArray, feat), dev(DeviceArray, q)
    if precision == "prepared":
        _lib.check(lib.avl_sim_prepare_map(d_feat.ptr, N, D, D, None, None), "avl_sim_prepare_map")
    code = _lib.SIM_AUTO if blocks else ops.PRECISION[precision]
    nb = C.c_size_t(0)
    _lib.check(lib.avl_sim_workspace_bytes_n(N, D, Q, C.byref(nb)), "avl_sim_workspace_bytes_n")
    n = nb.value

    def run(ws_ptr, ws_bytes):
        outs = [filled(DeviceArray, (N, Q), np.float32), filled(DeviceArray, (N,), np.int32), filled(DeviceArray, (N,), np.float32)]
        if blocks:
            rc = lib.avl_sim_scores_blocks(d_feat.ptr, None, N, D, D, d_q.ptr, Q, D, cb.ctypes.data, ce.ctypes.data, outs[0].ptr, outs[1].ptr,
                                           outs[2].ptr, code, ws_ptr, ws_bytes, None)
        else:
            rc = lib.avl_sim_scores_ws(d_feat.ptr, N, D, D, d_q.ptr, Q, D, outs[0].ptr, outs[1].ptr, outs[2].ptr, code, ws_ptr, ws_bytes, None)
        _lib.check(rc, "avl_sim_scores")
        _lib.check(lib.avl_device_sync(), "avl_device_sync")
        assert tails_intact(outs), "the call wrote past the end of an output"
        return [o.numpy() for o in outs]

    host = np.full(n + CANARY, 0x5A, np.uint8)
    host[n:] = 0xA5
    buf = DeviceArray.from_numpy(host)
    sc, am, best = run(buf.ptr, n)
    got = buf.numpy()
    assert (got[n:] == 0xA5).all(), "the call wrote past avl_sim_workspace_bytes_n"
    np.testing.assert_allclose(sc, ref, rtol=0, atol=1e-4)
    assert np.all(ref[np.arange(N), am] >= ref.max(axis=1) - 2e-4)
    np.testing.assert_allclose(best, ref.max(axis=1), rtol=0, atol=1e-4)
    used = np.flatnonzero(got[:n] != 0x5A)
    sizes = [None, 255]
    if len(used):
        sizes.append((int(used[-1]) // 256 + 1) * 256 - 1)             # every part of the layout is a multiple of 256 bytes
    for size in sizes:
        short = None if size is None else DeviceArray.from_numpy(np.full(size + CANARY, 0x5A, np.uint8))
        again = run(None if short is None else short.ptr, 0 if size is None else size)
        for a, b, what in zip(again, (sc, am, best), ("scores", "argmax", "best")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, size)
        if short is not None and len(used):                           # (a call that needs no workspace may do as it likes with 255 bytes)
            assert (short.numpy() == 0x5A).all(), f"the call wrote into a buffer of {size} bytes that is too short for it"


def test_sim_exact_matrix_core_sweep(env):
    """The exact fp32 matrix-core precision writes a query image of nkc * Qtot * (KC + 4) * 4 bytes into a workspace sized by the
    split image of the same plan: run_mfma_f32 checks that it fits before it launches and returns AVL_ERR_STATE otherwise.  One map
    row against every D and Q at which the plan changes shape: every call is AVL_OK, the tail of a buffer of exactly
    avl_sim_workspace_bytes_n holds, and the score row is the float64 product to test_sim_gpu.py's tolerance for this precision."""
    _lib, lib, ops, DeviceArray = env
    for D in (1, 127, 128, 129, 512, 1536, 2050):
        for Q in (1, 3, 64, 65, 100, 128, 170):
            feat, q, ref = sim_inputs(1, D, Q, D + Q)
            d_feat, d_q = dev(DeviceArray, feat), dev(DeviceArray, q)
            nb = C.c_size_t(0)
            _lib.check(lib.avl_sim_workspace_bytes_n(1, D, Q, C.byref(nb)), "avl_sim_workspace_bytes_n")
            n = nb.value
            host = np.full(n + CANARY, 0x5A, np.uint8)
            host[n:] = 0xA5
            buf = DeviceArray.from_numpy(host)
            outs = [filled(DeviceArray, (1, Q), np.float32), filled(DeviceArray, (1,), np.int32), filled(DeviceArray, (1,), np.float32)]
            rc = lib.avl_sim_scores_ws(d_feat.ptr, 1, D, D, d_q.ptr, Q, D, outs[0].ptr, outs[1].ptr, outs[2].ptr, _lib.SIM_EXACT, buf.ptr, n, None)
            assert rc == AVL_OK, (D, Q, lib.avl_last_error())
            _lib.check(lib.avl_device_sync(), "avl_device_sync")
            np.testing.assert_allclose(outs[0].numpy(), ref, rtol=0, atol=1e-4, err_msg=f"D={D} Q={Q}")
            assert ref[0, int(outs[1].numpy()[0])] >= ref.max() - 2e-4, (D, Q)
            assert (buf.numpy()[n:] == 0xA5).all() and tails_intact(outs), (D, Q)
