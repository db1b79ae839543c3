"""The selection kernels (avl_topk_f32 beyond the wave path, avl_argmax_f32) and the row movers of the multi-GPU merge
(avl_rows_add_f64[_async], avl_rows_div_f32, avl_scatter_rows, avl_gather_rows) through the C ABI, bit for bit against NumPy:
NaN / signed zero / infinity / tie order, both kernels of every narrow | wide and byte | 16-byte switch, padded leading dimensions,
a row offset, the grid-stride loops behind the block caps, and the out-of-range and argument checks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from avlmaps_amd import _lib, ops
    from avlmaps_amd.device import DeviceArray
    lib = _lib.load()
    _lib.require_gpu()
    return _lib, lib, ops, DeviceArray


@pytest.fixture(scope="module")
def ops(env):
    return env[2]


# ---- avl_topk_f32, k > 64 ------------------------------------------------------------------------------------------------------

def neg_nan():
    return np.array([0xFFC00000], np.uint32).view(np.float32)[0]                     # a NaN with the sign bit set


def mixed(n, seed):
    """normal values with NaN of both signs, both zeros, both infinities, and repeated values"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(np.float32)
    p = rng.permutation(n)
    m = max(1, n // 16)
    v[p[:m]] = np.nan
    v[p[m:2 * m]] = neg_nan()
    v[p[2 * m:3 * m]] = 0.0
    v[p[3 * m:4 * m]] = -0.0
    v[p[4 * m:5 * m]] = np.inf
    v[p[5 * m:6 * m]] = -np.inf
    v[p[6 * m:8 * m]] = v[p[8 * m]]
    assert np.signbit(v[np.isnan(v)]).any() and not np.signbit(v[np.isnan(v)]).all()
    return v


def topk_vectors():
    rng = np.random.default_rng(9)
    out = {f"mixed{n}": mixed(n, n) for n in (65, 4096, 70001)}
    for name, pair in (("negzero_then_zero", (-0.0, 0.0)), ("zero_then_negzero", (0.0, -0.0))):
        v = -rng.random(300).astype(np.float32) - 0.5                                # the zeros are the largest values
        v[[7, 8, 150, 299]] = [pair[0], pair[1], pair[0], pair[1]]
        out[name] = v
    v = rng.standard_normal(500).astype(np.float32)
    v[[0, 499, 77]] = np.inf
    v[[1, 498, 250]] = -np.inf
    out["inf"] = v
    v = rng.random(8000).astype(np.float32)
    v[1500:6500] = np.float32(0.75)                                                  # 5000 exact ties in the middle of the order
    out["ties5000"] = v
    out["all_equal"] = np.full(4096, 3.0, np.float32)
    return out


TOPK = topk_vectors()


@pytest.mark.parametrize("name", list(TOPK))
def test_topk_beyond_the_wave_path_orders_like_stable_argsort(ops, name):
    """k > 64: value descending, ties (and +0 / -0) by ascending index, NaN of either sign last in index order --
    np.argsort(-v, kind="stable")[:k], the order the header promises for every k"""
    v = TOPK[name]
    order = np.argsort(-v, kind="stable")
    for k in sorted({65, 100, len(v)}):
        if k > len(v):
            continue                                                                 # (avl_topk_f32 requires k <= N)
        idx, val = ops.topk_f32(v, k)
        bad = np.flatnonzero(idx != order[:k])[:4]
        assert np.array_equal(idx, order[:k]), (name, k, bad, idx[bad], order[:k][bad])
        assert np.array_equal(val, v[order[:k]], equal_nan=True), (name, k)
        assert np.array_equal(np.signbit(val), np.signbit(v[order[:k]])), (name, k)  # the values are the elements themselves


# ---- avl_argmax_f32 -------------------------------------------------------------------------------------------------------------

ARGMAX_N = (1, 63, 255, 257, 65536, 65537, 200001)


@pytest.mark.parametrize("N", ARGMAX_N)
def test_argmax_first_maximum_at_every_size(ops, N):
    """less than a block, one element more than a block, the 65536 threads of the launch and one more (the stride loop), a
    maximum in the first and in the last element, twice in different blocks, all -inf, +inf"""
    rng = np.random.default_rng(N)
    base = rng.standard_normal(N).astype(np.float32)
    a, b = N // 5, N - 1                                     # N > 256: different blocks, and b's block has the lower number at 200001
    cases = {"first": (0,), "last": (N - 1,), "twice": (a, b), "twice_same_thread": (N // 7, N // 7 + 65536)}
    for name, at in cases.items():
        if at[-1] >= N:
            continue
        v = base.copy()
        v[list(at)] = 9.0
        i, x = ops.argmax_f32(v)
        assert (i, x) == (int(np.argmax(v)), 9.0) and i == at[0], (name, N, i, x)
    i, x = ops.argmax_f32(base)
    assert i == int(np.argmax(base)) and np.float32(x) == base[i], (N, i, x)
    v = np.full(N, -np.inf, np.float32)
    assert ops.argmax_f32(v) == (0, -np.inf)
    v[N // 2] = -3.0e38
    assert ops.argmax_f32(v) == (N // 2, float(np.float32(-3.0e38)))
    v = base.copy()
    v[[N // 3, N - 1]] = np.inf
    assert ops.argmax_f32(v) == (int(np.argmax(v)), np.inf) and int(np.argmax(v)) == N // 3


def test_argmax_signed_zeros_compare_equal(ops):
    for v in ([-0.0, 0.0], [0.0, -0.0]):
        i, x = ops.argmax_f32(np.array(v, np.float32))
        assert i == 0 and x == 0.0


@pytest.mark.parametrize("N", ARGMAX_N)
def test_argmax_ignores_nan(ops, N):
    """with at least one value that is not NaN the index is np.nanargmax's; an all-NaN vector gives index 0"""
    rng = np.random.default_rng(100 + N)
    assert ops.argmax_f32(np.full(N, np.nan, np.float32))[0] == 0
    if N == 1:
        return
    base = rng.standard_normal(N).astype(np.float32)
    nan_at = {"ends": [0, N - 1], "most": np.flatnonzero(rng.random(N) < 0.9), "all_but_last": np.arange(N - 1),
              "around_max": [max(int(np.argmax(base)) - 1, 0)]}
    for name, at in nan_at.items():
        v = base.copy()
        v[at] = np.nan
        v[1 if name == "ends" else -1] = base[1]                                     # at least one number stays
        i, x = ops.argmax_f32(v)
        assert i == int(np.nanargmax(v)) and np.float32(x) == v[i], (name, N, i, x)
    v = np.full(N, -np.inf, np.float32)                      # the only numbers are -inf: np.nanargmax counts a NaN as -inf, so index 0
    v[0] = np.nan
    assert ops.argmax_f32(v) == (int(np.nanargmax(v)), -np.inf) and int(np.nanargmax(v)) == 0
    v[: N - 1] = np.nan
    assert ops.argmax_f32(v) == (int(np.nanargmax(v)), -np.inf) and int(np.nanargmax(v)) == 0


# ---- avl_rows_add_f64 / avl_rows_add_f64_async ------------------------------------------------------------------------------------

def rows_add(env, sync, n, cols, rows, row0, nrows, src, dst, flag=None):
    """one call on device copies; -> (return code, dst on the host, flag value or None)"""
    _lib, lib, ops, DeviceArray = env
    d_rows, d_src, d_dst = DeviceArray.from_numpy(rows), DeviceArray.from_numpy(src), DeviceArray.from_numpy(dst)
    if sync:
        rc = lib.avl_rows_add_f64(n, cols, d_rows.ptr, row0, nrows, d_src.ptr, src.shape[1], d_dst.ptr, dst.shape[1], None)
        return rc, d_dst.numpy(), None
    d_flag = DeviceArray((1,), np.int32).zero_()
    rc = lib.avl_rows_add_f64_async(n, cols, d_rows.ptr, row0, nrows, d_src.ptr, src.shape[1], d_dst.ptr, dst.shape[1], d_flag.ptr, None)
    return rc, d_dst.numpy(), int(d_flag.numpy()[0])


def rows_add_reference(dst, rows, row0, src, cols):
    want = dst.copy()
    for i, r in enumerate(rows):
        if 0 <= r - row0 < len(want):
            want[r - row0, :cols] += src[i, :cols]
    return want


# n = 3 at every width (16 | 17 is the narrow | wide switch); 70000 x 16 elements exceed the narrow kernel's 256 threads x 16 blocks
# per CU of a 256-CU device, 40000 rows exceed the four rows per block of the wide kernel's 16 blocks per CU: both must stride
ROWS_ADD_CASES = [(3, c) for c in (1, 4, 16, 17, 64, 65, 130)] + [(70_000, 16), (40_000, 17)]


@pytest.mark.parametrize("sync", [False, True], ids=["async", "sync"])
@pytest.mark.parametrize("row0", [0, 1000])
@pytest.mark.parametrize("n,cols", ROWS_ADD_CASES)
def test_rows_add_is_the_sequential_float64_loop(env, n, cols, row0, sync):
    """dst[r - row0, :cols] += src[i, :cols] with ld_src = cols + 3 and ld_dst = cols + 5; distinct rows in random order; the
    padding columns and the rows that are not named stay as they were; a second call adds on top of the first"""
    rng = np.random.default_rng(n + cols)
    nrows = n + 37
    dst = rng.standard_normal((nrows, cols + 5))
    want = dst
    for step in range(2):
        rows = (row0 + rng.permutation(nrows)[:n]).astype(np.int64)
        src = rng.standard_normal((n, cols + 3))
        want = rows_add_reference(dst, rows, row0, src, cols)
        rc, got, flag = rows_add(env, sync, n, cols, rows, row0, nrows, src, dst)
        assert rc == 0 and flag in (None, 0)
        assert np.array_equal(got[:, cols:], dst[:, cols:])                          # padding untouched
        assert np.array_equal(got, want), (step, np.argwhere(got != want)[:4])
        hit = np.zeros(nrows, bool)
        hit[rows - row0] = True
        assert np.array_equal(got[~hit], dst[~hit]) and (got[hit, :cols] != dst[hit, :cols]).any()
        dst = got                                                                    # the sum so far is the next call's input


@pytest.mark.parametrize("cols", [4, 17])
def test_rows_add_out_of_range_rows_and_argument_checks(env, cols):
    _lib, lib, ops, DeviceArray = env
    rng = np.random.default_rng(cols)
    row0, nrows, n = 1000, 9, 7
    rows = np.array([1003, 999, 1008, 1009, 1000, -1, 5], np.int64)                  # 999, 1009, -1 and 5 lie outside [1000, 1009)
    src, dst = rng.standard_normal((n, cols + 3)), rng.standard_normal((nrows, cols + 5))
    want = rows_add_reference(dst, rows, row0, src, cols)
    assert (want != dst).any(axis=1).sum() == 3
    rc, got, flag = rows_add(env, False, n, cols, rows, row0, nrows, src, dst)
    assert rc == 0 and flag == 1 and np.array_equal(got, want)                       # flagged, and every in-range row is right
    rc, got, _ = rows_add(env, True, n, cols, rows, row0, nrows, src, dst)
    assert rc != 0 and "outside" in lib.avl_last_error().decode()
    ok = rows[[0, 2, 4]]
    rc, got, flag = rows_add(env, False, 3, cols, ok, row0, nrows, src, dst)
    assert rc == 0 and flag == 0 and np.array_equal(got, rows_add_reference(dst, ok, row0, src, cols))
    # an empty call needs no pointers; a leading dimension below cols is refused before anything runs
    assert lib.avl_rows_add_f64(0, cols, None, row0, nrows, None, cols, None, cols, None) == 0
    assert lib.avl_rows_add_f64_async(0, cols, None, row0, nrows, None, cols, None, cols, None, None) == 0
    d_rows, d_src, d_dst, d_flag = (DeviceArray.from_numpy(a) for a in (ok, src, dst, np.zeros(1, np.int32)))
    for ld_src, ld_dst in ((cols - 1, cols + 5), (cols + 3, cols - 1)):
        assert lib.avl_rows_add_f64(3, cols, d_rows.ptr, row0, nrows, d_src.ptr, ld_src, d_dst.ptr, ld_dst, None) != 0
        assert "bad shape" in lib.avl_last_error().decode()
        assert lib.avl_rows_add_f64_async(3, cols, d_rows.ptr, row0, nrows, d_src.ptr, ld_src, d_dst.ptr, ld_dst, d_flag.ptr, None) != 0
    assert np.array_equal(d_dst.numpy(), dst) and int(d_flag.numpy()[0]) == 0


# ---- avl_rows_div_f32 -----------------------------------------------------------------------------------------------------------

SENTINEL = np.float32(-7.25)


def rows_div(env, acc, rows, w4, n_out, with_flag=True):
    _lib, lib, ops, DeviceArray = env
    k, D = acc.shape
    d_out = DeviceArray.from_numpy(np.full((n_out, D), SENTINEL, np.float32))
    d_flag = DeviceArray((1,), np.int32).zero_()
    d_acc, d_rows, d_w4 = DeviceArray.from_numpy(acc), DeviceArray.from_numpy(rows), DeviceArray.from_numpy(w4)      # (held until the copy back)
    rc = lib.avl_rows_div_f32(k, D, d_acc.ptr, d_rows.ptr, d_w4.ptr, d_out.ptr, n_out, d_flag.ptr if with_flag else None, None)
    assert rc == 0, lib.avl_last_error()
    return d_out.numpy(), int(d_flag.numpy()[0])


def div_inputs(k, D, seed):
    """acc (k, D), rows (k,) distinct, w4 (n_out, 4) with junk in columns 1..3.  acc[0, 0] / w[rows[0]] is a pair whose float64
    quotient, rounded to float32, is NOT the float32 quotient of the float32-rounded operands (searched here, asserted by the
    caller): a kernel that divides in float32 cannot pass."""
    rng = np.random.default_rng(seed)
    n_out = k + 13
    acc = rng.standard_normal((k, D)) * 40.0
    rows = rng.permutation(n_out)[:k].astype(np.int64)
    w4 = np.concatenate([rng.uniform(0.5, 90.0, (n_out, 1)), rng.uniform(1e3, 1e6, (n_out, 3))], axis=1)
    while True:
        a, w = rng.standard_normal() * 40.0, rng.uniform(0.5, 90.0)
        if np.float32(a / w) != np.float32(a) / np.float32(w):
            break
    acc[0, 0], w4[rows[0], 0] = a, w
    return acc, rows, np.ascontiguousarray(w4), n_out


@pytest.mark.parametrize("k,D", [(k, D) for D in (1, 63, 64, 65, 512) for k in (1, 5)] + [(40_000, 65)])
def test_rows_div_is_the_float64_quotient_rounded_once(env, k, D):
    """out[rows[i]] = float32(acc[i] / w4[rows[i], 0]) in float64; rows of `out` that are not named keep their content.  40000 rows
    exceed four rows per block at the cap of 16 blocks per CU: the wave loop strides."""
    acc, rows, w4, n_out = div_inputs(k, D, 1000 * D + k)
    if k >= 5:
        w4[rows[1], 0] = 0.0                                                         # x / 0 = +-inf, 0 / 0 = NaN
        acc[1, 0] = 0.0
        acc[2, D // 2] = np.inf
        acc[3, D - 1] = -np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = (acc / w4[rows, :1]).astype(np.float32)
        f32 = acc.astype(np.float32) / w4[rows, :1].astype(np.float32)
        wrong_stride = (acc / w4.reshape(-1)[rows][:, None]).astype(np.float32)      # what reading w4[r] for w4[4 r] would give
    assert ref[0, 0] != f32[0, 0] and (k * D < 64 or (ref != f32).sum() >= 5)          # these inputs tell float32 division apart
    assert not np.array_equal(wrong_stride, ref, equal_nan=True)
    want = np.full((n_out, D), SENTINEL, np.float32)
    want[rows] = ref
    got, flag = rows_div(env, acc, rows, w4, n_out)
    assert flag == 0 and np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4]
    if k >= 5:
        assert np.isnan(got[rows[1], 0]) and np.isinf(got[rows[2], D // 2]) and got[rows[3], D - 1] == -np.inf


@pytest.mark.parametrize("D", [1, 65])
def test_rows_div_skips_and_flags_rows_outside_the_output(env, D):
    acc, rows, w4, n_out = div_inputs(6, D, D)
    for bad in (-1, n_out):
        r = rows.copy()
        r[2] = bad
        want = np.full((n_out, D), SENTINEL, np.float32)
        keep = np.arange(6) != 2
        want[r[keep]] = (acc[keep] / w4[r[keep], :1]).astype(np.float32)
        got, flag = rows_div(env, acc, r, w4, n_out)
        assert flag == 1 and np.array_equal(got, want), bad
        got, _ = rows_div(env, acc, r, w4, n_out, with_flag=False)                   # no flag to raise: the row is skipped all the same
        assert np.array_equal(got, want), bad
    want = np.full((n_out, D), SENTINEL, np.float32)
    want[rows] = (acc / w4[rows, :1]).astype(np.float32)
    got, _ = rows_div(env, acc, rows, w4, n_out, with_flag=False)
    assert np.array_equal(got, want)


# ---- avl_scatter_rows / avl_gather_rows -----------------------------------------------------------------------------------------

def scatter(env, src, rows, n_dst, fill=0xA5):
    _lib, lib, ops, DeviceArray = env
    d_dst = DeviceArray.from_numpy(np.full((n_dst, src.shape[1]), fill, np.uint8))
    d_flag = DeviceArray((1,), np.int32).zero_()
    d_src, d_rows = DeviceArray.from_numpy(src), DeviceArray.from_numpy(rows)
    assert d_src.ptr % 16 == 0 and d_dst.ptr % 16 == 0
    rc = lib.avl_scatter_rows(d_src.ptr, src.shape[1], d_rows.ptr, len(rows), d_dst.ptr, n_dst, d_flag.ptr, None)
    assert rc == 0, lib.avl_last_error()
    return d_dst.numpy(), int(d_flag.numpy()[0])


def gather(env, src, rows, src_offset=0):
    """rows of src[src_offset:] (bytes) viewed as (-1, row_bytes)"""
    _lib, lib, ops, DeviceArray = env
    rb = src.shape[1]
    d_src, d_rows = DeviceArray.from_numpy(src), DeviceArray.from_numpy(rows)
    d_dst = DeviceArray.from_numpy(np.full((len(rows), rb), 0x5A, np.uint8))
    _lib.check(lib.avl_gather_rows(d_src.ptr + src_offset, rb, d_rows.ptr, len(rows), d_dst.ptr, None), "avl_gather_rows")
    return d_dst.numpy()


@pytest.mark.parametrize("row_bytes,n", [(rb, n) for rb in (16, 48, 2048) for n in (1, 1000)] + [(16, 40_000)])
def test_scatter_rows_is_fancy_index_assignment(env, row_bytes, n):
    """dst[rows] = src on byte views; the rows of dst that are not named keep their bytes; 40000 rows exceed the block cap"""
    rng = np.random.default_rng(row_bytes + n)
    n_dst = n + 29
    src = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
    rows = rng.permutation(n_dst)[:n].astype(np.int64)
    want = np.full((n_dst, row_bytes), 0xA5, np.uint8)
    want[rows] = src
    got, flag = scatter(env, src, rows, n_dst)
    assert flag == 0 and np.array_equal(got, want)
    if n >= 1000:                                                                    # rows outside [0, n_dst) are skipped and flagged
        bad = rows.copy()
        bad[[3, 500, n - 1]] = [-1, n_dst, n_dst + 5]
        keep = (bad >= 0) & (bad < n_dst)
        want = np.full((n_dst, row_bytes), 0xA5, np.uint8)
        want[bad[keep]] = src[keep]
        got, flag = scatter(env, src, bad, n_dst)
        assert flag == 1 and np.array_equal(got, want)


def test_scatter_rows_refuses_rows_it_cannot_move_as_16_byte_words(env):
    _lib, lib, ops, DeviceArray = env
    d_src, d_dst = DeviceArray.from_numpy(np.zeros((8, 48), np.uint8)), DeviceArray.from_numpy(np.full((8, 48), 0xA5, np.uint8))
    d_rows = DeviceArray.from_numpy(np.arange(4, dtype=np.int64))
    assert lib.avl_scatter_rows(d_src.ptr, 12, d_rows.ptr, 4, d_dst.ptr, 8, None, None) != 0
    assert "16 bytes" in lib.avl_last_error().decode()
    assert lib.avl_scatter_rows(d_src.ptr + 4, 16, d_rows.ptr, 4, d_dst.ptr, 8, None, None) != 0
    assert "aligned" in lib.avl_last_error().decode()
    assert lib.avl_scatter_rows(d_src.ptr, 16, d_rows.ptr, 4, d_dst.ptr + 4, 8, None, None) != 0
    assert (d_dst.numpy() == 0xA5).all()
    assert lib.avl_scatter_rows(None, 16, None, 0, None, 8, None, None) == 0         # nothing to move
    assert lib.avl_scatter_rows(d_src.ptr, 16, d_rows.ptr, 4, d_dst.ptr, 8, None, None) == 0      # a null flag is accepted


# 3 | 12: the byte kernel; 16 | 2048: a wave per row.  100000 x 12 bytes exceed the byte kernel's 256 threads x 16 blocks per CU
# (1.05 M on 256 CUs), 40000 rows the four rows per block of the wide kernel at the same cap
@pytest.mark.parametrize("row_bytes,n_src,n", [(3, 50, 200), (12, 50, 200), (16, 50, 200), (2048, 50, 200), (12, 5000, 100_000), (16, 5000, 40_000)])
def test_gather_rows_is_fancy_indexing(env, row_bytes, n_src, n):
    rng = np.random.default_rng(row_bytes + n)
    src = rng.integers(0, 256, (n_src, row_bytes), dtype=np.uint8)
    rows = rng.integers(0, n_src, n).astype(np.int64)                                # indices repeat
    rows[:2] = [n_src - 1, 0]
    assert len(np.unique(rows)) < n
    assert np.array_equal(gather(env, src, rows), src[rows])


def test_gather_rows_from_a_base_that_is_not_16_byte_aligned(env):
    """16-byte rows that start 4 bytes into an allocation cannot be moved as 16-byte words: the byte kernel, and still exact"""
    rng = np.random.default_rng(4)
    raw = rng.integers(0, 256, 4 + 300 * 16, dtype=np.uint8)
    src = np.concatenate([raw, np.zeros(12, np.uint8)]).reshape(-1, 16)              # the upload; the rows start at byte 4
    rows = rng.integers(0, 300, 1000).astype(np.int64)
    rows[:2] = [299, 0]
    assert np.array_equal(gather(env, src, rows, src_offset=4), raw[4:].reshape(300, 16)[rows])


@pytest.mark.parametrize("row_bytes", [16, 2048])
def test_gather_after_scatter_over_a_permutation_is_the_identity(env, row_bytes):
    rng = np.random.default_rng(row_bytes)
    n = 777
    src = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
    perm = rng.permutation(n).astype(np.int64)
    placed, flag = scatter(env, src, perm, n)
    assert flag == 0 and np.array_equal(placed[perm], src)
    assert np.array_equal(gather(env, placed, perm), src)
