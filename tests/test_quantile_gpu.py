"""Open-set quantile queries on the GPU (csrc/avl_colselect.hip through ops.column_order_stats, column_quantiles and cols_above, and
VLMap.index_map_quantile / quantile_labels / get_quantile_predict_mask).

Oracle: np.sort of every column and plain NumPy counts and comparisons; it never calls the code under test.  In the sorted column
NaN is the largest value and -0 = +0, so the counts around a value are np.searchsorted's on both sides, which for a value that is
not NaN are (column < v).sum() and (column <= v).sum() (asserted).  Every comparison is np.array_equal (equal_nan where a NaN may
occur): the results are elements of the matrix, integer counts, or float64 expressions of two elements."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_host_mirror import Cfg  # noqa: E402

# every N and every Q of the list at least once: 1, 2 and the sizes around a wave; 4099 and 70 001 rows span several workgroups of a
# pass (70 001 crosses 65 536); 65 and 130 columns need a second group of 64 slots and a second or third word per row
SHAPES = [(1, 1), (2, 2), (63, 63), (64, 64), (65, 65), (257, 130), (257, 2), (65, 63), (4099, 64), (4099, 130), (70001, 1), (70001, 65)]
KINDS = ["bits", "ties", "special"]
PERCENTILES = [0, 33.3, 95, 100]


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


# ------------------------------------------------------------------ inputs
def _special_column(c, N, rng):
    f = np.float32
    kind = c % 6
    if kind == 0:
        return np.full(N, f(0.375))                                                       # all equal
    if kind == 1:
        return rng.choice(np.array([0.0, -0.0, 1.0, -1.0], f), N)                          # +-0 are one value
    if kind == 2:
        return rng.choice(np.array([np.inf, -np.inf, 0.0, 3e38, -3e38], f), N)
    if kind == 3:
        return rng.choice(np.array([1e-45, -1e-45, 1e-40, -1e-40, 0.0, 1.2e-38], f), N)    # denormals around zero
    if kind == 4:
        return -np.abs(rng.standard_normal(N)).astype(f) - f(0.5)                          # all negative
    return rng.standard_normal(N).astype(f)


@functools.lru_cache(maxsize=None)
def matrix(N, Q, kind):
    rng = np.random.default_rng(1000 * Q + N)
    if kind == "bits":                                           # any bit pattern but a NaN: every digit of every pass decides somewhere
        bits = rng.integers(0, 1 << 32, (N, Q), dtype=np.uint64).astype(np.uint32)
        nan = (bits & 0x7FFFFFFF) > 0x7F800000
        bits[nan] &= np.uint32(0xFF7FFFFF)                       # (clears an exponent bit: finite)
        x = bits.view(np.float32)
    elif kind == "ties":                                         # five distinct values per column
        values = rng.standard_normal((5, Q)).astype(np.float32)
        x = values[rng.integers(0, 5, (N, Q)), np.arange(Q)]
    else:
        x = np.stack([_special_column(c, N, rng) for c in range(Q)], axis=1)
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert not np.isnan(x).any()
    x.setflags(write=False)
    return x


def slots_of(N, Q):
    """every column at k = 0, 1, N // 2, N - 2, N - 1 (clipped: small N name a k twice), column after column"""
    ks = np.clip(np.array([0, 1, N // 2, N - 2, N - 1], np.int64), 0, N - 1)
    return np.repeat(np.arange(Q, dtype=np.int64), len(ks)), np.tile(ks, Q)


# ------------------------------------------------------------------ oracle
def oracle_stats(x, columns, ks):
    srt = np.sort(x, axis=0)
    N = len(x)
    out = [np.zeros(len(columns), np.float32), np.zeros(len(columns), np.float32)] + [np.zeros(len(columns), np.int64) for _ in range(3)]
    for s, (c, k) in enumerate(zip(columns, ks)):
        col, v = srt[:, c], srt[k, c]
        out[0][s], out[1][s] = v, col[min(k + 1, N - 1)]
        out[2][s], out[3][s] = np.searchsorted(col, v, "left"), np.searchsorted(col, v, "right")
        out[4][s] = np.isnan(col).sum()
        if not np.isnan(v):
            assert out[2][s] == (x[:, c] < v).sum() and out[3][s] == (x[:, c] <= v).sum()
    return out


def pct(x, q):
    """np.percentile of the float64 columns (inf - inf inside NumPy's interpolation is a NaN, not a warning worth reading)"""
    with np.errstate(invalid="ignore"):
        return np.percentile(np.asarray(x).astype(np.float64), q, axis=0)


def oracle_words(above):
    """(N, Q) bool -> (N, ceil(Q / 64)) uint64, bit c % 64 of word c / 64"""
    N, Q = above.shape
    G = (Q + 63) // 64
    padded = np.zeros((N, G * 64), np.uint8)
    padded[:, :Q] = above
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(N, G)


def thresholds_of(x, rng):
    """per column in turn: the float64 95th percentile, an element of the column (strict >), +inf, -inf, NaN, a value between"""
    N, Q = x.shape
    thr = pct(x, 95)
    for c in range(Q):
        if c % 6 == 1:
            thr[c] = np.float64(x[rng.integers(0, N), c])
        elif c % 6 == 2:
            thr[c] = np.inf
        elif c % 6 == 3:
            thr[c] = -np.inf
        elif c % 6 == 4:
            thr[c] = np.nan
        elif c % 6 == 5:
            thr[c] = np.float64(np.median(x[:, c].astype(np.float64))) + 1e-12
    return thr


def check_stats(got, want):
    for name, g, w in zip(got._fields, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.flatnonzero(~((g == w) | (np.isnan(g.astype(np.float64)) & np.isnan(w.astype(np.float64)))))
        assert bad.size == 0, (name, bad[:8], g[bad[:8]], w[bad[:8]])


# ------------------------------------------------------------------ 1. every shape and content
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,Q", SHAPES)
def test_order_statistics_quantiles_and_membership(ops, N, Q, kind):
    x = matrix(N, Q, kind)
    columns, ks = slots_of(N, Q)
    assert Q < 13 or len(columns) > ops.COLSELECT_SLOTS
    got = ops.column_order_stats(x, columns, ks)
    check_stats(got, oracle_stats(x, columns, ks))
    for q in PERCENTILES:
        want = pct(x, q)
        with np.errstate(invalid="ignore"):
            quant = ops.column_quantiles(x, q)
        assert quant.dtype == np.float64 and quant.shape == (Q,) and np.array_equal(quant, want, equal_nan=True), (q, quant, want)
    thr = thresholds_of(x, np.random.default_rng(N + Q))
    above = x.astype(np.float64) > thr
    mc = Q // 2
    bits, counts, mask = ops.cols_above(x, thr, column=mc)
    assert bits.dtype == np.uint64 and np.array_equal(bits, oracle_words(above))
    assert counts.dtype == np.int64 and np.array_equal(counts, above.sum(axis=0))
    assert mask.dtype == np.uint8 and mask.shape == (N,) and np.array_equal(mask, above[:, mc].astype(np.uint8))
    bits2, counts2 = ops.cols_above(x, thr)
    assert np.array_equal(bits2, bits) and np.array_equal(counts2, counts)


# ------------------------------------------------------------------ 2. NaNs
def test_columns_with_nans(ops):
    N, Q = 4099, 5
    x = matrix(N, Q, "ties").copy()
    rng = np.random.default_rng(7)
    x[rng.random(N) < 0.3, 1] = np.nan
    x[:, 3] = np.nan                                             # nothing but NaNs
    x[17, 4] = np.float32(np.uint32(0xFFC00123).view(np.float32))      # one NaN with a sign and a payload
    columns, ks = slots_of(N, Q)
    got = ops.column_order_stats(x, columns, ks)
    want = oracle_stats(x, columns, ks)
    check_stats(got, want)
    assert np.isnan(got.v_k).any() and (~np.isnan(got.v_k)).any()
    assert got.nan_count.reshape(Q, -1)[:, 0].tolist() == [0, int(np.isnan(x[:, 1]).sum()), 0, N, 1]
    for q in (0, 50, 95, 100):
        quant = ops.column_quantiles(x, q)
        assert np.array_equal(quant, pct(x, q), equal_nan=True)
        assert np.isnan(quant).tolist() == [False, True, False, True, True]
    thr = np.array([0.0, 0.0, np.nan, -np.inf, 0.0])
    bits, counts, mask = ops.cols_above(x, thr, column=1)
    with np.errstate(invalid="ignore"):
        above = x.astype(np.float64) > thr
    assert np.array_equal(bits, oracle_words(above)) and np.array_equal(counts, above.sum(axis=0)) and counts[3] == 0
    assert np.array_equal(mask, above[:, 1].astype(np.uint8))


# ------------------------------------------------------------------ 3. a column slice of a wider matrix, device inputs, repeatability
def test_a_column_slice_of_a_wider_matrix(ops):
    import torch
    from avlmaps_amd.device import DeviceArray
    N, Q, W = 4099, 7, 19
    wide = matrix(N, W, "bits")
    view = wide[:, 5:5 + Q]
    assert view.strides == (4 * W, 4) and not view.flags.c_contiguous
    columns, ks = slots_of(N, Q)
    want = oracle_stats(np.ascontiguousarray(view), columns, ks)
    thr = pct(view, 90)
    above = view.astype(np.float64) > thr
    tview = torch.from_numpy(wide.copy()).cuda()[:, 5:5 + Q]
    assert tview.stride() == (W, 1)
    for scores in (view, tview, DeviceArray.from_numpy(np.ascontiguousarray(view))):
        check_stats(ops.column_order_stats(scores, columns, ks), want)
        assert np.array_equal(ops.column_quantiles(scores, 90), thr)
        bits, counts, mask = ops.cols_above(scores, thr, column=Q - 1)
        assert np.array_equal(bits, oracle_words(above)) and np.array_equal(counts, above.sum(axis=0))
        assert np.array_equal(mask, above[:, Q - 1].astype(np.uint8))
    assert np.array_equal(ops.column_quantiles(view, 90, columns=[6, 0, 6]), thr[[6, 0, 6]])


def test_two_runs_give_identical_bytes_and_device_results(ops):
    from avlmaps_amd.device import DeviceArray
    N, Q = 70001, 65
    x = DeviceArray.from_numpy(matrix(N, Q, "bits"))
    columns, ks = slots_of(N, Q)
    thr = DeviceArray.from_numpy(pct(matrix(N, Q, "bits"), 95))
    runs = []
    for _ in range(2):
        st = ops.column_order_stats(x, columns, ks)
        bits, counts, mask = ops.cols_above(x, thr, column=64, device=True)
        assert isinstance(bits, DeviceArray) and bits.shape == (N, 2) and bits.dtype == np.uint64
        assert isinstance(mask, DeviceArray) and mask.shape == (N,) and mask.dtype == np.uint8 and isinstance(counts, np.ndarray)
        runs.append(b"".join(a.tobytes() for a in st) + bits.numpy().tobytes() + counts.tobytes() + mask.numpy().tobytes())
    assert runs[0] == runs[1]


def test_no_slots_and_no_rows(ops):
    x = matrix(65, 65, "ties")
    st = ops.column_order_stats(x, [], [])
    assert all(len(a) == 0 for a in st) and st.v_k.dtype == np.float32 and st.count_le.dtype == np.int64
    bits, counts, mask = ops.cols_above(np.zeros((0, 3), np.float32), np.zeros(3), column=2)
    assert bits.shape == (0, 1) and counts.tolist() == [0, 0, 0] and mask.shape == (0,)


# ------------------------------------------------------------------ 4. map layer
NAMES = ["chair", "table", "floor"]


@functools.lru_cache(maxsize=None)
def synthetic_scores():
    """3001 voxels of a 40 x 40 x 12 scene at (20, 30, 0) of a 100-cell map, several per column, with scores on a grid of 1 / 64 (ties)"""
    rng = np.random.default_rng(5)
    cells = np.argwhere(np.ones((40, 40, 12), bool))
    cells = cells[rng.permutation(len(cells))[:3001]]
    grid_pos = (cells + np.array([20, 30, 0])).astype(np.int32)
    scores = (rng.integers(0, 64, (len(cells), 3)) / 64).astype(np.float32)
    return grid_pos, np.ascontiguousarray(scores)


def synthetic_vlmap():
    from avlmaps_amd.map import AVLMap
    grid_pos, scores = synthetic_scores()
    cfg = Cfg(map_config=Cfg(map_type="vlmap", grid_size=100, cell_size=0.05,
                             pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                                           base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0])),
              params=Cfg(cs=0.05))
    vm = AVLMap(cfg).vlmap
    vm.grid_pos, vm.scores_mat, vm.categories = grid_pos.copy(), scores.copy(), list(NAMES)
    # the obstacle crop: rows 25 .. 54 and columns 28 .. 61 of the map, so voxels lie outside it on three sides
    vm.rmin, vm.rmax, vm.cmin, vm.cmax = 25, 54, 28, 61
    vm.obstacles_cropped = np.zeros((30, 34), np.uint8)
    return vm


def test_index_map_quantile_and_labels(ops):
    grid_pos, scores = synthetic_scores()
    vm = synthetic_vlmap()
    N = len(scores)
    for percentile in (95.0, 50.0, 0.0, 100.0):
        thr = pct(scores, percentile)
        assert np.array_equal(vm.quantile_thresholds(percentile), thr)
        above = scores.astype(np.float64) > thr
        for cid, name in enumerate(NAMES):
            got = vm.index_map_quantile(name, percentile)
            assert got.dtype == bool and got.shape == (N,) and np.array_equal(got, above[:, cid])
        words, counts = vm.quantile_labels(percentile)
        assert np.array_equal(words, oracle_words(above)) and np.array_equal(counts, above.sum(axis=0))
    assert np.array_equal(vm.index_map_quantile("chair"), scores[:, 0].astype(np.float64) > np.percentile(scores[:, 0].astype(np.float64), 95))
    assert vm.index_map_quantile("chair", 95).sum() < 0.06 * N and not vm.index_map_quantile("chair", 100).any()
    # where the quantile is an element (t = 0) the mask holds what lies above it: N - count_le of that slot
    for percentile, k in ((0.0, 0), (100.0, N - 1), (50.0, 1500)):
        assert ops.quantile_index(percentile, N) == (k, 0.0)
        st = ops.column_order_stats(scores, [0, 1, 2], [k, k, k])
        for cid, name in enumerate(NAMES):
            assert int(vm.index_map_quantile(name, percentile).sum()) == N - int(st.count_le[cid])
    dev = vm._scores_device()
    vm.quantile_thresholds(95.0)
    assert vm._scores_device() is dev                            # uploaded once per scores_mat
    vm.scores_mat = scores.copy()
    assert vm._scores_device() is not dev and vm._quantile_cache == {}


def test_get_quantile_predict_mask_equals_pooling_with_numpy(ops):
    grid_pos, scores = synthetic_scores()
    vm = synthetic_vlmap()
    inside = 0
    for percentile in (95.0, 60.0):
        for cid, name in enumerate(NAMES):
            hit = scores[:, cid].astype(np.float64) > np.percentile(scores[:, cid].astype(np.float64), percentile)
            want = np.zeros_like(vm.obstacles_cropped)
            for (row, col, _), h in zip(grid_pos, hit):
                r, c = int(row) - vm.rmin, int(col) - vm.cmin
                if h and 0 <= r < want.shape[0] and 0 <= c < want.shape[1]:
                    want[r, c] = 1
            got = vm.get_quantile_predict_mask(name, percentile)
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (name, percentile)
            inside += int(want.sum())
            assert hit[(grid_pos[:, 0] < vm.rmin) | (grid_pos[:, 1] > vm.cmax)].any()     # voxels of the mask outside the crop: dropped
    assert inside > 100
    # the device mask is what the instance and heat chains take as it stands
    cid, mask, counts = vm._quantile_mask_device("table", 95.0)
    hit = scores[:, 1].astype(np.float64) > np.percentile(scores[:, 1].astype(np.float64), 95.0)
    assert cid == 1 and counts[1] == hit.sum()
    with ops.label_voxels(vm._device_pos(), mask, connectivity=26) as inst:
        assert np.array_equal(inst.labels > 0, hit)
    heat = vm.heatmap_from_mask(mask, 0.05, 0.1).numpy()
    assert np.array_equal(heat == 1, hit)


# ------------------------------------------------------------------ 5. the app
def test_index_map_quantile_flag_on_a_disk_dataset(tmp_path, capsys):
    """apps.index_map --quantile on a synthetic scene in the on-disk layout: the heat is 1 exactly on the voxels above the category's
    own percentile (at most N - 1 - k of them, k the percentile's rank: fewer only where scores tie), and --instances lists that
    mask's connected components, which partition it"""
    import re
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd import ops
    from avlmaps_amd.apps import create_map, index_map
    scene = make(tmp_path / "scene", frames=6, H=96, W=128)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                  "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(scene), "--config", str(cfg), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    capsys.readouterr()
    heat = index_map.main(["--data-dir", str(scene), "--config", str(cfg), "--query", "sofa", "--text-model", "hash",
                           "--categories", "sofa,table,chair", "--quantile", "90", "--instances", "--min-voxels", "1"])
    out = capsys.readouterr().out
    N = len(heat)
    k, _ = ops.quantile_index(90, N)
    hits = int((heat == 1.0).sum())
    assert heat.dtype == np.float32 and heat.max() == 1.0 and 0.08 * N < hits <= N - 1 - k
    assert f"{hits} of {N} voxels lie above the 90th percentile" in out and "of 'sofa'" in out
    sizes = [int(m) for m in re.findall(r"instance \d+: (\d+) voxels", out)]
    assert f"{len(sizes)} instances of 'sofa'" in out and sum(sizes) == hits
