"""Object instances in 3-D on the GPU (csrc/avl_instances.hip through ops.label_voxels, VLMap.get_instances_3d and
AVLMap.index_object_instance).

Oracle: SciPy on the dense array of the masked voxels' bounding box -- ndimage.label with generate_binary_structure(3, 1 | 2 | 3),
find_objects for the boxes, np.add.at for the counts and the coordinate sums -- plus NumPy sorts for `first` and `best`.  Every
comparison is np.array_equal: all results are integers (or one of the given scores) that are unique by definition."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_host_mirror import Cfg  # noqa: E402

RANK = {6: 1, 18: 2, 26: 3}
COLS = 12


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


# ------------------------------------------------------------------ oracle and inputs
def oracle(pos, mask, connectivity, scores=None):
    """-> labels (N,) int32, n, table (n, 12) int64, best_score (n,) float32"""
    pos, m = np.asarray(pos, np.int64).reshape(-1, 3), np.asarray(mask).astype(bool)
    labels = np.zeros(len(pos), np.int32)
    if not m.any():
        return labels, 0, np.zeros((0, COLS), np.int64), np.zeros((0,), np.float32)
    idx, p = np.flatnonzero(m), pos[m]
    lo = p.min(0)
    q = p - lo
    dense = np.zeros(q.max(0) + 1, np.uint8)
    dense[q[:, 0], q[:, 1], q[:, 2]] = 1
    lab, n = ndimage.label(dense, ndimage.generate_binary_structure(3, RANK[connectivity]))
    lv = lab[q[:, 0], q[:, 1], q[:, 2]]
    labels[m] = lv
    table = np.zeros((n, COLS), np.int64)
    np.add.at(table[:, 0], lv - 1, 1)
    for k, sl in enumerate(ndimage.find_objects(lab)):
        for c in range(3):
            table[k, 1 + 2 * c], table[k, 2 + 2 * c] = sl[c].start + lo[c], sl[c].stop - 1 + lo[c]
    for c in range(3):
        np.add.at(table[:, 7 + c], lv - 1, p[:, c])
    order = np.lexsort((idx, p[:, 2], p[:, 1], p[:, 0], lv))                 # by label, then cell, then voxel index
    _, at = np.unique(lv[order], return_index=True)
    table[:, 10] = idx[order[at]]
    best_score = np.zeros(n, np.float32)
    table[:, 11] = -1
    if scores is not None:
        s = np.asarray(scores, np.float32)[idx]
        order = np.lexsort((idx, -s.astype(np.float64), lv))                 # by label, then score descending, then voxel index
        _, at = np.unique(lv[order], return_index=True)
        table[:, 11] = idx[order[at]]
        best_score = np.asarray(scores, np.float32)[table[:, 11]]
    return labels, n, table, best_score


def voxel_list(dense, rng, unmasked=True, offset=(0, 0, 0)):
    """a shuffled voxel list whose masked voxels are the set cells of `dense`, with about as many unmasked voxels in other cells"""
    cells = np.argwhere(dense)
    mask = np.ones(len(cells), np.uint8)
    if unmasked:
        free = np.argwhere(~dense.astype(bool))
        free = free[rng.permutation(len(free))[:max(len(cells), 1)]]
        cells, mask = np.concatenate([cells, free]), np.concatenate([mask, np.zeros(len(free), np.uint8)])
    perm = rng.permutation(len(cells))
    return (cells[perm] + np.asarray(offset)).astype(np.int32), mask[perm]


def check(ops, pos, mask, connectivity, scores=None):
    want = oracle(pos, mask, connectivity, scores)
    with ops.label_voxels(pos, mask, connectivity=connectivity, scores=scores) as got:
        assert got.n == want[1], (got.n, want[1])
        assert got.labels.dtype == np.int32 and np.array_equal(got.labels, want[0])
        assert got.table.dtype == np.int64 and got.table.shape == (want[1], COLS)
        for c in range(COLS):
            assert np.array_equal(got.table[:, c], want[2][:, c]), f"table column {c}"
        assert got.best_score.dtype == np.float32 and np.array_equal(got.best_score, want[3])
        if want[1]:
            assert np.array_equal(got.centers, want[2][:, 7:10] / want[2][:, 0:1].astype(np.float64))
    return want


@functools.lru_cache(maxsize=None)
def random_box(shape, density, seed=0, offset=(0, 0, 0)):
    rng = np.random.default_rng(seed)
    dense = rng.random(shape) < density
    pos, mask = voxel_list(dense, rng, offset=offset)
    scores = rng.choice(np.array([0, 0.25, 0.5, 1], np.float32), len(pos))
    for a in (pos, mask, scores):
        a.setflags(write=False)
    return pos, mask, scores


# ------------------------------------------------------------------ 1. small random boxes
@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("density", [0.1, 0.3, 0.6])
def test_small_random_boxes(ops, density, connectivity):
    pos, mask, _ = random_box((9, 7, 5), density)
    assert 0 < mask.sum() < len(mask)
    check(ops, pos, mask, connectivity)


# ------------------------------------------------------------------ 2. many waves and workgroups
@pytest.mark.parametrize("density,connectivity,least,largest", [(0.1, 26, 500, 400), (0.3, 6, 2000, 0), (0.2, 18, 200, 8000)])
def test_many_waves_and_workgroups(ops, density, connectivity, least, largest):
    pos, mask, scores = random_box((64, 64, 16), density)
    _, n, table, _ = check(ops, pos, mask, connectivity, scores)
    assert n >= least and table[:, 0].max() >= largest          # the input is what it claims: many instances / one long union chain


def test_labels_over_two_rounds_of_the_offsets_scan(ops):
    """1024 * 1024 + 1 voxels are 1025 scan blocks of 1024, one more than the one-workgroup scan of the block counts has threads: its
    second round carries the total of the first, and the last voxel, the only one of block 1024, is compacted behind it"""
    rng = np.random.default_rng(6)
    n_vox = 1024 * 1024 + 1
    cells = np.argwhere(np.ones((1025, 1024, 1), bool))[rng.permutation(1025 * 1024)[:n_vox]].astype(np.int32)
    mask = (rng.random(n_vox) < 0.3).astype(np.uint8)
    mask[-1] = 1                                                # the voxel whose place comes from the carried total
    labels, n, _, _ = oracle(cells, mask, 26)
    assert n > 1024                                             # 8-connected sites at 30 %: far below percolation, tens of thousands
    with ops.label_voxels(cells, mask, connectivity=26) as got:
        assert got.n == n, (got.n, n)
        assert got.labels.dtype == np.int32 and np.array_equal(got.labels, labels)


# ------------------------------------------------------------------ 3. heights beyond one 64-bit word
@pytest.mark.parametrize("shape,density,connectivity", [((3, 3, 130), 0.5, 6), ((40, 40, 70), 0.08, 26)])
def test_tall_boxes(ops, shape, density, connectivity):
    pos, mask, _ = random_box(shape, density)
    check(ops, pos, mask, connectivity)


# ------------------------------------------------------------------ 4. chains
def serpentine_3d(H=24, W=24, D=5):
    """a one-voxel-wide line: every second row of every second layer, joined at alternating ends and between the layers"""
    m = np.zeros((H, W, D), bool)
    rows = list(range(0, H, 2))
    for li, h in enumerate(range(0, D, 2)):
        m[rows, :, h] = True
        for k in range(len(rows) - 1):
            m[rows[k] + 1, W - 1 if k % 2 == 0 else 0, h] = True
        if h + 2 < D:                                      # on to the next layer, at the row where this layer's line ends
            m[rows[-1] if li % 2 == 0 else rows[0], 0, h + 1] = True
    return m


def test_the_serpentine_is_one_line():
    m = serpentine_3d()
    lab, n = ndimage.label(m, ndimage.generate_binary_structure(3, 1))
    assert n == 1
    nb = ndimage.convolve(m.astype(int), ndimage.generate_binary_structure(3, 1).astype(int), mode="constant") - 1
    assert nb[m].max() <= 3 and (nb[m] == 2).mean() > 0.8          # a line: nearly every voxel has exactly two neighbours


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_serpentine_is_one_instance(ops, connectivity):
    pos, mask = voxel_list(serpentine_3d(), np.random.default_rng(1))
    assert check(ops, pos, mask, connectivity)[1] == 1


@pytest.mark.parametrize("flat,counts", [(False, {26: 1, 18: 200, 6: 200}), (True, {26: 1, 18: 1, 6: 200})])
def test_diagonals(ops, flat, counts):
    k = np.arange(200, dtype=np.int32)
    pos = np.stack([k, k, np.zeros_like(k) if flat else k], axis=1)[np.random.default_rng(2).permutation(200)]
    for connectivity, n in counts.items():
        assert check(ops, pos, np.ones(200, np.uint8), connectivity)[1] == n


# ------------------------------------------------------------------ 5. edges
def test_no_voxels_and_no_masked_voxel(ops):
    with ops.label_voxels(np.zeros((0, 3), np.int32), np.zeros((0,), np.uint8)) as got:
        assert got.n == 0 and got.labels.shape == (0,) and got.table.shape == (0, COLS) and got.best_score.shape == (0,)
    pos, mask, _ = random_box((9, 7, 5), 0.3)
    with ops.label_voxels(pos, np.zeros_like(mask)) as got:
        assert got.n == 0 and got.labels.dtype == np.int32 and not got.labels.any() and got.labels.shape == (len(pos),)
        assert got.table.shape == (0, COLS) and got.table.dtype == np.int64 and got.centers.shape == (0, 3)


def test_one_voxel_and_a_full_box(ops):
    _, n, table, _ = check(ops, np.array([[7, -3, 2]], np.int32), np.ones(1, np.uint8), 26)
    assert n == 1 and table[0].tolist() == [1, 7, 7, -3, -3, 2, 2, 7, -3, 2, 0, -1]
    for connectivity in (6, 26):
        pos, mask = voxel_list(np.ones((8, 8, 8), bool), np.random.default_rng(3), unmasked=False)
        _, n, table, _ = check(ops, pos, mask, connectivity)
        assert n == 1 and table[0, 0] == 512


def test_voxels_that_share_a_cell(ops):
    pos = np.array([[4, 4, 4], [0, 0, 0], [4, 4, 4], [0, 0, 1], [4, 4, 4], [0, 0, 0]], np.int32)
    mask = np.array([1, 1, 1, 1, 0, 1], np.uint8)              # voxel 4 lies in a masked cell and is not masked itself
    with ops.label_voxels(pos, mask, connectivity=6) as got:
        assert got.n == 2 and got.labels.tolist() == [2, 1, 2, 1, 0, 1]
        assert got.table[:, 0].tolist() == [3, 2] and got.table[:, 10].tolist() == [1, 0]
    check(ops, pos, mask, 6, scores=np.array([1, 0.5, 1, 0.5, 9, 0.5], np.float32))


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_a_shifted_map_has_the_same_labels(ops, connectivity):
    pos, mask, _ = random_box((9, 7, 5), 0.3)
    shifted = (pos + np.array([5000, 7000, 3])).astype(np.int32)
    want = check(ops, shifted, mask, connectivity)
    assert np.array_equal(want[0], oracle(pos, mask, connectivity)[0])
    check(ops, (pos - np.array([5000, 7000, 3])).astype(np.int32), mask, connectivity)


def test_the_largest_box_and_one_cell_more(ops):
    from avlmaps_amd._lib import AvlError
    side = ops.INSTANCES_MAX_BOX_SIDE
    assert side == 1 << 20
    far = np.array([[0, 0, 0], [side - 1, side - 1, side - 1], [side - 1, side - 1, side - 2], [5, 5, 5]], np.int32)
    with ops.label_voxels(far, np.array([1, 1, 1, 0], np.uint8), scores=np.array([1, 2, 3, 4], np.float32)) as got:      # a 60-bit cell key
        assert got.n == 2 and got.labels.tolist() == [1, 2, 2, 0]
        assert got.table.tolist() == [[1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                                      [2, side - 1, side - 1, side - 1, side - 1, side - 2, side - 1, 2 * side - 2, 2 * side - 2, 2 * side - 3, 2, 2]]
        assert got.best_score.tolist() == [1, 3]
    for axis in range(3):
        pos = np.zeros((3, 3), np.int32)
        pos[1, axis] = side + 1                                 # a masked pair 2^20 + 1 cells apart
        pos[2, axis] = -(1 << 30)                               # an unmasked voxel does not count
        with pytest.raises(AvlError, match="bounding box"):
            ops.label_voxels(pos, np.array([1, 1, 0], np.uint8))
        pos[1, axis] = side - 1
        assert check(ops, pos, np.array([1, 1, 0], np.uint8), 26)[1] == 2


def test_bad_arguments(ops):
    pos, mask, _ = random_box((9, 7, 5), 0.3)
    with pytest.raises(ValueError):
        ops.label_voxels(pos, mask, connectivity=8)
    with pytest.raises(ValueError):
        ops.label_voxels(pos[:, :2], mask)
    with pytest.raises(ValueError):
        ops.label_voxels(pos, mask[:-1])
    with pytest.raises(TypeError):
        ops.label_voxels(pos.astype(np.float32), mask)


# ------------------------------------------------------------------ 6. scores
@pytest.mark.parametrize("connectivity", [6, 26])
def test_scores_with_ties(ops, connectivity):
    pos, mask, scores = random_box((9, 7, 5), 0.6)
    _, n, table, best = check(ops, pos, mask, connectivity, scores)
    big = table[:, 0] >= 8
    assert big.any() and (best[big] == 1).all()                # eight draws from four values: the maximum is shared, ties occur
    assert (check(ops, pos, mask, connectivity)[2][:, 11] == -1).all()
    signed = np.where(scores == 0, np.float32(-0.0), -scores).astype(np.float32)        # -0 and negative scores
    check(ops, pos, mask, connectivity, signed)


# ------------------------------------------------------------------ 7. device inputs and outputs
def test_device_inputs_and_outputs(ops):
    from avlmaps_amd.device import DeviceArray
    pos, _, scores = random_box((64, 64, 16), 0.2)
    category = np.random.default_rng(4).integers(0, 3, len(pos)).astype(np.int32)
    mask = ops.mask_from_argmax(DeviceArray.from_numpy(category), 1)
    assert isinstance(mask, DeviceArray)
    want = oracle(pos, category == 1, 18, scores)
    runs = []
    for _ in range(2):
        with ops.label_voxels(DeviceArray.from_numpy(pos), mask, 18, scores=DeviceArray.from_numpy(scores), device=True) as got:
            assert isinstance(got.labels, DeviceArray) and got.labels.shape == (len(pos),) and got.labels.dtype == np.int32
            labels = got.labels.numpy()
            assert got.n == want[1] and np.array_equal(labels, want[0]) and np.array_equal(got.table, want[2])
            assert np.array_equal(got.best_score, want[3])
            for k in (1, got.n // 2, got.n):
                m = got.mask_of(k)
                assert isinstance(m, DeviceArray) and m.dtype == np.uint8 and np.array_equal(m.numpy(), (want[0] == k).astype(np.uint8))
            with pytest.raises(IndexError):
                got.mask_of(got.n + 1)
            with pytest.raises(IndexError):
                got.mask_of(0)
            runs.append((labels.tobytes(), got.table.tobytes(), got.best_score.tobytes()))
    assert runs[0] == runs[1]
    with pytest.raises(ValueError):
        got.mask_of(1)                                           # closed


def test_torch_inputs(ops):
    import torch
    pos, mask, scores = random_box((9, 7, 5), 0.3)
    want = oracle(pos, mask, 26, scores)
    dev = torch.device("cuda")
    with ops.label_voxels(torch.from_numpy(pos.copy()).to(dev), torch.from_numpy(mask.astype(bool)).to(dev),
                          scores=torch.from_numpy(scores.copy()).to(dev)) as got:
        assert got.n == want[1] and np.array_equal(got.labels, want[0]) and np.array_equal(got.table, want[2])


# ------------------------------------------------------------------ 8. map layer
NAMES = ["chair", "table", "floor"]


@functools.lru_cache(maxsize=None)
def synthetic_map():
    """voxels of a 40 x 40 x 12 scene at (20, 30, 0) of a 100-cell map: a floor, a table, two chairs of 60 and 75 voxels, one of them
    under a shelf of the same category that is not connected to it, and a chair fragment of 8 voxels"""
    cat = -np.ones((40, 40, 12), np.int32)
    cat[:, :, 0] = 2
    cat[5:15, 5:12, 4] = 1
    cat[3:7, 20:25, 1:4] = 0                    # 60
    cat[20:25, 20:25, 1:4] = 0                  # 75
    cat[20:25, 20:25, 8:10] = 0                 # 50, above the second chair
    cat[30:32, 5:7, 1:3] = 0                    # 8
    rng = np.random.default_rng(5)
    cells = np.argwhere(cat >= 0)
    cells = cells[rng.permutation(len(cells))]
    c = cat[cells[:, 0], cells[:, 1], cells[:, 2]]
    scores = (rng.integers(0, 64, (len(cells), 3)) / 128).astype(np.float32)
    scores[np.arange(len(cells)), c] += 1
    grid_pos = (cells + np.array([20, 30, 0])).astype(np.int32)
    return grid_pos, np.ascontiguousarray(scores), c


def synthetic_avlmap():
    from avlmaps_amd.map import AVLMap
    grid_pos, scores, _ = synthetic_map()
    cfg = Cfg(map_config=Cfg(map_type="vlmap", grid_size=100, cell_size=0.05,
                             pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                                           base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0])),
              params=Cfg(cs=0.05))
    av = AVLMap(cfg)
    av.vlmap.grid_pos, av.vlmap.scores_mat, av.vlmap.categories = grid_pos.copy(), scores.copy(), list(NAMES)
    return av


def test_get_instances_3d(ops):
    grid_pos, scores, cat = synthetic_map()
    av = synthetic_avlmap()
    vm = av.vlmap
    for name, connectivity in (("chair", 26), ("chair", 6), ("table", 26), ("floor", 18)):
        cid = NAMES.index(name)
        labels, n, table, best = oracle(grid_pos, cat == cid, connectivity, scores[:, cid])
        assert n == {"chair": 4, "table": 1, "floor": 1}[name]
        for min_voxels in (1, 50, 61, 10 ** 6):
            got = vm.get_instances_3d(name, min_voxels=min_voxels, connectivity=connectivity)
            keep = [k for k in range(n) if table[k, 0] >= min_voxels]
            assert [it.label for it in got] == [k + 1 for k in keep]
            for it, k in zip(got, keep):
                assert isinstance(it, ops.Instance3D) and it.count == table[k, 0] and it.bbox == tuple(table[k, 1:7].tolist())
                center = table[k, 7:10] / np.float64(table[k, 0])
                assert it.center == tuple(center.tolist()) and it.cell == (int(np.rint(center[0])), int(np.rint(center[1])))
                assert it.best_voxel == table[k, 11] and it.best_score == float(best[k]) == float(scores[it.best_voxel, cid])
                assert labels[it.best_voxel] == it.label
    assert [it.count for it in vm.get_instances_3d("chair", min_voxels=50)] == [60, 75, 50]
    cached = vm._instances_cache[1]
    vm.get_instances_3d("chair", min_voxels=1)
    assert vm._instances_cache[1] is cached                      # the same category again: the labelling is reused
    vm.get_instances_3d("table")
    assert vm._instances_cache[1] is not cached and cached.labels_dev is None
    bare = synthetic_avlmap().vlmap
    bare.scores_mat = bare.categories = None
    with pytest.raises(Exception, match="init_categories"):
        bare.get_instances_3d("chair")


def test_index_object_instance(ops):
    from avlmaps_amd.utils.visualize_utils import get_heatmap_from_mask_3d
    grid_pos, scores, cat = synthetic_map()
    av = synthetic_avlmap()
    labels, n, table, _ = oracle(grid_pos, cat == 0, 26)
    assert n == 4 and table[:, 0].tolist() == [60, 75, 50, 8]
    for k in (1, 2, 3):
        heat = av.index_object_instance("chair", k, decay_rate=0.1)
        want = get_heatmap_from_mask_3d(grid_pos, labels == k, cell_size=0.05, decay_rate=0.1)
        assert heat.dtype == np.float32 and heat.shape == (len(grid_pos),) and np.array_equal(heat, want)
        assert np.array_equal(heat == 1, labels == k)
    with pytest.raises(IndexError):
        av.index_object_instance("chair", 4)                     # 8 voxels: filtered by min_voxels = 50
    assert np.array_equal(av.index_object_instance("chair", 4, min_voxels=8) == 1, labels == 4)
    for k in (0, 5):
        with pytest.raises(IndexError):
            av.index_object_instance("chair", k, min_voxels=1)
    goal = av.index_goal(extra=[av.index_object_instance("chair", 2)])        # the heat goes into the fused goal as it stands
    assert goal.value == 1 and goal.voxel == np.flatnonzero(labels == 2)[0]
