"""The scene inventory on the GPU (csrc/avl_objects.hip through ops.label_voxel_classes, ops.pick_columns, ops.pool_rows,
VLMap.get_objects and AVLMap.index_scene_object).

Oracle of the labelling: scipy.ndimage.label once per class on the dense array of that class's voxels, all components then sorted
by (first cell, class) and renumbered; of the table: find_objects, np.add.at and NumPy sorts, as in test_instances_gpu.py; of the
pooled rows: the two nested loops of the definition.  Every comparison is np.array_equal: all results are integers, given scores,
or float64 sums whose order of additions is pinned."""
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


# ------------------------------------------------------------------ oracles and inputs
def oracle_labels(pos, classes, connectivity):
    """-> labels (N,) int32, n: SciPy per class, the components sorted by (first cell, class)"""
    pos, classes = np.asarray(pos, np.int64).reshape(-1, 3), np.asarray(classes, np.int64)
    labels = np.zeros(len(pos), np.int32)
    part = classes >= 0
    if not part.any():
        return labels, 0
    lo = pos[part].min(0)
    shape = pos[part].max(0) - lo + 1
    comps = []                                                   # (first cell, class, voxel indices)
    for cls in np.unique(classes[part]):
        idx = np.flatnonzero(classes == cls)
        q = pos[idx] - lo
        dense = np.zeros(shape, np.uint8)
        dense[q[:, 0], q[:, 1], q[:, 2]] = 1
        lab, n = ndimage.label(dense, ndimage.generate_binary_structure(3, RANK[connectivity]))
        lv = lab[q[:, 0], q[:, 1], q[:, 2]]
        order = np.lexsort((q[:, 2], q[:, 1], q[:, 0], lv))
        _, at = np.unique(lv[order], return_index=True)
        for k in range(n):
            comps.append((tuple(q[order[at[k]]].tolist()), int(cls), idx[lv == k + 1]))
    comps.sort(key=lambda c: (c[0], c[1]))
    for k, (_, _, idx) in enumerate(comps):
        labels[idx] = k + 1
    return labels, len(comps)


def oracle_table(pos, labels, n, scores=None):
    """test_instances_gpu.py's table oracle on given labels -> table (n, 12) int64, best_score (n,) float32"""
    pos, labels = np.asarray(pos, np.int64).reshape(-1, 3), np.asarray(labels)
    table = np.zeros((n, COLS), np.int64)
    best_score = np.zeros(n, np.float32)
    if n == 0:
        return table, best_score
    idx = np.flatnonzero(labels > 0)
    p, lv = pos[idx], labels[idx].astype(np.int64)
    np.add.at(table[:, 0], lv - 1, 1)
    for c in range(3):
        table[:, 1 + 2 * c] = np.iinfo(np.int64).max
        table[:, 2 + 2 * c] = np.iinfo(np.int64).min
        np.minimum.at(table[:, 1 + 2 * c], lv - 1, p[:, c])
        np.maximum.at(table[:, 2 + 2 * c], lv - 1, p[:, c])
        np.add.at(table[:, 7 + c], lv - 1, p[:, c])
    order = np.lexsort((idx, p[:, 2], p[:, 1], p[:, 0], lv))                 # by label, then cell, then voxel index
    _, at = np.unique(lv[order], return_index=True)
    table[:, 10] = idx[order[at]]
    table[:, 11] = -1
    if scores is not None:
        s = np.asarray(scores, np.float32)[idx]
        order = np.lexsort((idx, -s.astype(np.float64), lv))                 # by label, then score descending, then voxel index
        _, at = np.unique(lv[order], return_index=True)
        table[:, 11] = idx[order[at]]
        best_score = np.asarray(scores, np.float32)[table[:, 11]]
    return table, best_score


def check(ops, pos, classes, connectivity, scores=None):
    labels, n = oracle_labels(pos, classes, connectivity)
    table, best = oracle_table(pos, labels, n, scores)
    with ops.label_voxel_classes(pos, classes, connectivity=connectivity, scores=scores) as got:
        assert got.n == n, (got.n, n)
        assert got.labels.dtype == np.int32 and np.array_equal(got.labels, labels)
        assert got.table.dtype == np.int64 and got.table.shape == (n, COLS)
        for c in range(COLS):
            assert np.array_equal(got.table[:, c], table[:, c]), f"table column {c}"
        assert got.best_score.dtype == np.float32 and np.array_equal(got.best_score, best)
        assert got.classes_of.dtype == np.int32 and np.array_equal(got.classes_of, np.asarray(classes)[table[:, 10]])
    return labels, n, table


@functools.lru_cache(maxsize=None)
def random_classes(shape, density, ids, seed=0, offset=(0, 0, 0), ignored=True, weights=None):
    """a shuffled voxel list, one voxel per chosen cell of the box: class ids[k] with probability weights[k] (equal ones when None),
    and about as many ignored voxels (class -1 or -5) in other cells"""
    rng = np.random.default_rng(seed)
    dense = rng.random(shape) < density
    cells = np.argwhere(dense)
    classes = rng.choice(np.asarray(ids, np.int32), len(cells), p=weights)
    if ignored:
        free = np.argwhere(~dense)
        free = free[rng.permutation(len(free))[:max(len(cells), 1)]]
        cells = np.concatenate([cells, free])
        classes = np.concatenate([classes, rng.choice(np.array([-1, -5], np.int32), len(free))])
    perm = rng.permutation(len(cells))
    pos, classes = (cells[perm] + np.asarray(offset)).astype(np.int32), classes[perm].astype(np.int32)
    scores = rng.choice(np.array([0, 0.25, 0.5, 1], np.float32), len(pos))
    for a in (pos, classes, scores):
        a.setflags(write=False)
    return pos, classes, scores


# ------------------------------------------------------------------ 1. small random boxes
@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("density", [0.3, 0.6, 0.9])
def test_small_random_boxes(ops, density, connectivity):
    pos, classes, scores = random_classes((9, 7, 5), density, (0, 7, 1000), offset=(-40, 3, -2))
    assert (classes < 0).any() and len(np.unique(classes[classes >= 0])) == 3
    check(ops, pos, classes, connectivity, scores)


# ------------------------------------------------------------------ 2. many waves and workgroups; one class is label_voxels
def test_many_waves_and_workgroups(ops):
    # class 0 fills 30 % of the box, above the percolation threshold of 26-connected sites; the other four 5 % each, far below it
    pos, classes, scores = random_classes((64, 64, 16), 0.5, (0, 1, 2, 3, 4), weights=(0.6, 0.1, 0.1, 0.1, 0.1))
    _, n, table = check(ops, pos, classes, 26, scores)
    assert n >= 2000 and table[:, 0].max() >= 3000, (n, table[:, 0].max())     # the input is what it claims: thousands of objects, one long union chain
    pos, classes, scores = random_classes((64, 64, 16), 0.5, (3,))
    check(ops, pos, classes, 26, scores)
    with ops.label_voxels(pos, classes >= 0, connectivity=26, scores=scores) as one, \
            ops.label_voxel_classes(pos, classes, connectivity=26, scores=scores) as got:
        assert got.n == one.n and got.labels.tobytes() == one.labels.tobytes() and got.table.tobytes() == one.table.tobytes()
        assert got.best_score.tobytes() == one.best_score.tobytes() and (got.classes_of == 3).all()


@functools.lru_cache(maxsize=None)
def shared_cells_and_mask(n_vox):
    """n_vox voxels dealt unevenly among a quarter of the cells of a 9 x 9 x 5 box at (-3, 40, 2), and a random 60 % mask.  A
    quarter of the cells, because a box in which every cell is masked is one component at every connectivity"""
    rng = np.random.default_rng(1)
    cells = np.argwhere(rng.random((9, 9, 5)) < 0.25)
    weight = rng.random(len(cells)) ** 3                         # a few voxels in some cells, dozens in others
    pos = (cells[rng.choice(len(cells), n_vox, p=weight / weight.sum())] + np.array([-3, 40, 2])).astype(np.int32)
    mask = rng.random(n_vox) < 0.6
    for a in (pos, mask):
        a.setflags(write=False)
    return pos, mask


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("n_vox", [1500, 1025 + 1024])           # two and three scan blocks of the compaction
def test_label_voxels_is_label_classes_with_one_class(ops, n_vox, connectivity):
    """avl_label_voxels and avl_label_classes are one labeller (csrc/avl_voxel_label.h) under two policies: a mask is one class,
    whichever id the class has (7 goes through class - smallest class), also where cells hold several voxels"""
    pos, mask = shared_cells_and_mask(n_vox)
    _, per_cell = np.unique(pos, axis=0, return_counts=True)
    assert (per_cell >= 2).sum() >= 50 and (per_cell >= 3).sum() >= 10 and 0.55 < mask.mean() < 0.65
    q = pos[mask] - pos[mask].min(0)
    dense = np.zeros(q.max(0) + 1, np.uint8)
    dense[q[:, 0], q[:, 1], q[:, 2]] = 1
    assert ndimage.label(dense, ndimage.generate_binary_structure(3, 3))[1] >= 2
    with ops.label_voxels(pos, mask, connectivity=connectivity) as one:
        labels, n = one.labels.copy(), one.n
    assert labels.dtype == np.int32 and n >= 2 and labels.max() == n and not labels[~mask].any()
    for cls in (0, 7):
        classes = np.where(mask, cls, -1).astype(np.int32)
        with ops.label_voxel_classes(pos, classes, connectivity=connectivity) as got:
            assert np.array_equal(got.n, n) and got.labels.dtype == np.int32 and np.array_equal(got.labels, labels), cls
    want, want_n = oracle_labels(pos, np.where(mask, 0, -1), connectivity)
    assert n == want_n and np.array_equal(labels, want)


# ------------------------------------------------------------------ 3 .. 7. shapes whose answer is known
def test_two_slabs_face_to_face(ops):
    cells = np.argwhere(np.ones((4, 6, 3), bool))
    classes = (cells[:, 1] >= 3).astype(np.int32) * 5            # columns 0..2: class 0, columns 3..5: class 5
    perm = np.random.default_rng(1).permutation(len(cells))
    for connectivity in (6, 18, 26):
        labels, n, table = check(ops, cells[perm].astype(np.int32), classes[perm], connectivity)
        assert n == 2 and table[:, 0].tolist() == [36, 36]
        assert np.array_equal(labels, 1 + (classes[perm] == 5))


def test_checkerboard_of_two_classes(ops):
    cells = np.argwhere(np.ones((6, 5, 4), bool))
    classes = (cells.sum(1) % 2).astype(np.int32)
    perm = np.random.default_rng(2).permutation(len(cells))
    pos, classes = cells[perm].astype(np.int32), classes[perm]
    assert check(ops, pos, classes, 6)[1] == len(cells)          # no face neighbour has the voxel's class
    assert check(ops, pos, classes, 18)[1] == 2                  # edge neighbours differ on two axes: the same parity
    assert check(ops, pos, classes, 26)[1] == 2


def test_voxels_that_share_a_cell(ops):
    pos = np.array([[4, 4, 4], [4, 4, 4]], np.int32)
    with ops.label_voxel_classes(pos, np.array([3, 3], np.int32)) as got:
        assert got.n == 1 and got.labels.tolist() == [1, 1] and got.table[0, 0] == 2 and got.classes_of.tolist() == [3]
    with ops.label_voxel_classes(pos, np.array([9, 3], np.int32)) as got:         # numbered by class, not by voxel index
        assert got.n == 2 and got.labels.tolist() == [2, 1] and got.classes_of.tolist() == [3, 9]
    # runs of several ranks in a cell and in its neighbours: every rank of the class is found, whatever lies between
    pos = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 1], [0, 1, 0], [0, 1, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1], [5, 5, 5]], np.int32)
    classes = np.array([2, 1, 2, 1, 0, 0, 2, 0, -1, 1, 1], np.int32)
    for connectivity in (6, 18, 26):
        check(ops, pos, classes, connectivity, scores=np.arange(len(pos), dtype=np.float32))
    labels, n, _ = check(ops, pos, classes, 26)
    assert n == 4 and labels.tolist() == [2, 1, 2, 1, 3, 3, 2, 3, 0, 1, 4]


def test_first_cells_that_interleave_in_raster_order(ops):
    """class 1 begins at (0, 0, 0), class 0 at (0, 0, 2), class 1 again at (0, 2, 0), class 0 again at (0, 2, 2): numbering by first
    cell interleaves the classes, numbering class by class would not"""
    pos = np.array([[0, 0, 0], [0, 0, 2], [0, 2, 0], [0, 2, 2], [1, 2, 0], [1, 0, 2]], np.int32)
    classes = np.array([1, 0, 1, 0, 1, 0], np.int32)
    labels, n, _ = check(ops, pos, classes, 6)
    assert n == 4 and labels.tolist() == [1, 2, 3, 4, 3, 2]
    pos, classes, _ = random_classes((5, 5, 5), 0.5, (0, 1), seed=3)
    _, n, table = check(ops, pos, classes, 6)
    owner = classes[table[:, 10]]
    assert n > 4 and (np.diff(owner) != 0).sum() > 2             # the classes alternate along the numbering


# ------------------------------------------------------------------ 8. nothing takes part
def test_no_voxels_and_no_participating_voxel(ops):
    with ops.label_voxel_classes(np.zeros((0, 3), np.int32), np.zeros((0,), np.int32)) as got:
        assert got.n == 0 and got.labels.shape == (0,) and got.table.shape == (0, COLS) and got.best_score.shape == (0,)
        assert got.classes_of.shape == (0,)
    pos, classes, _ = random_classes((9, 7, 5), 0.3, (0, 7, 1000))
    with ops.label_voxel_classes(pos, np.full(len(pos), -1, np.int32)) as got:
        assert got.n == 0 and got.labels.dtype == np.int32 and not got.labels.any() and got.labels.shape == (len(pos),)
        assert got.table.shape == (0, COLS) and got.classes_of.shape == (0,)


# ------------------------------------------------------------------ 9. the second round of the block-count scan
def test_labels_over_two_rounds_of_the_offsets_scan(ops):
    """1024 * 1024 + 1 voxels are 1025 scan blocks of 1024, one more than the one-workgroup scan of the block counts has threads"""
    rng = np.random.default_rng(6)
    n_vox = 1024 * 1024 + 1
    cells = np.argwhere(np.ones((1025, 1024, 1), bool))[rng.permutation(1025 * 1024)[:n_vox]].astype(np.int32)
    classes = rng.choice(np.array([-1, -1, -1, 0, 1], np.int32), n_vox)            # 20 % each of two classes
    classes[-1] = 1                                             # the voxel whose place comes from the carried total
    labels, n = oracle_labels(cells, classes, 26)
    assert n > 1024
    with ops.label_voxel_classes(cells, classes, connectivity=26) as got:
        assert got.n == n, (got.n, n)
        assert got.labels.dtype == np.int32 and np.array_equal(got.labels, labels)


def test_the_largest_box_and_one_cell_more(ops):
    from avlmaps_amd._lib import AvlError
    side = ops.INSTANCES_MAX_BOX_SIDE
    pos = np.zeros((3, 3), np.int32)
    pos[1, 0] = side
    pos[2, 0] = -(1 << 30)                                       # an ignored voxel does not count
    with pytest.raises(AvlError, match="bounding box"):
        ops.label_voxel_classes(pos, np.array([0, 1, -1], np.int32))
    pos[1, 0] = side - 1
    assert check(ops, pos, np.array([0, 1, -1], np.int32), 26)[1] == 2


# ------------------------------------------------------------------ 10. the column pick
@pytest.mark.parametrize("C", [1, 63, 64, 65])
def test_pick_columns(ops, C):
    rng = np.random.default_rng(C)
    N = 1000
    wide = rng.standard_normal((N, C + 3)).astype(np.float32)
    cols = rng.integers(0, C, N).astype(np.int32)
    cols[::7], cols[3::11] = -1, C                               # outside 0 .. C - 1 on both sides
    inside = (cols >= 0) & (cols < C)
    for rows in (np.ascontiguousarray(wide[:, :C]), wide[:, :C]):  # contiguous, and a view with ld = C + 3 > C
        want = np.where(inside, np.take_along_axis(rows, np.clip(cols, 0, C - 1)[:, None].astype(np.int64), axis=1)[:, 0], np.float32(0))
        got = ops.pick_columns(rows, cols)
        assert got.dtype == np.float32 and got.shape == (N,) and np.array_equal(got, want)
    from avlmaps_amd.device import DeviceArray
    got = ops.pick_columns(DeviceArray.from_numpy(np.ascontiguousarray(wide[:, :C])), DeviceArray.from_numpy(cols), device=True)
    assert isinstance(got, DeviceArray) and np.array_equal(got.numpy(), want)
    assert ops.pick_columns(np.zeros((0, C), np.float32), np.zeros(0, np.int32)).shape == (0,)


# ------------------------------------------------------------------ 11. the pooled rows
def pool_oracle(rows, labels, n, chunk):
    """the definition: two nested loops of sequential float64 additions"""
    sums = np.zeros((n, rows.shape[1]), np.float64)
    for k in range(1, n + 1):
        members = np.flatnonzero(labels == k)                    # ascending voxel index
        total = np.zeros(rows.shape[1], np.float64)
        for c0 in range(0, len(members), chunk):
            partial = np.zeros(rows.shape[1], np.float64)
            for i in members[c0:c0 + chunk]:
                partial = partial + rows[i].astype(np.float64)
            total = total + partial
        sums[k - 1] = total
    return sums


@functools.lru_cache(maxsize=None)
def pool_labels():
    """objects 1 .. 5 of 1, 255, 256, 257 and 256 * 65 + 1 members, object 6 without a member (n = 6), 50 voxels each of label 0,
    7 = n + 1 and -3; shuffled, N not a multiple of 64"""
    sizes = [1, 255, 256, 257, 256 * 65 + 1]
    labels = np.concatenate([np.full(s, k + 1, np.int32) for k, s in enumerate(sizes)] + [np.full(50, v, np.int32) for v in (0, 7, -3)])
    labels = labels[np.random.default_rng(7).permutation(len(labels))]
    assert len(labels) % 64 != 0
    labels.setflags(write=False)
    return labels, 6


@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_pool_rows(ops, C):
    labels, n = pool_labels()
    rng = np.random.default_rng(100 + C)
    N = len(labels)
    # magnitudes 1e-12 .. 1: another order of the additions rounds differently
    rows = (rng.random((N, C)) * 10.0 ** rng.integers(-12, 1, (N, C))).astype(np.float32)
    want = pool_oracle(rows, labels, n, ops.POOL_CHUNK)
    assert not np.array_equal(want, pool_oracle(rows, labels, n, 64)[:, :C])      # the chunk length is part of the definition
    got = ops.pool_rows(rows, labels, n)
    assert got.dtype == np.float64 and got.shape == (n, C) and np.array_equal(got, want)
    assert not got[5].any() and got[:5].all()                    # the object without a member: zeros
    assert ops.pool_rows(rows, labels, n).tobytes() == got.tobytes()
    wide = np.concatenate([rows, np.ones((N, 2), np.float32)], axis=1)
    assert np.array_equal(ops.pool_rows(wide[:, :C], labels, n), want)             # a view with ld = C + 2
    assert np.array_equal(ops.pool_rows(rows, labels, 3), want[:3])               # labels 4 .. 7 are now outside 1 .. n
    assert ops.pool_rows(rows, labels, 0).shape == (0, C)
    assert not ops.pool_rows(np.zeros((0, C), np.float32), np.zeros(0, np.int32), 2).any()


def test_pool_rows_device_inputs(ops):
    from avlmaps_amd.device import DeviceArray
    labels, n = pool_labels()
    rows = np.random.default_rng(8).random((len(labels), 5)).astype(np.float32)
    got = ops.pool_rows(DeviceArray.from_numpy(rows), DeviceArray.from_numpy(labels), n, device=True)
    assert isinstance(got, DeviceArray) and got.shape == (n, 5) and np.array_equal(got.numpy(), pool_oracle(rows, labels, n, ops.POOL_CHUNK))


# ------------------------------------------------------------------ 12. map layer
NAMES = ["chair", "table", "floor"]


@functools.lru_cache(maxsize=None)
def synthetic_map():
    """test_instances_gpu.py's scene: voxels of a 40 x 40 x 12 scene at (20, 30, 0) of a 100-cell map: a floor, a table, two chairs of
    60 and 75 voxels, a shelf of the chair category above the second one, a chair fragment of 8 voxels -- and three voxels on the
    first chair's seat whose row maximum says "table" while the chair's mean does not"""
    cat = -np.ones((40, 40, 12), np.int32)
    cat[:, :, 0] = 2
    cat[5:15, 5:12, 4] = 1
    cat[3:7, 20:25, 1:4] = 0                    # 60
    cat[20:25, 20:25, 1:4] = 0                  # 75
    cat[20:25, 20:25, 8:10] = 0                 # 50, above the second chair
    cat[30:32, 5:7, 1:3] = 0                    # 8
    cat[4, 21:24, 4] = 1                        # 3 "table" voxels on the first chair
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


def test_get_objects(ops):
    from avlmaps_amd.map.scene_objects import SceneObjects, objects_from_json
    grid_pos, scores, cat = synthetic_map()
    av = synthetic_avlmap()
    vm = av.vlmap
    for connectivity in (26, 6):
        scene = vm.get_objects(min_voxels=0, connectivity=connectivity, exclude=())
        assert isinstance(scene, SceneObjects) and scene.names == NAMES
        labels, n = oracle_labels(grid_pos, cat, connectivity)
        assert scene.n == n == len(scene.objects) and np.array_equal(scene.voxel_objects.labels.numpy(), labels)
        for cid, name in enumerate(NAMES):                       # per category: get_instances_3d's objects, in order
            mine = [it for it in scene.objects if it.category == cid]
            want = vm.get_instances_3d(name, min_voxels=0, connectivity=connectivity)
            assert len(mine) == len(want) > 0 and all(it.name == name for it in mine)
            for it, w in zip(mine, want):
                assert it[1:7] == w[1:7]                         # count, bbox, center, best_voxel, best_score, cell; the labels differ
        # mean_scores, voted and margin against NumPy on scores_mat and the labels
        sums = pool_oracle(scores, labels, n, ops.POOL_CHUNK)
        mean = sums / np.bincount(labels, minlength=n + 1)[1:, None].astype(np.float64)
        assert np.array_equal(scene.mean_scores, mean)
        top = np.sort(mean, axis=1)
        assert np.array_equal(scene.voted, np.argmax(mean, axis=1)) and np.array_equal(scene.margin, top[:, -1] - top[:, -2])
        for it in scene.objects:
            k = it.label - 1
            assert (it.voted, it.voted_name, it.margin, it.mean_score) == (scene.voted[k], NAMES[scene.voted[k]], scene.margin[k], mean[k, it.category])
    # the three "table" voxels on the chair are an object of their own that still votes "table"; vote_labels follows the listing
    scene = vm.get_objects(min_voxels=0, exclude=())
    seat = [it for it in scene.objects if it.category == 1 and it.count == 3]
    assert len(seat) == 1 and seat[0].voted == 1
    assert np.array_equal(scene.vote_labels(), cat) and scene.vote_labels().dtype == np.int32
    # the JSON round-trips
    assert objects_from_json(scene.to_json()) == scene.objects
    # min_voxels filters but keeps the labels, and reuses the labelling
    vo = scene.voxel_objects
    big = vm.get_objects(min_voxels=50, exclude=())
    assert big.voxel_objects is vo and [it for it in scene.objects if it.count >= 50] == big.objects
    assert 0 < len(big.objects) < scene.n and [it.count for it in big.objects if it.category == 0] == [60, 75, 50]
    assert vm.get_objects(min_voxels=50, exclude=()) is big
    # exclude removes a category's objects; the others keep their voxels, with new numbers
    nofloor = vm.get_objects(min_voxels=0, exclude=("floor",))
    assert nofloor.voxel_objects is not vo and vo.labels_dev is None
    want_labels, want_n = oracle_labels(grid_pos, np.where(cat == 2, -1, cat), 26)
    assert nofloor.n == want_n == scene.n - 1 and np.array_equal(nofloor.voxel_objects.labels.numpy(), want_labels)
    assert all(it.name != "floor" for it in nofloor.objects) and {it.name for it in nofloor.objects} == {"chair", "table"}
    assert vm.get_objects(min_voxels=0).n == scene.n             # the default excludes "other", which this map does not have
    bare = synthetic_avlmap().vlmap
    bare.scores_mat = bare.categories = None
    with pytest.raises(Exception, match="init_categories"):
        bare.get_objects()


def test_index_scene_object(ops):
    grid_pos, scores, cat = synthetic_map()
    av = synthetic_avlmap()
    scene = av.vlmap.get_objects(min_voxels=50)
    chairs = [it for it in scene.objects if it.name == "chair"]
    assert [it.count for it in chairs] == [60, 75, 50]
    for k, it in enumerate(chairs, start=1):
        heat = av.index_scene_object(it.label, decay_rate=0.1)
        want = av.index_object_instance("chair", k, decay_rate=0.1)
        assert heat.dtype == np.float32 and heat.shape == (len(grid_pos),) and heat.tobytes() == want.tobytes()
    small = [k + 1 for k in range(scene.n) if scene.voxel_objects.table[k, 0] < 50]
    with pytest.raises(IndexError):
        av.index_scene_object(small[0])                          # fewer than min_voxels = 50
    assert (av.index_scene_object(small[0], min_voxels=1) == 1).sum() == scene.voxel_objects.table[small[0] - 1, 0]
    for label in (0, scene.n + 1):
        with pytest.raises(IndexError):
            av.index_scene_object(label, min_voxels=1)
    goal = av.index_goal(extra=[av.index_scene_object(chairs[1].label)])      # the heat goes into the fused goal as it stands
    assert goal.value == 1 and cat[goal.voxel] == 0


# ------------------------------------------------------------------ 13. the app
def test_index_map_inventory_flags_on_a_disk_dataset(tmp_path, capsys):
    """apps.index_map --inventory / --inventory-json on a synthetic scene in the on-disk layout: the printed objects are those of
    the JSON, they partition the voxels that are not "other" (min_voxels = 1), and the query's own output is unchanged"""
    import re
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map, index_map
    from avlmaps_amd.map.scene_objects import objects_from_json
    scene = make(tmp_path / "scene", frames=6, H=96, W=128)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                  "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(scene), "--config", str(cfg), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    base = ["--data-dir", str(scene), "--config", str(cfg), "--query", "sofa", "--text-model", "hash", "--categories", "sofa,table,chair"]
    plain = index_map.main(base)
    capsys.readouterr()
    path = tmp_path / "objects.json"
    heat = index_map.main(base + ["--inventory", "--inventory-json", str(path), "--min-voxels", "1", "--connectivity", "6"])
    out = capsys.readouterr().out
    assert np.array_equal(heat, plain)                           # the inventory does not touch the query's heat
    objects = objects_from_json(path.read_text())
    lines = re.findall(r"object (\d+): '(\w+)'(?: \(voted '\w+'\))?, (\d+) voxels", out)
    assert len(lines) == len(objects) > 0 and f"{len(objects)} objects of at least 1 voxels" in out and f"wrote {path}" in out
    assert [(int(a), b, int(c)) for a, b, c in lines] == [(it.label, it.name, it.count) for it in objects]
    assert [it.label for it in objects] == list(range(1, len(objects) + 1)) and {it.name for it in objects} <= {"sofa", "table", "chair"}
    assert sum(it.count for it in objects if it.name == "sofa") == int((heat == 1.0).sum())      # the sofas' voxels are the query's mask
