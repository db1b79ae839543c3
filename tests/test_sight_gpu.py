"""GPU tests of the cell-to-cell line of sight (csrc/avl_sight.hip): ops.line_of_sight and ops.visible_counts against the scalar
restatement of tests/_sight_ref.py with np.array_equal -- no tolerance, no pair left out -- and Map.get_viewpoints /
get_viewpoint_pos / apps.plan_path --view end to end.  Every scene asserts, through the restatement's own bookkeeping, that it
contains the cases it is there for."""
import functools
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent / "tools"))

import _sight_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

GS, VH = 48, 8


# ------------------------------------------------------------------ the scene
@functools.lru_cache(maxsize=None)
def scene():
    """(grid_pos (N, 3) int32, transparent (N,) uint8): a full-height wall along row 20 with a door gap at columns 22 .. 24, a second
    full-height wall along row 30 (columns 0 .. 15), a half-height partition along row 10, a table top (occupied at h = 3, free
    below), a lone voxel for the asymmetric pair, a few rows outside the grid and, last, a second row in the cell (20, 5, 2)"""
    wall = [(20, c, h) for c in range(GS) if not 22 <= c <= 24 for h in range(VH)]
    second = [(30, c, h) for c in range(16) for h in range(VH)]
    partition = [(10, c, h) for c in range(5, 31) for h in range(4)]
    table = [(r, c, 3) for r in range(34, 38) for c in range(30, 36)]
    lone = [(41, 41, 6)]
    outside = [(-1, 5, 5), (GS, 0, 0), (5, 5, VH), (5, -3, 1), (2 ** 31 - 1, 0, 0), (0, 0, -2 ** 31)]
    pos = np.array(wall + second + partition + table + lone + outside + [(20, 5, 2)], np.int64).astype(np.int32)
    transparent = np.zeros(len(pos), np.uint8)
    transparent[len(wall):len(wall) + len(second)] = 1                       # the second wall can be switched off ...
    transparent[len(wall) + len(second) + len(partition):len(wall) + len(second) + len(partition) + len(table)] = 255      # ... and the table
    assert 550 <= len(pos) <= 700
    return pos, transparent


def pairs():
    """(eyes, targets) (M, 3) int32 each: the named cases first, then random pairs of the whole grid"""
    rng = np.random.default_rng(5)
    e, t = [], []

    def add(a, b):
        e.append(a)
        t.append(b)
    add((0, 0, 0), (0, 0, 0))                                               # 0: n = 0 ...
    add((20, 7, 1), (20, 7, 1))                                             # 1: ... in an occupied cell
    add((19, 7, 1), (20, 7, 1))                                             # 2: n = 1, onto a voxel
    add((20, 7, 1), (21, 8, 2))                                             # 3: n = 1, from a voxel
    add((35, 5, 2), (5, 5, 2))                                              # 4: two walls in a row, the second wall first ...
    add((5, 5, 5), (35, 5, 5))                                              # 5: ... and from the other side the first (above the partition)
    add((25, 5, 2), (15, 5, 2))                                             # 6: through the cell two rows share
    add((20, 7, 1), (25, 7, 1))                                             # 7: the eye inside the wall, looking out
    add((40, 41, 6), (42, 42, 6))                                           # 8: the asymmetric pair: passes the lone voxel ...
    add((42, 42, 6), (40, 41, 6))                                           # 9: ... and back: passes (41, 42, 6)
    add((25, 23, 4), (15, 23, 4))                                           # 10: through the door
    add((12, 10, 6), (8, 10, 6))                                            # 11: over the partition
    add((12, 10, 2), (8, 10, 2))                                            # 12: into it
    add((36, 28, 1), (36, 38, 1))                                           # 13: under the table
    add((36, 28, 3), (36, 38, 3))                                           # 14: through its top
    add((36, 32, 0), (36, 32, 7))                                           # 15: straight up through it
    add((21, 3, 2), (29, 3, 2))                                             # 16: between the two walls: both ends next to a voxel
    add((17, 9, 2), (24, 9, 2))                                             # 17 - 19: the wall 3, 2, 1 cells before the target: end_margin 3 decides
    add((17, 9, 2), (22, 9, 2))
    add((17, 9, 2), (21, 9, 2))
    centre = (24, 26, 4)
    for drive in range(3):                                                  # all 8 octants under each of the three driving axes
        for sign in itertools.product((1, -1), repeat=3):
            d = [1, 2]
            d.insert(drive, 3)
            add(centre, tuple(centre[k] + sign[k] * d[k] for k in range(3)))
    for axis in range(3):                                                   # axis-aligned, both ways
        for s in (1, -1):
            add(centre, tuple(centre[k] + (s * 3 if k == axis else 0) for k in range(3)))
    for d in ((3, 3, 0), (3, -3, 0), (0, 3, 3), (-3, 0, 3), (3, 3, 3), (-3, 3, -3), (17, 17, 0), (-20, 20, 0)):       # exact diagonals
        add(centre, tuple(centre[k] + d[k] for k in range(3)))
    for k, lim in enumerate((GS, GS, VH)):                                  # either end outside on each axis and side
        for v in (-1, lim, -2 ** 31, 2 ** 31 - 1):
            bad = list(centre)
            bad[k] = v
            add(tuple(bad), centre)
            add(centre, tuple(bad))
    add((-1, -1, -1), (GS, GS, VH))
    n = len(e)
    eyes = np.concatenate([np.array(e, np.int64), rng.integers(0, (GS, GS, VH), (1400, 3))]).astype(np.int32)
    targets = np.concatenate([np.array(t, np.int64), rng.integers(0, (GS, GS, VH), (1400, 3))]).astype(np.int32)
    return eyes, targets, n


@functools.lru_cache(maxsize=None)
def pair_ref(with_transparent, end_margin):
    pos, tr = scene()
    eyes, targets, _ = pairs()
    stats = {}
    return S.los_ref(pos, GS, VH, eyes, targets, tr if with_transparent else None, end_margin, stats), stats


def test_the_scene_contains_its_cases():
    pos, tr = scene()
    want, st = pair_ref(False, 0)
    N = len(pos)
    assert len(st["octants"]) == 24 and st["axis_aligned"] == {0, 1, 2} and st["diagonal"] >= 8 and st["point"] >= 2
    assert len(st["invalid_kinds"]) == 12 and st["invalid"] >= 25 and st["eye_occupied"] >= 2 and st["nothing_tested"] >= 4
    assert st["blocked"] > 300 and st["visible"] > 300 and st["second_blocker_behind"] >= 1 and st["blocked_by_shared_cell"] >= 1
    assert st["target_occupied"] >= 1
    assert want[:4].tolist() == [-1, -1, -1, -1]
    assert tuple(pos[want[4]]) == (30, 5, 2) and tuple(pos[want[5]]) == (20, 5, 5)          # the nearer wall's voxel either way
    assert want[6] == N - 1 and tuple(pos[N - 1]) == (20, 5, 2)                              # the larger of the two rows
    assert want[7] == -1                                                                     # the eye's own cell does not block
    assert tuple(pos[want[8]]) == (41, 41, 6) and want[9] == -1                              # eye -> target, not target -> eye
    assert want[10] == want[11] == want[13] == -1 and tuple(pos[want[12]]) == (10, 10, 2)
    assert tuple(pos[want[14]]) == (36, 30, 3) and tuple(pos[want[15]]) == (36, 32, 3) and want[16] == -1
    assert all(tuple(pos[i]) == (20, 9, 2) for i in want[17:20])
    assert pair_ref(False, 1)[0][17:20].tolist() == [want[17], want[17], -1]
    assert pair_ref(False, 3)[0][17:20].tolist() == [want[17], -1, -1] and pair_ref(False, 3)[1]["occupied_inside_margin"] >= 1
    assert (pair_ref(False, 100)[0] >= 0).sum() == 0 and pair_ref(False, 100)[1]["invalid"] == st["invalid"]
    wt, stt = pair_ref(True, 0)
    assert tuple(pos[wt[4]]) == (20, 5, 2) and wt[14] == wt[15] == -1                        # the second wall off: the first shows; the table off
    assert stt["blocked_behind_transparent"] >= 1 and stt["visible_through_transparent"] >= 1 and not np.array_equal(wt, want)


@pytest.mark.parametrize("end_margin", [0, 1, 3, 100])
@pytest.mark.parametrize("with_transparent", [False, True])
def test_line_of_sight_equals_the_restatement(with_transparent, end_margin):
    from avlmaps_amd import ops
    pos, tr = scene()
    eyes, targets, _ = pairs()
    want, _ = pair_ref(with_transparent, end_margin)
    with ops.cell_index(pos, GS, VH) as index:
        got = ops.line_of_sight(index, eyes, targets, tr if with_transparent else None, end_margin)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
        if with_transparent:                                                # bool: non-zero is transparent, as the bytes are
            assert np.array_equal(ops.line_of_sight(index, eyes, targets, tr != 0, end_margin), want)


def test_line_of_sight_sizes_and_inputs():
    import torch
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    pos, tr = scene()
    eyes, targets, _ = pairs()
    want, _ = pair_ref(True, 1)
    with ops.cell_index(pos, GS, VH) as index:
        for M in (0, 1, 255, 256, 257):
            got = ops.line_of_sight(index, eyes[:M], targets[:M], tr, 1)
            assert got.shape == (M,) and np.array_equal(got, want[:M]), M
        dev = ops.line_of_sight(index, DeviceArray.from_numpy(eyes), DeviceArray.from_numpy(targets), DeviceArray.from_numpy(tr), 1, device=True)
        assert isinstance(dev, DeviceArray) and np.array_equal(dev.numpy(), want)
        got = ops.line_of_sight(index, torch.from_numpy(eyes).cuda(), torch.from_numpy(targets).cuda(), torch.from_numpy(tr != 0).cuda(), 1)
        assert np.array_equal(got, want)
        assert np.array_equal(ops.line_of_sight(index, eyes.astype(np.int64).tolist(), targets.astype(np.int64), tr, 1), want)
        with pytest.raises(TypeError):
            ops.line_of_sight(index, DeviceArray.from_numpy(eyes.astype(np.int64)), targets)
    with ops.cell_index(np.zeros((0, 3), np.int32), GS, VH) as empty:      # a map without voxels hides nothing
        got = ops.line_of_sight(empty, eyes, targets, np.zeros(0, np.uint8))
        assert np.array_equal(got, np.where(want == -2, -2, -1))
    with pytest.raises(ValueError):
        ops.line_of_sight(empty, eyes, targets)                             # closed


# ------------------------------------------------------------------ counts
@functools.lru_cache(maxsize=None)
def count_cells():
    """(eyes (257, 3), targets (1025, 3)): eyes all over the grid at every height, one of them outside; targets: the table, parts of
    the partition and of the walls, free cells, and two cells outside the grid"""
    rng = np.random.default_rng(9)
    pos, _ = scene()
    eyes = rng.integers(0, (GS, GS, VH), (257, 3))
    eyes[2] = (24, GS, 3)                                                   # outside, among the first three
    eyes[0] = (36, 27, 2)                                                   # next to the table, below its top
    inside = pos[(pos >= 0).all(axis=1) & (pos < (GS, GS, VH)).all(axis=1)]
    targets = rng.permutation(np.concatenate([inside[rng.permutation(len(inside))[:500]], rng.integers(0, (GS, GS, VH), (525, 3))]))
    targets[1] = (36, 31, 3)                                                # a voxel of the table, near eyes[0]
    targets[7] = (5, 5, VH)                                                 # outside, among the first 63
    targets[40] = (-1, 0, 0)
    assert len(targets) == 1025
    return eyes.astype(np.int32), targets.astype(np.int32)


@pytest.mark.parametrize("E,T", [(5, 0), (5, 1), (5, 63), (5, 64), (5, 65), (5, 1025), (0, 65), (1, 65), (3, 65), (4, 65), (257, 65)])
def test_visible_counts_equals_the_restatement(E, T):
    from avlmaps_amd import ops
    pos, tr = scene()
    eyes, targets = count_cells()
    eyes, targets = eyes[:E], targets[:T]
    stats = {}
    want_v, want_f = S.counts_ref(pos, GS, VH, eyes, targets, tr, 1, -1, stats)
    if E >= 3:
        assert stats["eye_outside"] == 1 and want_v[2] == 0 and want_f[2] == -1
    if E >= 3 and T >= 63:
        assert stats["target_outside"] >= 1 and stats["blocked"] >= 1 and stats["visible"] >= 1 and (want_v > 0).any()
        assert (want_f > 0).any()                                           # a first target that is not simply target 0
    with ops.cell_index(pos, GS, VH) as index:
        got_v, got_f = ops.visible_counts(index, eyes, targets, tr, end_margin=1)
        assert got_v.dtype == np.uint32 and got_f.dtype == np.int32 and got_v.shape == got_f.shape == (E,)
        assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)
        only_v, none = ops.visible_counts(index, eyes, targets, tr, end_margin=1, want_first=False)
        assert none is None and np.array_equal(only_v, want_v)
    if T == 0:
        assert (want_v == 0).all() and (want_f == -1).all()


def test_visible_counts_range_inputs_and_the_sum_over_pairs():
    import torch
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    pos, tr = scene()
    eyes, targets = count_cells()
    eyes, targets = eyes[:5], targets[:200]
    d2 = ((targets[1].astype(np.int64) - eyes[0]) ** 2).sum()
    assert d2 == 17                                                         # (36, 27, 2) -> (36, 31, 3): 16 + 1
    with ops.cell_index(pos, GS, VH) as index:
        seen = {}
        for max_range, r2 in ((None, -1), (np.sqrt(17.0) - 1e-9, 16), (np.sqrt(17.0), 17), (np.sqrt(17.0) + 1e-9, 17), (4.5, 20), (0.0, 0), (0.5, 0),
                              (1.0, 1), (20, 400), (1e6, 10 ** 12), (3.0e9, 9 * 10 ** 18)):
            stats = {}
            want_v, want_f = S.counts_ref(pos, GS, VH, eyes, targets, tr, 0, r2, stats)
            got_v, got_f = ops.visible_counts(index, eyes, targets, tr, max_range=max_range)
            assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f), max_range
            seen[r2] = (want_v, want_f, stats)
        # the table's voxel is seen from below once it is in range: the bound below, at and above its squared distance
        assert seen[16][1][0] != 1 and seen[17][1][0] == 1 and seen[17][0][0] == seen[16][0][0] + seen[17][2]["at_range"] > seen[16][0][0]
        assert "at_range" in seen[17][2] and seen[16][2]["beyond_range"] > seen[20][2]["beyond_range"] > 0
        assert np.array_equal(seen[10 ** 12][0], seen[-1][0]) and np.array_equal(seen[9 * 10 ** 18][0], seen[-1][0])
        want_v, want_f, _ = seen[20]
        # the count is the sum of line_of_sight over the pairs in range
        ee, tt = np.repeat(eyes, len(targets), axis=0), np.tile(targets, (len(eyes), 1))
        blocker = ops.line_of_sight(index, ee, tt, tr).reshape(len(eyes), len(targets))
        in_range = ((ee.astype(np.int64) - tt) ** 2).sum(axis=1).reshape(blocker.shape) <= 20
        sees = (blocker == ops.LOS_VISIBLE) & in_range
        assert np.array_equal(sees.sum(axis=1).astype(np.uint32), want_v)
        assert np.array_equal(np.where(sees.any(axis=1), sees.argmax(axis=1), -1).astype(np.int32), want_f)
        # device-resident inputs and results
        dv, df = ops.visible_counts(index, DeviceArray.from_numpy(eyes), DeviceArray.from_numpy(targets), DeviceArray.from_numpy(tr),
                                    max_range=4.5, device=True)
        assert isinstance(dv, DeviceArray) and isinstance(df, DeviceArray) and dv.dtype == np.uint32 and df.dtype == np.int32
        assert np.array_equal(dv.numpy(), want_v) and np.array_equal(df.numpy(), want_f)
        dv, df = ops.visible_counts(index, eyes, targets, tr, max_range=4.5, want_first=False, device=True)
        assert df is None and np.array_equal(dv.numpy(), want_v)
        tv, tf = ops.visible_counts(index, torch.from_numpy(eyes).cuda(), torch.from_numpy(targets).cuda(), torch.from_numpy(tr).cuda(),
                                    max_range=4.5)
        assert np.array_equal(tv, want_v) and np.array_equal(tf, want_f)
        # without `transparent` the table hides its own voxels from below
        nv, nf = ops.visible_counts(index, eyes, targets, max_range=4.5)
        rv, rf = S.counts_ref(pos, GS, VH, eyes, targets, None, 0, 20)
        assert np.array_equal(nv, rv) and np.array_equal(nf, rf) and not np.array_equal(rv, want_v)


# ------------------------------------------------------------------ the map layer
RS, RVH, RCS = 40, 8, 0.1
EYE = 0.55                                                                  # metres: height cell 5


def room():
    """A VLMap of a 30 x 30-cell room (walls on rows and columns 5 and 34, full height) with, from north to south: a cross wall W1 along
    row 14 with a door at columns 20 .. 22; a half-height partition along row 19 (columns 7 .. 16, h 0 .. 3); a free-standing
    full-height wall W2 along row 24 (columns 5 .. 26: the way round is at its east end) with a picture on its NORTH face (row 23,
    columns 10 .. 13, h 4 .. 6).  get_pos returns the picture's island as mask_foreground's dilation would leave it, a ring two
    cells out, without the cells inside W2."""
    from avlmaps_amd.apps.common import load_config
    from avlmaps_amd.map import VLMap

    class Room(VLMap):
        def get_pos(self, name):
            ring = [(21, c) for c in range(8, 16)] + [(r, 15) for r in (22, 23)] + [(25, c) for c in range(15, 7, -1)] + [(r, 8) for r in (23, 22)]
            if name != "picture":
                return [], [], []
            return [np.array(ring, np.int64)], [[23.0, 11.5]], [[21, 25, 8, 15]]

    cfg = load_config(overrides={"map_config.grid_size": RS, "map_config.cell_size": RCS}).map_config
    vm = Room(cfg)
    cols = lambda c0, c1, r, hs: [(r, c, h) for c in range(c0, c1 + 1) for h in hs]          # noqa: E731
    full = range(RVH)
    outline = cols(5, 34, 5, full) + cols(5, 34, 34, full) + [(r, c, h) for r in range(6, 34) for c in (5, 34) for h in full]
    w1 = [x for x in cols(6, 33, 14, full) if not 20 <= x[1] <= 22]
    part = cols(7, 16, 19, range(4))
    w2 = cols(6, 26, 24, full)
    picture = cols(10, 13, 23, (4, 5, 6))
    vm.grid_pos = np.array(outline + w1 + part + w2 + picture, np.int32)
    n = len(vm.grid_pos)
    vm.occupied_ids = -np.ones((RS, RS, RVH), np.int32)
    vm.occupied_ids[tuple(vm.grid_pos.T)] = np.arange(n)
    mask = np.zeros(n, bool)
    mask[n - len(picture):] = True
    vm.generate_obstacle_map()
    assert (vm.rmin, vm.rmax, vm.cmin, vm.cmax) == (5, 34, 5, 34)
    return vm, mask


def test_viewpoints_of_a_picture_behind_a_wall():
    from avlmaps_amd import ops
    from avlmaps_amd.navigator import Navigator
    vm, mask = room()
    vp = vm.get_viewpoints(mask, eye_height=EYE, max_range=2.5)
    free = np.argwhere(np.asarray(vm.get_obstacle_cropped()) != 0) + (5, 5)
    assert np.array_equal(vp.cells, free) and vp.n_targets == 12 and vp.eye_h == 5         # the window of 25 cells holds the whole room
    eyes = np.concatenate([free, np.full((len(free), 1), 5)], axis=1)
    stats = {}
    want_v, want_f = S.counts_ref(vm.grid_pos, RS, RVH, eyes, vm.grid_pos[mask], mask, 0, 625, stats)
    assert np.array_equal(vp.visible, want_v) and np.array_equal(vp.first, want_f)
    assert stats["beyond_range"] > 0 and stats["visible_through_transparent"] > 0          # the picture does not hide itself
    r, c = vp.cells[:, 0], vp.cells[:, 1]
    assert (vp.visible[r > 24] == 0).all() and (r > 24).sum() > 200                         # behind the full-height wall: nothing
    assert (vp.visible[(r > 14) & (r < 24)] > 0).any()
    north = r < 14
    assert (vp.visible[north] > 0).any() and (vp.visible[north] == 0).any()                 # through the door: from some cells only
    over = (r > 14) & (r < 19) & (c >= 8) & (c <= 15)
    assert (vp.visible[over] > 0).all() and over.sum() == 32                                # over the half-height partition ...
    low = vm.get_viewpoints(mask, eye_height=0.15, max_range=2.5)
    assert low.eye_h == 1 and (low.visible[over] == 0).all() and (low.visible > 0).any()    # ... which a low camera cannot see over
    assert np.array_equal(vp.mask(), np.isin(np.arange(900).reshape(30, 30), (r[vp.visible > 0] - 5) * 30 + c[vp.visible > 0] - 5))
    best = vp.best(len(vp))
    order = sorted(np.flatnonzero(vp.visible).tolist(), key=lambda i: (-int(vp.visible[i]), i))       # most first, ties in raster order
    assert best.tolist() == order and vp.best().tolist() == order[:1]

    def sees(cell):
        e = np.tile([[int(cell[0]), int(cell[1]), 5]], (12, 1)).astype(np.int32)
        with ops.cell_index(vm.grid_pos, RS, RVH) as index:
            return int((ops.line_of_sight(index, e, vm.grid_pos[mask], mask) == ops.LOS_VISIBLE).sum())

    start = [30.0, 10.0]                                                    # south of W2
    nav = Navigator()
    nav.build_visgraph(vm.get_obstacle_cropped(), vm.rmin, vm.cmin)
    try:
        contour_pos, _ = vm.get_nearest_reachable_pos(start, "picture", nav)
        assert contour_pos[0] == 25 and sees(contour_pos) == 0              # the contour point: right behind the wall, sees nothing
        pos, path = vm.get_viewpoint_pos(start, mask, nav, eye_height=EYE, max_range=2.5)
        k, path2 = nav.plan_to_viewpoint(start, vp)
        assert pos == vp.cells[k].tolist() and path == path2 and path[0] == start and path[-1] == [float(pos[0]), float(pos[1])]
        assert pos[0] < 24 and sees(pos) == int(vp.visible[k]) >= max(1, int(np.ceil(0.5 * int(vp.visible.max()))))
        keep = vp.select(0.5)
        lens = nav.path_lengths(start, vp.cells[keep].astype(np.float64))
        assert np.isfinite(lens).any() and keep[int(np.argmin(lens))] == k                  # the shortest way among the cells that see enough
    finally:
        nav.close()
    crow, crow_path = vm.get_viewpoint_pos(start, vp)                       # without a navigator: as the crow flies
    d2 = ((vp.cells[keep] - np.array(start)) ** 2).sum(axis=1)
    assert crow == vp.cells[keep][int(np.argmin(d2))].tolist() and crow_path == [start, crow] and sees(crow) > 0


def test_plan_path_view_on_a_synthetic_scene(tmp_path, capsys):
    """apps.plan_path --view in process (the recipe of test_relations_gpu's scene): a goal cell with a non-zero visible count and a
    path to it, the goal Map.get_viewpoint_pos gives, --nearest path and --render included"""
    import json
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map, plan_path
    from avlmaps_amd.apps.common import HashClip, load_config
    from avlmaps_amd.map import VLMap
    scene_dir = make(tmp_path / "scene", frames=4, H=96, W=128)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                  "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(scene_dir), "--config", str(cfg), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    vm = VLMap(load_config(str(cfg)).map_config, data_dir=str(scene_dir))
    assert vm.load_map(str(scene_dir))
    vm.clip_feat_dim = vm.grid_feat.shape[1]
    vm.clip_model = HashClip(vm.clip_feat_dim)
    vm.init_categories(["sofa", "chair", "other"])
    vm.generate_obstacle_map()
    from avlmaps_amd.navigator import Navigator
    counts = {q: vm.get_viewpoints(q, max_range=2.0) for q in ("sofa", "chair", "other")}
    query = max(counts, key=lambda q: int(counts[q].visible.max(initial=0)))
    vp = counts[query]
    assert vp.visible.max(initial=0) > 0, "no category of the scene is visible from any free cell"
    free = np.argwhere(vm.get_obstacle_cropped()) + (vm.rmin, vm.cmin)
    nav = Navigator()
    nav.build_visgraph(vm.get_obstacle_cropped(), vm.rmin, vm.cmin)
    keep = vp.select(0.9)
    some = vp.cells[keep].astype(np.float64)

    def fits(s):
        """the goal of the first call below can be reached from s and is not s itself"""
        near, _ = vm.get_viewpoint_pos(s, vp, min_fraction=0.9)
        return near != [int(s[0]), int(s[1])] and np.isfinite(nav.path_lengths(s, [near])).all()
    try:
        start = next((s for s in ([float(c[0]), float(c[1])] for c in free[::max(1, len(free) // 48)]) if fits(s)), None)
        assert start is not None, f"no sampled start of the scene reaches a viewpoint ({len(free)} free cells, {len(some)} viewpoints)"
        by_travel = int(keep[int(np.argmin(nav.path_lengths(start, some)))])
    finally:
        nav.close()
    want, _ = vm.get_viewpoint_pos(start, vp, min_fraction=0.9)
    capsys.readouterr()
    base = ["--data-dir", str(scene_dir), "--config", str(cfg), "--text-model", "hash", "--categories", "sofa,chair,other", "--query", query,
            "--start", str(start[0]), str(start[1]), "--view", "--view-range", "2.0", "--view-fraction", "0.9"]
    out = plan_path.main(base)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert out["goal_kind"] == "viewpoint" and out["goal"] == [float(want[0]), float(want[1])] and out["visible"] > 0
    at = int(np.flatnonzero((vp.cells == want).all(axis=1))[0])
    assert out["visible"] == int(vp.visible[at]) >= 0.9 * int(vp.visible.max()) and out["view_targets"] == vp.n_targets
    assert out["view_cells"] == int((vp.visible > 0).sum()) and out["path"][0] == start and out["path"][-1] == out["goal"]
    png = tmp_path / "view.png"
    out = plan_path.main(base + ["--nearest", "path", "--render", str(png)])
    assert out["goal"] == [float(v) for v in vp.cells[by_travel]] and out["visible"] == int(vp.visible[by_travel])
    assert out["path"][0] == start and out["path"][-1] == out["goal"] and png.exists()
