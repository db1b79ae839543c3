"""CPU tests of the explored map: the restatement the GPU tests compare against (on rays worked out by hand), the .npz round
trip, the errors of a map without an explored map, and the argument checks of ops.carve_free_space / ops.frontier_mask, all of
which happen before any device work."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import _explore_ref as R  # noqa: E402

GS, CS = 48, 0.25
K = R.calib(4.0, 4.5, 3.5)            # 7 x 9 frames: pixel (v, u) = (3, 4) looks straight ahead, (3, 8) 45 degrees to the right
BAND = dict(h_min=0.0, h_max=1.5, min_depth=0.125, max_depth=4.0)


def one_ray(z, u, v, T, **kw):
    return R.ray_cells(np.float32(z), u, v, np.linalg.inv(K), T, GS, CS, **{**BAND, **kw})


def test_restatement_on_three_rays_by_hand():
    # Ray 1: camera at (0.125, 0.125, 1.0) looking along +x, pixel (3, 4): Kinv (4.5, 3.5, 1) = (0, 0, 1), depth 2 -> p = (0, 0, 2),
    # P = (2.125, 0.125, 1.0).  Level ray at height 1.0, inside [0, 1.5]: t0 = 0, t1 = 1.  a = cell(O): int(0.125 / 0.25) = 0 ->
    # (24, 24); b: int(2.125 / 0.25) = 8 -> row 16, col 24.  Walk up the column 24, rows 24 .. 17; the hit's end cell (16, 24) stays.
    T = R.camera((0.125, 0.125, 1.0))
    assert one_ray(2.0, 4, 3, T) == [(r, 24) for r in range(24, 16, -1)]
    # the same ray at depth 5 >= max_depth is far: s = 4 / 5, P.x = 0.125 + 5 * 0.8 = 4.125 -> int(16.5) = 16 -> row 8, and the end
    # cell IS marked: rows 24 .. 8
    assert one_ray(5.0, 4, 3, T) == [(r, 24) for r in range(24, 7, -1)]
    # Ray 2: pixel (3, 8): Kinv (8.5, 3.5, 1) = (1, 0, 1), depth 2 -> p = (2, 0, 2), P = O + (z, -x, -y) = (2.125, -1.875, 1.0).
    # b: row 24 - 8 = 16; int(-1.875 / 0.25) = int(-7.5) = -7 (toward zero) -> col 24 + 7 = 31.  dr = 8, dc = 7, err = -1, -2, -3:
    # both coordinates move; at err = -4, e2 = -8 is not > -dr and only the row moves (err = 3); then both move again, err = 2, 1,
    # 0, and the step from (17, 30) lands on the end (16, 31), which a hit leaves unmarked.
    got = one_ray(2.0, 8, 3, T)
    assert got == [(24, 24), (23, 25), (22, 26), (21, 27), (20, 27), (19, 28), (18, 29), (17, 30)]
    # Ray 3: the camera at height 2.0, above the band, pixel (6, 4): Kinv (4.5, 6.5, 1) = (0, 0.75, 1), depth 4 (= max_depth: far,
    # s = 1) -> p = (0, 3, 4), P = (4.125, 0.125, 2 - 3) = (4.125, 0.125, -1).  dz = -3: ta = (0 - 2) / -3 = 2/3, tb = (1.5 - 2) / -3
    # = 1/6 -> t0 = 1/6, t1 = 2/3: it enters the band from above and leaves it through the floor.  x(t0) = 0.125 + 4/6 = 0.79 ->
    # int(3.17) = 3 -> row 21; x(t1) = 0.125 + 8/3 = 2.79 -> int(11.17) = 11 -> row 13.  t1 < 1: the end cell counts.
    T_high = R.camera((0.125, 0.125, 2.0))
    stats = {}
    assert one_ray(4.0, 4, 6, T_high, stats=stats) == [(r, 24) for r in range(21, 12, -1)]
    assert stats["slab_enters"] == 1 and stats["slab_leaves"] == 1 and stats["far"] == 1
    # a hit that leaves the band before its end marks the cell where it leaves: depth 3.5 < max_depth, same geometry scaled
    stats = {}
    cells = one_ray(3.5, 4, 6, T_high, stats=stats)
    assert stats["hit"] == 1 and stats["slab_leaves"] == 1 and cells[-1] == R.cell(GS, CS, 0.125 + (2.0 / 2.625) * 3.5, 0.125)


def test_restatement_drops_and_skips():
    T = R.camera((0.125, 0.125, 1.0))
    for z in (0.0, -1.0, np.nan, 0.125):                     # p.z > min_depth is strict
        assert one_ray(z, 4, 3, T) == []
    assert one_ray(2.0, 4, 3, R.camera((0.125, 0.125, 2.0))) == []        # a level ray above the band
    assert one_ray(2.0, 4, 0, R.camera((0.125, 0.125, 2.0))) == []        # and one that climbs from there
    assert one_ray(2.0, 4, 3, R.camera((7.0, 0.0, 1.0))) == []            # a camera outside the grid: int(28) -> row -4
    # a ray that leaves the grid stops at the border: from x = 5.625 (row 2) ahead
    assert one_ray(5.0, 4, 3, R.camera((5.625, 0.125, 1.0))) == [(2, 24), (1, 24), (0, 24)]


def test_walk_reaches_its_end_in_every_octant():
    """the strict-inequality form of the walk ends exactly on b for every (dr, dc), so a hit's end cell is well defined"""
    a = (40, 40)
    for dr in range(-33, 34):
        for dc in range(-33, 34):
            b = (a[0] + dr, a[1] + dc)
            cells = R.walk(a, b, 100, True)
            assert cells[0] == a and cells[-1] == b and len(cells) == max(abs(dr), abs(dc)) + 1
            steps = np.abs(np.diff(np.array(cells), axis=0))
            assert steps.size == 0 or (steps.max() == 1 and np.all(steps.sum(axis=1) >= 1))
            assert R.walk(a, b, 100, False) == cells[:-1]


def test_carve_ref_folds_a_minimum_and_marks_the_camera_cell():
    depth = np.full((2, 7, 9), 2.0, np.float32)
    Ts = np.stack([R.camera((0.125, 0.125, 1.0)), R.camera((0.125, 0.125, 1.0), yaw=90)])
    a = R.carve_ref(None, depth, K, Ts, [7, 3], GS, CS, stride=3, **BAND)
    assert a[24, 24] == 3 and a[20, 24] == 7 and a[24, 20] == 3 and a[0, 0] == -1
    b = R.carve_ref(R.carve_ref(None, depth[1:], K, Ts[1:], [3], GS, CS, stride=3, **BAND), depth[:1], K, Ts[:1], [7], GS, CS, stride=3, **BAND)
    assert np.array_equal(a, b)
    # a stride above the frame height leaves no lattice row: only the camera cell
    c = R.carve_ref(None, depth[:1], K, Ts[:1], [0], GS, CS, stride=15, **BAND)
    assert np.argwhere(c >= 0).tolist() == [[24, 24]]


def test_frontier_ref_by_hand():
    free = np.ones((3, 4), bool)
    free[1, 2] = False                                     # an obstacle
    explored = np.zeros((3, 4), bool)
    explored[:, :2] = True
    # column 1 borders the unexplored free column 2, except in row 1 where the neighbour is the obstacle: known, no frontier through it
    assert R.frontier_ref(free, explored).tolist() == [[0, 1, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0]]


# ------------------------------------------------------------------ Map
def _config():
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": GS, "map_config.cell_size": CS}).map_config


def test_npz_round_trip_and_missing_file(tmp_path):
    from avlmaps_amd.map import VLMap
    vm = VLMap(_config())
    assert vm.first_seen is None and not vm.load_explored_map(tmp_path)
    fs = np.full((GS, GS), -1, np.int32)
    fs[10:20, 5:9] = np.arange(40).reshape(10, 4)
    (tmp_path / "vlmap").mkdir()
    params = dict(gs=GS, cs=CS, stride=4, h_min=0.0, h_max=1.5, min_depth=0.1, max_depth=6.0, n_frames=40)
    np.savez_compressed(tmp_path / "vlmap" / VLMap.EXPLORED_FILE, first_seen=fs, **params)
    assert vm.load_explored_map(tmp_path)
    assert vm.first_seen.dtype == np.int32 and np.array_equal(vm.first_seen, fs) and vm.explored_params == params
    assert np.array_equal(vm.generate_explored_map(), fs >= 0)
    other = VLMap({**_config(), "grid_size": GS + 2})
    with pytest.raises(ValueError, match="does not belong"):
        other.load_explored_map(tmp_path)
    assert other.first_seen is None


def test_map_methods_need_an_explored_map():
    from avlmaps_amd.map import VLMap
    vm = VLMap(_config())
    for call in (vm.generate_explored_map, vm.get_explored_cropped, vm.generate_known_free_map, vm.get_known_free_cropped, vm.get_frontiers):
        with pytest.raises(RuntimeError, match="no explored map"):
            call()


def test_plan_to_nearest_frontier_needs_a_frontier():
    from avlmaps_amd.navigator import Navigator
    nav = Navigator()
    with pytest.raises(ValueError, match="no frontier"):
        nav.plan_to_nearest_frontier((1, 1), (np.zeros((0, 2), np.int64), np.zeros((0,), np.int64)))
    with pytest.raises(RuntimeError):
        nav.plan_to_nearest_frontier((1, 1), [[2, 2]])          # a frontier, but no graph


# ------------------------------------------------------------------ ops: everything is checked before the device is touched
def _carve_args():
    return dict(first_seen=None, depth=np.ones((2, 6, 8), np.float32), calib=R.calib(4.0, 4.0, 3.0), transforms=np.stack([np.eye(4)] * 2),
                frame_ids=[0, 1], gs=GS, cs=CS)


@pytest.mark.parametrize("change, error", [
    (dict(depth=np.ones((2, 6, 8), np.float64)), TypeError),
    (dict(depth=np.ones((2, 6, 8), np.int32)), TypeError),
    (dict(first_seen=np.zeros((GS, GS), np.int64)), TypeError),
    (dict(first_seen=np.zeros((GS, GS + 1), np.int32)), ValueError),
    (dict(depth=np.ones((6,), np.float32)), ValueError),
    (dict(transforms=np.stack([np.eye(4)] * 3)), ValueError),
    (dict(transforms=np.eye(3)), ValueError),
    (dict(frame_ids=[0]), ValueError),
    (dict(frame_ids=[0, -1]), ValueError),
    (dict(frame_ids=[0.5, 1.0]), ValueError),
    (dict(calib=np.eye(4)), ValueError),
    (dict(stride=0), ValueError),
    (dict(h_min=1.0, h_max=0.5), ValueError),
    (dict(gs=0), ValueError),
    (dict(cs=0.0), ValueError),
    (dict(min_depth=2.0, max_depth=1.0), ValueError),
])
def test_carve_free_space_rejects_bad_arguments(change, error):
    from avlmaps_amd import ops
    with pytest.raises(error):
        ops.carve_free_space(**{**_carve_args(), **change})


def test_frontier_mask_rejects_bad_arguments():
    from avlmaps_amd import ops
    ok = np.ones((3, 4), bool)
    with pytest.raises(TypeError):
        ops.frontier_mask(ok.astype(np.int32), ok)
    with pytest.raises(TypeError):
        ops.frontier_mask(ok, ok.astype(np.float32))
    with pytest.raises(ValueError):
        ops.frontier_mask(ok, np.ones((4, 3), bool))
    with pytest.raises(ValueError):
        ops.frontier_mask(np.ones((3,), bool), np.ones((3,), bool))
    with pytest.raises(ValueError):
        ops.frontier_mask(np.ones((0, 3), bool), np.ones((0, 3), bool))


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    lib = _lib.load()
    kinv, T, ids = np.eye(3), np.eye(4), np.zeros(1, np.int32)
    args = lambda **kw: [kw.get(k, d) for k, d in (("depth", 1), ("u16", 0), ("div", 1000.0), ("F", 1), ("H", 6), ("W", 8),
                                                    ("kinv", kinv.ctypes.data), ("T", T.ctypes.data), ("ids", ids.ctypes.data), ("gs", GS),
                                                    ("cs", CS), ("stride", 4), ("h_min", 0.0), ("h_max", 1.5), ("dmin", 0.1), ("dmax", 6.0),
                                                    ("fs", 1), ("stream", None))]       # noqa: E731
    for bad, word in ((dict(stride=0), b"stride"), (dict(h_min=2.0), b"height band"), (dict(gs=0), b"grid size"), (dict(cs=-1.0), b"cell size"),
                      (dict(fs=None), b"null"), (dict(H=0), b"bad batch"), (dict(dmax=0.05), b"depth range")):
        assert lib.avl_carve_free_space(*args(**bad)) != 0 and word in lib.avl_last_error()
    neg = np.array([-2], np.int32)
    assert lib.avl_carve_free_space(*args(ids=neg.ctypes.data)) != 0 and b"negative" in lib.avl_last_error()
    assert lib.avl_frontier_mask(None, None, 3, 3, None, None) != 0 and b"null" in lib.avl_last_error()
    assert lib.avl_frontier_mask(1, 1, 0, 3, 1, None) != 0 and b"bad shape" in lib.avl_last_error()


def test_plan_path_flags():
    from avlmaps_amd.apps import plan_path
    base = ["--data-dir", "scene", "--start", "1", "2"]
    a = plan_path.parse_args(base + ["--goal", "frontier"])
    assert a.goal == "frontier" and a.known_free and a.query is None          # a frontier goal is planned on the known-free map
    a = plan_path.parse_args(base + ["--query", "sofa", "--known-free"])
    assert a.goal == "object" and a.known_free
    assert not plan_path.parse_args(base + ["--query", "sofa"]).known_free
    for bad in (["--goal", "frontier", "--query", "sofa"], ["--goal", "frontier", "--area", "kitchen"], ["--goal", "frontier", "--nearest", "path"], []):
        with pytest.raises(SystemExit):
            plan_path.parse_args(base + bad)
