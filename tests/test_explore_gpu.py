"""GPU tests of the explored map (csrc/avl_explore.hip): avl_carve_free_space against the scalar restatement of tests/_explore_ref.py
with np.array_equal -- no tolerance, no excluded rays -- avl_frontier_mask against a NumPy expression, and the Map / Navigator
layers end to end.  Every scene asserts, through the restatement's own bookkeeping, that it contains the cases it is there for."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import _explore_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CS = 0.25
K79 = R.calib(4.0, 4.5, 3.5)          # 7 x 9 frames: pixel (3, 4) looks straight ahead, (3, 8) exactly 45 degrees to the right
K68 = R.calib(4.0, 4.0, 3.0)          # 6 x 8 frames: no pixel on the optical axis
BAND = dict(h_min=0.0, h_max=1.5, min_depth=0.125, max_depth=4.0)
WIDE = dict(h_min=-50.0, h_max=50.0, min_depth=0.125, max_depth=4.0)       # a band no ray of these scenes leaves


def both(depth, calib, Ts, ids, gs, stride=1, first_seen=None, **kw):
    """(the device's map, the restatement's map, the restatement's statistics)"""
    from avlmaps_amd import ops
    stats = {}
    want = R.carve_ref(first_seen, depth, calib, Ts, ids, gs, CS, stride=stride, stats=stats, **kw)
    got = ops.carve_free_space(None if first_seen is None else first_seen.copy(), depth, calib, Ts, ids, gs, CS, stride=stride, **kw)
    assert got.dtype == np.int32 and got.shape == (gs, gs)
    return got, want, stats


def depths(shape, seed, lo=0.3, hi=3.9):
    return np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32)


@pytest.mark.parametrize("gs", [48, 50])
def test_every_octant_and_the_axis_and_diagonal_walks(gs):
    origin = (0.125, 0.125, 1.0)                                          # the centre of a cell, so the 45-degree ray walks a diagonal
    Ts = np.stack([R.camera(origin, yaw=y) for y in (0, 90, 180, 270)])
    depth = depths((4, 7, 9), 1)
    depth[:, 3, 4] = 2.0                                                  # straight ahead: along a column (yaw 0, 180) or a row (90, 270)
    depth[:, 3, 8] = 2.0                                                  # 45 degrees: dr == dc
    depth[0, 0, 0] = 0.13                                                 # ends in the camera's own cell: a == b
    got, want, stats = both(depth, K79, Ts, [0, 1, 2, 3], gs, **WIDE)
    assert np.array_equal(got, want)
    assert len(stats["octants"]) == 8 and all(stats.get(k) for k in ("along_row", "along_col", "diagonal", "point", "hit"))
    assert (want >= 0).sum() > 100


def test_depth_values_and_far_rays():
    T = R.camera((0.125, 0.125, 1.0))[None]
    depth = np.full((1, 7, 9), 2.0, np.float32)
    depth[0, 0, :4] = [0.0, np.nan, -1.0, 0.125]                          # zero, NaN, negative, exactly min_depth: dropped
    depth[0, 0, 6] = 4.0                                                  # exactly max_depth: far
    depth[0, 1, 0] = np.inf                                               # p * (max_depth / inf) is not finite: skipped
    depth[0, 3, 4] = 2.0                                                  # a hit straight ahead: its end cell (16, 24) stays unseen ...
    got, want, stats = both(depth, K79, T, [0], 48, **WIDE)
    assert np.array_equal(got, want)
    assert stats["dropped"] == 4 and stats["far"] == 1 and stats["not_finite"] == 1
    assert got[17, 24] == 0 and got[16, 24] == -1
    depth[0, 3, 4] = 5.0                                                  # ... and the far ray marks its last cell, row 24 - int(4.125 / 0.25)
    got, want, stats = both(depth, K79, T, [0], 48, **WIDE)
    assert np.array_equal(got, want) and stats["far"] == 2
    assert got[8, 24] == 0 and got[7, 24] == -1


def test_hit_cell_crossed_by_another_ray():
    from avlmaps_amd import ops
    Ts = np.stack([R.camera((0.125, 0.125, 1.0))] * 2)
    depth = np.zeros((2, 7, 9), np.float32)
    depth[0, 3, 4], depth[1, 3, 4] = 2.0, 3.0                             # frame 5 ends in (16, 24); frame 9 walks through it
    got, want, _ = both(depth, K79, Ts, [5, 9], 48, **BAND)
    assert np.array_equal(got, want)
    assert got[17, 24] == 5 and got[16, 24] == 9 and got[13, 24] == 9 and got[12, 24] == -1
    alone = ops.carve_free_space(None, depth[:1], K79, Ts[:1], [5], 48, CS, stride=1, **BAND)
    assert alone[16, 24] == -1


def test_height_slab():
    # 7 x 9 frames, rows 0 .. 6 look up to down: (v + 0.5 - 3.5) / 4 = -0.75 .. 0.75 per metre of depth, row 3 is level
    depth = depths((5, 7, 9), 2, 1.0, 3.9)
    Ts = np.stack([R.camera((0.125, 0.3, 1.0)),                           # inside the band: level rays inside, rising rays leave it
                   R.camera((-0.4, 0.125, 2.0), yaw=90),                  # above it: level rays outside, rising rays wholly above, falling ones enter
                   R.camera((0.2, -0.3, 1.25), yaw=180, pitch=20.0),      # pitched down
                   R.camera((0.3, 0.2, 0.75), yaw=270, roll=15.0),        # rolled
                   R.camera((-0.2, -0.1, -0.5), pitch=-30.0)])            # below the floor, looking up: enters through h_min
    got, want, stats = both(depth, K79, Ts, [0, 1, 2, 3, 4], 48, **BAND)
    assert np.array_equal(got, want)
    for k in ("level_inside", "level_outside", "slab_empty", "slab_inside", "slab_enters", "slab_leaves"):
        assert stats.get(k), (k, stats)
    # a ray that leaves the band marks the cell where it leaves, hit or not: the single ray of pixel (0, 4), 0.75 up per metre from
    # height 1.0, leaves at depth 2/3: x = 0.125 + 2/3 -> int(3.17) = 3 -> row 21 is its last cell
    one = np.zeros((1, 7, 9), np.float32)
    one[0, 0, 4] = 3.0
    got, want, stats = both(one, K79, Ts[:1], [0], 48, **BAND)
    assert np.array_equal(got, want) and stats["hit"] == 1 and stats["slab_leaves"] == 1
    assert np.argwhere(got >= 0).tolist() == [[21, 23], [22, 23], [23, 23], [24, 23]]          # column 24 - int(0.3 / 0.25)


@pytest.mark.parametrize("gs", [48, 50])
def test_grid_edges_and_both_sides_of_zero(gs):
    half = gs * CS / 2
    Ts = np.stack([R.camera((-0.1, 0.1, 1.0), yaw=45.0),                  # around the map's centre lines: int() truncates toward zero on both sides
                   R.camera((0.1, -0.1, 1.0), yaw=225.0),
                   R.camera((half - 0.6, 0.3, 1.0)),                      # near the border, looking out: rays leave the grid
                   R.camera((-half + 0.3, -half + 0.4, 1.0), yaw=200.0)])
    depth = depths((4, 6, 8), 3, 0.2, 6.0)                                # some beyond max_depth
    got, want, stats = both(depth, K68, Ts, [0, 1, 2, 3], gs, **WIDE)
    assert np.array_equal(got, want)
    assert stats.get("leaves_grid") and stats.get("far") and stats.get("hit")
    assert (want[: gs // 2] >= 0).any() and (want[gs // 2:] >= 0).any() and (want[:, : gs // 2] >= 0).any() and (want[:, gs // 2:] >= 0).any()
    # a camera outside the grid marks nothing, not even where its rays would cross the map
    out = np.stack([R.camera((half + 1.0, 0.0, 1.0), yaw=180.0)])
    got, want, stats = both(depth[:1], K68, out, [0], gs, **WIDE)
    assert np.array_equal(got, want) and not (got >= 0).any() and stats["starts_outside"] == 48


@pytest.mark.parametrize("stride", [1, 2, 3, 13])
@pytest.mark.parametrize("shape, calib", [((6, 8), K68), ((7, 9), K79)])
def test_strides(stride, shape, calib):
    Ts = np.stack([R.camera((0.3, -0.2, 1.0), yaw=30.0), R.camera((-1.0, 0.5, 0.5), yaw=160.0, pitch=5.0)])
    depth = depths((2,) + shape, 4)
    got, want, stats = both(depth, calib, Ts, [0, 1], 50, stride=stride, **BAND)
    assert np.array_equal(got, want)
    rays = sum(stats.get(k, 0) for k in ("hit", "far", "slab_empty", "level_outside", "dropped"))
    assert rays == 2 * len(range(stride // 2, shape[0], stride)) * len(range(stride // 2, shape[1], stride))
    if stride == 13 and shape[0] == 6:                                    # no lattice row at all: the camera cells alone
        assert rays == 0 and (got >= 0).sum() == 2


def test_the_fold_is_a_minimum():
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    Ts = np.stack([R.camera((0.1, 0.1, 1.0), yaw=y) for y in (0.0, 40.0, 80.0, 20.0)])
    depth = depths((4, 6, 8), 5)
    ids = np.array([12, 7, 30, 9])                                        # not from zero, not ascending; frames 0, 1 and 3 overlap
    kw = dict(stride=1, **WIDE)
    want = R.carve_ref(None, depth, K68, Ts, ids, 48, CS, **kw)
    once = ops.carve_free_space(None, depth, K68, Ts, ids, 48, CS, **kw)
    assert np.array_equal(once, want)
    overlap = (R.carve_ref(None, depth[:1], K68, Ts[:1], ids[:1], 48, CS, **kw) >= 0) & (R.carve_ref(None, depth[3:], K68, Ts[3:], ids[3:], 48, CS, **kw) >= 0)
    assert overlap.sum() > 5 and np.all(want[overlap] <= 9)               # two frames see a cell: the smaller id stays
    # two calls, continuing a host map in place
    fs = np.full((48, 48), -1, np.int32)
    assert ops.carve_free_space(fs, depth[:2], K68, Ts[:2], ids[:2], 48, CS, **kw) is fs
    ops.carve_free_space(fs, depth[2:], K68, Ts[2:], ids[2:], 48, CS, **kw)
    assert np.array_equal(fs, want)
    # reversed order, frame by frame, on a device map
    dev = DeviceArray.from_numpy(np.full((48, 48), -1, np.int32))
    for k in (3, 2, 1, 0):
        assert ops.carve_free_space(dev, DeviceArray.from_numpy(depth[k]), K68, Ts[k], ids[k:k + 1], 48, CS, device=True, **kw) is dev
    assert np.array_equal(dev.numpy(), want)
    # more frames than one launch takes (16): the same frames again with larger ids change nothing
    many = ops.carve_free_space(want.copy(), np.concatenate([depth] * 5), K68, np.concatenate([Ts] * 5), np.arange(100, 120), 48, CS, **kw)
    assert np.array_equal(many, want)


def test_uint16_depth_equals_float32():
    from avlmaps_amd import ops
    Ts = np.stack([R.camera((0.1, 0.1, 1.0), yaw=10.0), R.camera((0.4, -0.3, 1.0), yaw=100.0)])
    mm = (np.random.default_rng(6).integers(0, 40, (2, 7, 9)) * 125).astype(np.uint16)      # multiples of 1/8 m: value / 1000 is exact in float32
    mm[0, 0, 0] = 0
    f32 = (mm / 1000.0).astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), mm / 1000.0)
    kw = dict(stride=1, **BAND)
    a = ops.carve_free_space(None, mm, K79, Ts, [0, 1], 48, CS, depth_div=1000.0, **kw)
    b = ops.carve_free_space(None, f32, K79, Ts, [0, 1], 48, CS, **kw)
    assert np.array_equal(a, b) and np.array_equal(a, R.carve_ref(None, f32, K79, Ts, [0, 1], 48, CS, **kw)) and (a >= 0).sum() > 50


# ------------------------------------------------------------------ frontier
def frontier_cases():
    rng = np.random.default_rng(8)
    yield np.ones((1, 1), bool), np.ones((1, 1), bool)
    yield np.ones((1, 1), bool), np.zeros((1, 1), bool)
    for shape in ((1, 7), (7, 1)):
        yield rng.random(shape) < 0.8, rng.random(shape) < 0.5
    free, explored = np.ones((9, 11), bool), np.ones((9, 11), bool)
    explored[0, 3:6] = explored[4:7, 0] = explored[8, 8:] = explored[2:5, 10] = False        # unknown cells on all four borders
    explored[4, 4:7] = False
    free[4, 5] = free[3, 5] = False                                      # an obstacle next to unexplored space
    yield free, explored
    yield rng.random((9, 11)) < 0.8, rng.random((9, 11)) < 0.5
    yield rng.random((9, 11)) < 0.8, np.ones((9, 11), bool)               # all explored: no frontier
    yield rng.random((9, 11)) < 0.8, np.zeros((9, 11), bool)              # none explored: no frontier
    yield rng.random((70, 130)) < 0.85, rng.random((70, 130)) < 0.6       # more than one block each way


def test_frontier_mask_equals_the_numpy_expression():
    from avlmaps_amd import ops
    for i, (free, explored) in enumerate(frontier_cases()):
        got = ops.frontier_mask(free, explored)
        assert got.dtype == np.uint8 and np.array_equal(got, R.frontier_ref(free, explored)), i
        assert np.array_equal(ops.frontier_mask(free.astype(np.uint8), explored.astype(np.uint8), device=True).numpy(), got)
    free, explored = list(frontier_cases())[4]
    got = ops.frontier_mask(free, explored)
    assert got[1, 4] == 1 and got[0, 2] == 1 and got[8, 7] == 1           # frontier cells at and next to the image border
    assert got[2, 5] == 0                                                 # (2, 5) borders only the obstacle (3, 5): known, no frontier through it
    assert not ops.frontier_mask(*list(frontier_cases())[6]).any() and not ops.frontier_mask(*list(frontier_cases())[7]).any()


# ------------------------------------------------------------------ end to end
GS = 48


def _config():
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": GS, "map_config.cell_size": CS,
                                  "map_config.cam_calib_mat": [4.0, 0, 4.0, 0, 4.0, 3.0, 0, 0, 1]}).map_config


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """three depth frames with poses and a map file with a few voxels: all create_explored_map and load_map need"""
    from scipy.spatial.transform import Rotation
    from avlmaps_amd.utils.mapping_utils import save_3d_map
    sc = tmp_path_factory.mktemp("explore") / "scene"
    (sc / "depth").mkdir(parents=True)
    (sc / "vlmap").mkdir()
    poses = []
    for i, yaw in enumerate((0.0, 25.0, -40.0)):
        q = Rotation.from_euler("y", yaw, degrees=True).as_quat()
        poses.append([0.3 * i, 0.0, -0.2 * i, *q])
        np.save(sc / "depth" / f"{i:06d}.npy", depths((6, 8), 10 + i, 0.5, 7.0))
    np.savetxt(sc / "poses.txt", np.array(poses))
    occupied = -np.ones((GS, GS, 6), np.int32)
    pos = np.array([[10, 10, 2], [12, 30, 1], [30, 20, 3], [20, 8, 2]], np.int32)
    occupied[pos[:, 0], pos[:, 1], pos[:, 2]] = np.arange(4)
    save_3d_map(sc / "vlmap" / "vlmaps.h5df", np.zeros((4, 8), np.float32), pos, np.ones(4, np.float32), occupied, [0, 1, 2],
                np.zeros((4, 3), np.uint8))
    return sc


def test_create_explored_map_round_trips_through_load_map(scene):
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.map.vlmap_builder import VLMapBuilder
    cfg = _config()
    vm = VLMap(cfg)
    first_seen = vm.create_explored_map(scene, stride=2, batch=2)         # two batches: 2 + 1 frames
    assert first_seen.dtype == np.int32 and first_seen.shape == (GS, GS) and set(np.unique(first_seen)) == {-1, 0, 1, 2}
    builder = VLMapBuilder(scene, cfg, vm.pose_path, vm.rgb_paths, vm.depth_paths, vm.base2cam_tf, vm.base_transform)
    Ts = np.stack(builder.frame_transforms(np.loadtxt(scene / "poses.txt").reshape(-1, 7)))
    depth = np.stack([np.load(p) for p in sorted((scene / "depth").glob("*.npy"))])
    want = R.carve_ref(None, depth, np.array(cfg["cam_calib_mat"]).reshape(3, 3), Ts, [0, 1, 2], GS, CS, stride=2, h_min=0.0, h_max=1.5,
                       min_depth=0.1, max_depth=6.0)
    assert np.array_equal(first_seen, want)
    assert vm.explored_params == dict(gs=GS, cs=CS, stride=2, h_min=0.0, h_max=1.5, min_depth=0.1, max_depth=6.0, n_frames=3)
    other = VLMap(cfg)
    assert other.load_map(str(scene))
    assert np.array_equal(other.first_seen, first_seen) and other.explored_params == vm.explored_params
    other.generate_obstacle_map()
    crop = other.get_obstacle_cropped()
    known = other.get_known_free_cropped()
    assert known.shape == crop.shape and known.dtype == bool
    assert np.array_equal(known, crop & (first_seen >= 0)[other.rmin:other.rmax + 1, other.cmin:other.cmax + 1])
    assert np.array_equal(other.get_explored_cropped(), (first_seen >= 0)[other.rmin:other.rmax + 1, other.cmin:other.cmax + 1])
    assert np.array_equal(other.generate_known_free_map(0, 1.5), other.obstacles_map & (first_seen >= 0))
    # a scene without the file loads as ever
    (scene / "vlmap" / VLMap.EXPLORED_FILE).rename(scene / "vlmap" / "explored.bak")
    try:
        plain = VLMap(cfg)
        assert plain.load_map(str(scene)) and plain.first_seen is None
    finally:
        (scene / "vlmap" / "explored.bak").rename(scene / "vlmap" / VLMap.EXPLORED_FILE)


def _two_rooms(door=(23, 25)):
    """(occupied_ids, seen): a 40 x 40 walled hall with a walled inner room that has a door (rows door[0] .. door[1] - 1) to the west
    and one to the east; the hall around the room has been seen, the inside of the room has not"""
    occupied = -np.ones((GS, GS, 6), np.int32)
    wall = np.zeros((GS, GS), bool)
    wall[4, 4:44] = wall[43, 4:44] = wall[4:44, 4] = wall[4:44, 43] = True          # the hall
    wall[14, 14:34] = wall[33, 14:34] = wall[14:34, 14] = wall[14:34, 33] = True    # the room
    wall[door[0]:door[1], 14] = wall[door[0]:door[1], 33] = False                   # its doors
    occupied[wall, 2] = 1 + np.arange(wall.sum())
    seen = np.zeros((GS, GS), bool)
    seen[5:43, 5:43] = True
    seen[15:33, 15:33] = False
    return occupied, seen


def test_known_free_map_keeps_the_planner_out_of_the_unseen_room():
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.navigator import Navigator
    vm = VLMap(_config())
    vm.occupied_ids, seen = _two_rooms()
    vm.first_seen = np.where(seen, 3, -1).astype(np.int32)
    vm.generate_obstacle_map()
    start, goal = (24.0, 8.0), (24.0, 39.0)                               # west and east of the room, level with its doors

    def length(path):
        return float(np.sum(np.linalg.norm(np.diff(np.asarray(path, dtype=np.float64), axis=0), axis=1)))

    def enters_room(path):
        pts = np.asarray(path, dtype=np.float64)
        along = np.concatenate([np.linspace(a, b, 200) for a, b in zip(pts[:-1], pts[1:])])
        return bool(np.any((along[:, 0] >= 15) & (along[:, 0] < 33) & (along[:, 1] >= 15) & (along[:, 1] < 33)))

    nav = Navigator()
    try:
        nav.build_visgraph(vm.get_obstacle_cropped(), vm.rmin, vm.cmin)
        through = nav.plan_to(start, goal)
        assert enters_room(through)                                       # the plain map routes through the room nobody looked into
        known = vm.get_known_free_cropped()
        assert known.shape == vm.get_obstacle_cropped().shape
        nav.build_visgraph(known, vm.rmin, vm.cmin)
        around = nav.plan_to(start, goal)
        assert not enters_room(around)
        assert length(around) > length(through)                            # 40.6 cells around the room against 31 through it
        # where to look next: the doors are the frontier, the nearer one is the west door
        centres, sizes = vm.get_frontiers(min_cells=2)
        assert len(centres) == 2 and sizes.tolist() == [2, 2]
        frontier = np.zeros((GS, GS), bool)
        frontier[23:25, 14] = frontier[23:25, 33] = True
        assert all(frontier[r, c] for r, c in centres)
        k, path = nav.plan_to_nearest_frontier(start, (centres, sizes))
        assert centres[k, 1] == 14 and [int(path[-1][0]), int(path[-1][1])] == centres[k].tolist()
        assert len(vm.get_frontiers(min_cells=3)[0]) == 0
    finally:
        nav.close()


def test_plan_path_goes_to_the_nearest_frontier(tmp_path):
    """apps.plan_path --goal frontier on the two-room map, saved as a scene: the goal is the west door, the path ends on it and
    stays out of the unseen room; --known-free --render draws on the known-free crop"""
    import yaml
    from PIL import Image
    from avlmaps_amd.apps import plan_path
    from avlmaps_amd.utils.mapping_utils import save_3d_map
    occupied, seen = _two_rooms(door=(21, 27))                            # six cells wide: get_frontiers' default keeps islands of 5 and more
    pos = np.argwhere(occupied > 0).astype(np.int32)
    pos = pos[np.argsort(occupied[pos[:, 0], pos[:, 1], pos[:, 2]])]
    occupied[occupied > 0] -= 1                                           # ids = rows of grid_pos; the wall cell with id 0 does not count upstream
    sc = tmp_path / "scene"
    (sc / "vlmap").mkdir(parents=True)
    save_3d_map(sc / "vlmap" / "vlmaps.h5df", np.zeros((len(pos), 8), np.float32), pos, np.ones(len(pos), np.float32), occupied, [0],
                np.full((len(pos), 3), 200, np.uint8))
    np.savez_compressed(sc / "vlmap" / "explored.npz", first_seen=np.where(seen, 0, -1).astype(np.int32), gs=GS, cs=CS, stride=4, h_min=0.0,
                        h_max=1.5, min_depth=0.1, max_depth=6.0, n_frames=1)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"grid_size": GS, "cell_size": CS}, "params": {"gs": GS, "cs": CS}}))
    base = ["--data-dir", str(sc), "--config", str(cfg), "--text-model", "hash", "--start", "24", "8"]
    out = plan_path.main(base + ["--goal", "frontier", "--render", str(tmp_path / "f.png")])
    assert out["goal_kind"] == "frontier" and out["frontiers"] == 2 and out["frontier_cells"] == 6
    assert out["goal"] == [23.0, 14.0] and out["path"][-1] == out["goal"] and out["path"][0] == [24.0, 8.0]
    img = np.asarray(Image.open(tmp_path / "f.png"))
    assert img.shape[2] == 3 and tuple(img[24 - out_rmin(occupied), 8 - out_rmin(occupied)]) == (0, 255, 0)
    with pytest.raises(SystemExit):
        plan_path.main(base + ["--goal", "frontier", "--query", "door"])


def out_rmin(occupied):
    """the first row (= first column, the hall is square) of the obstacle crop: the smallest row that holds a counted voxel"""
    return int(np.argwhere(occupied > 0)[:, 0].min())
