"""Rooms and doorways on the GPU (csrc/avl_rooms.hip through ops.grow_labels, segment_rooms, lift_labels_2d and their users
Map.get_rooms, VLMap.get_voxel_rooms, SceneObjects.assign_rooms, AVLMap.name_rooms / index_room) against tests/_rooms_ref.py: the
heap Dijkstra ordered by (pair, label), SciPy's distance transform and labelling, and plain loops for the tables.

Every comparison is np.array_equal: the owner of a cell is the minimum over an exactly defined set, and the tables are integers.
T = 32 cells per tile side and C = 64 sweeps per tile and round are the kernel's constants (test_rooms_host.py checks that the
source says the same)."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tools"))
sys.path.insert(0, str(HERE))
from _rooms_ref import grow_ref, rooms_ref, three_rooms  # noqa: E402
from _travel_ref import serpentine, spiral  # noqa: E402

T, C = 32, 64
BIG = 2 ** 31 - 1
CATS = ["sofa", "table", "lamp", "other"]


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    assert (ops.TRAVEL_TILE, ops.TRAVEL_SWEEPS) == (T, C)
    return ops


def seeds_at(H, W, *items):
    s = np.zeros((H, W), np.int32)
    for r, c, label in items:
        s[r, c] = label
    return s


def check(ops, free, seeds, name=""):
    """owner and both planes equal the reference; returns (growth, owner)"""
    owner, A, B = grow_ref(free, seeds)
    g = ops.grow_labels(free, seeds)
    assert g.owner.dtype == np.int32 and g.owner.shape == owner.shape
    assert np.array_equal(g.field.straight, A) and np.array_equal(g.field.diagonal, B), name
    assert np.array_equal(g.owner, owner), (name, int((g.owner != owner).sum()))
    return g, owner


# ------------------------------------------------------------------ grow_labels
@pytest.mark.parametrize("density", [0.25, 0.4])
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (33, 65), (64, 64), (70, 100)])
def test_random_maps(ops, shape, density):
    H, W = shape
    for n_seeds in (1, 3, 8):
        rng = np.random.default_rng(1000 * H + 10 * W + n_seeds + int(100 * density))
        free = (rng.random((H, W)) >= density).astype(np.uint8)
        seeds = np.zeros((H, W), np.int32)
        at = rng.choice(H * W, size=min(n_seeds, H * W), replace=False)          # wherever they fall: some on obstacle cells
        labels = rng.choice(np.array([1, 2, 7, 1000, 2 ** 20 + 3, 2 ** 30, BIG - 1, BIG]), size=len(at), replace=False)
        seeds.ravel()[at] = labels
        check(ops, free, seeds, (shape, density, n_seeds))


def test_seeds_on_obstacle_cells(ops):
    rng = np.random.default_rng(5)
    free = (rng.random((40, 50)) >= 0.3).astype(np.uint8)
    blocked = np.argwhere(free == 0)
    seeds = seeds_at(40, 50, *[(int(r), int(c), 10 * k + 3) for k, (r, c) in enumerate(blocked[::37][:6])])
    assert (seeds > 0).sum() == 6 and not free[seeds > 0].any()
    check(ops, free, seeds)


def test_a_corridor_with_seeds_at_both_ends(ops):
    free = np.ones((1, 41), np.uint8)
    for left, right in ((5, 9), (9, 5)):
        g, _ = check(ops, free, seeds_at(1, 41, (0, 0, left), (0, 40, right)))
        assert g.owner[0, 20] == min(left, right)                                # the middle cell: both walks have 20 steps
        assert g.owner[0, 19] == left and g.owner[0, 21] == right


def test_two_fronts_meet_in_a_third_tile(ops):
    free = np.ones((3 * T, 3 * T), np.uint8)
    g, owner = check(ops, free, seeds_at(3 * T, 3 * T, (0, 0, 8), (3 * T - 1, 3 * T - 1, 3)))
    mid = owner[T:2 * T, T:2 * T]
    assert (mid == 8).any() and (mid == 3).any()
    assert g.rounds >= 2 and g.tile_runs >= 9


def test_three_seeds_at_equal_distance_from_a_tile_corner(ops):
    free = np.ones((2 * T, 2 * T), np.uint8)
    for labels in ((4, 2, 9), (9, 4, 2), (2, 9, 4)):
        seeds = seeds_at(2 * T, 2 * T, (T - 6, T, labels[0]), (T, T - 6, labels[1]), (T + 6, T, labels[2]))     # 6 straight steps from (T, T)
        g, owner = check(ops, free, seeds, labels)
        assert owner[T, T] == min(labels)


def test_serpentine_inside_one_tile_longer_than_the_cap(ops):
    free = serpentine(T, T)
    g, _ = check(ops, free, seeds_at(T, T, (0, 0, 6), (T - 2, 0, 2)))
    assert g.field.reached == int(free.sum())


def test_serpentine_over_three_by_three_tiles(ops):
    free = serpentine(3 * T, 3 * T)
    check(ops, free, seeds_at(3 * T, 3 * T, (0, 0, 6), (3 * T - 2, 0, 2)))


def test_spiral(ops):
    free = spiral(65)
    check(ops, free, seeds_at(65, 65, (0, 0, 11), (32, 32, 5)))


def test_a_diagonal_gap_is_not_crossed(ops):
    free = np.zeros((6, 6), np.uint8)
    free[:3, :3] = 1
    free[3:, 3:] = 1                                                             # the blocks touch only at the corner (2, 2) - (3, 3)
    g, _ = check(ops, free, seeds_at(6, 6, (0, 0, 4)))
    assert (g.owner[3:, 3:] == 0).all() and (g.owner[:3, :3] == 4).all()


def test_a_sealed_pocket_gets_zero(ops):
    free = np.ones((20, 20), np.uint8)
    free[5:12, 5] = free[5:12, 11] = free[5, 5:12] = free[11, 5:12] = 0
    g, _ = check(ops, free, seeds_at(20, 20, (0, 0, 3), (19, 19, 2)))
    assert (g.owner[6:11, 6:11] == 0).all() and (g.owner[free == 0] == 0).all()


def test_windows_and_device_inputs(ops):
    from avlmaps_amd.device import DeviceArray
    rng = np.random.default_rng(9)
    free = (rng.random((80, 90)) >= 0.3).astype(np.uint8)
    seeds = seeds_at(80, 90, (10, 12, 5), (50, 70, 2), (40, 40, 77), (3, 3, 9))
    win = (7, 71, 9, 83)
    r0, r1, c0, c1 = win
    owner, A, B = grow_ref(free[r0:r1, c0:c1], seeds[r0:r1, c0:c1])
    host = ops.grow_labels(free, seeds, window=win)
    assert np.array_equal(host.owner, owner) and np.array_equal(host.field.straight, A)
    dev = ops.grow_labels(DeviceArray.from_numpy(free), DeviceArray.from_numpy(seeds), device=True, window=win)
    assert isinstance(dev.owner, DeviceArray) and np.array_equal(dev.owner.numpy(), owner)
    assert np.array_equal(dev.field.straight.numpy(), A) and np.array_equal(dev.field.diagonal.numpy(), B)
    whole = ops.grow_labels(free.astype(bool), DeviceArray.from_numpy(seeds))
    assert np.array_equal(whole.owner, grow_ref(free, seeds)[0])


def test_the_same_input_twice_gives_the_same_bytes(ops):
    rng = np.random.default_rng(2)
    free = (rng.random((70, 100)) >= 0.25).astype(np.uint8)
    seeds = seeds_at(70, 100, (1, 1, 3), (60, 90, 2), (30, 50, 1))
    a, b = ops.grow_labels(free, seeds), ops.grow_labels(free, seeds)
    assert a.owner.tobytes() == b.owner.tobytes()


def test_no_seed_is_a_value_error(ops):
    from avlmaps_amd.device import DeviceArray
    free = np.ones((8, 9), np.uint8)
    with pytest.raises(ValueError, match="no seed"):
        ops.grow_labels(free, np.zeros((8, 9), np.int32))
    with pytest.raises(ValueError, match="no seed"):
        ops.grow_labels(free, DeviceArray.from_numpy(np.zeros((8, 9), np.int32)))
    with pytest.raises(ValueError, match="negative"):
        ops.grow_labels(free, DeviceArray.from_numpy(seeds_at(8, 9, (1, 1, -4), (2, 2, 3))))


# ------------------------------------------------------------------ segment_rooms
def check_rooms(ops, free, radius, least, name=""):
    want = rooms_ref(free, radius, least)
    got = ops.segment_rooms(free, radius, least)
    assert got.n == want["n"], (name, got.n, want["n"])
    assert got.labels.dtype == np.int32 and np.array_equal(got.labels, want["labels"]), name
    assert np.array_equal(got.seeds, want["seeds"]) and np.array_equal(got.clearance, want["clearance"]), name
    assert got.rooms.dtype == np.int64 and got.rooms.shape == (want["n"], 10) and np.array_equal(got.rooms, want["rooms"]), name
    assert got.doors.dtype == np.int64 and got.doors.shape == want["doors"].shape and np.array_equal(got.doors, want["doors"]), name
    return got, want


def test_three_rooms(ops):
    free = three_rooms()
    got, _ = check_rooms(ops, free, 4, 20)
    assert got.n == 3 and not ((got.labels == 0) & (free != 0)).any()
    assert got.doors[:, :3].tolist() == [[1, 2, 4], [2, 3, 4]]
    assert got.doors[:, 8].tolist() == [33, 66]
    dev = ops.segment_rooms(free, 4, 20, device=True)
    assert np.array_equal(dev.labels.numpy(), got.labels) and np.array_equal(dev.rooms, got.rooms) and np.array_equal(dev.doors, got.doors)


def test_a_dropped_seed_is_renumbered_away_and_its_room_absorbed(ops):
    free = three_rooms()
    free[:, 80:] = 0                                                             # the right room's core shrinks below the others'
    sizes = rooms_ref(free, 4, 1)["rooms"][:, 7]
    assert len(sizes) == 3 and sizes[2] < sizes[0] and sizes[2] < sizes[1]
    got, _ = check_rooms(ops, free, 4, int(sizes[2]) + 1)
    assert got.n == 2 and not ((got.labels == 0) & (free != 0)).any()
    free = three_rooms()
    free[:, :20] = 0                                                             # now the left one: the others move down by one
    sizes = rooms_ref(free, 4, 1)["rooms"][:, 7]
    assert sizes[0] < sizes[1] and sizes[0] < sizes[2]
    got, _ = check_rooms(ops, free, 4, int(sizes[0]) + 1)
    assert got.n == 2 and got.labels[35, 50] == 1 and got.labels[35, 80] == 2 and got.labels[35, 25] == 1


def test_no_room_at_all(ops):
    got, _ = check_rooms(ops, three_rooms(), 40, 1)
    assert got.n == 0 and not got.labels.any() and got.rooms.shape == (0, 10) and got.doors.shape == (0, 10) and got.field is None


def test_one_room_has_no_door(ops):
    free = np.ones((40, 45), np.uint8)
    free[0] = free[-1] = 0
    free[:, 0] = free[:, -1] = 0
    got, _ = check_rooms(ops, free, 3, 1)
    assert got.n == 1 and got.doors.shape == (0, 10)


def test_two_rooms_that_touch_along_two_doors(ops):
    free = np.ones((60, 70), np.uint8)
    free[:2] = free[-2:] = 0
    free[:, :2] = free[:, -2:] = 0
    free[:, 34:36] = 0
    free[10:13, 34:36] = 1
    free[45:49, 34:36] = 1
    got, _ = check_rooms(ops, free, 4, 10)
    assert got.n == 2 and len(got.doors) == 1
    i, j, contacts, rmin, rmax, cmin, cmax = got.doors[0, :7].tolist()
    assert (i, j, contacts) == (1, 2, 7) and rmin == 10 and rmax == 48 and cmin >= 33 and cmax <= 36


def test_a_map_without_an_obstacle_is_a_value_error(ops):
    with pytest.raises(ValueError, match="no zero cell"):
        ops.segment_rooms(np.ones((9, 9), np.uint8), 2)


def test_lift_labels_2d(ops):
    rng = np.random.default_rng(4)
    labels = rng.integers(0, 5, (30, 41)).astype(np.int32)
    pos = np.stack([rng.integers(90, 140, 500), rng.integers(190, 250, 500), rng.integers(0, 20, 500)], 1).astype(np.int32)
    want = np.zeros(500, np.int32)
    r, c = pos[:, 0] - 100, pos[:, 1] - 200
    inside = (r >= 0) & (r < 30) & (c >= 0) & (c < 41)
    want[inside] = labels[r[inside], c[inside]]
    assert inside.any() and not inside.all()
    got = ops.lift_labels_2d(labels, pos, (100, 200))
    assert got.dtype == np.int32 and np.array_equal(got, want)


# ------------------------------------------------------------------ the map layer
@pytest.fixture(scope="module")
def avmap(tmp_path_factory):
    """An AVLMap over a synthetic scene with its area map (the recipe of the travel tests' map), its voxels and features as built,
    whose obstacle crop is then replaced by walls alone: a border, and a wall two cells thick along the middle column with a door in
    rows 13 .. 15.  Three cells of door against a radius of two: the two sides are rooms 1 and 2."""
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map
    from avlmaps_amd.apps.common import HashAudioText, HashClip, HashImageEncoder, load_config
    from avlmaps_amd.map import AVLMap
    from avlmaps_amd.map.area_map import AreaMap
    tmp = tmp_path_factory.mktemp("rooms")
    sc = make(tmp / "scene", frames=8, H=96, W=128)
    cfg_path = tmp / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                       "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(sc), "--config", str(cfg_path), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    AreaMap().create_map(sc, image_encoder=HashImageEncoder())
    av = AVLMap(load_config(str(cfg_path)), data_dir=str(sc), area_text_model=HashClip(768), audio_text_model=HashAudioText())
    assert av.load_map(str(sc))
    vm = av.vlmap
    vm.clip_feat_dim = vm.grid_feat.shape[1]
    vm.clip_model = HashClip(vm.clip_feat_dim)
    vm.init_categories(CATS)
    vm.generate_obstacle_map()
    h, w = vm.obstacles_cropped.shape
    assert h >= 24 and w >= 24, (h, w)
    walls = np.ones((h, w), dtype=np.asarray(vm.obstacles_cropped).dtype)
    walls[0, :] = walls[h - 1, :] = walls[:, 0] = walls[:, w - 1] = 0
    walls[:, w // 2 - 1:w // 2 + 1] = 0
    walls[13:16, w // 2 - 1:w // 2 + 1] = 1
    vm.obstacles_cropped = walls
    return av


DOOR, CORE = 0.2, 0.01                                                           # metres: a radius of 2 cells, cores of 4 cells or more


def test_get_rooms_equals_segment_rooms_on_the_crop(ops, avmap):
    vm = avmap.vlmap
    free = np.asarray(vm.obstacles_cropped) != 0
    rooms = vm.get_rooms(DOOR, CORE)
    assert rooms.params["radius"] == DOOR / (2 * vm.cs) and rooms.params["min_seed_cells"] == int(np.ceil(CORE / vm.cs ** 2))
    seg = ops.segment_rooms(free, rooms.params["radius"], rooms.params["min_seed_cells"])
    ref = rooms_ref(free, rooms.params["radius"], rooms.params["min_seed_cells"])
    for got in (rooms.labels, seg.labels):
        assert np.array_equal(got, ref["labels"])
    assert np.array_equal(rooms.room_table, seg.rooms) and np.array_equal(rooms.room_table, ref["rooms"])
    assert np.array_equal(rooms.door_table, seg.doors) and np.array_equal(rooms.door_table, ref["doors"])
    assert rooms.n == 2 and rooms.window == (int(vm.rmin), int(vm.cmin)) and rooms.cs == vm.cs
    assert rooms.doors[:, :2].tolist() == [[1, 2]] and rooms.route(1, 2) == [1, 2]
    h, w = free.shape
    assert rooms.room_of([vm.rmin + h // 2, vm.cmin + 3]) == 1 and rooms.room_of([vm.rmin + h // 2, vm.cmin + w - 4]) == 2
    sealed = np.array(vm.obstacles_cropped, copy=True)
    sealed[13:16, w // 2 - 1:w // 2 + 1] = 0                                      # the customised map: the door is shut
    vm.obstacles_new_cropped = sealed
    try:
        shut = vm.get_rooms(DOOR, CORE, customized=True)
    finally:
        del vm.obstacles_new_cropped
    assert shut.n == 2 and shut.doors.shape == (0, 10) and shut.route(1, 2) is None and shut.neighbours(1) == []
    assert np.array_equal(shut.labels, rooms_ref(sealed != 0, shut.params["radius"], shut.params["min_seed_cells"])["labels"])


def test_get_voxel_rooms_equals_numpy_indexing(ops, avmap):
    from avlmaps_amd.device import DeviceArray
    vm = avmap.vlmap
    rooms = vm.get_rooms(DOOR, CORE)
    pos = np.asarray(vm.grid_pos)
    r, c = pos[:, 0] - rooms.window[0], pos[:, 1] - rooms.window[1]
    h, w = rooms.shape
    inside = (r >= 0) & (r < h) & (c >= 0) & (c < w)
    want = np.zeros(len(pos), np.int32)
    want[inside] = rooms.labels[r[inside], c[inside]]
    got = vm.get_voxel_rooms(rooms)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (want == 1).any() and (want == 2).any()
    dev = vm.get_voxel_rooms(rooms, device=True)
    assert isinstance(dev, DeviceArray) and np.array_equal(dev.numpy(), want)
    moved = type(rooms)(rooms.labels, rooms.room_table, rooms.door_table, None, (rooms.window[0] + 7, rooms.window[1] - 5), rooms.cs)
    r, c = pos[:, 0] - moved.window[0], pos[:, 1] - moved.window[1]
    inside = (r >= 0) & (r < h) & (c >= 0) & (c < w)
    want = np.zeros(len(pos), np.int32)
    want[inside] = rooms.labels[r[inside], c[inside]]
    assert not inside.all() and np.array_equal(vm.get_voxel_rooms(moved), want)           # voxels outside the crop: room 0


def test_assign_rooms_equals_a_bincount_vote(ops, avmap):
    vm = avmap.vlmap
    rooms = vm.get_rooms(DOOR, CORE)
    scene = vm.get_objects(min_voxels=3, exclude=())
    assert len(scene.objects) >= 2
    got = scene.assign_rooms(rooms)
    voxel_room = vm.get_voxel_rooms(rooms)
    labels = scene._host_labels()
    want = []
    for it in scene.objects:
        votes = np.bincount(voxel_room[labels == it.label], minlength=rooms.n + 1)[1:]
        want.append(int(np.argmax(votes)) + 1 if votes.max() > 0 else 0)
    assert got.dtype == np.int32 and got.tolist() == want
    assert len(set(want) - {0}) == 2                                             # objects on both sides of the wall
    for k in (0, 1, 2):
        assert [it.label for it in scene.in_room(k)] == [it.label for it, room in zip(scene.objects, want) if room == k]


def test_name_rooms_is_the_mean_frame_score(ops, avmap):
    """on the rooms of the map, and on a hand-made Rooms laid over the frames' own cells: three rooms side by side along the axis the
    camera moved most, the third without a frame of its own"""
    from avlmaps_amd.map import Rooms
    av = avmap
    names = ["kitchen", "bedroom", "corridor"]
    cells = np.clip(av.dataloader.habitat_tfs_to_cells(av.area_map.robot_pose_list), -1, np.iinfo(np.int32).max)
    scores = [np.asarray(av.area_map.index_map(name, with_init_cat=False)).reshape(-1) for name in names]
    assert len(cells) == len(scores[0]) >= 2
    lo, hi = cells.min(axis=0), cells.max(axis=0)
    axis = int(np.argmax(hi - lo))
    shape = hi - lo + 1 + np.array([0, 0])
    shape[axis] += 4                                                             # room 3: beyond the last frame
    labels = np.ones(tuple(int(v) for v in shape), np.int32)
    index = [slice(None), slice(None)]
    index[axis] = slice(int(hi[axis] - lo[axis]) // 2 + 1, None)
    labels[tuple(index)] = 2
    index[axis] = slice(int(hi[axis] - lo[axis]) + 1, None)
    labels[tuple(index)] = 3
    made = Rooms(labels, np.zeros((3, 10), np.int64), np.zeros((0, 10), np.int64), None, (int(lo[0]), int(lo[1])), av.vlmap.cs)
    seen = 0
    for rooms in (av.get_rooms(door_width=DOOR, min_core_area=CORE), made):
        got = av.name_rooms(names, rooms)
        want = []
        for k in range(1, rooms.n + 1):
            frames = [f for f, cell in enumerate(cells) if rooms.room_of(cell) == k]
            seen += len(frames)
            if not frames:
                want.append(None)
                assert np.isnan(av.room_scores[k - 1]).all()
                continue
            means = []
            for s in scores:
                total = 0.0
                for f in frames:
                    total += float(s[f])
                means.append(total / len(frames))
            assert av.room_scores[k - 1].tolist() == means
            want.append(names[int(np.argmax(means))])
        assert got == want and len(got) == rooms.n
    assert seen >= len(cells) and got[2] is None and got[0] is not None
    ids = [k + 1 for k, name in enumerate(got) if name == got[0]]
    assert np.array_equal(av.index_room_2d(got[0]), np.isin(made.labels, ids).astype(np.float64))
    voxel_room = av.vlmap.get_voxel_rooms(made)
    assert np.array_equal(av.index_room(got[0]), np.isin(voxel_room, ids).astype(np.float64))
    with pytest.raises(LookupError):
        av.index_room("pantry")


def test_index_room_and_the_goal_inside_a_room(ops, avmap):
    av = avmap
    vm = av.vlmap
    rooms = av.get_rooms(door_width=DOOR, min_core_area=CORE)
    voxel_room = vm.get_voxel_rooms(rooms)
    for k in (1, 2):
        heat = av.index_room(k)
        assert heat.dtype == np.float64 and np.array_equal(heat, (voxel_room == k).astype(np.float64))
        assert np.array_equal(av.index_room_2d(k), (rooms.labels == k).astype(np.float64))
        goal = av.index_goal(obj="table", extra=[heat], decay_rates={"obj": 0.001})
        want = av.index_object("table", decay_rate=0.001).astype(np.float64) * heat
        assert np.array_equal(goal.heat, want) and goal.voxel == int(np.argmax(want))
        assert goal.value > 0 and voxel_room[goal.voxel] == k and rooms.room_of(goal.cell) == k
    with pytest.raises(ValueError):
        av.index_room(3)
