"""The travel-distance field on the GPU (csrc/avl_travel.hip through ops.travel_field, TravelField, travel_decay_2d and their
users Map.get_travel_field / get_reachable_cropped, VLMap.get_travel_distribution_map and AVLMap.index_goal_2d_travel) against
the heap Dijkstra on integer pairs of tests/_travel_ref.py.

Every comparison is np.array_equal on both integer planes: the minimum over walks is unique (sqrt(2) is irrational) and the kernel
orders pairs exactly in integers.  The decay maps are NumPy's float64 expressions bit for bit.  T = ops.TRAVEL_TILE = 32 cells per
tile side and C = ops.TRAVEL_SWEEPS = 64 sweeps per tile and round are the kernel's constants (test_travel_host.py checks that the
source says the same)."""
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tools"))
sys.path.insert(0, str(HERE))
from _travel_ref import UNREACHED, check_walk, decay_ref, distance_ref, serpentine, spiral, travel_ref  # noqa: E402

T, C = 32, 64
CATS = ["sofa", "table", "lamp", "other"]


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    assert (ops.TRAVEL_TILE, ops.TRAVEL_SWEEPS) == (T, C)
    return ops


def one(H, W, *cells):
    m = np.zeros((H, W), np.uint8)
    for r, c in cells:
        m[r, c] = 1
    return m


def random_map(seed, H, W, density, n_sources):
    rng = np.random.default_rng(seed)
    free = (rng.random((H, W)) >= density).astype(np.uint8)
    src = np.zeros((H, W), np.uint8)
    src.ravel()[rng.choice(H * W, size=min(n_sources, H * W), replace=False)] = 1     # wherever they fall: some on obstacle cells
    return free, src


def check(ops, free, src, name=""):
    """both planes equal the reference; returns (field, A, B)"""
    A, B = travel_ref(free, src)
    f = ops.travel_field(free, src)
    assert f.straight.dtype == np.int32 and f.diagonal.dtype == np.int32 and f.shape == A.shape
    assert np.array_equal(f.straight, A), (name, int((f.straight != A).sum()))
    assert np.array_equal(f.diagonal, B), (name, int((f.diagonal != B).sum()))
    assert f.reached == int((A >= 0).sum()), name
    return f, A, B


# ------------------------------------------------------------------ shapes and the closed form
@pytest.mark.parametrize("shape", [(1, 1), (1, 45), (39, 1), (T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, 3 * T - 1)])
def test_shapes(ops, shape):
    H, W = shape
    free, src = random_map(H * 131 + W, H, W, 0.25, 2)
    free[src != 0] = 1
    check(ops, free, src, shape)
    check(ops, np.ones(shape, np.uint8), one(H, W, (H - 1, W // 2)), shape)


def test_empty_map_has_the_closed_form(ops):
    H, W = 2 * T + 5, 3 * T - 3
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for r0, c0 in ((0, 0), (H - 1, W - 1), (T - 1, T), (T, T - 1), (T, 2 * T), (H // 2, W // 2)):      # corners, tile borders, centre
        f = ops.travel_field(np.ones((H, W), np.uint8), one(H, W, (r0, c0)))
        dr, dc = np.abs(rr - r0), np.abs(cc - c0)
        assert np.array_equal(f.straight, np.abs(dr - dc)) and np.array_equal(f.diagonal, np.minimum(dr, dc)), (r0, c0)
        assert f.reached == H * W and f.rounds >= 1 and f.tile_runs >= f.rounds


# ------------------------------------------------------------------ the rule
def test_source_on_an_obstacle_cell(ops):
    free = np.ones((40, 44), np.uint8)
    free[10:20, 12:25] = 0
    f, A, B = check(ops, free, one(40, 44, (14, 18)), "buried")                  # no free neighbour: only the source is reached
    assert f.reached == 1 and (A[14, 18], B[14, 18]) == (0, 0)
    f, A, B = check(ops, free, one(40, 44, (10, 18)), "edge")                    # on the blob's edge: it steps onto the free row above
    assert (A[9, 18], B[9, 18]) == (1, 0) and A[10, 17] == UNREACHED and f.reached == 40 * 44 - 130 + 1
    # the diagonal step off a source obstacle: from the blob's corner both edge-sharing cells are free, from its edge one is not
    f, A, B = check(ops, free, one(40, 44, (10, 12)), "corner")
    assert (A[9, 11], B[9, 11]) == (0, 1)
    f, A, B = check(ops, free, one(40, 44, (10, 18)), "edge diagonal")
    assert (A[9, 17], B[9, 17]) == (2, 0)                                        # around, not across the corner of (10, 17)


def test_a_diagonal_gap_is_not_crossed(ops):
    free = np.ones((36, 36), np.uint8)
    for k in range(36):
        free[k, 35 - k] = 0                                                      # an anti-diagonal wall of cells that touch diagonally
    f, A, B = check(ops, free, one(36, 36, (3, 4)), "diagonal wall")
    assert A[35, 35] == UNREACHED and f.reached == 36 * 35 // 2
    free[17, 18] = 1                                                             # one wall cell missing: a way through
    f, A, B = check(ops, free, one(36, 36, (3, 4)), "diagonal wall with a door")
    assert A[35, 35] >= 0


def test_sealed_pockets(ops):
    free = np.ones((50, 70), np.uint8)
    free[20, 30:41] = free[30, 30:41] = 0
    free[20:31, 30] = free[20:31, 40] = 0                                        # a closed box around rows 21..29, cols 31..39
    f, A, B = check(ops, free, one(50, 70, (2, 3)), "outside")
    assert np.all(A[21:30, 31:40] == UNREACHED) and np.all(B[21:30, 31:40] == UNREACHED)
    f, A, B = check(ops, free, one(50, 70, (25, 35), (22, 38)), "inside only")
    assert f.reached == 81 and np.all(A[:20] == UNREACHED)


# ------------------------------------------------------------------ scheduling
def test_serpentine_inside_one_tile_longer_than_the_cap(ops):
    free = serpentine(T - 1, T)                                                  # one tile; the corridor is ~16 * 33 cells long
    f, A, B = check(ops, free, one(T - 1, T, (0, 0)), "serpentine in a tile")
    assert A.max() + B.max() > 4 * C and f.rounds > 4 and f.tile_runs == f.rounds


def test_serpentine_over_three_by_three_tiles(ops):
    free = serpentine(3 * T - 1, 3 * T - 2)                                      # every corridor row crosses all three tile columns
    f, A, B = check(ops, free, one(3 * T - 1, 3 * T - 2, (0, 0)), "serpentine over 3 x 3 tiles")
    assert A.max() > 40 * T
    free = serpentine(3 * T - 2, 3 * T - 1).T.copy()                             # and columnwise
    check(ops, free, one(3 * T - 1, 3 * T - 2, (3 * T - 2, 0)), "serpentine over 3 x 3 tiles, transposed")


def test_spiral(ops):
    n = 2 * T + 9
    free = spiral(n)
    f, A, B = check(ops, free, one(n, n, (0, 0)), "spiral inwards")
    assert f.reached == int(free.sum()) and A.max() > 10 * n
    centre = np.argwhere((A + B) == (A + B).max())[0]
    check(ops, free, one(n, n, tuple(centre)), "spiral outwards")


def test_two_fronts_meet_in_a_third_tile(ops):
    H, W = T + 7, 3 * T
    free = np.ones((H, W), np.uint8)
    free[5:H - 5, T + T // 2 - 3] = 0                                            # a partial wall inside the middle tile
    f, A, B = check(ops, free, one(H, W, (3, 2), (H - 4, 3 * T - 3)), "two fronts")
    assert f.reached == int(free.sum())


@pytest.mark.parametrize("density", [0.3, 0.45])
@pytest.mark.parametrize("n_sources", [1, 3, 50])
def test_random_maps(ops, density, n_sources):
    for seed in (1, 2, 3):
        H, W = 2 * T + 13 + seed, 3 * T - 7 - seed
        free, src = random_map(1000 * seed + n_sources + int(100 * density), H, W, density, n_sources)
        if n_sources == 1:
            free[max(0, np.argwhere(src)[0][0] - 1):np.argwhere(src)[0][0] + 2, :] |= (seed == 1)      # seed 1: the source can get out
        check(ops, free, src, (density, n_sources, seed))


def test_windows_and_device_inputs(ops):
    """a window of larger images (leading dimensions above W), a device-resident free map and source mask, (M, 2) cells"""
    from avlmaps_amd.device import DeviceArray
    big_free, big_src = random_map(17, 90, 101, 0.3, 40)
    r0, r1, c0, c1 = 7, 7 + T + 9, 11, 11 + 2 * T + 3
    free, src = big_free[r0:r1, c0:c1].copy(), big_src[r0:r1, c0:c1].copy()
    assert src.any()
    A, B = travel_ref(free, src)
    for f_in, s_in in ((big_free, big_src), (DeviceArray.from_numpy(big_free), DeviceArray.from_numpy(big_src))):
        f = ops.travel_field(f_in, s_in, window=(r0, r1, c0, c1))
        assert np.array_equal(f.straight, A) and np.array_equal(f.diagonal, B)
    f = ops.travel_field(big_free, np.argwhere(src), window=(r0, r1, c0, c1))    # cells are relative to the window
    assert np.array_equal(f.straight, A) and np.array_equal(f.diagonal, B)
    f = ops.travel_field(free != 0, np.argwhere(src).astype(np.int32), device=True)
    assert isinstance(f.straight, DeviceArray) and np.array_equal(f.straight.numpy(), A) and np.array_equal(f.diagonal.numpy(), B)
    assert np.array_equal(f.reachable(), A >= 0)
    with pytest.raises(ValueError, match="no source"):
        ops.travel_field(DeviceArray.from_numpy(free), DeviceArray.from_numpy(np.zeros_like(src)))
    with pytest.raises(ValueError, match="no source"):
        ops.travel_field(big_free, one(90, 101, (0, 0)), window=(r0, r1, c0, c1))


def test_the_same_input_twice_gives_the_same_planes(ops):
    free, src = random_map(23, 2 * T + 3, 2 * T + 5, 0.4, 5)
    a, b = ops.travel_field(free, src), ops.travel_field(free, src)
    assert np.array_equal(a.straight, b.straight) and np.array_equal(a.diagonal, b.diagonal) and a.reached == b.reached


# ------------------------------------------------------------------ distance and decay
def test_distance_and_decay_equal_numpy(ops):
    free, src = random_map(31, T + 11, 2 * T + 2, 0.3, 3)
    free[20:30, 40:50] = 1
    free[20, 40:50] = free[29, 40:50] = free[20:30, 40] = free[20:30, 49] = 0    # a pocket: unreached free cells
    src[20:30, 40:50] = 0                                                        # none in the pocket or on its walls
    for device in (False, True):
        f = ops.travel_field(free, src, device=device)
        A, B = travel_ref(free, src)
        assert (A[25, 45] == UNREACHED) and free[25, 45]
        d = f.distance()
        assert d.dtype == np.float64 and np.array_equal(d, distance_ref(A, B)) and np.isinf(d[25, 45])
        for rate in (0.1, 0.013):
            for cs in (1.0, 0.05):
                for normalize in (False, True):
                    got = ops.travel_decay_2d(f, rate, cell_size=cs, normalize=normalize)
                    want = decay_ref(A, B, rate, cs, normalize)
                    assert got.dtype == np.float64 and np.array_equal(got, want), (rate, cs, normalize, int((got != want).sum()))
        assert ops.travel_decay_2d(f, 0.0)[25, 45] == 0.0                          # unreached is 0 even without any decay
        dev = ops.travel_decay_2d(f, 0.1, normalize=True, device=True)
        assert np.array_equal(dev.numpy(), decay_ref(A, B, 0.1, 1.0, True))


def test_normalising_a_constant_map_is_a_value_error(ops):
    free = np.ones((6, 9), np.uint8)
    f = ops.travel_field(free, free)                                             # every cell a source: t = 1 everywhere
    assert np.array_equal(ops.travel_decay_2d(f, 0.1), np.ones((6, 9)))
    with pytest.raises(ValueError, match="constant"):
        ops.travel_decay_2d(f, 0.1, normalize=True)
    f = ops.travel_field(free, one(6, 9, (0, 0)))
    with pytest.raises(ValueError, match="constant"):
        ops.travel_decay_2d(f, 0.0, normalize=True)                              # no decay: 1 everywhere


def test_descend_on_device_fields(ops):
    for free, src in (random_map(41, 2 * T + 1, T + 9, 0.35, 4), (spiral(T + 5), one(T + 5, T + 5, (0, 0)))):
        f = ops.travel_field(free, src, device=True)
        A, B = f.planes()
        cells = np.argwhere(A >= 0)
        for r, c in cells[::max(1, len(cells) // 50)]:
            walk = f.descend((r, c))
            assert walk[0] == (r, c)
            check_walk(free, src, A, B, walk)                                    # legal steps, the start's pair, ends on a source
        unreached = np.argwhere(A < 0)
        if len(unreached):
            with pytest.raises(ValueError, match="not reached"):
                f.descend(tuple(unreached[0]))


# ------------------------------------------------------------------ the map layer
@pytest.fixture(scope="module")
def avmap(tmp_path_factory):
    """An AVLMap over a synthetic scene with its area and sound maps (the recipe of the 2-D goal tests), whose obstacle crop is then
    replaced by two_rooms() and whose voxels are preset: the "sofa" on its box in the left room, a "table" in the right room."""
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map
    from avlmaps_amd.apps.common import HashAudioText, HashClip, HashImageEncoder, load_config
    from avlmaps_amd.map import AVLMap
    from avlmaps_amd.map.area_map import AreaMap
    tmp = tmp_path_factory.mktemp("travel")
    sc = make(tmp / "scene", frames=8, H=96, W=128)
    cfg_path = tmp / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                       "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(sc), "--config", str(cfg_path), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    AreaMap().create_map(sc, image_encoder=HashImageEncoder())
    rng = np.random.default_rng(11)
    db = {i: {"audio_features": rng.standard_normal(1024).astype(np.float32),
              "locations": [np.array([rng.uniform(-1.5, 1.5), 0.0, rng.uniform(-1.5, 1.5)]) for _ in range(1 + i % 5)]}
          for i in range(14)}
    (sc / "audio_video").mkdir()
    (sc / "audio_video" / "audio_data_level_3.pkl").write_bytes(pickle.dumps(db))
    av = AVLMap(load_config(str(cfg_path)), data_dir=str(sc), area_text_model=HashClip(768), audio_text_model=HashAudioText())
    assert av.load_map(str(sc))
    vm = av.vlmap
    vm.clip_feat_dim = vm.grid_feat.shape[1]
    vm.clip_model = HashClip(vm.clip_feat_dim)
    vm.generate_obstacle_map()
    h, w = vm.obstacles_cropped.shape
    assert h >= 24 and w >= 24, (h, w)
    r0, c0 = int(vm.rmin), int(vm.cmin)
    rooms, wall, sofa_box = two_rooms(h, w, np.asarray(vm.obstacles_cropped).dtype)

    def block(ra, rb, ca, cb, heights):
        rr, cc, hh = np.meshgrid(np.arange(ra, rb), np.arange(ca, cb), np.asarray(heights), indexing="ij")
        return np.stack([rr.ravel(), cc.ravel(), hh.ravel()], 1)
    ra, rb, ca, cb = sofa_box
    sofa = [block(r0 + ra, r0 + rb, c0 + ca, c0 + cb, [3, 9])]
    table = [block(r0 + h // 2, r0 + h // 2 + 5, c0 + wall + 6, c0 + wall + 11, [5])]
    other = [block(r0, r0 + h, c0, c0 + w, [0])[::7]]
    pos = np.concatenate(sofa + table + other).astype(np.int32)
    label = np.concatenate([np.full(len(sofa[0]), 0), np.full(len(table[0]), 1), np.full(len(other[0]), 3)])
    order = rng.permutation(len(pos))
    pos, label = pos[order], label[order]
    scores = rng.random((len(pos), len(CATS))).astype(np.float32) * 0.5
    scores[np.arange(len(pos)), label] = 1.0
    scores[:, 2] = -1.0
    vm.grid_pos, vm.categories, vm.scores_mat = pos, list(CATS), scores
    vm.obstacles_cropped = rooms
    return av, wall, sofa_box


def two_rooms(h, w, dtype=np.uint8):
    """-> (free map, the wall's column, the sofa's box (r0, r1, c0, c1)): a border of obstacles, a wall one cell thick along the
    middle column with a door in rows 13 .. 15, a sofa of 10 x 6 cells in the LEFT room's top corner against the wall, and a table
    in the right room"""
    wall = w // 2
    rooms = np.ones((h, w), dtype=dtype)
    rooms[0, :] = rooms[h - 1, :] = rooms[:, 0] = rooms[:, w - 1] = 0
    rooms[:, wall] = 0
    rooms[13:16, wall] = 1
    box = (1, 11, wall - 6, wall)
    rooms[box[0]:box[1], box[2]:box[3]] = 0
    rooms[h // 2:h // 2 + 5, wall + 6:wall + 11] = 0
    return rooms, wall, box


def smoothed(ops, vm, name):
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(vm.get_predict_mask(name).astype(np.float32), sigma=1) > 0.5


def test_get_travel_distribution_map_equals_the_stand_alone_calls(ops, avmap):
    vm = avmap[0].vlmap
    free = np.asarray(vm.obstacles_cropped) != 0
    for name in ("sofa", "table"):
        mask = smoothed(ops, vm, name)
        assert np.array_equal(ops.mask_smooth_2d(vm.get_predict_mask(name), 1), mask)
        A, B = travel_ref(free, mask)
        for rate in (0.1, 0.01):
            got = vm.get_travel_distribution_map(name, decay_rate=rate)
            alone = ops.travel_decay_2d(ops.travel_field(free, mask), rate, normalize=True)
            assert got.dtype == np.float64 and got.shape == free.shape
            assert np.array_equal(got, alone) and np.array_equal(got, decay_ref(A, B, rate, 1.0, True)), (name, rate)
            assert got.max() == 1.0 and got.min() == 0.0
    with pytest.raises(ValueError, match="no target"):
        vm.get_travel_distribution_map("lamp")


def test_index_goal_2d_travel_equals_the_product_of_its_factors(ops, avmap):
    av = avmap[0]
    vm = av.vlmap
    win = (slice(int(vm.rmin), int(vm.rmax) + 1), slice(int(vm.cmin), int(vm.cmax) + 1))
    h, w = vm.obstacles_cropped.shape
    start = [int(vm.rmin) + h - 3, int(vm.cmin) + 3]

    def start_factor(rate):
        return ops.travel_decay_2d(vm.get_travel_field([start]), rate)
    combos = [
        (dict(obj="sofa"), lambda: [vm.get_travel_distribution_map("sofa", 0.1)]),
        (dict(obj="sofa", sound="dog"), lambda: [vm.get_travel_distribution_map("sofa", 0.1), av.index_sound_2d("dog")[win]]),
        (dict(obj=["sofa", ("table", 0.01)], area="kitchen"),
         lambda: [vm.get_travel_distribution_map("sofa", 0.1), vm.get_travel_distribution_map("table", 0.01), av.index_area_2d("kitchen")[win]]),
        (dict(obj="table", start=start), lambda: [vm.get_travel_distribution_map("table", 0.1), start_factor(0.01)]),
        (dict(obj="table", start=start, start_decay_rate=0.03), lambda: [vm.get_travel_distribution_map("table", 0.1), start_factor(0.03)]),
    ]
    for kwargs, parts in combos:
        parts = parts()
        want = parts[0].astype(np.float64)
        for p in parts[1:]:
            want = want * p.astype(np.float64)
        goal = av.index_goal_2d_travel(**kwargs)
        assert goal.heat.dtype == np.float64 and np.array_equal(goal.heat, want), kwargs
        r, c = np.unravel_index(np.argmax(want), want.shape)
        assert goal.cell.tolist() == [r + vm.rmin, c + vm.cmin] and goal.value == want[r, c]
        lean = av.index_goal_2d_travel(want_heat=False, **kwargs)
        assert lean.heat is None and lean.cell.tolist() == goal.cell.tolist() and lean.value == goal.value


def test_the_travel_goal_is_in_the_right_room(ops, avmap):
    """The sofa stands in the left room against the dividing wall; the robot stands in the right room, two cells from the wall and
    level with the sofa, and asks for the sofa near itself (decay 0.04 per cell).  By the straight line the best free cell is on
    the robot's side of the wall, two cells from the sofa and a walk through the door away from it; by the travel distance it is
    in the sofa's room."""
    av, wall, box = avmap
    vm = av.vlmap
    h, w = vm.obstacles_cropped.shape
    free = np.asarray(vm.obstacles_cropped) != 0
    me = (4, wall + 3)
    start = [int(vm.rmin) + me[0], int(vm.cmin) + me[1]]
    rr, cc = np.indices((h, w))
    near_me = 1.0 - np.hypot(rr - me[0], cc - me[1]) * 0.04
    near_me[near_me < 0] = 0
    euclid = vm.get_distribution_map("sofa", 0.1) * near_me * free
    er, ec = np.unravel_index(np.argmax(euclid), euclid.shape)
    assert ec > wall and euclid[er, ec] > 0                                       # the wrong room
    goal = av.index_goal_2d_travel(obj="sofa", start=start, start_decay_rate=0.04)
    heat = goal.heat * free                                                       # where the robot can stand
    gr, gc = np.unravel_index(np.argmax(heat), heat.shape)
    assert gc < wall and heat[gr, gc] > 0                                         # the right one
    d = vm.get_travel_field(smoothed(ops, vm, "sofa")).distance()
    assert d[gr, gc] <= 2.0 and d[er, ec] > 10.0                                  # beside the sofa / a walk through the door away
    raw = av.index_goal_2d_travel(obj="sofa", start=start, start_decay_rate=0.04, want_heat=False)
    assert int(raw.cell[1] - vm.cmin) < wall                                      # the unmasked goal cell is on the sofa's side as well


def test_get_reachable_cropped_equals_the_reference(ops, avmap):
    vm = avmap[0].vlmap
    saved = vm.obstacles_cropped
    h, w = saved.shape
    sealed = np.array(saved, copy=True)
    sealed[13:16, w // 2] = 0                                                     # close the door
    try:
        for rooms in (saved, sealed):
            vm.obstacles_cropped = rooms
            for cell in ((h - 3, 3), (5, w - 4), (12, w // 2)):                   # left room, right room, inside the wall
                pos = [float(vm.rmin + cell[0]) + 0.4, float(vm.cmin + cell[1]) + 0.7]
                A, _ = travel_ref(np.asarray(rooms) != 0, one(h, w, cell))
                got = vm.get_reachable_cropped(pos)
                assert got.dtype == bool and np.array_equal(got, A >= 0), cell
        left = vm.get_reachable_cropped([vm.rmin + h - 3, vm.cmin + 3])
        assert left[h - 3, 3] and not left[5, w - 4]                              # sealed: the other room is out of reach
    finally:
        vm.obstacles_cropped = saved
    with pytest.raises(ValueError, match="outside"):
        vm.get_travel_field([[vm.rmin - 1, vm.cmin]])
    f = vm.get_travel_field(one(h, w, (h - 3, 3)))
    assert np.array_equal(f.reachable(), vm.get_reachable_cropped([vm.rmin + h - 3, vm.cmin + 3]))
