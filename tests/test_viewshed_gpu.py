"""GPU tests of the 2-D viewshed (csrc/avl_viewshed.hip): ops.viewshed_gain and ops.viewshed_seen against the scalar
restatement of tests/_viewshed_ref.py with np.array_equal -- every output is an integer -- a cross-check of `seen` against the 3-D
line of sight on a one-layer voxel map, and Map.get_exploration_views / get_next_best_view / plan_exploration against the
restatement's candidate table and greedy tour.

The random maps have about 25 % obstacles and 50 % explored cells, so most sight lines end after a few cells; the hand-made map
(two rooms, a door, a few pillars) is the open one on which lines run the whole radius.  The reference of one (map, flag) is
computed once per eye and radius and shared by the tests that need it."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import _viewshed_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# 1, 2: windows smaller than a word; 31, 32, 33: the window width 2 R + 1 crosses the 64-bit ballot and the next 32-bit word; 127: the
# limit, every word of a 256-bit LDS row
RADII = (1, 2, 31, 32, 33, 127)


def _random_map(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.random((H, W)) > 0.25, rng.random((H, W)) > 0.5


def _rooms_map():
    """70 x 150: a walled hall cut in two by a wall at column 75 with a door (rows 33 .. 36), four pillars; the west room has been
    seen but for its south-west corner, the east room has not, and the door's own cells have"""
    H, W = 70, 150
    free = np.ones((H, W), bool)
    free[0, :] = free[-1, :] = free[:, 0] = free[:, -1] = False
    free[:, 75] = False
    free[33:37, 75] = True
    for r, c in ((20, 30), (50, 40), (15, 110), (45, 120)):
        free[r:r + 3, c:c + 3] = False
    explored = np.zeros((H, W), bool)
    explored[:, :76] = True
    explored[50:, :25] = False
    return free, explored


MAPS = {"tiny": _random_map(5, 5, 1), "wide": _random_map(70, 150, 2), "odd": _random_map(129, 131, 3), "rooms": _rooms_map()}
_CACHES = {}


def _cache(name, ou):
    return _CACHES.setdefault((name, ou), {})


def _eyes(name):
    """(E, 2) int32: the four corners, the mid-edge cells, an opaque cell, an unknown cell, a known-free cell, a duplicate and two
    eyes outside the image"""
    free, explored = MAPS[name]
    H, W = free.shape
    opaque = np.argwhere(~free)[len(np.argwhere(~free)) // 2]
    unknown = np.argwhere(free & ~explored)[len(np.argwhere(free & ~explored)) // 2]
    known = (10, 3) if name == "rooms" else np.argwhere(free & explored)[len(np.argwhere(free & explored)) // 3]
    eyes = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), tuple(opaque),
            tuple(unknown), tuple(known), (0, 0), (-1, 3), (H // 2, W)]
    return np.array(eyes, np.int32)


def test_the_maps_contain_their_cases():
    for name, (free, explored) in MAPS.items():
        assert free.dtype == explored.dtype == np.dtype(bool) and free.shape == explored.shape
        eyes = _eyes(name)
        H, W = free.shape
        inside = [(r, c) for r, c in eyes.tolist() if 0 <= r < H and 0 <= c < W]
        assert len(inside) == len(eyes) - 2 and len(set(inside)) < len(inside)                  # two outside, one twice
        assert any(not free[r, c] for r, c in inside) and any(free[r, c] and not explored[r, c] for r, c in inside)
    for name in ("wide", "odd"):
        free, explored = MAPS[name]
        assert 0.2 < 1 - free.mean() < 0.3 and 0.45 < explored.mean() < 0.55
    # on the open map lines do run far: the known cell sees along more than 64 cells, some of them through the door
    free, explored = MAPS["rooms"]
    eye = _eyes("rooms")[10]
    far = [t for t in R._visible(_cache("rooms", False), R.classes(free, explored)[0], 70, 150, eye, 127)
           if max(abs(t[0] - eye[0]), abs(t[1] - eye[1])) > 64]
    assert len(far) > 200 and any(t[1] > 76 for t in far)


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("radius", RADII)
def test_gain_and_seen_equal_the_restatement(name, radius):
    from avlmaps_amd import ops
    free, explored = MAPS[name]
    eyes = _eyes(name)
    for ou in (False, True):
        cache = _cache(name, ou)
        want = R.gain_ref(free, explored, eyes, radius, ou, cache)
        got = ops.viewshed_gain(free, explored, eyes, radius, opaque_unknown=ou)
        assert got.dtype == np.int32 and got.shape == (len(eyes), 8)
        assert np.array_equal(got, want), (name, radius, ou, np.argwhere(got != want)[:5])
        outside = (eyes[:, 0] < 0) | (eyes[:, 0] >= free.shape[0]) | (eyes[:, 1] < 0) | (eyes[:, 1] >= free.shape[1])
        assert outside.sum() == 2 and (want[outside] == -1).all() and (want[~outside] >= 0).all()
        seen_want = R.seen_ref(free, explored, eyes, radius, ou, cache=cache)
        seen = ops.viewshed_seen(free, explored, eyes, radius, opaque_unknown=ou)
        assert seen.dtype == np.uint8 and seen.shape == free.shape and set(np.unique(seen)) <= {0, 1}
        assert np.array_equal(seen, seen_want), (name, radius, ou, np.argwhere(seen != seen_want)[:5])
        # an eye's gains add up to the unknown cells under its own seen mask
        unknown = free & ~explored
        for e in (2, 9, len(eyes) - 1):
            own = ops.viewshed_seen(free, explored, eyes[e:e + 1], radius, opaque_unknown=ou)
            inside = 0 <= eyes[e, 0] < free.shape[0] and 0 <= eyes[e, 1] < free.shape[1]
            if inside:
                own[eyes[e, 0], eyes[e, 1]] = 0             # the eye's own cell is seen, but is no target
                assert int(got[e].sum()) == int(np.count_nonzero(own[unknown]))
            else:
                assert not own.any() and (got[e] == -1).all()


def test_eye_counts_inputs_and_a_second_run():
    import torch
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    free, explored = MAPS["wide"]
    H, W = free.shape
    rng = np.random.default_rng(7)
    many = np.stack([rng.integers(-2, H + 2, 300), rng.integers(-2, W + 2, 300)], axis=1).astype(np.int32)
    cache = _cache("wide", False)
    want = R.gain_ref(free, explored, many, 2, False, cache)
    assert (want[:, 0] == -1).any() and (want.sum(1) > 0).any()
    for E in (0, 1, 300):
        got = ops.viewshed_gain(free, explored, many[:E], 2)
        assert got.shape == (E, 8) and np.array_equal(got, want[:E])
    # bool, uint8, host and device inputs; a list of eyes; device results; the same bytes on a second run
    f8, x8 = free.astype(np.uint8), explored.astype(np.uint8) * 255            # any nonzero byte is true
    dev = ops.viewshed_gain(DeviceArray.from_numpy(f8), DeviceArray.from_numpy(x8), DeviceArray.from_numpy(many), 2, device=True)
    assert isinstance(dev, DeviceArray) and np.array_equal(dev.numpy(), want)
    assert np.array_equal(ops.viewshed_gain(f8, explored, many.astype(np.int64).tolist(), 2), want)
    got = ops.viewshed_gain(torch.from_numpy(free).cuda(), torch.from_numpy(x8).cuda(), torch.from_numpy(many).cuda(), 2)
    assert np.array_equal(got, want)
    eyes = _eyes("wide")
    first = ops.viewshed_gain(free, explored, eyes, 33)
    assert first.tobytes() == ops.viewshed_gain(free, explored, eyes, 33).tobytes()
    with pytest.raises(TypeError):
        ops.viewshed_gain(free, explored, DeviceArray.from_numpy(many.astype(np.int64)), 2)

    # seen: M = 0, 1 and 17 eyes; out= ORs into what is there, on the host and on the device
    seventeen = many[want[:, 0] >= 0][:17]
    assert len(seventeen) == 17
    assert not ops.viewshed_seen(free, explored, np.zeros((0, 2), np.int32), 33).any()
    for M in (1, 17):
        assert np.array_equal(ops.viewshed_seen(f8, x8, seventeen[:M], 2), R.seen_ref(free, explored, seventeen[:M], 2, cache=cache))
    before = (rng.random((H, W)) > 0.9).astype(np.uint8)
    want_or = R.seen_ref(free, explored, seventeen, 2, out=before, cache=cache)
    assert (want_or >= before).all() and (want_or != before).any() and (want_or != R.seen_ref(free, explored, seventeen, 2, cache=cache)).any()
    mine = before.copy()
    assert ops.viewshed_seen(free, explored, seventeen, 2, out=mine) is mine and np.array_equal(mine, want_or)
    dmask = DeviceArray.from_numpy(before)
    assert ops.viewshed_seen(free, explored, seventeen, 2, out=dmask, device=True) is dmask and np.array_equal(dmask.numpy(), want_or)
    assert np.array_equal(ops.viewshed_seen(free, explored, np.zeros((0, 2), np.int32), 2, out=before.copy()), before)
    second = ops.viewshed_seen(free, explored, eyes, 33)
    assert second.tobytes() == ops.viewshed_seen(free, explored, eyes, 33).tobytes()


def test_seen_agrees_with_the_3d_line_of_sight_on_a_one_layer_voxel_map():
    """the voxels of a map with one height layer (vh = 1, which ops.cell_index takes) are the opaque cells of the west room of the
    hand-made map: the 3-D walk without a height difference is the 2-D walk, so line_of_sight tells the same as seen on every
    cell in range"""
    from avlmaps_amd import ops
    free, explored = MAPS["rooms"][0][:, :70], MAPS["rooms"][1][:, :70]          # a square image: the voxel grid is gs x gs
    gs, radius = 70, 33
    eye = np.array([34, 40], np.int32)
    assert free[eye[0], eye[1]]
    pos = np.concatenate([np.argwhere(~free), np.zeros((int((~free).sum()), 1), np.int64)], axis=1).astype(np.int32)
    rr, cc = np.mgrid[0:gs, 0:gs]
    in_range = ((rr - eye[0]) ** 2 + (cc - eye[1]) ** 2 <= radius * radius) & ((rr != eye[0]) | (cc != eye[1]))
    targets = np.stack([rr[in_range], cc[in_range], np.zeros(int(in_range.sum()), np.int64)], axis=1).astype(np.int32)
    eyes3 = np.broadcast_to(np.array([eye[0], eye[1], 0], np.int32), targets.shape).copy()
    with ops.cell_index(pos, gs, 1) as index:
        los = ops.line_of_sight(index, eyes3, targets)
    seen = ops.viewshed_seen(free, explored, eye.reshape(1, 2), radius)
    assert np.array_equal(seen[in_range] != 0, los == ops.LOS_VISIBLE)
    assert 0.5 < (los == ops.LOS_VISIBLE).mean() < 1.0                              # the pillars and the walls hide something
    assert seen[eye[0], eye[1]] == 1 and not seen[~in_range & ((rr != eye[0]) | (cc != eye[1]))].any()


# ---------------------------------------------------------------------------------------------------------------- the Map layer
GS, CS = 48, 0.25


def _config():
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": GS, "map_config.cell_size": CS}).map_config


def _hall(seen_all=False):
    """a Map without a scene directory, as tests/test_explore_gpu.py builds its own: a 40 x 40 walled hall with a walled inner room
    that has a door to the west and one to the east; the hall around the room has been seen, the inside of the room has not"""
    from avlmaps_amd.map import VLMap
    occupied = -np.ones((GS, GS, 6), np.int32)
    wall = np.zeros((GS, GS), bool)
    wall[4, 4:44] = wall[43, 4:44] = wall[4:44, 4] = wall[4:44, 43] = True
    wall[14, 14:34] = wall[33, 14:34] = wall[14:34, 14] = wall[14:34, 33] = True
    wall[21:27, 14] = wall[21:27, 33] = False
    occupied[wall, 2] = 1 + np.arange(wall.sum())
    seen = np.zeros((GS, GS), bool)
    seen[5:43, 5:43] = True
    if seen_all:
        seen[:] = True
    else:
        seen[15:33, 15:33] = False
    vm = VLMap(_config())
    vm.occupied_ids = occupied
    vm.first_seen = np.where(seen, 3, -1).astype(np.int32)
    vm.generate_obstacle_map()
    return vm


def test_exploration_views_next_best_view_and_the_tour_equal_the_restatement():
    from avlmaps_amd import ops
    from avlmaps_amd.navigator import Navigator
    vm = _hall()
    before = vm.first_seen.copy()
    rmin, cmin = int(vm.rmin), int(vm.cmin)
    free, explored = np.asarray(vm.get_obstacle_cropped()) != 0, vm.get_explored_cropped().copy()
    start = [24.0, 8.0]
    pos = (24 - rmin, 8 - cmin)
    radius = int(2.0 / CS)
    views = vm.get_exploration_views(start, max_range=2.0)
    want = R.views_ref(free, explored, pos, radius)
    assert len(views) == len(want["cells"]) > 20 and views.radius == radius == 8
    assert np.array_equal(views.cells, want["cells"] + (rmin, cmin)) and np.array_equal(views.gain, want["gain"])
    assert np.array_equal(views.total, want["total"]) and np.array_equal(views.heading, want["heading"])
    assert np.array_equal(views.distance, want["distance"]) and views.distance.min() >= 0
    assert views.total.max() > 0 and (views.total == 0).any()
    assert views.select().tolist() == R.select_ref(want["total"])
    # without a position every candidate stays, the ones inside the unseen room's doorways included
    everywhere = vm.get_exploration_views(max_range=2.0)
    assert len(everywhere) >= len(views) and (everywhere.distance == -1).all()
    assert np.array_equal(everywhere.cells, R.views_ref(free, explored, None, radius)["cells"] + (rmin, cmin))
    # the next best view, with the field's walk and with a navigator's path
    k = R.next_view_ref(want)
    cell = [int(v) for v in want["cells"][k] + (rmin, cmin)]
    goal, heading, gain, path = vm.get_next_best_view(start, max_range=2.0)
    assert (goal, heading, gain) == (cell, int(want["heading"][k]), int(want["total"][k])) and gain > 0
    assert path[0] == [24, 8] and path[-1] == goal and all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(path[:-1], path[1:]))
    nav = Navigator()
    try:
        nav.build_visgraph(vm.get_known_free_cropped(), vm.rmin, vm.cmin)
        goal2, heading2, gain2, path2 = vm.get_next_best_view(start, navigator=nav, max_range=2.0)
        assert (goal2, heading2, gain2) == (goal, heading, gain)
        assert path2[0] == start and [int(path2[-1][0]), int(path2[-1][1])] == goal
        i, path3 = nav.plan_to_next_best_view(start, views)
        assert i in views.select().tolist() and [int(path3[-1][0]), int(path3[-1][1])] == views.cells[i].tolist()
    finally:
        nav.close()
    # the greedy tour; the conservative one too
    for ou in (False, True):
        tour = vm.plan_exploration(start, k=3, max_range=2.0, opaque_unknown=ou)
        want_tour, explored_after = R.tour_ref(free, explored, pos, radius, 3, opaque_unknown=ou)
        assert [(t[0], t[1], t[2]) for t in tour] == [([c[0] + rmin, c[1] + cmin], h, g) for c, h, g in want_tour]
        assert len(tour) == 3 and all(t[2] > 0 for t in tour) and tour[0][3][0] == [24, 8] and tour[1][3][0] == tour[0][0]
    # the gain of a fixed cell never grows along the (optimistic) tour: what is explored stays explored
    tour = vm.plan_exploration(start, k=3, max_range=2.0)
    fixed = (views.cells[views.best()] - (rmin, cmin)).astype(np.int32).reshape(1, 2)
    known, gains = explored.copy(), []
    for cell, _, _, _ in tour:
        gains.append(int(ops.viewshed_gain(free, known, fixed, radius).sum()))
        known |= ops.viewshed_seen(free, known, np.array([[cell[0] - rmin, cell[1] - cmin]], np.int32), radius) != 0
    gains.append(int(ops.viewshed_gain(free, known, fixed, radius).sum()))
    assert gains == sorted(gains, reverse=True) and gains[0] > gains[-1]
    assert np.array_equal(vm.first_seen, before) and np.array_equal(vm.get_explored_cropped(), explored)
    # limits of the range
    with pytest.raises(ValueError, match="31.75 m"):
        vm.get_exploration_views(start, max_range=32.0)
    with pytest.raises(ValueError):
        vm.get_exploration_views(start, max_range=0.2)


def test_a_fully_explored_map_returns_the_start():
    vm = _hall(seen_all=True)
    start = [24.0, 8.0]
    assert vm.get_next_best_view(start, max_range=2.0) == (start, None, 0, [start])
    assert vm.plan_exploration(start, k=3, max_range=2.0) == []
    views = vm.get_exploration_views(start, max_range=2.0)
    assert len(views) > 20 and not views.total.any() and views.best() is None


def test_plan_path_goes_to_the_next_best_view(tmp_path):
    """apps.plan_path --goal nbv on the hall, saved as a scene: the goal, its gain and the tour are Map.plan_exploration's, the path
    is the navigator's on the known-free map, --render tints what the first view would see"""
    import yaml
    from PIL import Image
    from avlmaps_amd.apps import plan_path
    from avlmaps_amd.utils.mapping_utils import save_3d_map
    vm = _hall()
    occupied = vm.occupied_ids.copy()
    pos = np.argwhere(occupied > 0).astype(np.int32)
    pos = pos[np.argsort(occupied[pos[:, 0], pos[:, 1], pos[:, 2]])]
    occupied[occupied > 0] -= 1                                           # ids = rows of grid_pos; the wall cell with id 0 does not count upstream
    sc = tmp_path / "scene"
    (sc / "vlmap").mkdir(parents=True)
    save_3d_map(sc / "vlmap" / "vlmaps.h5df", np.zeros((len(pos), 8), np.float32), pos, np.ones(len(pos), np.float32), occupied, [0],
                np.full((len(pos), 3), 200, np.uint8))
    np.savez_compressed(sc / "vlmap" / "explored.npz", first_seen=vm.first_seen, gs=GS, cs=CS, stride=4, h_min=0.0, h_max=1.5,
                        min_depth=0.1, max_depth=6.0, n_frames=1)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"grid_size": GS, "cell_size": CS}, "params": {"gs": GS, "cs": CS}}))
    base = ["--data-dir", str(sc), "--config", str(cfg), "--text-model", "hash", "--start", "24", "8", "--goal", "nbv"]
    out = plan_path.main(base + ["--view-range", "2.0", "--nbv-count", "2", "--render", str(tmp_path / "n.png")])
    loaded = _hall()
    loaded.occupied_ids = occupied                                        # the map the app planned on: without the wall cell of id 0
    loaded.generate_obstacle_map()
    tour = loaded.plan_exploration([24.0, 8.0], k=2, max_range=2.0)
    assert out["goal_kind"] == "nbv" and out["goal"] == [float(v) for v in tour[0][0]] and out["gain"] == tour[0][2] > 0
    assert out["heading_octant"] == tour[0][1] and [v["gain"] for v in out["views"]] == [t[2] for t in tour] and len(tour) == 2
    assert out["path"][0] == [24.0, 8.0] and out["path"][-1] == out["goal"]
    img = np.asarray(Image.open(tmp_path / "n.png"))
    assert img.shape[2] == 3 and tuple(img[24 - int(loaded.rmin), 8 - int(loaded.cmin)]) == (0, 255, 0)
    for bad in (["--query", "door"], ["--view-fraction", "0.5"], ["--nbv-count", "0"]):
        with pytest.raises(SystemExit):
            plan_path.main(base + bad)
    with pytest.raises(SystemExit):
        plan_path.main(base[:-2] + ["--goal", "frontier", "--nbv-conservative"])
