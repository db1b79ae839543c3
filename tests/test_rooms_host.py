"""Rooms and doorways without a GPU: the C ABI of csrc/avl_rooms.hip (declared, exported, bound, every argument refused before any
device work), the Python surface and its checks, Rooms (route, save, load), the tie rule of SceneObjects.assign_rooms, the apps'
flags, and the reference itself (tests/_rooms_ref.py): its heap Dijkstra against the tight-predecessor fixed point."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
from _rooms_ref import door_table_ref, grow_ref, rooms_ref, route_ref, three_rooms, tight_fixed_point  # noqa: E402
from _travel_ref import travel_ref  # noqa: E402

SYMBOLS = ("avl_grow_labels_workspace_bytes", "avl_grow_labels", "avl_room_seeds_workspace_bytes", "avl_room_seeds", "avl_room_table",
           "avl_room_doors_workspace_bytes", "avl_room_doors", "avl_room_door_table", "avl_lift_labels_2d")


@pytest.fixture(scope="module")
def lib():
    from avlmaps_amd.build import build
    build()
    from avlmaps_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.avl_last_error().decode()


# ------------------------------------------------------------------ the reference
def test_the_dijkstra_equals_the_tight_predecessor_fixed_point():
    rng = np.random.default_rng(7)
    for trial in range(30):
        H, W = (int(v) for v in rng.integers(3, 19, 2))
        free = (rng.random((H, W)) >= rng.choice([0.2, 0.35])).astype(np.uint8)
        seeds = np.zeros((H, W), np.int32)
        at = rng.choice(H * W, size=int(rng.integers(1, 6)), replace=False)                     # wherever they fall: some on obstacle cells
        seeds.ravel()[at] = rng.choice(np.array([1, 2, 3, 50, 2 ** 31 - 1]), size=len(at), replace=False)
        owner, A, B = grow_ref(free, seeds)
        A2, B2 = travel_ref(free, seeds > 0)
        assert np.array_equal(A, A2) and np.array_equal(B, B2), trial
        assert np.array_equal(owner, tight_fixed_point(free, seeds, A, B)), trial
        assert np.array_equal(owner[seeds > 0], seeds[seeds > 0]) and not owner[A < 0].any()
        assert set(np.unique(owner)) <= set(np.unique(seeds))


def test_the_three_room_map_of_the_reference():
    free = three_rooms()
    ref = rooms_ref(free, 4, 20)
    assert ref["n"] == 3 and not ((ref["labels"] == 0) & (free != 0)).any()
    assert ref["doors"][:, :3].tolist() == [[1, 2, 4], [2, 3, 4]] and ref["doors"][:, 8].tolist() == [33, 66]
    assert ref["rooms"][:, 0].sum() == int(free.sum())
    both = np.tile(np.array([[1, 2]], np.int32), (3, 1))
    E = np.array([[1.0, 1.0], [2.0, 2.0], [2.0, 1.0]])
    assert door_table_ref(both, E).tolist() == [[1, 2, 3, 0, 2, 0, 1, 1, 0, 0]]                # the first of the largest clearance


# ------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_bound(lib):
    from avlmaps_amd import _lib
    from avlmaps_amd.build import SOURCES
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert re.search(rf"AVL_API\s+int\s+{name}\s*\(", text), name
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS, name
    assert SOURCES["avl_rooms.hip"] == ["-ffp-contract=off"]


def test_the_tile_scheme_is_shared_not_copied():
    """one legal-step rule, one mark, one round loop for the distance field and the label growth: both sources include the header,
    neither defines the pieces itself; the label kernel uses the travel kernel's tiles and never packs a label into the state"""
    from avlmaps_amd import ops
    csrc = ROOT / "avlmaps_amd" / "csrc"
    head = (csrc / "avl_travel_tile.h").read_text()
    for piece in ("travel_legal_in", "travel_mark(", "travel_dr(", "travel_dc(", "travel_halo_readers", "travel_run_rounds"):
        assert piece in head, piece
    for name in ("avl_travel.hip", "avl_rooms.hip"):
        src = (csrc / name).read_text()
        assert '#include "avl_travel_tile.h"' in src and "travel_legal_in<" in src and "travel_run_rounds(" in src, name
        assert "int travel_dr(" not in src and "void travel_mark(" not in src, name
    src = (csrc / "avl_rooms.hip").read_text()
    assert f"constexpr int kTravelTile = {ops.TRAVEL_TILE};" in head and f"constexpr int kTravelSweeps = {ops.TRAVEL_SWEEPS};" in head
    assert not re.search(r"constexpr int k(Travel|Cost|Many|Grow)(Tile|Threads|Cells|Sweeps|Halo|MaxSide)\b", src)
    assert "travel_take_mark(" in src and "travel_wake(" in src                      # the round's prologue and epilogue are the header's
    assert "avl_travel2d(" in src                                                   # phase 1 is the existing entry point


def test_arguments_are_refused_before_any_device_work(lib):
    """every pointer below is fake and must never be dereferenced"""
    n = C.c_size_t(77)
    assert lib.avl_grow_labels_workspace_bytes(10, 10, None) != 0 and "null" in _err(lib)
    assert lib.avl_room_seeds_workspace_bytes(10, 10, None) != 0 and "null" in _err(lib)
    assert lib.avl_room_doors_workspace_bytes(10, None) != 0 and "null" in _err(lib)
    for H, W in ((16385, 4), (4, 16385), (0, 4), (4, -1)):
        assert lib.avl_grow_labels_workspace_bytes(H, W, C.byref(n)) != 0 and "bad shape" in _err(lib) and n.value == 77
        assert lib.avl_room_seeds_workspace_bytes(H, W, C.byref(n)) != 0 and "bad shape" in _err(lib) and n.value == 77
        assert lib.avl_grow_labels(0x1000, W, 0x2000, W, H, W, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 1 << 40, None) != 0
        assert "bad shape" in _err(lib)
        assert lib.avl_room_seeds(0x1000, H, W, 2.0, 1, 0x2000, 0x3000, 0x4000, 1 << 40, None) != 0 and "bad shape" in _err(lib)
        assert lib.avl_room_table(0x1000, 0x2000, 0x3000, H, W, 3, 0x4000, None) != 0 and "bad shape" in _err(lib)
        assert lib.avl_room_doors(0x1000, 0x2000, H, W, 3, 0x3000, 0x4000, 1 << 40, None) != 0 and "bad shape" in _err(lib)
        assert lib.avl_lift_labels_2d(0x1000, H, W, 0x2000, 5, 0, 0, 0x3000, None) != 0 and "bad shape" in _err(lib)
    assert lib.avl_grow_labels_workspace_bytes(16384, 16384, C.byref(n)) == 0 and n.value >= 23 * 16384 * 16384
    assert lib.avl_grow_labels_workspace_bytes(100, 30, C.byref(n)) == 0 and n.value >= 23 * 100 * 30
    ok = dict(free=0x1000, ldf=30, seeds=0x2000, lds=30, H=100, W=30, a=0x3000, b=0x4000, owner=0x5000, stats=0x6000, ws=0x7000, n=n.value)

    def grow(**kw):
        a = dict(ok, **kw)
        rc = lib.avl_grow_labels(a["free"], a["ldf"], a["seeds"], a["lds"], a["H"], a["W"], a["a"], a["b"], a["owner"], a["stats"], a["ws"],
                                 a["n"], None)
        return rc, _err(lib)
    for kw, word in ((dict(free=None), "null"), (dict(seeds=None), "null"), (dict(a=None), "null"), (dict(b=None), "null"),
                     (dict(owner=None), "null"), (dict(stats=None), "null"), (dict(ldf=29), "free rows of 29"),
                     (dict(lds=7), "seed rows of 7"), (dict(ws=None), "workspace"), (dict(n=n.value - 1), "workspace")):
        rc, msg = grow(**kw)
        assert rc != 0 and word in msg, (kw, msg)

    assert lib.avl_room_seeds_workspace_bytes(100, 30, C.byref(n)) == 0 and n.value >= 100 * 30
    for args, word in (((None, 100, 30, 2.0, 1, 0x2000, 0x3000, 0x4000, n.value), "null"),
                       ((0x1000, 100, 30, 2.0, 1, None, 0x3000, 0x4000, n.value), "null"),
                       ((0x1000, 100, 30, 2.0, 1, 0x2000, None, 0x4000, n.value), "null"),
                       ((0x1000, 100, 30, -1.0, 1, 0x2000, 0x3000, 0x4000, n.value), "radius"),
                       ((0x1000, 100, 30, float("nan"), 1, 0x2000, 0x3000, 0x4000, n.value), "radius"),
                       ((0x1000, 100, 30, 2.0, 0, 0x2000, 0x3000, 0x4000, n.value), "min_seed_cells"),
                       ((0x1000, 100, 30, 2.0, 1, 0x2000, 0x3000, None, n.value), "workspace"),
                       ((0x1000, 100, 30, 2.0, 1, 0x2000, 0x3000, 0x4000, n.value - 1), "workspace")):
        assert lib.avl_room_seeds(*args, None) != 0 and word in _err(lib), (args, _err(lib))

    for args, word in (((None, 0x2000, 0x3000, 10, 10, 3, 0x4000), "null"), ((0x1000, None, 0x3000, 10, 10, 3, 0x4000), "null"),
                       ((0x1000, 0x2000, None, 10, 10, 3, 0x4000), "null"), ((0x1000, 0x2000, 0x3000, 10, 10, 3, None), "null"),
                       ((0x1000, 0x2000, 0x3000, 10, 10, -1, 0x4000), "rooms"), ((0x1000, 0x2000, 0x3000, 10, 10, (1 << 24) + 1, 0x4000), "rooms")):
        assert lib.avl_room_table(*args, None) != 0 and word in _err(lib), (args, _err(lib))
    assert lib.avl_room_table(None, None, None, 10, 10, 0, None, None) == 0                    # no room: nothing to do

    assert lib.avl_room_doors_workspace_bytes(-1, C.byref(n)) != 0 and "rooms" in _err(lib)
    assert lib.avl_room_doors_workspace_bytes(3, C.byref(n)) == 0 and n.value >= 64 * (8 + 8 + 56 + 4 + 4)
    for args, word in (((None, 0x2000, 10, 10, 3, 0x3000, 0x4000, n.value), "null"), ((0x1000, None, 10, 10, 3, 0x3000, 0x4000, n.value), "null"),
                       ((0x1000, 0x2000, 10, 10, 3, None, 0x4000, n.value), "null"), ((0x1000, 0x2000, 10, 10, -2, 0x3000, 0x4000, n.value), "rooms"),
                       ((0x1000, 0x2000, 10, 10, 3, 0x3000, None, n.value), "workspace"),
                       ((0x1000, 0x2000, 10, 10, 3, 0x3000, 0x4000, n.value - 1), "workspace")):
        assert lib.avl_room_doors(*args, None) != 0 and word in _err(lib), (args, _err(lib))
    for args, word in (((0x1000, n.value, 3, 10, 65, 0x2000), "pairs"), ((0x1000, n.value, 3, 10, -1, 0x2000), "pairs"),
                       ((0x1000, n.value, 3, 0, 2, 0x2000), "width"), ((None, n.value, 3, 10, 2, 0x2000), "workspace"),
                       ((0x1000, n.value - 1, 3, 10, 2, 0x2000), "workspace"), ((0x1000, n.value, 3, 10, 2, None), "null")):
        assert lib.avl_room_door_table(*args, None) != 0 and word in _err(lib), (args, _err(lib))
    assert lib.avl_room_door_table(None, 0, 3, 10, 0, None, None) == 0                         # no pair: nothing to do

    for args, word in (((None, 10, 10, 0x2000, 5, 0, 0, 0x3000), "null"), ((0x1000, 10, 10, None, 5, 0, 0, 0x3000), "null"),
                       ((0x1000, 10, 10, 0x2000, 5, 0, 0, None), "null"), ((0x1000, 10, 10, 0x2000, -1, 0, 0, 0x3000), "negative")):
        assert lib.avl_lift_labels_2d(*args, None) != 0 and word in _err(lib), (args, _err(lib))
    assert lib.avl_lift_labels_2d(None, 10, 10, None, 0, 0, 0, None, None) == 0


# ------------------------------------------------------------------ the Python surface
def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_new_names_exist_with_their_signatures():
    E = inspect.Parameter.empty
    from avlmaps_amd import ops
    from avlmaps_amd.map import AVLMap, Map, Rooms, VLMap
    from avlmaps_amd.map.scene_objects import SceneObjects
    assert _params(ops.grow_labels) == [("free", E), ("seeds", E), ("device", False), ("stream", None), ("window", None)]
    assert _params(ops.segment_rooms) == [("free", E), ("radius", E), ("min_seed_cells", 1), ("device", False), ("stream", None)]
    assert _params(ops.lift_labels_2d)[:4] == [("labels", E), ("grid_pos", E), ("window", E), ("device", False)]
    assert ops.ROOM_TABLE_COLS == ops.DOOR_TABLE_COLS == 10
    assert _params(Map.get_rooms) == [("self", E), ("door_width", 0.9), ("min_core_area", 0.25), ("customized", False), ("known_free", False)]
    assert _params(VLMap.get_voxel_rooms) == [("self", E), ("rooms", E), ("device", False)]
    assert _params(SceneObjects.assign_rooms)[:2] == [("self", E), ("rooms", E)] and _params(SceneObjects.in_room) == [("self", E), ("k", E)]
    assert _params(AVLMap.name_rooms) == [("self", E), ("names", E), ("rooms", None)]
    assert _params(AVLMap.index_room) == [("self", E), ("room", E), ("decay_rate", None)]
    assert hasattr(AVLMap, "index_room_2d")
    for name in ("room_of", "centre", "mask", "area_m2", "doors", "neighbours", "route", "save", "load"):
        assert hasattr(Rooms, name), name
    assert "customize_obstacle_map" in Map.get_rooms.__doc__ or "customize_obstacle_map" in inspect.getdoc(Map.get_rooms)


def test_python_checks_come_before_the_device(lib):
    from avlmaps_amd import _lib, ops
    from avlmaps_amd.map.rooms import room_parameters
    free = np.ones((5, 7), np.uint8)
    with pytest.raises(ValueError, match="no seed"):
        ops.grow_labels(free, np.zeros((5, 7), np.int32))
    with pytest.raises(ValueError, match="no seed"):
        ops.grow_labels(free, np.eye(5, 7, dtype=np.int32), window=(0, 2, 3, 7))            # the window holds none of them
    with pytest.raises(ValueError, match="negative"):
        ops.grow_labels(free, -np.eye(5, 7, dtype=np.int32))
    with pytest.raises(ValueError, match="seed image"):
        ops.grow_labels(free, np.ones((5, 8), np.int32))
    with pytest.raises(ValueError):
        ops.grow_labels(np.ones((3, 4, 5), bool), np.ones((3, 4, 5), np.int32))
    with pytest.raises(ValueError):
        ops.grow_labels(free, np.ones((5, 7), np.int32), window=(0, 6, 0, 7))
    with pytest.raises(TypeError):
        ops.grow_labels(free, np.ones((5, 7), np.float64))
    with pytest.raises(_lib.AvlError, match="bad shape"):                                    # the library's argument error, no device involved
        ops.grow_labels(np.ones((1, 16385), bool), np.ones((1, 16385), np.int32))
    for bad in (dict(radius=-1.0), dict(radius=float("nan")), dict(radius=2.0, min_seed_cells=0)):
        with pytest.raises(ValueError):
            ops.segment_rooms(free, **bad)
    with pytest.raises(ValueError):
        ops.segment_rooms(np.ones((3, 4, 5), bool), 1.0)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        ops.lift_labels_2d(np.zeros((4, 4), np.int32), np.zeros((5, 2), np.int32), (0, 0))
    assert room_parameters(0.9, 0.25, 0.05) == (0.9 / (2 * 0.05), 100)
    assert room_parameters(0.9, 0.0, 0.05)[1] == 1 and room_parameters(1.0, 0.26, 0.1)[1] == 26
    for bad in ((-0.1, 0.25, 0.05), (0.9, -1.0, 0.05), (0.9, 0.25, 0.0)):
        with pytest.raises(ValueError):
            room_parameters(*bad)


def test_no_cpu_fallback_without_gpu(lib):
    """without a device every call ends in the library's error, never in a host computation"""
    from avlmaps_amd import _lib, ops
    free = three_rooms()
    seeds = np.zeros(free.shape, np.int32)
    seeds[10, 10] = 1
    calls = (lambda: ops.grow_labels(free, seeds), lambda: ops.segment_rooms(free, 4, 20),
             lambda: ops.lift_labels_2d(seeds, np.zeros((3, 3), np.int32), (0, 0)),
             lambda: ops.room_seeds(np.ones(free.shape), 0.5), lambda: ops.room_tables(seeds, seeds, np.ones(free.shape), 1))
    if _lib.device_count() > 0:
        assert ops.grow_labels(free, seeds).owner[10, 10] == 1
        return
    for call in calls:
        with pytest.raises(_lib.AvlError):
            call()


# ------------------------------------------------------------------ Rooms
def _rooms_of(ref, window=(100, 200), cs=0.05):
    from avlmaps_amd.map import Rooms
    return Rooms(ref["labels"], ref["rooms"], ref["doors"], ref["clearance"], window, cs, dict(door_width=0.4, min_core_area=0.05))


def test_rooms_reads_in_full_map_coordinates():
    free = three_rooms()
    ref = rooms_ref(free, 4, 20)
    rooms = _rooms_of(ref)
    assert rooms.n == 3 and rooms.shape == (70, 100)
    assert rooms.room_of([100 + 35.7, 200 + 10.2]) == 1 and rooms.room_of([135, 250]) == 2 and rooms.room_of([135, 290]) == 3
    assert rooms.room_of([100, 200]) == 0 and rooms.room_of([99, 250]) == 0 and rooms.room_of([135, 300]) == 0 and rooms.room_of([170, 250]) == 0
    for k in (1, 2, 3):
        r, c = rooms.centre(k)
        assert [r - 100, c - 200] == ref["rooms"][k - 1, 8:10].tolist() and rooms.room_of([r, c]) == k
        assert np.array_equal(rooms.mask(k), ref["labels"] == k)
        full = rooms.mask(k, gs=400)
        assert full.shape == (400, 400) and int(full.sum()) == int(ref["rooms"][k - 1, 0]) and np.array_equal(full[100:170, 200:300], ref["labels"] == k)
        assert rooms.area_m2(k) == float(ref["rooms"][k - 1, 0]) * 0.05 * 0.05
    assert rooms.doors[:, [0, 1, 2]].tolist() == [[1, 2, 4], [2, 3, 4]]
    assert (rooms.doors[:, [3, 4, 7]] - 100 == ref["doors"][:, [3, 4, 7]]).all() and (rooms.doors[:, [5, 6, 8]] - 200 == ref["doors"][:, [5, 6, 8]]).all()
    assert rooms.door(2, 1) == [int(ref["doors"][0, 7]) + 100, int(ref["doors"][0, 8]) + 200] and rooms.door(1, 3) is None
    assert rooms.neighbours(1) == [2] and rooms.neighbours(2) == [1, 3] and rooms.neighbours(3) == [2]
    for bad in (0, 4, -1):
        with pytest.raises(ValueError):
            rooms.centre(bad)


def test_route_takes_the_fewest_doors_and_visits_neighbours_in_ascending_id():
    from avlmaps_amd.map import Rooms
    rooms = _rooms_of(rooms_ref(three_rooms(), 4, 20))
    assert rooms.route(1, 3) == [1, 2, 3] and rooms.route(3, 1) == [3, 2, 1] and rooms.route(2, 2) == [2]
    # 1 - 2 - 4 - 6 and 1 - 3 - 5 - 6 tie at three doors: the search meets 2 before 3; 7 - 8 is an island of its own
    doors = np.zeros((7, 10), np.int64)
    doors[:, :2] = [[1, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5, 6], [7, 8]]
    table = np.zeros((8, 10), np.int64)
    graph = Rooms(np.zeros((4, 4), np.int32), table, doors, None, (0, 0), 0.1)
    assert graph.route(1, 6) == [1, 2, 4, 6] == route_ref(8, doors, 1, 6)
    assert graph.route(6, 1) == [6, 4, 2, 1] and graph.route(5, 4) == [5, 6, 4] == route_ref(8, doors, 5, 4)
    assert graph.route(1, 7) is None and graph.route(8, 7) == [8, 7]
    rng = np.random.default_rng(3)
    for _ in range(20):
        n = int(rng.integers(2, 9))
        pairs = sorted({tuple(sorted(int(v) for v in rng.choice(np.arange(1, n + 1), 2, replace=False))) for _ in range(int(rng.integers(1, 10)))})
        d = np.zeros((len(pairs), 10), np.int64)
        d[:, :2] = pairs
        g = Rooms(np.zeros((2, 2), np.int32), np.zeros((n, 10), np.int64), d, None, (0, 0), 0.1)
        for a in range(1, n + 1):
            for b in range(1, n + 1):
                assert g.route(a, b) == route_ref(n, d, a, b), (pairs, a, b)


def test_save_and_load(tmp_path):
    from avlmaps_amd.map import Rooms
    rooms = _rooms_of(rooms_ref(three_rooms(), 4, 20))
    rooms.save(tmp_path / "rooms.npz")
    back = Rooms.load(tmp_path / "rooms.npz")
    assert back.n == 3 and back.window == (100, 200) and back.cs == 0.05 and back.params == rooms.params
    for name in ("labels", "room_table", "door_table", "clearance"):
        a, b = getattr(rooms, name), getattr(back, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert back.route(1, 3) == [1, 2, 3] and back.centre(2) == rooms.centre(2)
    empty = Rooms(np.zeros((3, 3), np.int32), np.zeros((0, 10)), np.zeros((0, 10)), None, (1, 2), 0.1)
    empty.save(tmp_path / "empty.npz")
    back = Rooms.load(tmp_path / "empty.npz")
    assert back.n == 0 and back.clearance is None and back.doors.shape == (0, 10)


def test_the_tie_rule_of_assign_rooms():
    """the most voxels; the smallest room id among equals; 0 when no voxel lies in a room (column 0 never wins)"""
    from avlmaps_amd.map.rooms import majority_room
    counts = np.array([[0, 5, 2, 1],       # room 1
                       [9, 1, 4, 4],       # rooms 2 and 3 tie: 2
                       [7, 0, 0, 0],       # in no room, whatever column 0 says
                       [0, 0, 0, 3],       # room 3
                       [2, 6, 6, 6],       # all tie: 1
                       [0, 0, 0, 0]])
    got = majority_room(counts)
    assert got.dtype == np.int32 and got.tolist() == [1, 2, 0, 3, 1, 0]
    assert majority_room(np.zeros((2, 1), np.uint64)).tolist() == [0, 0] and majority_room(np.zeros((0, 4), np.uint64)).shape == (0,)
    assert majority_room(np.array([[0, 2 ** 40, 2 ** 40 + 1]], np.uint64)).tolist() == [2]


# ------------------------------------------------------------------ apps
def test_the_app_flags_parse():
    from avlmaps_amd.apps import generate_obstacle_map, index_map, plan_path
    base = ["--data-dir", "x", "--start", "3", "4"]
    a = plan_path.parse_args(base + ["--room", "2"])
    assert a.room == 2 and a.door_width is None and a.query is None and not plan_path.is_cross_modal(a)
    a = plan_path.parse_args(base + ["--room", "kitchen", "--door-width", "1.1", "--room-names", "kitchen,bedroom"])
    assert a.room == "kitchen" and a.door_width == 1.1 and a.room_names == "kitchen,bedroom" and plan_path.is_cross_modal(a)
    for bad in (["--room", "2", "--query", "sofa"], ["--room", "2", "--goal", "frontier"], ["--room", "2", "--area", "kitchen"],
                ["--room", "2", "--room-names", "a,b"], ["--room", "2", "--door-width", "-1"], ["--query", "sofa", "--door-width", "1.0"],
                ["--query", "sofa", "--room-names", "a"], []):
        with pytest.raises(SystemExit):
            plan_path.parse_args(base + bad)
    assert plan_path.parse_args(base + ["--query", "sofa"]).room is None

    inv = ["--data-dir", "x", "--modality", "object", "--query", "sofa", "--categories", "sofa,table", "--inventory"]
    a = index_map.parse_args(inv + ["--rooms", "--door-width", "0.8"])
    assert a.rooms and a.door_width == 0.8 and not index_map.parse_args(inv).rooms
    for bad in (inv[:-1] + ["--rooms"], inv + ["--door-width", "0.8"]):
        with pytest.raises(SystemExit):
            index_map.parse_args(bad)

    a = generate_obstacle_map.parse_args(["--data-dir", "x", "--rooms", "--door-width", "0.7", "--min-core-area", "0.5"])
    assert a.rooms and a.door_width == 0.7 and a.min_core_area == 0.5 and not generate_obstacle_map.parse_args(["--data-dir", "x"]).rooms
    with pytest.raises(SystemExit):
        generate_obstacle_map.parse_args(["--data-dir", "x", "--door-width", "0.7"])
    labels = np.array([[0, 1], [2, 3]])
    img = generate_obstacle_map.room_colours(labels, 3)
    assert img.shape == (2, 2, 3) and img.dtype == np.uint8 and img[0, 0].tolist() == [0, 0, 0]
    assert len({tuple(v) for v in img.reshape(-1, 3).tolist()}) == 4
