"""The cost-weighted travel field and the layered costmap without a GPU: the C ABI of csrc/avl_costfield.hip (declared, exported,
bound, every argument refused before any device work), the tables of ops.costmap against their closed forms, CostField.descend on
reference planes, plan_path's new flags, and the reference itself (tests/_costfield_ref.py) against scipy.sparse.csgraph.dijkstra
on the weighted graph and against the unweighted reference at price 1."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
from _costfield_ref import check_walk, cost_ref, costmap_ref, passable_ref, price_ref  # noqa: E402
from _travel_ref import NEIGHBOURS, UNREACHED, legal_step, serpentine, travel_ref  # noqa: E402

SYMBOLS = ("avl_costfield2d", "avl_costmap2d")


@pytest.fixture(scope="module")
def lib():
    from avlmaps_amd.build import build
    build()
    from avlmaps_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.avl_last_error().decode()


def random_map(seed, H, W, density, n_sources):
    rng = np.random.default_rng(seed)
    free = (rng.random((H, W)) >= density).astype(np.uint8)
    cost = rng.integers(0, 256, (H, W)).astype(np.uint8)       # about 1 free cell in 256 is lethal
    src = np.zeros((H, W), np.uint8)
    src.ravel()[rng.choice(H * W, size=min(n_sources, H * W), replace=False)] = 1
    return free, cost, src


# ------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_bound(lib):
    from avlmaps_amd import _lib
    from avlmaps_amd.build import SOURCES
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert re.search(rf"AVL_API\s+int\s+{name}\s*\(", text), name
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS, name
    assert SOURCES["avl_costfield.hip"] == ["-ffp-contract=off"]
    # the field runs in avl_travel2d's workspace: no size query of its own is exported
    assert not [s for s in _lib.EXPORTED_SYMBOLS if s.startswith("avl_cost") and s.endswith("_bytes")]
    src = (ROOT / "avlmaps_amd" / "csrc" / "avl_costfield.hip").read_text()
    assert '#include "avl_travel_tile.h"' in src and "travel_run_rounds(" in src and "travel_legal_in<" in src


def test_field_arguments_are_refused_before_any_device_work(lib):
    """every pointer below is fake and must never be dereferenced"""
    n = C.c_size_t(0)
    assert lib.avl_travel2d_workspace_bytes(100, 30, C.byref(n)) == 0
    ok = dict(free=0x1000, ldf=30, cost=0x7000, ldc=30, src=0x2000, lds=30, H=100, W=30, a=0x3000, b=0x4000, stats=0x5000, ws=0x6000,
              n=n.value)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.avl_costfield2d(a["free"], a["ldf"], a["cost"], a["ldc"], a["src"], a["lds"], a["H"], a["W"], a["a"], a["b"], a["stats"],
                                 a["ws"], a["n"], None)
        return rc, _err(lib)
    for H, W in ((16385, 4), (4, 16385), (0, 4), (4, -1)):
        rc, msg = call(H=H, W=W, ldf=max(W, 1), ldc=max(W, 1), lds=max(W, 1), n=1 << 40)
        assert rc != 0 and "bad shape" in msg, (H, W, msg)
    for H, W in ((2049, 2048), (2048, 2049), (16384, 257), (1, 16384)):      # H * W > 2^22 inside the side limit; the last one is fine
        rc, msg = call(H=H, W=W, ldf=W, ldc=W, lds=W, n=0)
        assert rc != 0, (H, W)
        assert ("at most 2^22" in msg) == (H * W > 1 << 22) and ("workspace" in msg) == (H * W <= 1 << 22), (H, W, msg)
    for kw, word in ((dict(free=None), "null"), (dict(cost=None), "null"), (dict(src=None), "null"), (dict(a=None), "null"),
                     (dict(b=None), "null"), (dict(stats=None), "null"), (dict(ldf=29), "free rows of 29"),
                     (dict(ldc=12), "cost rows of 12"), (dict(lds=7), "source rows of 7"), (dict(ws=None), "workspace"),
                     (dict(n=n.value - 1), "workspace")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)


def test_costmap_arguments_are_refused_before_any_device_work(lib):
    from avlmaps_amd.ops.costmap import _CostLayerC as Layer
    assert [f[0] for f in Layer._fields_] == ["d_distance", "d_table", "n_table"]
    good = (Layer * 8)(*[Layer(0x8000 + 0x100 * k, 0x9000 + 0x100 * k, 5) for k in range(8)])
    ok = dict(free=0x1000, ldf=30, H=20, W=30, layers=good, nl=2, out=0x2000)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.avl_costmap2d(a["free"], a["ldf"], a["H"], a["W"], a["layers"], a["nl"], a["out"], None)
        return rc, _err(lib)

    def with_layer(k, layer):
        arr = (Layer * 8)(*good)
        arr[k] = layer
        return arr
    for kw, word in ((dict(H=0), "bad shape"), (dict(W=16385, ldf=16385), "bad shape"), (dict(free=None), "null"), (dict(out=None), "null"),
                     (dict(ldf=29), "free rows of 29"), (dict(nl=-1), "layers"), (dict(nl=9), "layers"), (dict(layers=None), "null layer"),
                     (dict(layers=with_layer(1, Layer(None, 0x9000, 5))), "layer 1"), (dict(layers=with_layer(0, Layer(0x8000, None, 5))), "layer 0"),
                     (dict(layers=with_layer(1, Layer(0x8000, 0x9000, 0))), "table of 0")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    # (that layers past n_layers are never looked at needs a call that passes every check: tests/test_costfield_gpu.py makes it
    # with real device pointers; no call here may)


# ------------------------------------------------------------------ the Python surface
def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_new_names_exist_with_their_signatures():
    E = inspect.Parameter.empty
    from avlmaps_amd import ops
    from avlmaps_amd.map import Map, VLMap
    assert ops.COST_MAX_CELLS == 1 << 22 and ops.COST_MAX_LAYERS == 8 and (ops.COST_LETHAL, ops.COST_MAX) == (255, 254)
    assert _params(ops.inflation_table) == [("inscribed_cells", E), ("inflation_cells", E), ("scaling", E), ("peak", 100)]
    assert _params(ops.penalty_table) == [("radius_cells", E), ("penalty", E), ("lethal", False)]
    assert _params(ops.build_costmap) == [("free", E), ("layers", E), ("device", False), ("stream", None)]
    assert _params(ops.cost_field) == [("free", E), ("cost", E), ("sources", E), ("device", False), ("stream", None), ("window", None)]
    assert _params(ops.CostField.descend) == [("self", E), ("cell", E), ("waypoints", False)]
    assert _params(Map.get_costmap)[:8] == [("self", E), ("robot_radius", 0.15), ("inflation_radius", 0.5), ("cost_scaling", 5.0), ("avoid", ()),
                                            ("customized", False), ("known_free", False), ("device", False)]
    assert _params(Map.get_cost_field)[:3] == [("self", E), ("sources", E), ("costmap", None)]
    assert _params(Map.plan_cost_path)[:5] == [("self", E), ("start", E), ("goal", E), ("costmap", None), ("waypoints", True)]
    assert VLMap._avoid_distance is not Map._avoid_distance                      # names are resolved by VLMap
    m = Map.__new__(Map)
    m.obstacles_cropped = np.ones((4, 5), np.uint8)
    with pytest.raises(ValueError, match="by name needs a VLMap"):
        m._avoid_distance("carpet")
    # the tile geometry, the order and the round's body are the travel field's by one definition, not by an equal copy
    csrc = ROOT / "avlmaps_amd" / "csrc"
    head, src = (csrc / "avl_travel_tile.h").read_text(), (csrc / "avl_costfield.hip").read_text()
    assert f"constexpr int kTravelTile = {ops.TRAVEL_TILE};" in head and f"constexpr int kTravelSweeps = {ops.TRAVEL_SWEEPS};" in head
    assert not re.search(r"constexpr int k(Travel|Cost|Many|Grow)(Tile|Threads|Cells|Sweeps|Halo|MaxSide)\b", src)
    assert '#include "avl_travel_tile.h"' in src and "travel_tile_relax<" in src and "__syncthreads_or" not in src
    assert all("cost_less" not in p.read_text() for p in csrc.iterdir() if p.is_file())


def test_python_checks_come_before_the_device(lib):
    from avlmaps_amd import _lib, ops
    free, cost = np.ones((5, 7), np.uint8), np.ones((5, 7), np.uint8)
    with pytest.raises(ValueError, match="no source"):
        ops.cost_field(free, cost, np.zeros((5, 7), np.uint8))
    with pytest.raises(ValueError, match="sources must be"):
        ops.cost_field(free, cost, np.ones((5, 8), np.uint8))
    with pytest.raises(ValueError, match="outside"):
        ops.cost_field(free, cost, np.array([[5, 0]]))
    with pytest.raises(ValueError, match="cost plane"):
        ops.cost_field(free, np.ones((5, 8), np.uint8), np.array([[0, 0]]))
    with pytest.raises(ValueError, match="0 .. 255"):
        ops.cost_field(free, np.full((5, 7), 256), np.array([[0, 0]]))
    with pytest.raises(ValueError, match="0 .. 255"):
        ops.cost_field(free, np.full((5, 7), 1.0), np.array([[0, 0]]))
    with pytest.raises(ValueError):
        ops.cost_field(free, cost, np.array([[0, 0]]), window=(0, 6, 0, 7))
    with pytest.raises(_lib.AvlError, match="bad shape"):
        ops.cost_field(np.ones((1, 16385), bool), np.ones((1, 16385), np.uint8), np.array([[0, 0]]))
    with pytest.raises(_lib.AvlError, match=r"at most 2\^22"):                   # the library's refusal, no device involved
        ops.cost_field(np.ones((2049, 2048), bool), np.ones((2049, 2048), np.uint8), np.array([[0, 0]]))
    plane, table = np.zeros((5, 7)), np.zeros(3, np.uint8)
    with pytest.raises(ValueError, match="at most 8"):
        ops.build_costmap(free, [(plane, table)] * 9)
    with pytest.raises(ValueError, match="distance plane of layer 0"):
        ops.build_costmap(free, [(np.zeros((5, 8)), table)])
    with pytest.raises(ValueError, match="table of layer 1"):
        ops.build_costmap(free, [(plane, table), (plane, np.zeros(3, np.int32))])
    with pytest.raises(ValueError, match="table of layer 0"):
        ops.build_costmap(free, [(plane, np.zeros(0, np.uint8))])
    with pytest.raises(_lib.AvlError, match="bad shape"):
        ops.build_costmap(np.ones((1, 16385), bool), [])


def test_no_cpu_fallback_without_gpu(lib):
    from avlmaps_amd import _lib, ops
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    free = np.ones((8, 9), np.uint8)
    with pytest.raises(_lib.AvlError):
        ops.cost_field(free, free, np.array([[3, 4]]))
    with pytest.raises(_lib.AvlError):
        ops.build_costmap(free, [])
    with pytest.raises(_lib.AvlError):
        ops.distance_to_mask(free)


# ------------------------------------------------------------------ the tables
def test_inflation_table_has_its_closed_form_at_the_radius_edges():
    from avlmaps_amd import ops
    t = ops.inflation_table(3.0, 10.0, 0.25)
    assert t.dtype == np.uint8 and len(t) == 102                                # d^2 = 0 .. 100 and one entry beyond
    assert np.all(t[:9] == 255) and t[9] == 100                                 # d < 3 lethal; d = 3 exactly: the peak
    for d2 in (10, 16, 50, 99, 100):
        assert t[d2] == int(np.floor(100.0 * np.exp(-0.25 * (np.sqrt(float(d2)) - 3.0)))), d2
    assert t[100] == int(np.floor(100.0 * np.exp(-1.75))) == 17 and t[101] == 0  # d = 10 is still inside, beyond it 0
    t = ops.inflation_table(2.5, 4.2, 1.0, peak=254)                            # radii between lattice distances
    assert np.all(t[:7] == 255) and t[7] == int(np.floor(254.0 * np.exp(-(np.sqrt(7.0) - 2.5))))     # sqrt(6) < 2.5 <= sqrt(7)
    assert t[17] == int(np.floor(254.0 * np.exp(-(np.sqrt(17.0) - 2.5)))) and t[18] == 0 and len(t) == 19   # sqrt(17) <= 4.2 < sqrt(18)
    t = ops.inflation_table(3.0, 3.0, 5.0, peak=0)                              # the bare footprint: lethal inside, free of charge outside
    assert np.all(t[:9] == 255) and np.all(t[9:] == 0) and len(t) == 11
    t = ops.inflation_table(4.0, 2.0, 1.0)                                      # an inflation radius inside the robot: lethal, then nothing
    assert np.all(t[:16] == 255) and np.all(t[16:] == 0) and len(t) == 18
    assert np.array_equal(ops.inflation_table(0.0, 0.0, 1.0), np.array([100, 0], np.uint8))
    for bad in (dict(inscribed_cells=-1.0), dict(inflation_cells=float("inf")), dict(scaling=-0.1), dict(peak=255), dict(peak=-1)):
        with pytest.raises(ValueError):
            ops.inflation_table(**dict(dict(inscribed_cells=3.0, inflation_cells=10.0, scaling=0.25), **bad))


def test_penalty_table_has_its_closed_form_at_the_radius_edges():
    from avlmaps_amd import ops
    t = ops.penalty_table(6.0, 200)
    assert t.dtype == np.uint8 and len(t) == 38 and t[0] == 200
    for d2 in (1, 2, 9, 25, 35):
        assert t[d2] == int(np.floor(200.0 * (1.0 - np.sqrt(float(d2)) / 6.0))), d2
    assert t[35] > 0 and t[36] == 0 and t[37] == 0                              # 0 from the radius on
    lethal = ops.penalty_table(6.0, 200, lethal=True)
    assert lethal[0] == 255 and np.array_equal(lethal[1:], t[1:])
    assert np.array_equal(ops.penalty_table(0.0, 77), np.array([77, 0], np.uint8))       # only the cells themselves
    assert np.array_equal(ops.penalty_table(0.0, 77, lethal=True), np.array([255, 0], np.uint8))
    for bad in ((-1.0, 10), (3.0, 255), (3.0, -1), (float("nan"), 10)):
        with pytest.raises(ValueError):
            ops.penalty_table(*bad)


def test_costmap_restatement_on_a_hand_example():
    free = np.array([[1, 1, 0, 1]], np.uint8)
    d = np.array([[2.0, 1.0, 0.0, 1.0]])
    t = np.array([255, 40, 7], np.uint8)
    assert costmap_ref(free, []).tolist() == [[1, 1, 0, 1]]
    assert costmap_ref(free, [(d, t)]).tolist() == [[8, 41, 0, 41]]              # d^2 = 4 clamps to the last entry
    assert costmap_ref(free, [(d, t), (np.zeros((1, 4)), t)]).tolist() == [[0, 0, 0, 0]]       # a 255 in any layer is lethal
    big = np.array([200, 254], np.uint8)
    assert costmap_ref(free, [(d, big), (d, big)]).tolist() == [[254, 254, 0, 254]]            # the sum clamps at 254


# ------------------------------------------------------------------ the reference
def _scipy_prices(free, cost, src):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    ok, src = passable_ref(free, cost), np.asarray(src) != 0
    H, W = ok.shape
    rows, cols, w = [], [], []
    for r in range(H):
        for c in range(W):
            for dr, dc in NEIGHBOURS:
                if legal_step(ok, src, (r, c), (r + dr, c + dc)):
                    rows.append(r * W + c)
                    cols.append((r + dr) * W + c + dc)
                    w.append(float(cost[r + dr, c + dc]) * (np.sqrt(2.0) if dr and dc else 1.0))
    g = coo_matrix((w, (rows, cols)), shape=(H * W, H * W)).tocsr()
    return dijkstra(g, directed=True, indices=np.flatnonzero(src.ravel()), min_only=True).reshape(H, W)


def test_reference_agrees_with_scipy_dijkstra_on_the_weighted_graph():
    for seed, (H, W), density, ns in ((1, (23, 31), 0.25, 2), (2, (30, 17), 0.4, 3), (3, (1, 40), 0.1, 2)):
        free, cost, src = random_map(seed, H, W, density, ns)
        A, B = cost_ref(free, cost, src)
        want = _scipy_prices(free, cost, src)
        reached = A >= 0
        assert np.array_equal(reached, np.isfinite(want)) and np.array_equal(reached, B >= 0), seed
        d = price_ref(A, B)
        assert np.all(np.abs(d[reached] - want[reached]) <= 1e-12 * np.maximum(want[reached], 1.0)), seed
        assert np.all(A[src != 0] == 0) and np.all(B[src != 0] == 0)
        assert np.all(A[~passable_ref(free, cost) & (src == 0)] == UNREACHED)


def test_reference_at_price_one_is_the_travel_reference():
    free, _, src = random_map(7, 27, 33, 0.3, 3)
    A, B = cost_ref(free, np.ones_like(free), src)
    A1, B1 = travel_ref(free, src)
    assert np.array_equal(A, A1) and np.array_equal(B, B1)


def test_reference_counts_the_entered_cell():
    free = np.ones((1, 3), np.uint8)
    src = np.array([[1, 0, 0]], np.uint8)
    for own in (7, 0):                                                           # the source's own price never counts, even 0
        A, B = cost_ref(free, np.array([[own, 3, 5]], np.uint8), src)
        assert A.tolist() == [[0, 3, 8]] and B.tolist() == [[0, 0, 0]]
    A, B = cost_ref(np.array([[0, 1, 1]], np.uint8), np.array([[7, 3, 5]], np.uint8), src)       # nor when the source is an obstacle
    assert A.tolist() == [[0, 3, 8]]
    A, B = cost_ref(free, np.array([[7, 0, 5]], np.uint8), src)                  # a lethal cell is not entered
    assert A.tolist() == [[0, -1, -1]] and B.tolist() == [[0, -1, -1]]


# ------------------------------------------------------------------ descend
def _field(ops, free, cost, A, B):
    return ops.CostField(A, B, A.shape, int((A >= 0).sum()), 0, 0, passable_ref(free, cost), np.asarray(cost, np.uint8))


def test_descend_on_reference_planes():
    from avlmaps_amd import ops
    rng = np.random.default_rng(3)
    snake = serpentine(11, 9)
    cases = [random_map(5, 26, 33, 0.25, 3), random_map(6, 31, 22, 0.4, 20),
             (snake, rng.integers(1, 256, snake.shape).astype(np.uint8), np.eye(11, 9, dtype=np.uint8)[::-1].copy())]
    for free, cost, src in cases:
        A, B = cost_ref(free, cost, src)
        field = _field(ops, free, cost, A, B)
        assert np.array_equal(field.reachable(), A >= 0) and np.array_equal(field.cost(), price_ref(A, B))
        cells = np.argwhere(A >= 0)
        for r, c in cells[::max(1, len(cells) // 60)]:
            walk = field.descend((r, c))
            assert walk[0] == (r, c)
            check_walk(free, cost, src, A, B, walk)
            way = field.descend((r, c), waypoints=True)
            assert way[0] == walk[0] and way[-1] == walk[-1]
            it = iter(walk)
            assert all(p in it for p in way)                                     # a subsequence, in order
            assert ops.drop_collinear(walk) == way
        for r, c in np.argwhere(A < 0)[:3]:
            with pytest.raises(ValueError, match="not reached"):
                field.descend((r, c))
        with pytest.raises(ValueError, match="outside"):
            field.descend((A.shape[0], 0))


def test_waypoints_are_the_turning_cells():
    from avlmaps_amd import ops
    assert ops.drop_collinear([(0, 0)]) == [(0, 0)] and ops.drop_collinear([(0, 0), (0, 1)]) == [(0, 0), (0, 1)]
    walk = [(0, 0), (0, 1), (0, 2), (1, 3), (2, 4), (3, 4), (4, 4)]
    assert ops.drop_collinear(walk) == [(0, 0), (0, 2), (2, 4), (4, 4)]
    free = np.ones((3, 5), np.uint8)
    cost = np.full((3, 5), 9, np.uint8)
    cost[1, :] = 1                                                               # a cheap lane along the middle row
    src = np.zeros((3, 5), np.uint8)
    src[1, 4] = 1
    A, B = cost_ref(free, cost, src)
    field = _field(ops, free, cost, A, B)
    # entering (0, 0) costs 9 either way: straight from (1, 0) that is 4 + 9 = 13, diagonally from (1, 1) 3 + 9 sqrt(2) = 15.7
    assert (A[0, 0], B[0, 0]) == (13, 0)
    assert field.descend((0, 0)) == [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4)]
    assert field.descend((0, 0), waypoints=True) == [(0, 0), (1, 0), (1, 4)]


def test_descend_takes_the_first_neighbour_in_the_documented_order():
    from avlmaps_amd import ops
    free = np.ones((3, 3), np.uint8)
    cost = np.full((3, 3), 4, np.uint8)
    src = np.zeros((3, 3), np.uint8)
    src[1, 0] = src[1, 2] = src[0, 1] = src[2, 1] = 1
    A, B = cost_ref(free, cost, src)
    field = _field(ops, free, cost, A, B)
    assert field.descend((1, 1)) == [(1, 1), (1, 2)] and (A[1, 1], B[1, 1]) == (4, 0)          # E comes first
    assert field.descend((0, 0)) == [(0, 0), (0, 1)]


# ------------------------------------------------------------------ plan_path
def test_plan_path_cost_flags():
    from avlmaps_amd.apps import plan_path
    base = ["--data-dir", "x", "--query", "sofa", "--start", "3", "4"]
    a = plan_path.parse_args(base)
    assert a.planner == "visgraph" and a.avoid == [] and a.robot_radius is None
    a = plan_path.parse_args(base + ["--planner", "cost"])
    assert (a.robot_radius, a.inflation_radius, a.cost_scaling, a.avoid) == (0.15, 0.5, 5.0, [])
    a = plan_path.parse_args(base + ["--planner", "cost", "--avoid", "carpet:0.3:200", "--avoid", "plant", "--avoid", "rug:0.5",
                                     "--robot-radius", "0.2", "--inflation-radius", "0.8", "--cost-scaling", "3"])
    assert a.avoid == [("carpet", 0.3, 200), ("plant", 0.3, 200), ("rug", 0.5, 200)]
    assert (a.robot_radius, a.inflation_radius, a.cost_scaling) == (0.2, 0.8, 3.0)
    for bad in (["--avoid", "carpet"], ["--robot-radius", "0.2"], ["--inflation-radius", "1"], ["--cost-scaling", "2"],
                ["--planner", "visgraph", "--avoid", "carpet"],
                ["--planner", "cost", "--avoid", "carpet:x"], ["--planner", "cost", "--avoid", "carpet:0.3:300"],
                ["--planner", "cost", "--avoid", ":0.3"], ["--planner", "cost", "--avoid", "a:1:2:3"],
                ["--planner", "cost", "--robot-radius", "-1"], ["--planner", "cost", "--view"],
                ["--planner", "cost", "--nearest", "path"], ["--planner", "astar"]):
        with pytest.raises(SystemExit):
            plan_path.parse_args(base + bad)
    with pytest.raises(SystemExit):
        plan_path.parse_args(["--data-dir", "x", "--start", "3", "4", "--goal", "frontier", "--planner", "cost"])
