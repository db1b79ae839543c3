"""The travel-distance field without a GPU: the C ABI of csrc/avl_travel.hip (declared, exported, bound, every argument refused
before any device work), the Python surface and its checks, TravelField.descend on reference fields, and the reference itself
(tests/_travel_ref.py) against scipy.sparse.csgraph.dijkstra and the closed form of an empty map."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
from _travel_ref import (NEIGHBOURS, UNREACHED, check_walk, decay_ref, distance_ref, legal_step, pair_less, serpentine,  # noqa: E402
                         spiral, travel_ref)

SYMBOLS = ("avl_travel2d_workspace_bytes", "avl_travel2d", "avl_travel_decay_2d")


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
    src = np.zeros((H, W), np.uint8)
    idx = rng.choice(H * W, size=min(n_sources, H * W), replace=False)
    src.ravel()[idx] = 1                                       # wherever they fall: some on obstacle cells
    return free, src


# ------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_bound(lib):
    from avlmaps_amd import _lib
    from avlmaps_amd.build import SOURCES
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert re.search(rf"AVL_API\s+int\s+{name}\s*\(", text), name
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS, name
    assert SOURCES["avl_travel.hip"] == ["-ffp-contract=off"]


def test_the_decay_code_is_shared_not_copied():
    """one expression and one normalisation kernel for the Euclidean and the travel decay maps: both sources include the header,
    neither defines the pieces itself"""
    csrc = ROOT / "avlmaps_amd" / "csrc"
    head = (csrc / "avl_decay2d.h").read_text()
    assert "decay_value" in head and "decay_normalize_kernel" in head and "decay_minmax_reset" in head
    for name in ("avl_edt2d.hip", "avl_travel.hip"):
        src = (csrc / name).read_text()
        assert '#include "avl_decay2d.h"' in src and "decay_value(" in src and "decay_normalize(" in src, name
        assert "__ddiv_rn(" not in src and "edt_decay" not in src and "edt_normalize_kernel" not in src, name


def test_field_arguments_are_refused_before_any_device_work(lib):
    """every pointer below is fake and must never be dereferenced"""
    n = C.c_size_t(77)
    assert lib.avl_travel2d_workspace_bytes(10, 10, None) != 0 and "null" in _err(lib)
    for H, W in ((16385, 4), (4, 16385), (0, 4), (4, -1)):
        assert lib.avl_travel2d_workspace_bytes(H, W, C.byref(n)) != 0 and "bad shape" in _err(lib) and n.value == 77
        assert lib.avl_travel2d(0x1000, W, 0x2000, W, H, W, 0x3000, 0x4000, 0x5000, 0x6000, 1 << 40, None) != 0
        assert "bad shape" in _err(lib)
    assert lib.avl_travel2d_workspace_bytes(16384, 16384, C.byref(n)) == 0 and n.value >= 9 * 16384 * 16384
    assert lib.avl_travel2d_workspace_bytes(100, 30, C.byref(n)) == 0 and n.value >= 9 * 100 * 30
    ok = dict(free=0x1000, ldf=30, src=0x2000, lds=30, H=100, W=30, a=0x3000, b=0x4000, stats=0x5000, ws=0x6000, n=n.value)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.avl_travel2d(a["free"], a["ldf"], a["src"], a["lds"], a["H"], a["W"], a["a"], a["b"], a["stats"], a["ws"], a["n"], None)
        return rc, _err(lib)
    for kw, word in ((dict(free=None), "null"), (dict(src=None), "null"), (dict(a=None), "null"), (dict(b=None), "null"),
                     (dict(stats=None), "null"), (dict(ldf=29), "free rows of 29"), (dict(lds=7), "source rows of 7"),
                     (dict(ws=None), "workspace"), (dict(n=n.value - 1), "workspace")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)


def test_decay_arguments_are_refused_before_any_device_work(lib):
    ok = dict(a=0x1000, b=0x2000, H=100, W=30, cs=1.0, rate=0.1, norm=1, out=0x3000, flag=0x4000, ws=0x5000, n=512)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.avl_travel_decay_2d(a["a"], a["b"], a["H"], a["W"], a["cs"], a["rate"], a["norm"], a["out"], a["flag"], a["ws"], a["n"], None)
        return rc, _err(lib)
    for kw, word in ((dict(a=None), "null"), (dict(b=None), "null"), (dict(out=None), "null"), (dict(flag=None), "null"),
                     (dict(H=0), "bad shape"), (dict(W=16385), "bad shape"), (dict(rate=-0.1), "decay_rate"),
                     (dict(rate=float("nan")), "decay_rate"), (dict(cs=0.0), "cell_size"), (dict(cs=float("inf")), "cell_size"),
                     (dict(ws=None), "workspace"), (dict(n=16), "workspace")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)


# ------------------------------------------------------------------ the Python surface
def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_new_names_exist_with_their_signatures():
    E = inspect.Parameter.empty
    from avlmaps_amd import ops
    from avlmaps_amd.map import AVLMap, Map, VLMap
    assert ops.TRAVEL_MAX_SIDE == ops.EDT_MAX_SIDE == 16384 and ops.UNREACHED == UNREACHED == -1
    assert ops.TRAVEL_NEIGHBOURS == NEIGHBOURS
    assert _params(ops.travel_field)[:4] == [("free", E), ("sources", E), ("device", False), ("stream", None)]
    assert _params(ops.travel_decay_2d) == [("field", E), ("decay_rate", E), ("cell_size", 1.0), ("normalize", False), ("device", False),
                                            ("stream", None)]
    assert _params(Map.get_travel_field)[:4] == [("self", E), ("sources", E), ("customized", False), ("known_free", False)]
    assert _params(Map.get_reachable_cropped) == [("self", E), ("curr_pos", E), ("customized", False), ("known_free", False)]
    assert _params(VLMap.get_travel_distribution_map) == [("self", E), ("name", E), ("decay_rate", 0.1), ("customized", False)]
    assert _params(AVLMap.index_goal_2d_travel) == [("self", E), ("obj", None), ("area", None), ("sound", None), ("decay_rates", None),
                                                    ("want_heat", True), ("start", None), ("start_decay_rate", None)]
    # the kernel's tile and sweep cap, as the tests state them
    # ... which the shared header alone defines; the source holds the kernel as a call of the shared body, not a sweep loop
    csrc = ROOT / "avlmaps_amd" / "csrc"
    head, src = (csrc / "avl_travel_tile.h").read_text(), (csrc / "avl_travel.hip").read_text()
    for name, value in (("Tile", ops.TRAVEL_TILE), ("Sweeps", ops.TRAVEL_SWEEPS), ("Threads", 256), ("MaxSide", ops.TRAVEL_MAX_SIDE)):
        assert f"constexpr int kTravel{name} = {value};" in head, name
    assert not re.search(r"constexpr int k(Travel|Cost|Many|Grow)(Tile|Threads|Cells|Sweeps|Halo|MaxSide)\b", src)
    assert '#include "avl_travel_tile.h"' in src and "travel_tile_relax<" in src and "__syncthreads_or" not in src
    assert head.count("bool travel_less") == 1 and "bool travel_less" not in src


def test_python_checks_come_before_the_device(lib):
    from avlmaps_amd import _lib, ops
    from avlmaps_amd.map import AVLMap
    free = np.ones((5, 7), np.uint8)
    with pytest.raises(ValueError, match="no source"):
        ops.travel_field(free, np.zeros((5, 7), np.uint8))
    with pytest.raises(ValueError, match="no source"):
        ops.travel_field(free, np.zeros((0, 2), np.int64))
    with pytest.raises(ValueError, match="sources must be"):
        ops.travel_field(free, np.ones((5, 8), np.uint8))
    with pytest.raises(ValueError, match="sources must be"):
        ops.travel_field(free, np.ones((3, 2)))                              # float cells
    for cell in ((5, 0), (0, 7), (-1, 3)):
        with pytest.raises(ValueError, match="outside"):
            ops.travel_field(free, np.array([cell]))
    with pytest.raises(ValueError):
        ops.travel_field(np.ones((3, 4, 5), bool), np.array([[0, 0]]))
    with pytest.raises(ValueError):
        ops.travel_field(free, np.array([[0, 0]]), window=(0, 6, 0, 7))
    with pytest.raises(_lib.AvlError, match="bad shape"):                    # the library's argument error, no device involved
        ops.travel_field(np.ones((1, 16385), bool), np.array([[0, 0]]))
    A, B = travel_ref(free, np.eye(5, 7))
    field = ops.TravelField(A, B, A.shape, int((A >= 0).sum()), 0, 0, free != 0)
    with pytest.raises(ValueError):
        ops.travel_decay_2d(field, -1.0)
    with pytest.raises(ValueError):
        ops.travel_decay_2d(field, 0.1, cell_size=0.0)
    av = AVLMap.__new__(AVLMap)
    with pytest.raises(ValueError, match="at least one"):
        av.index_goal_2d_travel()
    with pytest.raises(ValueError, match="belongs to start"):
        av.index_goal_2d_travel(obj="sofa", start_decay_rate=0.1)


def test_no_cpu_fallback_without_gpu(lib):
    from avlmaps_amd import _lib, ops
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    free = np.ones((8, 9), np.uint8)
    with pytest.raises(_lib.AvlError):
        ops.travel_field(free, np.array([[3, 4]]))
    A, B = travel_ref(free, np.eye(8, 9))
    with pytest.raises(_lib.AvlError):
        ops.travel_decay_2d(ops.TravelField(A, B, A.shape, 72, 0, 0, free != 0), 0.1)


def test_plan_path_travel_flags():
    from avlmaps_amd.apps import plan_path
    base = ["--data-dir", "x", "--query", "sofa", "--start", "3", "4"]
    a = plan_path.parse_args(base + ["--goal-2d"])
    assert not a.travel and not a.travel_from_start
    a = plan_path.parse_args(base + ["--goal-2d", "--travel", "--travel-from-start"])
    assert a.goal_2d and a.travel and a.travel_from_start and plan_path.is_cross_modal(a)
    for bad in (["--travel"], ["--goal-2d", "--travel-from-start"]):
        with pytest.raises(SystemExit):
            plan_path.parse_args(base + bad)


# ------------------------------------------------------------------ the reference
def test_the_integer_order_is_the_order_of_the_lengths():
    """pair_less against exact arithmetic: a1 + b1 sqrt(2) < a2 + b2 sqrt(2) decided with Python's unbounded integers and, for small
    pairs where float64 separates them, against the float"""
    rng = np.random.default_rng(0)
    for _ in range(2000):
        p, q = tuple(int(v) for v in rng.integers(0, 60, 2)), tuple(int(v) for v in rng.integers(0, 60, 2))
        lp, lq = p[0] + p[1] * np.sqrt(2.0), q[0] + q[1] * np.sqrt(2.0)
        assert pair_less(p, q) == (lp < lq) and (p == q) == (lp == lq)
    # where float64 no longer separates neighbours: 2^27 diagonal steps against the nearest straight count
    b = 1 << 27
    a = int(np.floor(b * np.sqrt(2.0)))
    assert pair_less((a, 0), (0, b)) and pair_less((0, b), (a + 1, 0)) and not pair_less((a + 1, 0), (0, b))


def _scipy_distances(free, src):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    free, src = np.asarray(free) != 0, np.asarray(src) != 0
    H, W = free.shape
    rows, cols, w = [], [], []
    for r in range(H):
        for c in range(W):
            for dr, dc in NEIGHBOURS:
                if legal_step(free, src, (r, c), (r + dr, c + dc)):
                    rows.append(r * W + c)
                    cols.append((r + dr) * W + c + dc)
                    w.append(np.sqrt(2.0) if dr and dc else 1.0)
    g = coo_matrix((w, (rows, cols)), shape=(H * W, H * W)).tocsr()
    return dijkstra(g, directed=True, indices=np.flatnonzero(src.ravel()), min_only=True).reshape(H, W)


def test_reference_agrees_with_scipy_dijkstra():
    for seed, (H, W), density, ns in ((1, (23, 31), 0.3, 1), (2, (30, 17), 0.45, 3), (3, (28, 28), 0.3, 50), (4, (1, 40), 0.2, 2)):
        free, src = random_map(seed, H, W, density, ns)
        A, B = travel_ref(free, src)
        want = _scipy_distances(free, src)
        reached = A >= 0
        assert np.array_equal(reached, np.isfinite(want)), seed
        assert np.array_equal(reached, B >= 0)
        d = distance_ref(A, B)
        assert np.all(np.abs(d[reached] - want[reached]) <= 1e-12 * np.maximum(want[reached], 1.0)), seed
        assert np.all(A[src != 0] == 0) and np.all(B[src != 0] == 0)
        assert np.all(A[(free == 0) & (src == 0)] == UNREACHED)


def test_reference_has_the_closed_form_on_an_empty_map():
    H, W = 37, 29
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for r0, c0 in ((0, 0), (H - 1, W - 1), (18, 14), (5, 28)):
        src = np.zeros((H, W), np.uint8)
        src[r0, c0] = 1
        A, B = travel_ref(np.ones((H, W), np.uint8), src)
        dr, dc = np.abs(rr - r0), np.abs(cc - c0)
        assert np.array_equal(A, np.abs(dr - dc)) and np.array_equal(B, np.minimum(dr, dc))


def test_reference_obeys_the_rule():
    """no corner cutting, a source on an obstacle, a sealed pocket"""
    free = np.ones((5, 5), np.uint8)
    free[1, 2] = free[2, 1] = 0                               # two obstacles that touch diagonally: (1, 1) is cut off from (2, 2)
    free[0, 1] = free[1, 0] = 0
    src = np.zeros((5, 5), np.uint8)
    src[2, 2] = 1
    A, B = travel_ref(free, src)
    assert (A[1, 1], B[1, 1]) == (UNREACHED, UNREACHED) and (A[0, 0], B[0, 0]) == (UNREACHED, UNREACHED)
    free = np.ones((5, 5), np.uint8)
    free[1:4, 1:4] = 0
    src = np.zeros((5, 5), np.uint8)
    src[2, 2] = 1                                             # buried in a blob: no free neighbour
    A, B = travel_ref(free, src)
    assert (A >= 0).sum() == 1 and (A[2, 2], B[2, 2]) == (0, 0)
    src[:] = 0
    src[1, 1] = 1                                             # on the blob's corner: its diagonal step crosses two free cells
    A, B = travel_ref(free, src)
    assert (A[0, 0], B[0, 0]) == (0, 1) and (A[0, 1], B[0, 1]) == (1, 0) and (A[2, 2], B[2, 2]) == (UNREACHED, UNREACHED)


# ------------------------------------------------------------------ descend
def test_descend_on_reference_fields():
    from avlmaps_amd import ops
    cases = [random_map(5, 26, 33, 0.3, 3), random_map(6, 31, 22, 0.45, 50), (serpentine(11, 9), np.eye(11, 9, dtype=np.uint8)[::-1].copy()),
             (spiral(17), (np.arange(17 * 17).reshape(17, 17) == 0).astype(np.uint8))]
    for free, src in cases:
        A, B = travel_ref(free, src)
        field = ops.TravelField(A, B, A.shape, int((A >= 0).sum()), 0, 0, np.asarray(free) != 0)
        assert np.array_equal(field.reachable(), A >= 0) and np.array_equal(field.distance(), distance_ref(A, B))
        cells = np.argwhere(A >= 0)
        for r, c in cells[::max(1, len(cells) // 60)]:
            walk = field.descend((r, c))
            assert walk[0] == (r, c) and len(walk) == A[r, c] + B[r, c] + 1
            check_walk(free, src, A, B, walk)
        for r, c in np.argwhere(A < 0)[:3]:
            with pytest.raises(ValueError, match="not reached"):
                field.descend((r, c))
        with pytest.raises(ValueError, match="outside"):
            field.descend((A.shape[0], 0))


def test_descend_takes_the_first_neighbour_in_the_documented_order():
    from avlmaps_amd import ops
    free = np.ones((3, 3), np.uint8)
    src = np.zeros((3, 3), np.uint8)
    src[1, 0] = src[1, 2] = src[0, 1] = src[2, 1] = 1          # the centre is one straight step from four sources: E comes first
    A, B = travel_ref(free, src)
    field = ops.TravelField(A, B, A.shape, 9, 0, 0, free != 0)
    assert field.descend((1, 1)) == [(1, 1), (1, 2)]
    assert field.descend((0, 0)) == [(0, 0), (0, 1)]           # E before S
    assert field.descend((1, 2)) == [(1, 2)]


def test_decay_restatement_is_numpys_expression():
    A, B = travel_ref(*random_map(8, 12, 15, 0.3, 2))
    d = distance_ref(A, B)
    t = 1.0 - (np.where(np.isfinite(d), d, 0.0) / 0.05) * 0.01
    t[t < 0] = 0
    t[~np.isfinite(d)] = 0
    assert np.array_equal(decay_ref(A, B, 0.01, 0.05), t)
    n = decay_ref(A, B, 0.01, 0.05, normalize=True)
    assert n.min() == 0.0 and n.max() == 1.0 and np.array_equal(n, (t - t.min()) / (t.max() - t.min()))
