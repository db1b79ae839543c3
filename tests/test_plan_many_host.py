"""Host side of the many-goal planner: argument checks that raise before any device work, the C ABI of the avl_navmany_* entry
points, the --nearest option of apps.plan_path, and navigation_utils / Map on stub graphs.  CPU only."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


class StubGraph:
    """a NavGraph stand-in: nothing snaps, and plan_many answers with the distances it was given"""
    V = 0

    def __init__(self, dist):
        self.dist = np.asarray(dist, np.float64)
        self.calls = []

    def snap(self, points):
        pts = np.asarray(points, np.float64).reshape(-1, 2)
        return pts.copy(), np.zeros(len(pts), bool)

    def vertices(self):
        return np.zeros((0, 2), np.int32)

    def plan_many(self, start, goals):
        from avlmaps_amd.ops import NavPlanMany
        self.calls.append((list(start), np.asarray(goals).tolist()))
        d = self.dist[:len(goals)]
        finite = np.nonzero(np.isfinite(d))[0]
        best = int(finite[np.argmin(d[finite])]) if len(finite) else -1
        pm = NavPlanMany(self, 0, d, np.where(np.isfinite(d), 0, -1).astype(np.int32), best)
        pm.path = lambda k: [0, 1] if np.isfinite(d[k]) else []
        return pm


def test_navmany_abi_is_declared_bound_and_exported():
    import ctypes as C
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    declared = set(re.findall(r"AVL_API\s+[\w\s\*]+?\b(avl_navmany_\w+)\s*\(", text))
    assert declared == {"avl_navmany_snap", "avl_navmany_plan", "avl_navmany_path", "avl_navmany_count_walks", "avl_navmany_stats"}
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    build()
    lib = _lib.load()
    # bad arguments are refused before any device work
    best = C.c_int64(7)
    assert lib.avl_navmany_plan(None, 0.0, 0.0, None, 0, None, None, C.byref(best), None) != 0
    assert b"null" in lib.avl_last_error()
    assert lib.avl_navmany_snap(None, None, 0, None, None, None) != 0
    n = C.c_int(5)
    assert lib.avl_navmany_path(None, 0, None, C.byref(n), 0, None) != 0
    assert lib.avl_navmany_stats(None, None) != 0
    assert lib.avl_navmany_count_walks(None, 1) != 0


def test_many_goal_kernels_are_built_without_spills():
    from avlmaps_amd import build as B
    from kernel_regs import kernel_regs
    rows = [r for r in kernel_regs(B.CSRC / "avl_nav.hip") if any(k in r["name"] for k in ("nav_goals_kernel", "nav_snap_kernel",
                                                                                            "nav_any_free_kernel"))]
    assert len(rows) == 3, [r["name"] for r in rows]
    bad = [(r["name"], r["spill"], r["sgpr_spill"], r["scratch"]) for r in rows if r["spill"] or r["sgpr_spill"] or r["scratch"]]
    assert not bad, bad


def test_point_checks_come_before_device_work():
    from avlmaps_amd import ops
    g = ops.NavGraph(None, (8, 9), 0)                         # a closed graph: any device call would raise "closed"
    for bad in ([[8.0, 1.0]], [[1.0, 8.5]], [[-0.5, 1.0]], [[np.nan, 1.0]], [[1.0, np.inf]]):
        with pytest.raises(ValueError, match="outside"):
            g.snap(bad)
        with pytest.raises(ValueError, match="closed|outside"):
            g.plan_many([1.0, 1.0], bad)
    with pytest.raises(ValueError, match="closed"):
        g.plan_many([1.0, 1.0], [[7.0, 8.0]])                 # the corner itself is inside
    with pytest.raises(ValueError):
        g.snap([[1.0, 2.0, 3.0]])                             # not (M, 2)
    assert ops.NAV_MANY_MAX == 1 << 20
    g = ops.NavGraph(1, (8, 9), 0)
    with pytest.raises(ValueError, match="at most"):
        g._points(np.zeros((ops.NAV_MANY_MAX + 1, 2)), "goals")
    g._h = None


def test_nearest_option_parses_and_defaults_to_euclid():
    from avlmaps_amd.apps.plan_path import parse_args
    base = ["--data-dir", "x", "--query", "sofa", "--start", "1", "2"]
    assert parse_args(base).nearest == "euclid"
    assert parse_args(base + ["--nearest", "path"]).nearest == "path"
    assert parse_args(base + ["--nearest", "euclid"]).nearest == "euclid"
    for extra in (["--nearest", "walk"], ["--nearest", "path", "--area", "kitchen"], ["--nearest", "path", "--goal-2d"],
                  ["--nearest", "path", "--relation", "left", "--heading", "0"]):
        with pytest.raises(SystemExit):
            parse_args(base + extra)


def test_plan_to_nearest_pos_on_stub_graphs():
    from avlmaps_amd.utils.navigation_utils import NoPathError, path_lengths, plan_to_nearest_pos
    free = np.ones((8, 8), bool)
    goals = [[2.0, 2.0], [5.0, 5.5], [7.0, 0.0]]
    with pytest.raises(NoPathError):
        plan_to_nearest_pos([1, 1], goals, free, StubGraph([np.inf] * 3))      # nothing reachable
    with pytest.raises(NoPathError):
        plan_to_nearest_pos([1, 1], [], free, StubGraph([]))                   # nothing to reach
    assert issubclass(NoPathError, ValueError)
    g = StubGraph([np.inf, 4.0, 4.0])
    assert plan_to_nearest_pos([1, 1], goals, free, g) == (1, [[1.0, 1.0], [5.0, 5.5]])
    assert g.calls == [([1.0, 1.0], goals)]
    assert path_lengths([1, 1], goals, free, g).tolist() == [np.inf, 4.0, 4.0]
    assert plan_to_nearest_pos([5, 5.5], goals, free, StubGraph([9.0, 0.0, 1.0])) == (1, [[5.0, 5.5]])     # the goal is the start
    for bad_start, bad_goals in (([8.5, 1], goals), ([1, 1], [[2, 2], [2, 8]]), ([1, 1], [[np.nan, 2]])):
        with pytest.raises(ValueError, match="outside"):
            plan_to_nearest_pos(bad_start, bad_goals, free, StubGraph([1.0] * 3))
        with pytest.raises(ValueError, match="outside"):
            path_lengths(bad_start, bad_goals, free, StubGraph([1.0] * 3))


def test_navigator_and_map_surface():
    from avlmaps_amd.map.map import Map
    from avlmaps_amd.navigator import Navigator
    nav = Navigator()
    with pytest.raises(RuntimeError):
        nav.path_lengths([0, 0], [[1, 1]])
    with pytest.raises(RuntimeError):
        nav.plan_to_nearest([0, 0], [[1, 1]])
    nav.obs_map = np.ones((8, 8), bool)
    nav.rowmin, nav.colmin = 100, 200
    nav.visgraph = g = StubGraph([3.0, 2.0])
    assert nav.path_lengths([101, 201], [[102, 202], [105, 205.5]]).tolist() == [3.0, 2.0]
    assert g.calls[-1] == ([1.0, 1.0], [[2.0, 2.0], [5.0, 5.5]])               # cropped coordinates
    assert nav.plan_to_nearest([101, 201], [[102, 202], [105, 205.5]]) == (1, [[101.0, 201.0], [105.0, 205.5]])
    nav.visgraph = None

    class Nav:
        def plan_to_nearest(self, start, goals):
            self.goals = np.asarray(goals).tolist()
            return 5, [start, [1.0, 1.0]]

    m = Map.__new__(Map)
    m.cs = 0.05
    small = np.array([[0, 0], [0, 2], [2, 2], [2, 0]])
    a = np.array([[20, 20], [20, 30], [30, 30], [30, 20]])
    b = np.array([[50, 50], [50, 60], [60, 60], [60, 50]])
    box = lambda c: [c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max()]   # noqa: E731
    m.get_pos = lambda name: ([small, a, b], [[1, 1], [25, 25], [55, 55]], [box(small), box(a), box(b)])
    n = Nav()
    assert m.get_nearest_reachable_pos([40.0, 24.5], "sofa", n) == ([50, 60], [[40.0, 24.5], [1.0, 1.0]])
    assert n.goals == a.tolist() + b.tolist()                                    # island by island, the small one left out
    m.get_pos = lambda name: ([small], [[1, 1]], [box(small)])
    assert m.get_nearest_reachable_pos([4.0, 5.0], "sofa", n) == ([4.0, 5.0], [[4.0, 5.0]])


def test_plan_path_main_takes_the_goal_from_the_chosen_method(monkeypatch, capsys):
    """apps.plan_path.main on stub map and navigator classes: --nearest path takes goal AND path from
    Map.get_nearest_reachable_pos on the built navigator, the default plans to Map.get_nearest_pos's goal"""
    import json
    import types
    import avlmaps_amd.apps.common as common
    import avlmaps_amd.map as map_pkg
    import avlmaps_amd.navigator as nav_pkg
    from avlmaps_amd.apps import plan_path
    log = []

    class StubVLMap:
        rmin, cmin = 10, 20

        def __init__(self, map_config, data_dir=None):
            self.grid_feat = np.zeros((1, 8), np.float32)

        def load_map(self, data_dir):
            return True

        def init_categories(self, cats):
            log.append(("categories", list(cats)))

        def generate_obstacle_map(self, h_min, h_max):
            pass

        def get_obstacle_cropped(self):
            return np.ones((6, 7), bool)

        def get_nearest_pos(self, start, name):
            log.append(("euclid", name))
            return [12, 23]

        def get_nearest_reachable_pos(self, start, name, navigator):
            log.append(("path", name, navigator.built))
            return [14, 25], [start, [13.0, 24.0], [14.0, 25.0]]

    class StubNavigator:
        built = None

        def build_visgraph(self, obstacles, rmin, cmin):
            self.built = (obstacles.shape, rmin, cmin)

        def plan_to(self, start, goal):
            log.append(("plan_to", list(goal)))
            return [start, [float(goal[0]), float(goal[1])]]

        def close(self):
            log.append(("close",))

    monkeypatch.setattr(map_pkg, "VLMap", StubVLMap)
    monkeypatch.setattr(nav_pkg, "Navigator", StubNavigator)
    monkeypatch.setattr(common, "load_config", lambda path, overrides=None: types.SimpleNamespace(map_config=types.SimpleNamespace()))
    base = ["--data-dir", "x", "--query", "sofa", "--start", "11", "21", "--text-model", "hash"]
    out = plan_path.main(base + ["--nearest", "path"])
    assert out["goal"] == [14.0, 25.0] and out["path"] == [[11.0, 21.0], [13.0, 24.0], [14.0, 25.0]]
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert ("path", "sofa", ((6, 7), 10, 20)) in log and ("close",) in log
    assert not any(e[0] in ("euclid", "plan_to") for e in log)
    del log[:]
    out = plan_path.main(base)
    assert out["goal"] == [12.0, 23.0] and out["path"] == [[11.0, 21.0], [12.0, 23.0]]
    assert [e[0] for e in log] == ["categories", "euclid", "plan_to", "close"]
