"""Host side of the navigator: the goal helpers of Map (map.py:183-240) and navigation_utils' box distance on hand cases, argument
checks that raise before any device work, and the C ABI of csrc/avl_nav.hip (declared, exported, built without spills).  CPU only."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def _map(cs=0.05):
    from avlmaps_amd.map.map import Map
    m = Map.__new__(Map)
    m.cs = cs
    return m


def test_filter_small_objects():
    m = _map()
    boxes = [[0, 10, 0, 5], [0, 5, 0, 2], [3, 4, 0, 100], [0, 7, 0, 8]]      # areas 50, 10, 100, 56
    assert m.filter_small_objects(boxes) == [2, 3]                            # strictly above 50
    assert m.filter_small_objects(boxes, area_thres=10) == [0, 2, 3]
    assert m.filter_small_objects([]) == []


def test_get_bbox_and_dist_to_bbox_2d():
    from avlmaps_amd.utils.navigation_utils import get_bbox, get_dist_to_bbox_2d
    lo, hi = get_bbox(np.array([10.0, 20.0]), np.array([4.0, 6.0]))
    assert lo.tolist() == [8.0, 17.0] and hi.tolist() == [12.0, 23.0]
    c, sz = np.array([10.0, 20.0]), np.array([4.0, 6.0])
    assert get_dist_to_bbox_2d(c, sz, np.array([10.0, 21.0])) == 0             # inside
    assert get_dist_to_bbox_2d(c, sz, np.array([12.0, 23.0])) == 0             # on the corner
    assert get_dist_to_bbox_2d(c, sz, np.array([15.0, 21.0])) == 3.0           # beyond the row range only
    assert get_dist_to_bbox_2d(c, sz, np.array([9.0, 13.0])) == 4.0            # beyond the column range only
    assert get_dist_to_bbox_2d(c, sz, np.array([15.0, 27.0])) == math.sqrt(3.0 * 3.0 + 4.0 * 4.0)


def test_select_nearest_obj():
    m = _map()
    centers = [[10.0, 10.0], [30.0, 30.0], [10.0, 40.0]]
    boxes = [[8, 12, 8, 12], [20, 40, 20, 40], [9, 11, 30, 50]]
    assert m.select_nearest_obj(centers, boxes, [25.0, 25.0]) == 1             # inside the second box
    assert m.select_nearest_obj(centers, boxes, [10.0, 25.0]) == 2             # 5 from the third, 13 from the first
    assert m.select_nearest_obj(centers, boxes, [0.0, 0.0]) == 0
    # equal distances: the first box
    assert m.select_nearest_obj([[0.0, 0.0], [0.0, 10.0]], [[-1, 1, -1, 1], [-1, 1, 9, 11]], [0.0, 5.0]) == 0


def test_get_forward_pos():
    m = _map(cs=0.1)
    r, c = m.get_forward_pos([50.0, 60.0], 0.0, 1.0)                           # heading 0: towards smaller rows
    assert (r, c) == (40.0, 60.0)
    r, c = m.get_forward_pos([50.0, 60.0], 90.0, 2.0)
    assert abs(r - 50.0) < 1e-12 and c == 80.0


def test_nearest_point_on_polygon():
    from avlmaps_amd.map.map import Map
    sq = [[0, 0], [0, 10], [10, 10], [10, 0]]
    assert Map.nearest_point_on_polygon([5.0, 13.7], sq) == [5, 10]           # above the edge (0,10)-(10,10)
    assert Map.nearest_point_on_polygon([-3.0, -4.0], sq) == [0, 0]            # beyond a corner
    assert Map.nearest_point_on_polygon([4.6, 2.0], sq) == [4, 0]              # inside: the nearest edge, then int() truncation
    assert Map.nearest_point_on_polygon([12.5, 7.9], sq) == [10, 7]            # the closing edge (10,0)-(10,10)... via (10,10)-(10,0)
    # equidistant from two edges: the one earlier along the ring wins (smallest arc length)
    assert Map.nearest_point_on_polygon([5.0, 5.0], sq) == [0, 5]
    assert Map.nearest_point_on_polygon([1.0, 1.0], [[3, 3]]) == [3, 3]       # a one-point contour


def test_get_nearest_pos_chains_the_helpers():
    m = _map()
    contours = [np.array([[0, 0], [0, 2], [2, 2], [2, 0]]),                    # too small: filtered out
                np.array([[20, 20], [20, 30], [30, 30], [30, 20]]),
                np.array([[50, 50], [50, 60], [60, 60], [60, 50]])]
    centers = [[1.0, 1.0], [25.0, 25.0], [55.0, 55.0]]
    boxes = [[0, 2, 0, 2], [20, 30, 20, 30], [50, 60, 50, 60]]
    m.get_pos = lambda name: (contours, centers, boxes)
    assert m.get_nearest_pos([40.0, 24.5], "sofa") == [30, 24]
    m.get_pos = lambda name: ([], [], [])
    assert m.get_nearest_pos([4.0, 5.0], "sofa") == [4.0, 5.0]


def test_plan_arguments_are_checked_before_device_work():
    from avlmaps_amd import ops
    from avlmaps_amd.utils.navigation_utils import NoPathError, plan_to_pos_v2
    with pytest.raises(ValueError):
        ops.nav_graph(np.ones(5, bool))
    with pytest.raises(ValueError):
        ops.nav_graph(np.ones((0, 4), bool))
    with pytest.raises(ValueError):
        ops.nav_graph(np.ones((2, 40000), bool))
    with pytest.raises(TypeError):
        ops.nav_graph(np.array([["a"]]))
    free = np.ones((8, 8), bool)
    with pytest.raises(ValueError):
        plan_to_pos_v2([8.5, 1], [2, 2], free, object())                         # outside the map
    with pytest.raises(NoPathError):
        plan_to_pos_v2([1, 1], [2, 2], np.zeros((8, 8), bool), object())         # no free cell to snap to
    assert issubclass(NoPathError, ValueError)
    # start == goal needs no graph at all
    assert plan_to_pos_v2([3, 3], [3, 3], free, object()) == [[3.0, 3.0]]


def test_navigator_surface():
    from avlmaps_amd.navigator import Navigator
    nav = Navigator()
    nav.rowmin, nav.colmin = 100, 200
    assert nav._convert_full_map_pos_to_cropped_map_pos([105.5, 203]) == [5.5, 3]
    assert nav._convert_cropped_map_pos_to_full_map_pos([5.5, 3]) == [105.5, 203]
    assert nav.shift_path([[1, 2], [3.5, 4]], 10, 20) == [[11, 22], [13.5, 24]]
    with pytest.raises(RuntimeError):
        nav.plan_to([0, 0], [1, 1])
    nav.close()


def test_nav_abi_is_declared_and_bound():
    import re
    from avlmaps_amd import _lib, build
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    declared = set(re.findall(r"AVL_API\s+[\w\s\*]+?\b(avl_nav_\w+)\s*\(", text))
    assert declared == {"avl_nav_create", "avl_nav_destroy", "avl_nav_num_vertices", "avl_nav_vertices", "avl_nav_export_visibility",
                        "avl_nav_plan", "avl_nav_last_plan"}
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    assert build.SOURCES["avl_nav.hip"] == ["-ffp-contract=off"]


def test_nav_library_exports_and_validates():
    """the built library exports the entry points and rejects bad arguments before touching a device"""
    import ctypes as C
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    build()
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.avl_nav_create(None, 4, 4, None, C.byref(h)) != 0 and h.value is None
    buf = (C.c_uint8 * 4)()
    assert lib.avl_nav_create(buf, 0, 4, None, C.byref(h)) != 0
    assert b"map size" in lib.avl_last_error()
    assert lib.avl_nav_num_vertices(None, None) != 0


def test_nav_kernels_do_not_spill():
    from avlmaps_amd import build as B
    from kernel_regs import kernel_regs
    rows = kernel_regs(B.CSRC / "avl_nav.hip")
    names = {r["name"] for r in rows}
    for k in ("nav_vertex_count_kernel", "nav_visibility_kernel", "nav_mirror_kernel", "nav_query_kernel", "nav_round_kernel",
              "nav_pred_kernel"):
        assert any(k in n for n in names), k
    bad = [(r["name"], r["spill"], r["sgpr_spill"], r["scratch"]) for r in rows if r["spill"] or r["sgpr_spill"] or r["scratch"]]
    assert not bad, bad


def test_points_inside_fills_count_as_obstacles():
    """a float point whose int() cell is free can still lie inside a fill; there every segment is blocked, so it snaps"""
    from avlmaps_amd.utils.navigation_utils import _in_obstacle, plan_to_pos_v2
    free = np.ones((8, 8), bool)
    free[3, 4] = free[4, 3] = free[4, 4] = False          # window (3, 3): 3 obstacles, free corner (3, 3)
    assert not _in_obstacle(free, [3.2, 3.3])             # before the hypotenuse
    assert not _in_obstacle(free, [3.5, 3.5])             # on it
    assert _in_obstacle(free, [3.9, 3.9])                 # beyond it (int() cell (3, 3) is free)
    assert _in_obstacle(free, [4.0, 4.0])                 # an obstacle pixel
    assert not _in_obstacle(free, [3.0, 3.0])
    assert not _in_obstacle(free, [3.0, 3.7]) and not _in_obstacle(free, [3.6, 3.0])   # grid lines through the free corner
    assert not _in_obstacle(free, [2.9, 3.9])             # the window above: 1 obstacle
    # start == goal after both snap: no graph needed, the snapped cell twice (upstream's duplicated head)
    # nearest free cell by squared distance, first in np.where order: (4, 5) at 1.22 (ties (5, 4)) before (3, 3) at 1.62
    assert plan_to_pos_v2([3.9, 3.9], [3.9, 3.95], free, object()) == [[4.0, 5.0], [4.0, 5.0]]


def test_goal_helpers_match_the_reference_golden():
    """g11: the reference's filter_small_objects, select_nearest_obj, get_forward_pos and get_dist_to_bbox_2d, executed by
    tools/gen_golden.py on random boxes (ties in area, positions inside, on edge lines and outside)"""
    from avlmaps_amd.utils.navigation_utils import get_dist_to_bbox_2d
    g = np.load(ROOT / "tests" / "golden" / "g11_nav_helpers.npz")
    m = _map(cs=float(g["cs"]))
    for k in range(len(g["boxes"])):
        boxes, centers = g["boxes"][k].tolist(), g["centers"][k].tolist()
        assert m.filter_small_objects(boxes, area_thres=10) == np.nonzero(g["keep10"][k])[0].tolist()
        assert m.select_nearest_obj(centers, boxes, g["pos"][k].tolist()) == g["nearest"][k]
    got = [float(get_dist_to_bbox_2d(c, s, p)) for c, s, p in zip(g["dist_center"], g["dist_size"], g["dist_pos"])]
    assert np.array_equal(np.array(got), g["dist"])
    fwd = [m.get_forward_pos(list(p), a, mm) for p, a, mm in zip(g["fwd_pos"], g["fwd_angle"], g["fwd_meters"])]
    assert np.array_equal(np.array(fwd, np.float64), g["fwd"])
