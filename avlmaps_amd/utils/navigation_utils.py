"""Island extraction with the reference's name and return convention (avlmaps/utils/navigation_utils.py:10-36), used by
VLMap.get_pos.  Upstream calls cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE); with OpenCV installed this module
does exactly that.  Without it (OpenCV is not part of the ROCm image) the 8-connected components come from
scipy.ndimage.label: bounding boxes and centres -- which upstream derives from the contour extents, i.e. from the
component extents -- are identical; the contour itself is the component's full outer boundary (Moore tracing) rather than
OpenCV's corner-compressed polyline, and components are listed bottom-up like OpenCV lists them."""
from __future__ import annotations

import math

import numpy as np


def _trace_boundary(comp: np.ndarray, start):
    """outer boundary of an 8-connected component (bool image), Moore-neighbour tracing from its top-left pixel"""
    H, W = comp.shape
    nb = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]   # clockwise starting west
    pts = [start]
    cur, back = start, 0
    if comp.sum() == 1:
        return np.array(pts)
    for _ in range(4 * comp.size + 8):
        found = False
        for k in range(8):
            d = (back + k) % 8
            r, c = cur[0] + nb[d][0], cur[1] + nb[d][1]
            if 0 <= r < H and 0 <= c < W and comp[r, c]:
                back = (d + 5) % 8          # restart the scan just past the pixel we came from
                cur = (r, c)
                found = True
                break
        if not found or cur == start:
            break
        pts.append(cur)
    return np.array(pts)


def get_segment_islands_pos(segment_map, label_id, detect_internal_contours=False):
    """-> (contours [(n_i, 2) arrays of (row, col)], centers [[row, col]], bbox_list [[rmin, rmax, cmin, cmax]], hierarchy)"""
    mask = (np.asarray(segment_map) == label_id).astype(np.uint8)
    try:
        import cv2
    except Exception:
        cv2 = None
    hierarchy = None
    if cv2 is not None:
        mode = cv2.RETR_TREE if detect_internal_contours else cv2.RETR_EXTERNAL
        contours, hierarchy = cv2.findContours(mask, mode, cv2.CHAIN_APPROX_SIMPLE)
        contours_list = [np.stack([c.reshape((-1, 2))[:, 1], c.reshape((-1, 2))[:, 0]], axis=1) for c in contours]
    else:
        if detect_internal_contours:
            raise NotImplementedError("internal contours (cv2.RETR_TREE) need OpenCV")
        from scipy import ndimage
        lab, n = ndimage.label(mask, structure=np.ones((3, 3), dtype=int))
        contours_list = []
        for k in range(n, 0, -1):                      # raster order of the first pixel, reversed (bottom-up)
            comp = lab == k
            r0 = int(np.argmax(comp.any(axis=1)))
            c0 = int(np.argmax(comp[r0]))
            contours_list.append(_trace_boundary(comp, (r0, c0)))
    centers_list, bbox_list = [], []
    for c in contours_list:
        xmin, xmax, ymin, ymax = np.min(c[:, 0]), np.max(c[:, 0]), np.min(c[:, 1]), np.max(c[:, 1])
        bbox_list.append([xmin, xmax, ymin, ymax])
        centers_list.append([(xmin + xmax) / 2, (ymin + ymax) / 2])
    return contours_list, centers_list, bbox_list, hierarchy


def get_segment_islands_pos_device(foreground, label_id=1):
    """get_segment_islands_pos without OpenCV, on the GPU: the same (contours, centers, bbox_list, None) -- the same arrays, dtypes and
    bottom-up order (label n first) -- from ops.label_islands and ops.trace_islands (csrc/avl_islands.hip).  `foreground` is the
    0 / 1 uint8 DeviceArray ops.mask_foreground(..., device=True) leaves on the device (label_id must then be 1), or a host segment
    map; only the island table (for the contour lengths) and the contour points come back to the host.  Internal contours are not
    supported."""
    from .. import ops
    from ..device import DeviceArray, DeviceView
    if isinstance(foreground, (DeviceArray, DeviceView)):
        if label_id != 1:
            raise ValueError("a device foreground mask holds 0 / 1: label_id must be 1")
        mask = foreground
    else:
        mask = (np.asarray(foreground) == label_id).astype(np.uint8)
    with ops.label_islands(mask, device=True) as isl:
        traced = ops.trace_islands(isl)
    contours_list = [traced[k].astype(np.int64) for k in range(isl.n - 1, -1, -1)]
    centers_list, bbox_list = [], []
    for c in contours_list:         # the extents of the CONTOUR, as above: a trace that meets its start early covers less than the island
        xmin, xmax, ymin, ymax = np.min(c[:, 0]), np.max(c[:, 0]), np.min(c[:, 1]), np.max(c[:, 1])
        bbox_list.append([xmin, xmax, ymin, ymax])
        centers_list.append([(xmin + xmax) / 2, (ymin + ymax) / 2])
    return contours_list, centers_list, bbox_list, None


# ---------------------------------------------------------------------------------------- planning on the obstacle map
# The reference builds a pyvisgraph visibility graph over the cv2 contours of the obstacles (navigation_utils.py:77-127) and runs
# pyvisgraph's Dijkstra (:130-197).  Here the graph is built and searched on the GPU (csrc/avl_nav.hip, ops.NavGraph) over the
# raster model of DESIGN.md "Navigation"; neither pyvisgraph nor OpenCV is needed.


class NoPathError(ValueError):
    """the goal cannot be reached from the start on the obstacle map"""


def build_visgraph_with_obs_map(obs_map, vis=False):
    """-> ops.NavGraph of the obstacle map (nonzero / True = free).  `vis` (cv2 windows upstream) is accepted and ignored.
    The reference's use_internal_contour / internal_point corridor carving is not needed: a start inside a walled room is
    planned from as it is."""
    from .. import ops
    return ops.nav_graph(obs_map)


def _nearest_free(obstacles, pos):
    """the free cell with the smallest squared distance to the float point `pos`, first in np.where order (as upstream)"""
    rows, cols = np.where(np.asarray(obstacles) != 0)
    if len(rows) == 0:
        raise NoPathError("the obstacle map has no free cell")
    d2 = (rows - pos[0]) ** 2 + (cols - pos[1]) ** 2
    k = int(np.argmin(d2))
    return [float(rows[k]), float(cols[k])]


def _in_obstacle(obstacles, pos):
    """Is the float point inside the obstacle set of the raster model, where every segment from it is
    blocked?  Upstream's test is its int() cell.  With that cell free, the point can only be inside the triangle fill of the 2 x 2
    window with top-left at that cell (the free corner) when it lies strictly beyond the hypotenuse; on a grid line it lies on no
    bond, since the cell is the line segment's first end."""
    obs = np.asarray(obstacles) == 0
    H, W = obs.shape
    r, c = float(pos[0]), float(pos[1])
    fr, fc = int(r), int(c)
    if obs[fr, fc]:
        return True
    if r == fr or c == fc or fr + 1 >= H or fc + 1 >= W or obs[fr:fr + 2, fc:fc + 2].sum() < 3:
        return False
    return (r - fr) + (c - fc) > 1                     # the free corner is (fr, fc): the hypotenuse is u + v = 1


def _inside(obstacles, pos):
    H, W = np.shape(obstacles)
    r, c = float(pos[0]), float(pos[1])
    if not (np.isfinite(r) and np.isfinite(c) and 0.0 <= r <= H - 1 and 0.0 <= c <= W - 1):
        raise ValueError(f"point ({pos[0]}, {pos[1]}) lies outside the {H} x {W} obstacle map")
    return r, c


def plan_to_pos_v2(start, goal, obstacles, G=None, vis=False):
    """Shortest path on a cropped obstacle map (nonzero = free) from start to goal, both (row, col), as a list of [row, col] floats
    starting at the start.  G is the map's NavGraph (built here when None).  As upstream, a start on an obstacle cell snaps to the
    nearest free cell and that cell is listed twice at the head of the path.  A goal on an obstacle cell snaps by the same rule
    (upstream: pyvisgraph's closest_point).  Besides upstream's obstacle cell (int() of the point), a point that lies inside the
    obstacle set -- in a fill of the raster model, where no segment could leave it -- snaps too.  An unreachable goal raises
    NoPathError.  `vis` is accepted and ignored."""
    obstacles = np.asarray(obstacles)
    s = list(_inside(obstacles, start))
    g = list(_inside(obstacles, goal))
    path = []
    if _in_obstacle(obstacles, s):           # upstream: obstacles[int(row), int(col)] == 0; also a point inside a fill
        s = _nearest_free(obstacles, s)
        path.append(list(s))
    if _in_obstacle(obstacles, g):
        g = _nearest_free(obstacles, g)
    if s == g:                                   # pyvisgraph's shortest_path returns its origin alone
        path.append(list(s))
        return path
    own = G is None
    if own:
        G = build_visgraph_with_obs_map(obstacles)
    try:
        dist, ids = G.plan(s, g)
        if not ids:
            raise NoPathError(f"no path from {s} to {g} on the obstacle map")
        verts = G.vertices()
        for k in ids:
            if k == G.V:
                path.append(list(s))
            elif k == G.V + 1:
                path.append(list(g))
            else:
                path.append([float(verts[k, 0]), float(verts[k, 1])])
    finally:
        if own:
            G.close()
    return path


def _snapped_batch(start, goals, obstacles, G):
    """start and goals checked like plan_to_pos_v2's and snapped by its rule on the device -> (s, start_moved, goals (M, 2))"""
    from .. import _lib
    s = list(_inside(obstacles, start))
    goals = np.asarray(goals, dtype=np.float64).reshape(-1, 2)
    H, W = np.shape(obstacles)
    ok = np.isfinite(goals).all(axis=1) & (goals >= 0.0).all(axis=1) & (goals[:, 0] <= H - 1) & (goals[:, 1] <= W - 1)
    if not ok.all():
        _inside(obstacles, goals[int(np.argmin(ok))])        # raises, with plan_to_pos_v2's message
    try:
        out, moved = G.snap(np.vstack([np.array([s], np.float64), goals]))
    except _lib.AvlError as e:
        if "no free cell" in str(e):
            raise NoPathError("the obstacle map has no free cell") from None
        raise
    return [float(out[0, 0]), float(out[0, 1])], bool(moved[0]), out[1:]


def path_lengths(start, goals, obstacles, G=None):
    """(M,) float64 travel distances from start to every goal of (M, 2) `goals` on the obstacle map: for each goal the length of
    plan_to_pos_v2's path summed left to right, inf where that raises NoPathError -- from one shortest-path tree and one launch
    over the goals (NavGraph.plan_many) instead of one plan per goal.  Start and goals snap by plan_to_pos_v2's rule, on the
    device (NavGraph.snap); a goal equal to the start has length 0."""
    obstacles = np.asarray(obstacles)
    own = G is None
    if own:
        _inside(obstacles, start)                        # argument errors before any device work
        G = build_visgraph_with_obs_map(obstacles)
    try:
        s, _, goals = _snapped_batch(start, goals, obstacles, G)
        return G.plan_many(s, goals).dist
    finally:
        if own:
            G.close()


def plan_to_nearest_pos(start, goals, obstacles, G=None):
    """-> (k, path): the goal with the shortest travel distance from start (the first one on ties) and the path to it, as
    plan_to_pos_v2(start, goals[k], ...) returns it: a snapped start is listed twice, a goal equal to the start gives [start].
    NoPathError when no goal can be reached (also for an empty goal list)."""
    obstacles = np.asarray(obstacles)
    own = G is None
    if own:
        _inside(obstacles, start)
        G = build_visgraph_with_obs_map(obstacles)
    try:
        s, s_moved, goals = _snapped_batch(start, goals, obstacles, G)
        pm = G.plan_many(s, goals)
        k = int(pm.best)
        if k < 0:
            raise NoPathError(f"none of the {len(goals)} goals can be reached from {s} on the obstacle map")
        g = [float(goals[k, 0]), float(goals[k, 1])]
        path = [list(s)] if s_moved else []
        if s == g:
            path.append(list(s))
            return k, path
        verts = G.vertices()
        for v in pm.path(k):
            if v == G.V:
                path.append(list(s))
            elif v == G.V + 1:
                path.append(list(g))
            else:
                path.append([float(verts[v, 0]), float(verts[v, 1])])
        return k, path
    finally:
        if own:
            G.close()


def get_bbox(center, size):
    """(min corner, max corner) of the box of `size` centred at `center` (navigation_utils.py:200-206)"""
    center, size = np.asarray(center), np.asarray(size)
    half = size / 2
    return center - half, center + half


def get_dist_to_bbox_2d(center, size, pos):
    """distance from `pos` to the 2-D box (navigation_utils.py:209-266): 0 inside, the excess along the one axis on which `pos`
    lies outside, the Euclidean corner distance when it lies outside on both"""
    center, size, pos = np.asarray(center), np.asarray(size), np.asarray(pos)
    lo, hi = get_bbox(center, size)
    out_r = pos[0] < lo[0] or pos[0] > hi[0]
    out_c = pos[1] < lo[1] or pos[1] > hi[1]
    er = np.abs(pos[0] - center[0]) - size[0] / 2
    ec = np.abs(pos[1] - center[1]) - size[1] / 2
    if out_r and out_c:
        return np.sqrt(er * er + ec * ec)
    if out_r:
        return er
    if out_c:
        return ec
    return 0
