"""Visibility-graph navigation on an obstacle map (csrc/avl_nav.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib

NAV_MAX_VERTICES = 65536
NAV_MAX_SIDE = 32768
NAV_MANY_MAX = 1 << 20          # points per snap / goals per plan_many


class NavGraph:
    """The navigation graph of one obstacle map, resident on the device (csrc/avl_nav.hip): the padded obstacle raster, the path
    vertices and their V x V visibility bitset.  Node ids of a plan: vertices 0 .. V-1 (raster order), V = start, V + 1 = goal.
    Release the device memory with close() (also on garbage collection)."""

    def __init__(self, handle, shape, V):
        self._h = handle
        self.shape = shape
        self.V = V
        self.W64 = (V + 63) // 64
        self._verts = None
        self._many = 0              # serial of the last plan_many: its NavPlanMany alone may read paths

    def _handle(self):
        if self._h is None:
            raise ValueError("the navigation graph has been closed")
        return self._h

    def vertices(self) -> np.ndarray:
        """(V, 2) int32 (row, col) of the path vertices, raster order (cached on the host)"""
        if self._verts is None:
            out = np.zeros((self.V, 2), np.int32)
            if self.V:
                _lib.check(_lib.load().avl_nav_vertices(self._handle(), out.ctypes.data, None), "avl_nav_vertices")
            self._verts = out
        return self._verts

    def visibility_words(self) -> np.ndarray:
        """(V, ceil(V / 64)) uint64: bit b % 64 of word (a, b // 64) = a and b see each other"""
        out = np.zeros((self.V, self.W64), np.uint64)
        if self.V:
            _lib.check(_lib.load().avl_nav_export_visibility(self._handle(), out.ctypes.data, None), "avl_nav_export_visibility")
        return out

    def visibility(self) -> np.ndarray:
        """(V, V) bool, symmetric, False on the diagonal"""
        return unpack_rows(self.visibility_words(), self.V)

    def plan(self, start, goal):
        """float64 shortest path from start (row, col) to goal over the graph -> (distance, node ids start .. goal); (inf, [])
        when the goal is unreachable.  Both points must lie inside the map."""
        s = [float(start[0]), float(start[1])]
        t = [float(goal[0]), float(goal[1])]
        H, W = self.shape
        for r, c in (s, t):
            if not (np.isfinite(r) and np.isfinite(c) and 0.0 <= r <= H - 1 and 0.0 <= c <= W - 1):
                raise ValueError(f"point ({r}, {c}) lies outside the {H} x {W} map")
        cap = self.V + 2
        ids = np.zeros(cap, np.int32)
        dist, n = C.c_double(0.0), C.c_int(0)
        _lib.check(_lib.load().avl_nav_plan(self._handle(), s[0], s[1], t[0], t[1], C.byref(dist), ids.ctypes.data, C.byref(n), cap,
                                            None), "avl_nav_plan")
        return dist.value, ids[:n.value].tolist()

    def last_plan(self) -> dict:
        """the last plan's internals: dist (V + 2,) float64, pred (V + 2,) int32, qvis (2, V) bool (start row, goal row), sg bool"""
        N = self.V + 2
        dist, pred = np.zeros(N, np.float64), np.zeros(N, np.int32)
        q = np.zeros((2, max(self.W64, 1)), np.uint64)
        sg = np.zeros(1, np.int32)
        _lib.check(_lib.load().avl_nav_last_plan(self._handle(), dist.ctypes.data, pred.ctypes.data, q.ctypes.data, sg.ctypes.data,
                                                 None), "avl_nav_last_plan")
        return dict(dist=dist, pred=pred, qvis=unpack_rows(q[:, :self.W64], self.V), sg=bool(sg[0]))

    def _points(self, points, what):
        """(M, 2) float64 points checked like plan's: finite and inside the map"""
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 2))
        if len(pts) > NAV_MANY_MAX:
            raise ValueError(f"{len(pts)} {what}: at most {NAV_MANY_MAX} per call")
        H, W = self.shape
        ok = np.isfinite(pts).all(axis=1) & (pts[:, 0] >= 0.0) & (pts[:, 0] <= H - 1) & (pts[:, 1] >= 0.0) & (pts[:, 1] <= W - 1)
        if not ok.all():
            k = int(np.argmin(ok))
            raise ValueError(f"point ({pts[k, 0]}, {pts[k, 1]}) lies outside the {H} x {W} map")
        return pts

    def snap(self, points):
        """navigation_utils._in_obstacle + _nearest_free for (M, 2) points, on the device -> (points_out (M, 2) float64, moved (M,)
        bool): a point inside the obstacle set (an obstacle cell, or strictly inside a triangle fill) moves to the free cell with
        the smallest squared distance, the first in raster order on ties; the others come back unchanged.  AvlError when the map
        has no free cell."""
        pts = self._points(points, "points")
        out = np.empty_like(pts)
        moved = np.zeros(len(pts), np.uint8)
        _lib.check(_lib.load().avl_navmany_snap(self._handle(), pts.ctypes.data, len(pts), out.ctypes.data, moved.ctypes.data, None),
                   "avl_navmany_snap")
        return out, moved.astype(bool)

    def plan_many(self, start, goals) -> "NavPlanMany":
        """the shortest-path tree from start (row, col), computed once, and every goal of (M, 2) `goals` against it in one launch:
        dist, via and best of avl_navmany_plan.  dist[k] and path(k) equal plan(start, goals[k]) exactly."""
        handle = self._handle()
        s = self._points([start], "points")[0]
        pts = self._points(goals, "goals")
        M = len(pts)
        dist = np.empty(M, np.float64)
        via = np.empty(M, np.int32)
        best = C.c_int64(-1)
        _lib.check(_lib.load().avl_navmany_plan(handle, float(s[0]), float(s[1]), pts.ctypes.data, M, dist.ctypes.data,
                                                via.ctypes.data, C.byref(best), None), "avl_navmany_plan")
        self._many += 1
        return NavPlanMany(self, self._many, dist, via, int(best.value))

    def count_walks(self, on=True):
        """have the following plan_many calls count their walks for many_stats (off by default: counting costs a little per word)"""
        _lib.check(_lib.load().avl_navmany_count_walks(self._handle(), 1 if on else 0), "avl_navmany_count_walks")

    def many_stats(self) -> dict:
        """the pruning of the last plan_many (after count_walks()): walks started, and goal-vertex pairs with a finite candidate
        (the walks without pruning)"""
        n = np.zeros(2, np.uint64)
        _lib.check(_lib.load().avl_navmany_stats(self._handle(), n.ctypes.data), "avl_navmany_stats")
        return dict(walks=int(n[0]), candidates=int(n[1]))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            try:
                _lib.load().avl_nav_destroy(h)
            except Exception:
                pass

    def __del__(self):
        self.close()


class NavPlanMany:
    """One NavGraph.plan_many: dist (M,) float64 (inf = unreachable), via (M,) int32 (the node each goal hangs on: a vertex id,
    V = the start, -1 = unreachable), best (the first goal with the smallest finite distance, -1 = none) and path(k), the node ids
    start .. goal k (V = start, V + 1 = goal; [] when unreachable).  path() reads the tree kept on the graph, so it answers only
    until the graph's next plan_many."""

    def __init__(self, graph, serial, dist, via, best):
        self._g, self._serial = graph, serial
        self.dist, self.via, self.best = dist, via, best

    def path(self, k):
        k = int(k)
        if not 0 <= k < len(self.dist):
            raise IndexError(f"goal {k} of {len(self.dist)}")
        if self._g._many != self._serial:
            raise ValueError("the graph has planned another batch since: this one's paths are gone")
        cap = self._g.V + 2
        ids = np.zeros(cap, np.int32)
        n = C.c_int(0)
        _lib.check(_lib.load().avl_navmany_path(self._g._handle(), k, ids.ctypes.data, C.byref(n), cap, None), "avl_navmany_path")
        return ids[:n.value].tolist()


def unpack_rows(words: np.ndarray, n: int) -> np.ndarray:
    """(R, ceil(n / 64)) uint64 bit rows -> (R, n) bool (bit b % 64 of word b // 64)"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


def nav_graph(obstacle_map) -> NavGraph:
    """navigation_utils.py:77-127 build_visgraph_with_obs_map on the GPU: obstacle_map (H, W), nonzero / True = free, 0 = obstacle
    (Map.obstacles_cropped).  Raises AvlError above NAV_MAX_VERTICES path vertices."""
    obs = np.asarray(obstacle_map)
    if obs.ndim != 2 or obs.shape[0] < 1 or obs.shape[1] < 1:
        raise ValueError(f"the obstacle map must be a non-empty 2-D array, got shape {obs.shape}")
    if max(obs.shape) > NAV_MAX_SIDE:
        raise ValueError(f"the obstacle map is {obs.shape[0]} x {obs.shape[1]}; at most {NAV_MAX_SIDE} per side")
    if obs.dtype.kind not in "biuf":
        raise TypeError(f"the obstacle map must be boolean or numeric, got {obs.dtype}")
    free = np.ascontiguousarray(obs != 0, dtype=np.uint8)
    lib = _lib.load()
    _lib.require_gpu()
    h = C.c_void_p()
    _lib.check(lib.avl_nav_create(free.ctypes.data, free.shape[0], free.shape[1], None, C.byref(h)), "avl_nav_create")
    V = C.c_int64(0)
    rc = lib.avl_nav_num_vertices(h, C.byref(V))
    g = NavGraph(h, free.shape, int(V.value))
    _lib.check(rc, "avl_nav_num_vertices")
    return g
