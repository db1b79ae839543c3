"""Navigator with the reference's surface (avlmaps/navigator/navigator.py:7-65), planning on the GPU.

build_visgraph uploads the cropped obstacle map and builds the visibility graph on the device (ops.NavGraph); the graph stays
there between plan_to calls, which only compute the start and goal visibility rows and the shortest path.  A start inside a
walled room needs no corridor carving (upstream _check_if_start_in_graph_obstacle / _rebuild_visgraph), see DESIGN.md."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from ..utils.navigation_utils import (NoPathError, build_visgraph_with_obs_map, path_lengths, plan_to_nearest_pos,  # noqa: F401
                                      plan_to_pos_v2)


class Navigator:
    def __init__(self):
        self.visgraph = None
        self.obs_map = None
        self.rowmin = 0
        self.colmin = 0

    def build_visgraph(self, obstacle_map: np.ndarray, rowmin: float, colmin: float, vis: bool = False):
        """obstacle_map: the cropped map (nonzero / True = free); rowmin, colmin: its offset in the full map"""
        self.close()
        self.obs_map = np.asarray(obstacle_map)
        self.visgraph = build_visgraph_with_obs_map(self.obs_map, vis=vis)
        self.rowmin = rowmin
        self.colmin = colmin

    def plan_to(self, start_full_map: Tuple[float, float], goal_full_map: Tuple[float, float], vis: bool = False) -> List[List[float]]:
        """full-map (row, col) start and goal -> the path as full-map [row, col] points, first the start.  NoPathError when the goal
        cannot be reached."""
        if self.visgraph is None:
            raise RuntimeError("build_visgraph first")
        start = self._convert_full_map_pos_to_cropped_map_pos(start_full_map)
        goal = self._convert_full_map_pos_to_cropped_map_pos(goal_full_map)
        paths = plan_to_pos_v2(start, goal, self.obs_map, self.visgraph, vis)
        return self.shift_path(paths, self.rowmin, self.colmin)

    def path_lengths(self, start_full_map: Tuple[float, float], goals_full_map) -> np.ndarray:
        """(M,) float64 travel distances from the start to every goal of (M, 2) full-map points, inf where plan_to would raise
        NoPathError: one shortest-path tree from the start and one launch over the goals"""
        if self.visgraph is None:
            raise RuntimeError("build_visgraph first")
        start = self._convert_full_map_pos_to_cropped_map_pos(start_full_map)
        return path_lengths(start, self._goals_to_cropped(goals_full_map), self.obs_map, self.visgraph)

    def plan_to_nearest(self, start_full_map: Tuple[float, float], goals_full_map):
        """-> (index, path): the goal with the shortest travel distance (the first on ties) and plan_to's path to it, in full-map
        coordinates.  NoPathError when no goal can be reached."""
        if self.visgraph is None:
            raise RuntimeError("build_visgraph first")
        start = self._convert_full_map_pos_to_cropped_map_pos(start_full_map)
        k, paths = plan_to_nearest_pos(start, self._goals_to_cropped(goals_full_map), self.obs_map, self.visgraph)
        return k, self.shift_path(paths, self.rowmin, self.colmin)

    def plan_to_nearest_frontier(self, start_full_map: Tuple[float, float], frontiers):
        """-> (index, path): plan_to_nearest over the frontier centres of Map.get_frontiers (its (centres, sizes) pair, or an (n, 2)
        array of full-map cells): where to look next, by travel distance.  Build the graph on Map.get_known_free_cropped() so that
        the path stays in observed space.  ValueError when there is no frontier, NoPathError when none can be reached."""
        centres = frontiers[0] if isinstance(frontiers, tuple) else frontiers
        centres = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
        if len(centres) == 0:
            raise ValueError("plan_to_nearest_frontier: no frontier to go to")
        return self.plan_to_nearest(start_full_map, centres)

    def plan_to_viewpoint(self, start_full_map: Tuple[float, float], viewpoints, min_fraction: float = 0.5):
        """-> (index, path): plan_to_nearest over the cells of a Map.get_viewpoints result that see at least
        max(1, ceil(min_fraction * the best cell's count)) target voxels (Viewpoints.select); index is the chosen cell's row in
        viewpoints.cells.  ValueError when the target is visible from nowhere, NoPathError when no such cell can be reached."""
        keep = viewpoints.select(min_fraction)
        if len(keep) == 0:
            raise ValueError("plan_to_viewpoint: the target is visible from no candidate cell")
        k, path = self.plan_to_nearest(start_full_map, np.asarray(viewpoints.cells, dtype=np.float64)[keep])
        return int(keep[k]), path

    def plan_to_next_best_view(self, start_full_map: Tuple[float, float], views, min_fraction: float = 0.5, among=None):
        """-> (index, path): plan_to_nearest over the cells of a Map.get_exploration_views result that gain at least
        max(1, ceil(min_fraction * the best cell's gain)) unknown cells (ExplorationViews.select), or over the rows `among` of its
        cells; index is the chosen cell's row in views.cells.  ValueError when no cell gains anything, NoPathError when none can
        be reached."""
        keep = views.select(min_fraction) if among is None else np.asarray(among, dtype=np.int64).reshape(-1)
        if len(keep) == 0:
            raise ValueError("plan_to_next_best_view: no candidate cell gains anything")
        k, path = self.plan_to_nearest(start_full_map, np.asarray(views.cells, dtype=np.float64)[keep])
        return int(keep[k]), path

    def _goals_to_cropped(self, goals_full_map) -> np.ndarray:
        goals = np.asarray(goals_full_map, dtype=np.float64).reshape(-1, 2)
        return goals - np.array([self.rowmin, self.colmin], np.float64)

    def shift_path(self, paths: List[List[float]], row_shift: float, col_shift: float) -> List[List[float]]:
        return [[p[0] + row_shift, p[1] + col_shift] for p in paths]

    def _convert_full_map_pos_to_cropped_map_pos(self, full_map_pos: Tuple[float, float]) -> List[float]:
        return [full_map_pos[0] - self.rowmin, full_map_pos[1] - self.colmin]

    def _convert_cropped_map_pos_to_full_map_pos(self, cropped_map_pos: Tuple[float, float]) -> List[float]:
        return [cropped_map_pos[0] + self.rowmin, cropped_map_pos[1] + self.colmin]

    def close(self):
        """release the graph's device memory"""
        if getattr(self, "visgraph", None) is not None:
            self.visgraph.close()
            self.visgraph = None

    def __del__(self):
        self.close()
