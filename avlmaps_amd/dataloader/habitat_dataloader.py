"""VLMapsDataloaderHabitat with the reference's interface (avlmaps/dataloader/habitat_dataloader.py:21-133).

A full-map pose is (row, col, theta_deg), theta 0 pointing to negative rows; a cropped-map pose is the same shifted by
(rmin, cmin) of the obstacle map.  All conversions are float64 host math on 4 x 4 matrices, the same operations in the same
order as upstream, so that the integer cells (int() truncation in base_pos2grid_id_3d) come out identical.

Departure: the obstacle map (and with it rmin / cmin) is built on the first cropped-pose request instead of in the
constructor -- full-map conversions, all that AVLMap's area / sound / image queries use, do not need it."""
from __future__ import annotations

from pathlib import Path
from typing import List, Union

import numpy as np

from ..map.map import Map, cfg_get
from ..utils.mapping_utils import base_pos2grid_id_3d, base_rot_mat2theta, cvt_pose_vec2tf, grid_id2base_pos_3d


class VLMapsDataloaderHabitat:
    def __init__(self, data_dir: Union[Path, str], map_config, map: Map = None, load_gt_map: bool = False):
        self.data_dir = data_dir
        self.map_config = map_config
        self.cs = cfg_get(map_config, "cell_size")
        self.gs = cfg_get(map_config, "grid_size")
        self.camera_height = cfg_get(cfg_get(map_config, "pose_info"), "camera_height")
        if map is None:
            map = Map.create(map_config)
            assert map.load_map(data_dir), f"Map loading fails. It could be because the map hasn't been created at {data_dir}."
        self.map = map
        self.base2cam_tf, self.base_transform = self.map.base2cam_tf, self.map.base_transform
        self.base_poses = np.loadtxt(self.map.pose_path)
        self.init_base_tf = self.base_transform @ cvt_pose_vec2tf(self.base_poses[0]) @ np.linalg.inv(self.base_transform)
        self.inv_init_base_tf = np.linalg.inv(self.init_base_tf)
        self.full_map_pose = None  # (row, col, theta_deg)
        if load_gt_map:
            # upstream stops at "TODO: implement loading GT map option" (habitat_dataloader.py:85); its two getters below read
            # a gt_cropped nothing sets.  Here it is the scene's GT label map (map/gtmap.py) over the obstacle crop
            from ..map.gtmap import GTMap
            self.gt_map = GTMap(map_config)
            if not self.gt_map.load_map(data_dir, vlmap=self.map):
                raise FileNotFoundError(f"GT map loading fails. It could be because the GT map hasn't been created at {data_dir} "
                                        "(apps.create_map --gt).")
            self.gt_cropped = self.gt_map.grid_gt[self.rmin:self.rmax + 1, self.cmin:self.cmax + 1]

    # ---- ground truth (habitat_dataloader.py:90-107); only with load_gt_map=True
    def get_obstacles_cropped_no_floor(self) -> np.ndarray:
        floor_mask = self.gt_cropped == 2
        obstacles_cropped_no_floor = self.obstacles_cropped.copy()
        obstacles_cropped_no_floor[floor_mask] = 1
        return obstacles_cropped_no_floor

    def get_gt_semantic_cropped(self) -> np.ndarray:
        return self.gt_cropped

    # ---- obstacle map: only the cropped conversions need it
    def _ensure_obstacles(self):
        if getattr(self.map, "obstacles_cropped", None) is None:
            self.map.generate_obstacle_map()

    @property
    def obstacles(self):
        self._ensure_obstacles()
        return self.map.obstacles_map

    @property
    def obstacles_cropped(self):
        self._ensure_obstacles()
        return self.map.obstacles_cropped

    @property
    def rmin(self):
        self._ensure_obstacles()
        return self.map.rmin

    @property
    def rmax(self):
        self._ensure_obstacles()
        return self.map.rmax

    @property
    def cmin(self):
        self._ensure_obstacles()
        return self.map.cmin

    @property
    def cmax(self):
        self._ensure_obstacles()
        return self.map.cmax

    def get_obstacles_cropped(self) -> np.ndarray:
        return self.obstacles_cropped

    # ---- conversions (habitat_dataloader.py:100-133)
    def from_cropped_map_pose(self, row: int, col: int, theta_deg: float):
        self.full_map_pose = [row + self.rmin, col + self.cmin, theta_deg]

    def from_full_map_pose(self, row: int, col: int, theta_deg: float):
        self.full_map_pose = [row, col, theta_deg]

    def from_habitat_tf(self, tf_hab: np.ndarray):
        tf = self.inv_init_base_tf @ self.base_transform @ tf_hab @ np.linalg.inv(self.base_transform)
        theta_deg = np.rad2deg(base_rot_mat2theta(tf[:3, :3]))
        x, y, z = tf[:3, 3]
        row, col, _ = base_pos2grid_id_3d(self.gs, self.cs, x, y, z)
        self.full_map_pose = [row, col, theta_deg]

    def from_camera_tf(self, tf_cam: np.ndarray):
        tf_hab = self.base_transform @ self.inv_init_base_tf @ self.base2cam_tf @ tf_cam
        self.from_habitat_tf(tf_hab)

    def to_cropped_map_pose(self) -> List:
        assert self.full_map_pose is not None, "Please call from_xx() first."
        return [self.full_map_pose[0] - self.rmin, self.full_map_pose[1] - self.cmin, self.full_map_pose[2]]

    def to_full_map_pose(self) -> List:
        assert self.full_map_pose is not None, "Please call from_xx() first."
        return self.full_map_pose

    def to_habitat_tf(self) -> np.ndarray:
        assert self.full_map_pose is not None, "Please call from_xx() first."
        row, col, theta_deg = self.full_map_pose
        x, y, z = grid_id2base_pos_3d(row, col, 0, self.cs, self.gs)
        theta = np.deg2rad(theta_deg)
        tf = np.eye(4)
        tf[:3, 3] = [x, y, z]
        tf[0, 0] = np.cos(theta)
        tf[1, 1] = np.cos(theta)
        tf[0, 1] = -np.sin(theta)
        tf[1, 0] = np.sin(theta)
        return np.linalg.inv(self.base_transform) @ self.init_base_tf @ tf @ self.base_transform

    # ---- batch helpers for the AVLMap queries (one call per loaded map)
    def habitat_tfs_to_cells(self, tfs) -> np.ndarray:
        """(P, 2) int64 full-map (row, col) of every 4 x 4 habitat transform, converted one by one exactly as from_habitat_tf"""
        out = np.empty((len(tfs), 2), dtype=np.int64)
        for i, tf in enumerate(tfs):
            self.from_habitat_tf(np.asarray(tf, dtype=np.float64))
            out[i] = self.full_map_pose[:2]
        return out

    def habitat_positions_to_cells(self, positions) -> np.ndarray:
        """(L, 2) int64 cells of habitat positions (3,), each taken as the translation of an identity pose
        (avlmap.py:118-121, the sound locations)"""
        tfs = []
        for p in positions:
            tf = np.eye(4)
            tf[:3, 3] = p
            tfs.append(tf)
        return self.habitat_tfs_to_cells(tfs)
