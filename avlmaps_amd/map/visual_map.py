"""VisualMap with the reference's interface (avlmaps/map/visual_map.py:17-89).  Upstream localises a query image with HLoc
against the scene's frames; here the localiser is pluggable: localize(img, query_cam_intrinsic_mat) -> (cam_tf, base_tf) 4 x 4
habitat transforms, or None when the image cannot be placed (apps/common.FixedPoseLocalizer is a stand-in)."""
from __future__ import annotations

import numpy as np

from .map import cfg_get


class VisualMap:
    def __init__(self, map_config, data_dir: str = "", localizer=None) -> None:
        self.map_config = map_config
        pose_info = cfg_get(map_config, "pose_info")
        self.tf_base2cam = np.eye(4)
        self.tf_base2cam[:3, :3] = np.array(list(cfg_get(pose_info, "base2cam_rot"))).reshape((3, 3))
        self.tf_base2cam[1, 3] = cfg_get(pose_info, "camera_height")
        self.localizer = localizer
        self.data_dir = data_dir

    def localize_image(self, img: np.ndarray, query_cam_intrinsic_mat: np.ndarray = None, sim_cam_fov: float = 90, vis: bool = False):
        """(query_cam_tf, query_base_tf) or None.  Reference: visual_map.py:62-89 (intrinsics default to a pinhole camera with
        the given horizontal field of view)."""
        if query_cam_intrinsic_mat is None:
            h, w = np.asarray(img).shape[:2]
            f = w / 2.0 / np.tan(np.deg2rad(sim_cam_fov) / 2.0)
            query_cam_intrinsic_mat = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1.0]])
        return self.localizer(img, query_cam_intrinsic_mat)
