"""VisualMap with the reference's interface (avlmaps/map/visual_map.py:17-89).  Upstream localises a query image with HLoc
against the scene's frames.  Here the localiser is either a utils.localization_utils.HLocLocalizer (retrieval and pose geometry on
the GPU, the learned descriptor and matcher pluggable), composed as upstream composes it, or any callable
localize(img, query_cam_intrinsic_mat) -> (cam_tf, base_tf) 4 x 4 habitat transforms, or None when the image cannot be placed
(apps/common.FixedPoseLocalizer is a stand-in)."""
from __future__ import annotations

import os
from pathlib import Path

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
        try:
            self._cam_calib_mat = np.array(list(cfg_get(map_config, "cam_calib_mat")), dtype=np.float64).reshape((3, 3))
        except (KeyError, AttributeError, TypeError):
            self._cam_calib_mat = None

    @property
    def ref_cam_intrinsic_mat(self):
        """the reference frames' intrinsics: the config's cam_calib_mat (visual_map.py:22), else get_sim_cam_mat of the frame size
        (what localization_utils.py:462-463 falls back to), None before a frame size is known"""
        if self._cam_calib_mat is not None:
            return self._cam_calib_mat
        depth_paths = getattr(self, "depth_paths", None)
        if depth_paths:
            from ..utils.mapping_utils import get_sim_cam_mat, load_depth_npy
            h, w = load_depth_npy(depth_paths[0]).shape
            return get_sim_cam_mat(h, w)
        return None

    def _setup_paths(self, data_dir) -> None:
        """Reference: visual_map.py:43-54"""
        self.data_dir = Path(data_dir)
        self.rgb_dir = self.data_dir / "rgb"
        self.depth_dir = self.data_dir / "depth"
        self.pose_path = self.data_dir / "poses.txt"
        self.map_save_dir = self.data_dir / "visual_map"
        os.makedirs(self.map_save_dir, exist_ok=True)
        self.rgb_paths = sorted(self.rgb_dir.glob("*.png"))
        self.depth_paths = sorted(self.depth_dir.glob("*.npy"))

    def _setup_localizer(self, data_dir, global_descriptor=None, matcher=None, **kwargs) -> None:
        """Reference: visual_map.py:29-41.  The two learned parts are handed on to HLocLocalizer; a localizer that is already an
        HLocLocalizer keeps its own."""
        from ..utils.localization_utils import HLocLocalizer
        data_dir = Path(data_dir)
        self._setup_paths(data_dir)
        if isinstance(self.localizer, HLocLocalizer):
            loc = self.localizer
            loc.features_dir = str(self.map_save_dir)
            loc.global_descriptor = global_descriptor or loc.global_descriptor
            loc.matcher = matcher or loc.matcher
        else:
            loc = HLocLocalizer(self.map_save_dir, global_descriptor=global_descriptor, matcher=matcher, **kwargs)
        loc.init_video_with_images_folder(self.rgb_dir, frame_sample_interval=1, key=None)
        loc.init_depth_with_depth_folder(self.depth_dir, frame_sample_interval=1, key=None)
        loc.init_pose_with_pose_file(self.pose_path, frame_sample_interval=1)
        loc.compute_global_descriptor(loc.image_paths_list, reference=True, overwrite=False, descriptor_filename=data_dir.stem)
        self.localizer = loc

    def create_and_load_map(self, data_dir, global_descriptor=None, matcher=None, **kwargs) -> None:
        """Reference: visual_map.py:56-57"""
        self._setup_localizer(data_dir, global_descriptor=global_descriptor, matcher=matcher, **kwargs)

    def localize_image(self, img: np.ndarray, query_cam_intrinsic_mat: np.ndarray = None, sim_cam_fov: float = 90, vis: bool = False):
        """(query_cam_tf, query_base_tf) or None.  Reference: visual_map.py:62-89 (intrinsics default to a pinhole camera with
        the given horizontal field of view)."""
        if query_cam_intrinsic_mat is None:
            h, w = np.asarray(img).shape[:2]
            f = w / 2.0 / np.tan(np.deg2rad(sim_cam_fov) / 2.0)
            query_cam_intrinsic_mat = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1.0]])
        if hasattr(self.localizer, "localize_agent_with_depth"):
            ref_img_id, transform = self.localizer.localize_agent_with_depth(img, ref_intr_mat=self.ref_cam_intrinsic_mat,
                                                                            query_intr_mat=query_cam_intrinsic_mat, vis=vis)
            if ref_img_id == -1:
                return None
            tf = self.localizer.pose_list[ref_img_id] @ self.tf_base2cam
            query_cam_tf = tf @ transform
            query_base_tf = query_cam_tf @ np.linalg.inv(self.tf_base2cam)
            return query_cam_tf, query_base_tf
        return self.localizer(img, query_cam_intrinsic_mat)
