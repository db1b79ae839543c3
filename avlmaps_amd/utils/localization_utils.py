"""Image localization with the names of the reference's avlmaps/utils/localization_utils.py (cited per function, path:line in the
upstream repo).  Upstream's HLocLocalizer is NetVLAD retrieval, SuperPoint + SuperGlue matching and pycolmap's absolute pose; here
the two learned parts are constructor arguments, as LSeg, CLIP and AudioCLIP are elsewhere, and the geometry between "matches" and
"a pose" runs on the GPU (ops.retrieve_frame, ops.loc_lift, ops.pnp_ransac, ops.pnp_refine: csrc/avl_pnp.hip)."""
from __future__ import annotations

import math
import os
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np
from scipy.spatial.transform import Rotation as R

from .mapping_utils import cvt_pose_vec2tf, get_sim_cam_mat, load_depth_npy, load_rgb_png

MIN_MATCHES = 100                 # localization_utils.py:459
INLIER_RATIO = 0.1                # the design ratio of the trial budget and of min_inliers


def _missing(message: str):
    from ..map.avlmap import MissingSubMap
    return MissingSubMap(message)


def _frame_key(x: str) -> int:
    """the trailing number of a frame's file name (localization_utils.py:151, which splits the whole path at its first "." and so
    fails under a folder whose name holds one; here only the file name is read)"""
    return int(os.path.basename(x).split(".")[0].split("_")[-1])


def _sorted_paths(folder, pattern: str, key) -> List[str]:
    return sorted([str(x) for x in Path(folder).glob(pattern)], key=key)


class HLocLocalizer:
    """global_descriptor(img) -> (D,) float32 stands in for NetVLAD, matcher(img_ref, img_query) -> (mkpts0 (M, 2), mkpts1 (M, 2),
    confidence (M,)) for SuperPoint + SuperGlue; (x, y) pixels, mkpts0 in the reference image.  Reference: :127-145."""

    def __init__(self, features_dir, global_descriptor=None, matcher=None, max_error: float = 12.0, n_hyp: Optional[int] = None,
                 min_inliers: Optional[int] = None, seed: int = 0):
        from .. import ops
        self.features_dir = str(features_dir)
        os.makedirs(self.features_dir, exist_ok=True)
        self.images_dir = ""
        self.dataset_name = ""
        self.descriptor_file_prefix = "tmp_"
        self.global_descriptor = global_descriptor
        self.matcher = matcher
        self.max_error = float(max_error)                                       # :485
        self.n_hyp = int(ops.PNP_DEFAULT_HYPOTHESES if n_hyp is None else n_hyp)
        self.min_inliers = min_inliers                                          # None: ceil(INLIER_RATIO * M') per call
        self.seed = int(seed)
        self.image_paths_list: List[str] = []
        self.depth_paths_list: List[str] = []
        self.depth_extension = ".npy"
        self.pose_list: List[np.ndarray] = []
        self.ref_desc = None              # (N, D) float32 on the host
        self._ref_desc_dev = None         # the same, resident on the device (uploaded once)
        self.query_desc = None
        self.ref_features_path = self.query_features_path = None
        self.current_frame_id = -1
        self.last_estimate = None         # diagnostics of the last _get_relative_pose_with_depth call

    # ------------------------------------------------------------------ bookkeeping (:150-192)
    def init_video_with_images_folder(self, images_dir, frame_sample_interval=50, key=_frame_key, show=False):
        self.frame_sample_interval = frame_sample_interval
        self.images_dir = images_dir
        self.image_paths_list = _sorted_paths(images_dir, "*.png", key)

    def init_depth_with_depth_folder(self, depths_dir, frame_sample_interval=50, key=_frame_key, show=False, extension=".npy"):
        self.depth_extension = extension
        self.frame_sample_interval = frame_sample_interval
        self.depths_dir = depths_dir
        self.depth_paths_list = _sorted_paths(depths_dir, "*" + extension, key)

    def init_pose_with_pose_file(self, pose_path, frame_sample_interval=50):
        self.pose_list = [cvt_pose_vec2tf(pose) for pose in np.loadtxt(pose_path).reshape(-1, 7)]
        self.frame_sample_interval = frame_sample_interval

    # ------------------------------------------------------------------ descriptors (:310-406)
    def _features_path(self, reference: bool) -> str:
        return os.path.join(self.features_dir, self.descriptor_file_prefix + ("reference" if reference else "query") + "_features.npy")

    def _describe(self, images_list) -> np.ndarray:
        if self.global_descriptor is None:
            raise _missing("HLocLocalizer.compute_global_descriptor needs a global image descriptor (upstream: NetVLAD): "
                           "HLocLocalizer(..., global_descriptor=f) with f(img) -> (D,) float32")
        rows = []
        for img in images_list:
            if isinstance(img, (str, os.PathLike)):
                img = load_rgb_png(img)
            rows.append(np.asarray(self.global_descriptor(img), dtype=np.float32).reshape(-1))
        return np.ascontiguousarray(np.stack(rows, axis=0))

    def compute_global_descriptor(self, images_list, reference=True, overwrite=True, descriptor_filename=""):
        """Reference descriptors are cached as <features_dir>/<name>_reference_features.npy, one (N, D) float32 array (upstream: one
        HDF5 group per image); overwrite=False reuses a cache with one row per image."""
        if not self.dataset_name:
            self.dataset_name = descriptor_filename
        self.descriptor_file_prefix = (self.dataset_name + "_") if self.dataset_name else "tmp_"
        path = self._features_path(reference)
        if not reference:
            self.query_features_path = path
            self.query_desc = self._describe(images_list)
            return True
        self.ref_features_path = path
        desc = None
        if os.path.exists(path) and not overwrite:
            cached = np.load(path)
            if cached.ndim == 2 and cached.shape[0] == len(images_list):
                desc = np.ascontiguousarray(cached, dtype=np.float32)
        if desc is None:
            desc = self._describe(images_list)
            np.save(path, desc)
        self.ref_desc, self._ref_desc_dev = desc, None
        return True

    # ------------------------------------------------------------------ retrieval (:408-447)
    def localize_agent(self, rgb_obs):
        """the most similar reference frame's id and its score"""
        from .. import ops
        from ..device import DeviceArray
        if self.ref_desc is None:
            if not self.image_paths_list:
                raise _missing("HLocLocalizer.localize_agent needs reference frames: init_video_with_images_folder(...) and "
                               "compute_global_descriptor(image_paths_list, reference=True)")
            self.compute_global_descriptor(self.image_paths_list, reference=True, overwrite=False)
        self.compute_global_descriptor(rgb_obs if isinstance(rgb_obs, list) else [rgb_obs], reference=False, overwrite=True)
        if self._ref_desc_dev is None:
            self._ref_desc_dev = DeviceArray.from_numpy(self.ref_desc)
        top_id, max_sim = ops.retrieve_frame(self._ref_desc_dev, self.query_desc)
        self.current_frame_id = int(top_id[0])
        return int(top_id[0]), float(max_sim[0])

    # ------------------------------------------------------------------ relative pose (:449-515)
    def match_keypoints(self, rgb_ref, rgb_obs, vis: bool = False):
        if self.matcher is None:
            raise _missing("HLocLocalizer needs a key-point matcher (upstream: SuperPoint + SuperGlue): HLocLocalizer(..., matcher=m) "
                           "with m(img_ref, img_query) -> (mkpts0 (M, 2), mkpts1 (M, 2), confidence (M,))")
        mkpts0, mkpts1, confidence = self.matcher(rgb_ref, rgb_obs)
        return np.asarray(mkpts0), np.asarray(mkpts1), np.asarray(confidence)

    def _get_relative_pose_with_depth(self, rgb_ref, rgb_obs, depth_ref, ref_intr_mat=None, query_intr_mat=None, vis: bool = False):
        """4 x 4: the query camera in the reference camera's frame, inv([R|t; 0 0 0 1]); None below 100 matches (before any GPU
        work) and when the refined pose has fewer than min_inliers inliers (default ceil(0.1 M'))."""
        from .. import ops
        mkpts0, mkpts1, _ = self.match_keypoints(rgb_ref, rgb_obs, vis=vis)
        self.last_estimate = None
        if mkpts0.shape[0] < MIN_MATCHES:
            return None
        h, w = np.asarray(depth_ref).shape if not hasattr(depth_ref, "ptr") else depth_ref.shape
        if ref_intr_mat is None:
            ref_intr_mat = get_sim_cam_mat(h, w)
        if query_intr_mat is None:
            query_intr_mat = get_sim_cam_mat(h, w)
        corr = ops.loc_lift(depth_ref, ref_intr_mat, mkpts0, mkpts1)
        need = self.min_inliers if self.min_inliers is not None else int(math.ceil(INLIER_RATIO * corr.count))
        need = max(int(need), 3)
        if corr.count < need:
            self.last_estimate = dict(matches=int(mkpts0.shape[0]), lifted=corr.count, inliers=0, min_inliers=need)
            return None
        est = ops.pnp_ransac(corr, None, query_intr_mat, max_error=self.max_error, n_hyp=self.n_hyp, seed=self.seed)
        if est.count < 3:
            self.last_estimate = dict(matches=int(mkpts0.shape[0]), lifted=corr.count, inliers=est.count, min_inliers=need)
            return None
        ref = ops.pnp_refine(corr, None, est.pose_dev, query_intr_mat, max_error=self.max_error)
        self.last_estimate = dict(matches=int(mkpts0.shape[0]), lifted=corr.count, ransac_inliers=est.count, inliers=ref.count, min_inliers=need,
                                  cost=ref.cost, iterations=ref.iterations, pose=ref.pose, mask=ref.mask)
        if ref.count < need:
            return None
        transform = np.eye(4)
        transform[:3, :4] = ref.pose
        return np.linalg.inv(transform)

    def _load_depth(self, path: str) -> np.ndarray:
        if self.depth_extension == ".npy":
            return load_depth_npy(path).astype(float)
        from PIL import Image
        with Image.open(path) as im:                       # 16-bit PNG, cv2.IMREAD_ANYDEPTH upstream
            return np.asarray(im).astype(float)

    def localize_agent_with_depth(self, rgb_obs: np.ndarray, ref_intr_mat: np.ndarray = None, query_intr_mat: np.ndarray = None,
                                  depth_scale: float = 1.0, vis: bool = False) -> Tuple[int, Optional[np.ndarray]]:
        """(reference frame id, 4 x 4 relative pose), or (-1, None).  depth_scale: real depth / saved depth.  Reference: :517-558."""
        img_id, _ = self.localize_agent(rgb_obs)
        if not self.depth_paths_list:
            raise _missing("HLocLocalizer.localize_agent_with_depth needs the reference depth images: init_depth_with_depth_folder(...)")
        ref_img = load_rgb_png(self.image_paths_list[img_id])
        ref_depth = self._load_depth(self.depth_paths_list[img_id]) * depth_scale
        transform = self._get_relative_pose_with_depth(ref_img, rgb_obs, ref_depth, ref_intr_mat=ref_intr_mat, query_intr_mat=query_intr_mat,
                                                       vis=vis)
        if transform is None:
            return -1, None
        return img_id, transform


def get_frames_tfs(localizer: HLocLocalizer, segment_frames: List[np.ndarray], pose_list, init_tf_inv: np.ndarray,
                   ref_cam_mat: np.ndarray = None, query_cam_mat: np.ndarray = None, masked_obst: np.ndarray = None,
                   vis: bool = False) -> List[Optional[np.ndarray]]:
    """the habitat camera pose of every frame of a sound segment relative to the first frame, None where a frame could not be
    localized.  pose_list: per reference frame a pose file or a (px, py, pz, qx, qy, qz, qw) row.  Reference: :561-592."""
    tfs = []
    for frame in segment_frames:
        ref_img_id, transform = localizer.localize_agent_with_depth(frame, ref_intr_mat=ref_cam_mat, query_intr_mat=query_cam_mat, vis=vis)
        if ref_img_id == -1:
            tfs.append(None)
            continue
        tf = init_tf_inv @ get_cam_pose_habitat(pose_list[ref_img_id])
        tfs.append(tf @ transform)
    return tfs


def get_cam_pose_habitat(pose, camera_height: float = 1.5) -> np.ndarray:
    """the habitat camera pose of a base pose (a pose file's first line or a 7-vector): the rotation turned about x by 180 degrees
    and the position raised by the camera height.  Reference: :623-636."""
    if isinstance(pose, (str, os.PathLike)):
        with open(pose, "r") as f:
            row = [float(x) for x in f.readline().split()]
    else:
        row = [float(x) for x in np.asarray(pose, dtype=np.float64).reshape(-1)]
    pos = np.array(row[:3], dtype=float)
    rot = R.from_quat(row[3:7]).as_matrix() @ np.diag([1.0, -1.0, -1.0])
    pos[1] += camera_height
    out = np.eye(4)
    out[:3, :3] = rot
    out[:3, 3] = pos
    return out


def save_hab_tf(save_path: str, tf: Optional[np.ndarray]) -> None:
    """Reference: :639-644 (an empty file for a frame that was not localized)"""
    with open(save_path, "w") as f:
        if tf is None:
            return
        f.write(",".join(str(x) for x in np.asarray(tf).flatten().tolist()))
