"""The frame arguments of the ops that take the sight rays of depth frames -- carve_free_space, audit_rays, gt_vote, match_frames
(csrc/avl_sightray.h) -- checked and normalised in one place."""
from __future__ import annotations

import numpy as np

from ..device import _is_torch


def frame_args(who, depth, calib, transforms, frame_ids, stride, cs, min_depth, max_depth, h_band=None, depth_div=None):
    """-> (F, H, W, Kinv, T, ids): the frame count and size of depth ((F, H, W) or (H, W), uint16 or float32, host or device), the
    inverse of the 3 x 3 calib, the (F, 4, 4) float64 transforms and the (F,) int32 frame ids (None when frame_ids is None: the
    vote and the pose search have none).  h_band: (h_min, h_max), or None for an op without a height band.  TypeError on another depth dtype,
    ValueError on bad shapes or parameters, with `who` in the messages; nothing here touches the device.

    depth_div is checked only where one is passed, and only audit_rays and match_frames pass it: carve_free_space and gt_vote leave a bad
    divisor of uint16 depths to the library's AvlError, as they always have.  Kept as it is on purpose, not unified here."""
    if stride < 1:
        raise ValueError(f"{who}: stride {stride} < 1")
    if not (np.isfinite(cs) and cs > 0):
        raise ValueError(f"{who}: cell size {cs}")
    if h_band is not None and not (np.isfinite(h_band[0]) and np.isfinite(h_band[1]) and h_band[0] <= h_band[1]):
        raise ValueError(f"{who}: height band [{h_band[0]}, {h_band[1]}]")
    if not (np.isfinite(min_depth) and np.isfinite(max_depth) and 0 <= min_depth < max_depth):
        raise ValueError(f"{who}: depth range ({min_depth}, {max_depth})")
    ddt = str(depth.dtype) if _is_torch(depth) else np.dtype(getattr(depth, "dtype", object))
    if ddt not in ("torch.uint16", "torch.int16", "torch.float32", np.dtype(np.uint16), np.dtype(np.float32)):
        raise TypeError(f"depth must be uint16 (value / depth_div metres) or float32 metres, got {ddt}")
    if depth_div is not None and ddt in ("torch.uint16", "torch.int16", np.dtype(np.uint16)) and not (np.isfinite(depth_div) and depth_div > 0):
        raise ValueError(f"{who}: depth_div {depth_div}")
    dshape = tuple(int(s) for s in depth.shape)
    if len(dshape) == 2:
        dshape = (1,) + dshape
    if len(dshape) != 3 or dshape[1] < 1 or dshape[2] < 1:
        raise ValueError(f"{who}: depth must be (F, H, W) or (H, W), got shape {tuple(depth.shape)}")
    F, H, W = dshape
    K = np.asarray(calib, dtype=np.float64)
    if K.size != 9:
        raise ValueError(f"{who}: calib must be 3 x 3, got shape {K.shape}")
    T = np.ascontiguousarray(transforms, dtype=np.float64)
    if T.shape not in ((F, 4, 4), (4, 4)) or T.size != F * 16:
        raise ValueError(f"{who}: {F} frames but transforms of shape {T.shape}")
    ids = None
    if frame_ids is not None:
        ids = np.ascontiguousarray(np.asarray(frame_ids).reshape(-1))
        if ids.shape[0] != F:
            raise ValueError(f"{who}: {F} frames but {ids.shape[0]} frame ids")
        if F and (ids.dtype.kind not in "iu" or ids.min() < 0 or ids.max() > 2 ** 31 - 2):
            raise ValueError(f"{who}: frame ids are integers in [0, 2^31 - 2]")
        ids = ids.astype(np.int32)
    return F, H, W, np.ascontiguousarray(np.linalg.inv(K.reshape(3, 3))), T, ids
