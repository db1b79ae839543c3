"""Observed free space and its frontier (csrc/avl_explore.hip)."""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device, _is_torch
from ._args import _image_shape, _image_u8, _result
from ._rays import frame_args
from .builder import _global_depth

EXPLORE_MAX_SIDE = 16384
NEVER_SEEN = -1             # first_seen of a cell no sight ray crossed


def _mask_dtype_check(x, what):
    """bool / uint8 masks only (host array, DeviceArray / DeviceView or torch tensor): anything else would be cast quietly"""
    if _is_torch(x):
        ok = str(x.dtype) in ("torch.bool", "torch.uint8")
    else:
        ok = hasattr(x, "dtype") and np.dtype(x.dtype) in (np.dtype(bool), np.dtype(np.uint8))
    if not ok:
        raise TypeError(f"{what} must be a bool or uint8 mask, got {getattr(x, 'dtype', type(x).__name__)}")


def carve_free_space(first_seen, depth, calib, transforms, frame_ids, gs, cs, stride=4, h_min=0.0, h_max=1.5, min_depth=0.1,
                     max_depth=6.0, depth_div=1000.0, device=False, stream=None):
    """Fold the sight rays of F depth frames into first_seen (gs, gs) int32: the smallest frame id whose rays crossed a cell inside
    the height band [h_min, h_max], NEVER_SEEN (-1) where none did (avl_carve_free_space; the ray is defined at the top of
    csrc/avl_explore.hip).  first_seen: None (a new map), a host int32 array (updated in place and returned), or an int32
    DeviceArray / GPU tensor (updated in place; returned as it is with device=True, else copied back).  depth: (F, H, W) or (H, W),
    uint16 (value / depth_div metres) or float32 metres, host or device; calib: the 3 x 3 camera matrix; transforms: (F, 4, 4)
    camera -> map (VLMapBuilder.frame_transforms); frame_ids: (F,) ids >= 0.  The fold is a minimum: calls may come in any order
    and continue each other.  TypeError on other dtypes, ValueError on bad shapes or parameters, before any device work."""
    gs, stride = int(gs), int(stride)
    if not 1 <= gs <= EXPLORE_MAX_SIDE:
        raise ValueError(f"carve_free_space: grid size {gs} (1 .. {EXPLORE_MAX_SIDE})")
    F, H, W, Kinv, T, ids = frame_args("carve_free_space", depth, calib, transforms, frame_ids, stride, cs, min_depth, max_depth,
                                       h_band=(h_min, h_max))
    host_map = None
    if first_seen is not None:
        fdt = str(first_seen.dtype) if _is_torch(first_seen) else np.dtype(getattr(first_seen, "dtype", object))
        if fdt not in ("torch.int32", np.dtype(np.int32)):
            raise TypeError(f"first_seen must be int32, got {fdt}")
        if tuple(first_seen.shape) != (gs, gs):
            raise ValueError(f"carve_free_space: first_seen must be ({gs}, {gs}), got shape {tuple(first_seen.shape)}")
        if isinstance(first_seen, np.ndarray):
            host_map = first_seen
    lib = _lib.load()
    _lib.require_gpu()
    if first_seen is None:
        fs = DeviceArray((gs, gs), np.int32)
        _lib.check(lib.avl_memset(fs.ptr, 0xFF, fs.nbytes, stream), "avl_memset")       # every cell NEVER_SEEN
        fp = fs.ptr
    elif host_map is not None:
        fs = DeviceArray.from_numpy(host_map, stream)
        fp = fs.ptr
    else:
        fp, fs = as_device(first_seen, np.int32, stream)[0], first_seen
    keep_d = None
    if F:
        dp, _, keep_d, is_u16 = _global_depth(depth, stream)
        _lib.check(lib.avl_carve_free_space(dp, int(is_u16), float(depth_div), F, H, W, Kinv.ctypes.data, T.ctypes.data, ids.ctypes.data,
                                            gs, float(cs), stride, float(h_min), float(h_max), float(min_depth), float(max_depth), fp,
                                            stream), "avl_carve_free_space")
    if device:
        if isinstance(fs, DeviceArray):
            fs._keep = (keep_d,)
        else:
            _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")          # the staged depth may be released on return
        return fs
    out = host_map if host_map is not None and host_map.flags["C_CONTIGUOUS"] else np.empty((gs, gs), np.int32)
    _lib.check(lib.avl_memcpy_d2h(out.ctypes.data, fp, out.nbytes, stream), "avl_memcpy_d2h")       # (synchronous: the staged depth may go)
    if host_map is not None and out is not host_map:
        np.copyto(host_map, out)
    return out if host_map is None else host_map


def frontier_mask(free, explored, device=False, stream=None):
    """(H, W) uint8: 1 where a cell is explored and free and at least one of its 4 neighbours inside the image is unknown, i.e. not
    explored and free (avl_frontier_mask).  A cell that holds an obstacle is known whether or not a ray crossed it.  free, explored:
    bool / uint8 masks of one shape, host or device; any other dtype raises TypeError."""
    _mask_dtype_check(free, "free")
    _mask_dtype_check(explored, "explored")
    shape = _image_shape(free)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1 or _image_shape(explored) != shape:
        raise ValueError(f"frontier_mask: expected two non-empty 2-D masks of one shape, got {shape} and {_image_shape(explored)}")
    if max(shape) > EXPLORE_MAX_SIDE:
        raise ValueError(f"frontier_mask: sides up to {EXPLORE_MAX_SIDE}, got {shape}")
    lib = _lib.load()
    _lib.require_gpu()
    fp, (H, W), k1 = _image_u8(free, stream)
    ep, _, k2 = _image_u8(explored, stream)
    out = DeviceArray((H, W), np.uint8)
    _lib.check(lib.avl_frontier_mask(fp, ep, H, W, out.ptr, stream), "avl_frontier_mask")
    return _result(out, device, stream, keep=(k1, k2))
