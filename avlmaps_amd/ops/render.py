"""Headless rendering of heat maps (csrc/avl_render.hip)."""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device
from ._args import _is_dev, _result, _workspace

RENDER_MAX_SIDE = 8192


def jet_table() -> np.ndarray:
    """(256, 3) uint8 RGB: OpenCV's COLORMAP_JET built from its published definition, the piecewise-linear
    red(x) = clip(1.5 - |4 x - 3|, 0, 1), green(x) = clip(1.5 - |4 x - 2|, 0, 1), blue(x) = clip(1.5 - |4 x - 1|, 0, 1) at
    x = i / 255, scaled by 255 and rounded to the nearest byte, halves to even (dark blue (0, 0, 128) at 0, dark red (128, 0, 0)
    at 255).  NOT compared with the library: OpenCV is not installed where this project is built and tested, so single entries may
    differ from cv2's by a rounding step.  The kernels take the table as data; with OpenCV at hand pass
    cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET)[:, 0, ::-1] instead."""
    i = np.arange(256, dtype=np.int64)
    # in integers, doubled so that the half steps stay exact: 2 * 255 * channel = clip(765 - |8 i - 510 c|, 0, 510), c = 3, 2, 1
    twice = np.stack([np.clip(765 - np.abs(8 * i - 510 * c), 0, 510) for c in (3, 2, 1)], axis=1)
    half = twice // 2
    return (half + ((twice & 1) & (half & 1))).astype(np.uint8)          # an odd `twice` is a half: it goes to the even neighbour


def _heat_arg(heat, stream):
    """(N,) float32 / float64 heat, host or device -> (ptr, N, is_f64, keepalive); other dtypes are a TypeError (the index
    (heat * 255).astype(uint8) is computed in the heat's own dtype, so nothing is converted silently)"""
    if not _is_dev(heat):
        heat = np.asarray(heat)
    dt = np.dtype(str(heat.dtype).replace("torch.", ""))
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"heat must be float32 or float64, got {dt}")
    ptr, shape, keep = as_device(heat, dt, stream)
    n = int(np.prod(shape, dtype=np.int64))
    return ptr, n, int(dt == np.float64), keep


def _table_arg(table, stream):
    if table is None:
        table = jet_table()
    if isinstance(table, np.ndarray):
        if table.dtype != np.uint8 or table.shape != (256, 3):
            raise ValueError(f"the colour table must be (256, 3) uint8, got {table.dtype} {table.shape}")
    ptr, shape, keep = as_device(table, np.uint8, stream)
    if tuple(shape) != (256, 3):
        raise ValueError(f"the colour table must be (256, 3) uint8, got shape {tuple(shape)}")
    return ptr, keep


def _rgb_arg(rgb, n, stream):
    """(n, 3) uint8 colours, host or device; a host array of another dtype is cast like ops.rgb_topdown casts grid_rgb"""
    if isinstance(rgb, np.ndarray):
        rgb = np.ascontiguousarray(rgb).astype(np.uint8, copy=False)
    ptr, shape, keep = as_device(rgb, np.uint8, stream)
    if int(np.prod(shape, dtype=np.int64)) != 3 * n:
        raise ValueError(f"expected {n} RGB triples, got shape {tuple(shape)}")
    return ptr, keep


def _background3(background):
    bg = np.ascontiguousarray(np.asarray(background, dtype=np.uint8).reshape(3))
    return bg


def colorize_heat(heat, grid_rgb, transparency=0.5, table=None, as_uint8=False, device=False, stream=None):
    """convert_heatmap_to_rgb (visualize_utils.py:59-64) per voxel on the GPU, NumPy 2's bits:
        idx = (heat * 255).astype(np.uint8)                       (the product in the heat's dtype, float32 or float64)
        out = table[idx].astype(np.float32) * transparency + grid_rgb * (1 - transparency)          -> (N, 3) float64
    as_uint8=True: out.astype(np.uint8) instead, the truncation visualize_rgb_map_2d applies, (N, 3) uint8.
    table: (256, 3) uint8 RGB, default jet_table().  A heat outside [0, 1] or NaN raises AvlError (the uint8 cast is undefined
    there; nothing is clamped).  Inputs host or device-resident; device=True returns the DeviceArray."""
    lib = _lib.load()
    _lib.require_gpu()
    hp, n, is_f64, k1 = _heat_arg(heat, stream)
    rp, k2 = _rgb_arg(grid_rgb, n, stream)
    tp, k3 = _table_arg(table, stream)
    out = DeviceArray((n, 3), np.uint8 if as_uint8 else np.float64)
    _lib.check(lib.avl_render_colorize(hp, is_f64, rp, tp, n, float(transparency), None if as_uint8 else out.ptr,
                                       out.ptr if as_uint8 else None, stream), "avl_render_colorize")
    return _result(out, device, stream, keep=(k1, k2, k3))


def render_topdown(grid_pos, heat, grid_rgb, gs, window=None, transparency=0.5, table=None, background=(0, 0, 0), device=False,
                   stream=None):
    """The heat over the top-down colour map, (rmax - rmin + 1, cmax - cmin + 1, 3) uint8, without a dense heat image: per cell of
    window = (rmin, rmax, cmin, cmax) (inclusive, default the whole (gs, gs) map) the colour of the column's HIGHEST voxel blended
    with table[idx(the column's largest heat)] as colorize_heat(as_uint8=True) blends; cells without a voxel are `background`.
    Negative positions wrap once and a position outside the map raises AvlError, as ops.rgb_topdown; so does a heat outside [0, 1].
    Not upstream's behaviour: upstream has no such function (visualize_heatmap_2d takes a dense 2-D heat, and its colour map keeps
    the LAST voxel of a column, ops.rgb_topdown)."""
    lib = _lib.load()
    _lib.require_gpu()
    gs = int(gs)
    rmin, rmax, cmin, cmax = (0, gs - 1, 0, gs - 1) if window is None else (int(v) for v in window)
    H, W = rmax - rmin + 1, cmax - cmin + 1
    ws, nws = _workspace(lib.avl_render_topdown_work_bytes, "avl_render_topdown", H, W)      # rejects a bad window before any device work
    pp, pshape, k1 = as_device(grid_pos, np.int32, stream)
    n = int(pshape[0])
    hp, nh, is_f64, k2 = _heat_arg(heat, stream)
    if nh != n:
        raise ValueError(f"{n} voxels but {nh} heat values")
    rp, k3 = _rgb_arg(grid_rgb, n, stream)
    tp, k4 = _table_arg(table, stream)
    bg = _background3(background)
    out = DeviceArray((H, W, 3), np.uint8)
    _lib.check(lib.avl_render_topdown(pp, hp, is_f64, rp, tp, n, gs, rmin, rmax, cmin, cmax, float(transparency), bg.ctypes.data, out.ptr,
                                      ws.ptr, nws, stream), "avl_render_topdown")
    return _result(out, device, stream, keep=(k1, k2, k3, k4, ws))


def render_view(grid_pos, color, T, fx, fy, cx, cy, size, znear=0.5, smax=16, background=(0, 0, 0), device=False, stream=None):
    """A z-buffered splat of the voxels from a pinhole camera, (H, W, 3) uint8 for size = (W, H), each <= RENDER_MAX_SIDE.
    color: (N, 3) uint8 per voxel, normally colorize_heat(..., as_uint8=True, device=True).  T: (3, 4) float64 from cell
    coordinates (row, col, h, 1) to the camera frame (x right, y down, z forward, in cells): utils.visualize_utils.look_at or
    camera_of_frame.  Per voxel, in float64: p = T (row, col, h, 1); culled unless z > znear; u = fx * x / z + cx,
    v = fy * y / z + cy; a square of half-side min(0.5 * fx / z, 0.5 * smax) pixels around (u, v), i.e. pixels floor(u - half) ..
    floor(u + half) by floor(v - half) .. floor(v + half) clipped to the image.  A pixel shows the voxel with the smallest
    (float32(z), id); pixels no voxel covers are `background`.  No shading, no anti-aliasing."""
    lib = _lib.load()
    _lib.require_gpu()
    W, H = int(size[0]), int(size[1])
    ws, nws = _workspace(lib.avl_render_view_work_bytes, "avl_render_view", W, H)
    Tm = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
    if Tm.shape != (3, 4):
        raise ValueError(f"T must be (3, 4), got {Tm.shape}")
    pp, pshape, k1 = as_device(grid_pos, np.int32, stream)
    n = int(pshape[0])
    cp, k2 = _rgb_arg(color, n, stream)
    bg = _background3(background)
    out = DeviceArray((H, W, 3), np.uint8)
    _lib.check(lib.avl_render_view(pp, cp, n, Tm.ctypes.data, float(fx), float(fy), float(cx), float(cy), W, H, float(znear), float(smax),
                                   bg.ctypes.data, out.ptr, ws.ptr, nws, stream), "avl_render_view")
    return _result(out, device, stream, keep=(k1, k2, ws))
