"""2-D viewsheds on the explored map (csrc/avl_viewshed.hip): the unknown cells a candidate cell would see within
sensor range, per 45-degree sector, and the cells a set of eyes sees.  Upstream has no counterpart.

The sight line is line_of_sight's integer walk without the height axis, from the EYE to the TARGET (it is not symmetric), between
cell centres of one 2-D map: this is not the 3-D sight of ops/sight.py, and the only field of view is a sum of sectors."""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _image_shape, _image_u8, _result
from .explore import EXPLORE_MAX_SIDE, _mask_dtype_check

VIEWSHED_MAX_RADIUS = 127       # kViewMaxRadius: a window row of 2 R + 1 cells fits the 256 bits of an LDS bit row


def octant_of(dr, dc):
    """The sector of the offsets (dr, dc), vectorised: k = [k * 45, (k + 1) * 45) degrees of atan2(dr, dc), decided in integers.  If
    dc > 0 and dr >= 0 the sector is 0 when dr < dc, else 1; otherwise (dr, dc) becomes (-dc, dr), 2 is added and the rule repeats.
    -> int64 array of the broadcast shape; -1 for the zero offset, which has no sector."""
    dr, dc = np.broadcast_arrays(np.asarray(dr), np.asarray(dc))
    if dr.dtype.kind not in "iu" or dc.dtype.kind not in "iu":
        raise TypeError(f"octant_of: integer offsets, got {dr.dtype} and {dc.dtype}")
    dr, dc = dr.astype(np.int64), dc.astype(np.int64)
    zero = (dr == 0) & (dc == 0)
    k = np.zeros(dr.shape, np.int64)
    for _ in range(3):
        turn = ~((dc > 0) & (dr >= 0))
        dr, dc = np.where(turn, -dc, dr), np.where(turn, dr, dc)
        k += 2 * turn
    k += dr >= dc
    k[zero] = -1
    return k


def best_heading(gain, fov_octants=2):
    """-> (start (E,) int64, total (E,) int64): per row of gain (E, 8) (or one row (8,), then two scalars) the first sector of the
    cyclic run of fov_octants sectors with the largest sum -- the first such run among equals -- and that sum."""
    g = np.asarray(gain)
    one = g.ndim == 1
    if one:
        g = g[None]
    if g.ndim != 2 or g.shape[1] != 8:
        raise ValueError(f"best_heading: gain must be (E, 8) or (8,), got shape {np.asarray(gain).shape}")
    g = g.astype(np.int64)
    n = int(fov_octants)
    if not 1 <= n <= 8:
        raise ValueError(f"best_heading: fov_octants {fov_octants} (1 .. 8)")
    runs = sum(np.roll(g, -j, axis=1) for j in range(n))
    start = np.argmax(runs, axis=1).astype(np.int64)                # the first maximum
    total = runs[np.arange(len(g)), start] if len(g) else np.zeros((0,), np.int64)
    return (int(start[0]), int(total[0])) if one else (start, total)


def _eyes_arg(eyes, who):
    """(E, 2) int32 cells, host or device -> (the argument ready for as_device, E)"""
    shape = _image_shape(eyes)
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"{who}: eyes must be (E, 2) cells (row, col), got shape {shape}")
    if isinstance(eyes, (DeviceArray, DeviceView)):
        if eyes.dtype != np.dtype(np.int32):
            raise TypeError(f"{who}: eyes are int32 values, got {eyes.dtype}")
    elif _is_torch(eyes):
        if str(eyes.dtype) != "torch.int32":
            raise TypeError(f"{who}: eyes are int32 values, got {eyes.dtype}")
    else:
        eyes = np.asarray(eyes)
        if eyes.dtype.kind not in "iu" or (eyes.size and not (-2 ** 31 <= int(eyes.min()) and int(eyes.max()) <= 2 ** 31 - 1)):
            raise TypeError(f"{who}: eyes are int32 values, got {eyes.dtype}")
    return eyes, shape[0]


def _viewshed_args(who, free, explored, eyes, radius):
    """every check that needs no device -> (shape, eyes, E, radius)"""
    _mask_dtype_check(free, "free")
    _mask_dtype_check(explored, "explored")
    shape = _image_shape(free)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1 or _image_shape(explored) != shape:
        raise ValueError(f"{who}: expected two non-empty 2-D masks of one shape, got {shape} and {_image_shape(explored)}")
    if max(shape) > EXPLORE_MAX_SIDE:
        raise ValueError(f"{who}: sides up to {EXPLORE_MAX_SIDE}, got {shape}")
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)):
        raise TypeError(f"{who}: radius is an integer number of cells, got {radius!r}")
    if not 1 <= int(radius) <= VIEWSHED_MAX_RADIUS:
        raise ValueError(f"{who}: radius {radius} (1 .. {VIEWSHED_MAX_RADIUS} cells)")
    eyes, E = _eyes_arg(eyes, who)
    return shape, eyes, E, int(radius)


def viewshed_gain(free, explored, eyes, radius, opaque_unknown=False, device=False, stream=None):
    """(E, 8) int32: for every eye of `eyes` (E, 2) int32 (row, col) and every sector (octant_of) the number of unknown cells --
    free != 0 and explored == 0 -- within `radius` cells (dr^2 + dc^2 <= radius^2) that have a free sight line from the eye; a row
    of -1 for an eye outside the image (avl_viewshed_gain; the walk is defined at the top of csrc/avl_viewshed.hip).  Cells with
    free == 0 block the line, with opaque_unknown unknown cells block as well (only the first layer of unknown cells behind known
    space counts); the eye's own cell never blocks, the target is never tested, and an eye may stand on any cell.  free, explored:
    bool / uint8 masks of one shape, host or device, as frontier_mask's; eyes: a host array, a DeviceArray / DeviceView or a GPU
    tensor; 1 <= radius <= VIEWSHED_MAX_RADIUS; E = 0 is valid.  TypeError on other dtypes, ValueError on bad shapes or a radius
    outside the range, before any device work."""
    _, eyes, E, radius = _viewshed_args("viewshed_gain", free, explored, eyes, radius)
    lib = _lib.load()
    _lib.require_gpu()
    out = DeviceArray((E, 8), np.int32)
    keep = ()
    if E:
        fp, (H, W), k1 = _image_u8(free, stream)
        xp, _, k2 = _image_u8(explored, stream)
        ep, _, k3 = as_device(eyes, np.int32, stream)
        _lib.check(lib.avl_viewshed_gain(fp, xp, H, W, ep, E, radius, int(bool(opaque_unknown)), out.ptr, stream), "avl_viewshed_gain")
        keep = (k1, k2, k3)
    return _result(out, device, stream, keep=keep)


def viewshed_seen(free, explored, eyes, radius, opaque_unknown=False, out=None, device=False, stream=None):
    """(H, W) uint8: 1 on every cell, of any class, that is visible from at least one of the M eyes (viewshed_gain's rule: inside
    the image, within `radius`, no blocking cell strictly between) and on the eyes' own cells; eyes outside the image contribute
    nothing (avl_viewshed_seen).  explored | seen is what a visit of the eyes would add.  out: None, or an (H, W) uint8 mask the
    ones are OR-ed into -- a host array (updated in place and returned), or a DeviceArray / GPU tensor (updated in place; returned
    as it is with device=True, else copied back).  M = 0 is valid.  Errors as viewshed_gain's, before any device work."""
    shape, eyes, M, radius = _viewshed_args("viewshed_seen", free, explored, eyes, radius)
    host_out = None
    if out is not None:
        odt = str(out.dtype) if _is_torch(out) else np.dtype(getattr(out, "dtype", object))
        if odt not in ("torch.uint8", np.dtype(np.uint8)):
            raise TypeError(f"viewshed_seen: out must be uint8, got {odt}")
        if _image_shape(out) != shape:
            raise ValueError(f"viewshed_seen: out must be {shape}, got shape {_image_shape(out)}")
        if isinstance(out, np.ndarray):
            host_out = out
    lib = _lib.load()
    _lib.require_gpu()
    fp, (H, W), k1 = _image_u8(free, stream)
    xp, _, k2 = _image_u8(explored, stream)
    ep, k3 = None, None
    if M:
        ep, _, k3 = as_device(eyes, np.int32, stream)
    if out is None:
        seen = DeviceArray((H, W), np.uint8)
    elif host_out is not None:
        seen = DeviceArray.from_numpy(host_out, stream)
    else:
        seen = out
    sp = as_device(seen, np.uint8, stream)[0]
    _lib.check(lib.avl_viewshed_seen(fp, xp, H, W, ep, M, radius, int(bool(opaque_unknown)), int(out is not None), sp, stream),
               "avl_viewshed_seen")
    if device:
        if isinstance(seen, DeviceArray):
            seen._keep = (k1, k2, k3)
        else:
            _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")          # the staged inputs may be released on return
        return seen
    if host_out is None:
        res = np.empty((H, W), np.uint8)
    else:
        res = host_out if host_out.flags["C_CONTIGUOUS"] else np.empty((H, W), np.uint8)
    _lib.check(lib.avl_memcpy_d2h(res.ctypes.data, sp, res.nbytes, stream), "avl_memcpy_d2h")       # (synchronous: the staged inputs may go)
    if host_out is not None and res is not host_out:
        np.copyto(host_out, res)
    return res if host_out is None else host_out
