"""Cell-to-cell line of sight through a voxel map (csrc/avl_sight.hip): which target cells can be seen from which
eye cells, on the CellIndex of ops/audit.py.  Upstream has no counterpart.

The sight line is the audit's integer walk from the EYE to the TARGET (it is not symmetric); lines run between cell centres, and
neither a field of view nor a heading is modelled."""
from __future__ import annotations

import math

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _dev_u8
from .audit import CellIndex, _cells_i32

LOS_VISIBLE = -1            # line_of_sight: no blocker between the two cells
LOS_INVALID = -2            # line_of_sight: an end of the pair lies outside the grid
LOS_MAX_TARGETS = 65536     # visible_counts: targets per call


def _sight_cells(x, what):
    """_cells_i32, and the dtype of a device array checked here already: nothing is uploaded before every argument is looked at"""
    x, n = _cells_i32(x, what)
    if isinstance(x, (DeviceArray, DeviceView)):
        if x.dtype != np.dtype(np.int32):
            raise TypeError(f"{what}: cells are int32 values, got {x.dtype}")
    elif _is_torch(x) and str(x.dtype) != "torch.int32":
        raise TypeError(f"{what}: cells are int32 values, got {x.dtype}")
    return x, n


def _transparent_arg(x, who, N):
    """the optional per-voxel mask: None, or a bool / uint8 array of shape (N,), host or device"""
    if x is None:
        return None
    if _is_torch(x):
        ok = str(x.dtype) in ("torch.uint8", "torch.bool")
    elif isinstance(x, (DeviceArray, DeviceView)):
        ok = x.dtype == np.dtype(np.uint8)                   # (a device array is taken as it is: one byte per voxel)
    else:
        ok = isinstance(x, np.ndarray) and x.dtype in (np.dtype(np.uint8), np.dtype(bool))
    if not ok:
        raise TypeError(f"{who}: transparent must be uint8 or bool, got {getattr(x, 'dtype', type(x).__name__)}")
    if tuple(int(s) for s in x.shape) != (N,):
        raise ValueError(f"{who}: transparent must be ({N},), got shape {tuple(x.shape)}")
    return x


def _sight_common(who, index, transparent, end_margin):
    if not isinstance(index, CellIndex):
        raise TypeError(f"{who}: expected a CellIndex, got {type(index).__name__}")
    end_margin = int(end_margin)
    if end_margin < 0:
        raise ValueError(f"{who}: end_margin {end_margin} < 0")
    return _transparent_arg(transparent, who, index.N), min(end_margin, 2 ** 31 - 1)


def line_of_sight(index: CellIndex, eyes, targets, transparent=None, end_margin=0, device=False, stream=None):
    """(M,) int32, one value per pair eyes[m] -> targets[m] (both (M, 3) cells (row, col, h); host arrays, DeviceArray / DeviceView
    or GPU tensors): LOS_VISIBLE (-1) when no cell strictly between the eye and the last end_margin + 1 cells of the walk is
    occupied, LOS_INVALID (-2) when either end lies outside the grid, else the voxel row of the first blocker (avl_los_pairs; the
    walk and the blockers are defined at the top of csrc/avl_sight.hip).  The walk runs from the eye to the target and is not
    symmetric.  transparent: an optional (N,) uint8 / bool array; voxels where it is non-zero do not block.  TypeError on a
    non-CellIndex, non-integer cells or another transparent dtype, ValueError on bad shapes, a negative margin or eyes and targets
    of different lengths, before any device work."""
    transparent, end_margin = _sight_common("line_of_sight", index, transparent, end_margin)
    eyes, M = _sight_cells(eyes, "line_of_sight: eyes")
    targets, Mt = _sight_cells(targets, "line_of_sight: targets")
    if M != Mt:
        raise ValueError(f"line_of_sight: {M} eyes and {Mt} targets")
    lib = _lib.load()
    _lib.require_gpu()
    ip = index.ptr                                      # a closed index raises here
    out = DeviceArray((M,), np.int32)
    keep = ()
    if M:
        ep, _, ke = as_device(eyes, np.int32, stream)
        tp, _, kt = as_device(targets, np.int32, stream)
        xp, _, kx = (None, None, None) if transparent is None else _dev_u8(transparent, stream)
        _lib.check(lib.avl_los_pairs(ip, index.nbytes, index.N, index.gs, index.vh, ep, tp, M, xp, end_margin, out.ptr, stream),
                   "avl_los_pairs")
        keep = (ke, kt, kx)
    if device:
        out._keep = keep + (index,)
        return out
    return out.numpy(stream)


def visible_counts(index: CellIndex, eyes, targets, transparent=None, end_margin=0, max_range=None, want_first=True, device=False,
                   stream=None):
    """-> (visible (E,) uint32, first (E,) int32 or None): for every eye of `eyes` (E, 3) the number of the T cells of `targets`
    (T, 3) that lie inside the grid, within max_range and have a free sight line from the eye (line_of_sight's, with the same
    transparent and end_margin), and the smallest such target index, -1 when there is none (None with want_first=False)
    (avl_los_count).  An eye outside the grid sees nothing.  max_range is in cells, None = unlimited: a pair is in range when
    dr^2 + dc^2 + dh^2 <= max_range2 = floor(float(max_range) ** 2) -- the square is taken in float64, the floor as a Python integer;
    equality counts.  T <= LOS_MAX_TARGETS; E = 0 and T = 0 are valid.  With device=True both results are DeviceArrays.  Errors as
    line_of_sight's, and ValueError on too many targets or a max_range that is negative or not finite, before any device work."""
    transparent, end_margin = _sight_common("visible_counts", index, transparent, end_margin)
    eyes, E = _sight_cells(eyes, "visible_counts: eyes")
    targets, T = _sight_cells(targets, "visible_counts: targets")
    if T > LOS_MAX_TARGETS:
        raise ValueError(f"visible_counts: {T} targets (at most {LOS_MAX_TARGETS} per call)")
    if max_range is None:
        max_range2 = -1
    else:
        max_range = float(max_range)
        if not (math.isfinite(max_range) and max_range >= 0.0):
            raise ValueError(f"visible_counts: max_range {max_range} (cells; finite and >= 0, or None)")
        max_range2 = min(math.floor(max_range * max_range), 2 ** 62)
    lib = _lib.load()
    _lib.require_gpu()
    ip = index.ptr                                      # a closed index raises here
    visible = DeviceArray((E,), np.uint32)
    first = DeviceArray((E,), np.int32) if want_first else None
    keep = ()
    if E:
        ep, _, ke = as_device(eyes, np.int32, stream)
        tp, _, kt = as_device(targets, np.int32, stream)
        xp, _, kx = (None, None, None) if transparent is None else _dev_u8(transparent, stream)
        _lib.check(lib.avl_los_count(ip, index.nbytes, index.N, index.gs, index.vh, ep, E, tp, T, xp, end_margin, max_range2,
                                     visible.ptr, first.ptr if want_first else None, stream), "avl_los_count")
        keep = (ke, kt, kx)
    if device:
        visible._keep = keep + (index,)
        if want_first:
            first._keep = visible._keep
        return visible, first
    return visible.numpy(stream), (first.numpy(stream) if want_first else None)
