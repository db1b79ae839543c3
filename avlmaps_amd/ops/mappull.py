"""Resampling a finished voxel map backward: for every cell of the target grid the rows of map B that its centre came from under the
inverse of a 4 x 4 transform, and the voxel gathered from them (csrc/avl_mappull.hip).  ops.move_cells is a forward,
nearest-cell scatter and leaves pinholes under a rotation; this is the inverse mapping.  Upstream has no counterpart."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device
from ._args import _image_shape, _is_dev
from .audit import _cells_i32, _check_grid
from .mapdiff import _feat_shape, _shift3
from .mapfuse import _check_cell_size, _resident, _typed, _use_mask, check_transform, FUSE_ERR_SHARED

PULL_MAX_DIM = 8192
PULL_COUNTS = ("unselected_b", "outside_b", "below_support", "unused_b")
PULL_INTERP = ("nearest", "linear")


def check_interp(interp, who):
    if interp not in PULL_INTERP:
        raise ValueError(f"{who}: interp {interp!r} (one of {', '.join(PULL_INTERP)})")
    return PULL_INTERP.index(interp)


def check_min_support(min_support, who):
    s = float(min_support)
    if not 0.0 < s <= 1.0:
        raise ValueError(f"{who}: min_support {min_support!r} (0 < min_support <= 1)")
    return s


def inverse_transform(transform, who):
    """None, or the float64 inverse of the (4, 4) transform (check_transform), bottom row 0 0 0 1; ValueError when it is singular"""
    T = check_transform(transform, who)
    if T is None:
        return None
    try:
        with np.errstate(all="ignore"):
            P = np.linalg.inv(T)
    except np.linalg.LinAlgError:
        P = None
    if P is None or not np.isfinite(P).all() or not np.abs(P @ T - np.eye(4)).max() <= 1e-6:      # a rank-deficient matrix may invert to garbage
        raise ValueError(f"{who}: the transform is singular")
    P = np.ascontiguousarray(P, dtype=np.float64)
    P[3] = [0.0, 0.0, 0.0, 1.0]
    return P


def _scratch_i32(n_b, gs, vh):
    """the length of avl_map_pull_plan's int32 scratch array, as include/avlmaps_hip.h states it"""
    words = (gs * gs * vh + 31) // 32
    return 4 * n_b + 2 * words + words // 1024 + 512


class PullPlan:
    """pull_plan's result.  n_out target cells in ascending linear cell order ((row * gs + col) * vh + h), whatever the order of B's
    rows -- ops.fuse_plan orders by B's smallest row instead.  cells (n_out, 3) int32; members (n_out, 8) int32: the row of B of every
    corner, -1 = none (nearest mode and transform=None: the sole member in column 0); lam (n_out, 8) float64: the members' lambdas;
    counts (4,) int32 in the order of PULL_COUNTS; occupied_ids (gs, gs, vh) int32 or None.  The arrays are read back from the
    device on first use; the device copies feed pull_rows."""

    def __init__(self, n_b, gs, vh, n_out, counts, dev, stream):
        self.n_b, self.gs, self.vh, self.n_out, self.counts = n_b, gs, vh, int(n_out), counts
        self._dev, self._stream, self._host = dev, stream, {}

    def _get(self, name):
        if name not in self._host:
            d = self._dev[name]
            self._host[name] = None if d is None else d.numpy(self._stream)
        return self._host[name]

    cells = property(lambda self: self._get("cells"))
    members = property(lambda self: self._get("members"))
    lam = property(lambda self: self._get("lam"))
    occupied_ids = property(lambda self: self._get("occupied"))


def pull_plan(cells_b, w_b, gs, cs, vh, transform=None, shift=(0, 0, 0), use_b=None, interp="linear", min_support=0.5, want_occupied=True,
              stream=None, _inverse=None) -> PullPlan:
    """The members of every cell of the gs x gs x vh target grid of cell size cs in map B's cells (n_b, 3) (avl_map_pull_plan, one
    read-back of n_out, avl_map_pull_fill).  `transform` carries B's base frame into the target's (None = identity, integers only);
    the target cell c stands for the centre of c - shift, which goes through the INVERSE transform, inverted here once in float64.
    interp="nearest": the cell of B that the point falls into, lambda 1.  interp="linear": the eight cells of B whose centres bracket
    the point, with trilinear lambdas; the cell exists when the lambdas of the corners that selected rows of B own add up to
    min_support or more.  A row of B is selected when use_b (bool / uint8, None = all) is set, its cell lies inside the grid and its
    weight w_b (float32) is finite and > 0.  ValueError for a singular transform and when two selected rows of B share a cell.  The
    cells come out in ascending linear cell order, not in the forward path's order of B's rows."""
    gs, vh = _check_grid("pull_plan", gs, vh)
    cs = _check_cell_size(cs, "pull_plan")
    P = _inverse if _inverse is not None else inverse_transform(transform, "pull_plan")      # pull_map hands over the inverse it made
    shift = _shift3(shift, "pull_plan")
    mode = check_interp(interp, "pull_plan")
    support = check_min_support(min_support, "pull_plan")
    cells_b, n_b = _cells_i32(cells_b, "pull_plan: cells_b")
    w_b = _typed(w_b, (n_b,), np.float32, "pull_plan: w_b")
    use_b = _use_mask(use_b, n_b, "pull_plan: use_b")
    lib = _lib.load()
    ib = C.c_size_t(0)
    _lib.check(lib.avl_cell_index_work_bytes(n_b, gs, vh, C.byref(ib)), "avl_cell_index_work_bytes")
    _lib.require_gpu()
    si = _scratch_i32(n_b, gs, vh)
    Pp = P.ctypes.data if P is not None else None
    work, dev, keep, mask = [], {}, None, None                      # the scratch goes in any case, the plan's arrays when the plan fails
    try:
        index, scratch, head, counts = (DeviceArray(shape, dt) for shape, dt in (((ib.value,), np.uint8), ((si,), np.int32), ((8,), np.int32),
                                                                                 ((4,), np.int32)))
        work += [index, scratch, head, counts]
        keep = [as_device(cells_b, np.int32, stream), as_device(w_b, np.float32, stream)]
        mask = None if use_b is None else as_device(use_b, np.uint8, stream)
        _lib.check(lib.avl_map_pull_plan(keep[0][0], None if mask is None else mask[0], keep[1][0], n_b, Pp, shift.ctypes.data, gs, cs, vh, mode,
                                         support, index.ptr, ib.value, scratch.ptr, si, head.ptr, stream), "avl_map_pull_plan")
        h = head.numpy(stream)                                      # the one read-back: n_out has no bound from n_b
        if h[2] & FUSE_ERR_SHARED:
            raise ValueError("pull_plan: two selected rows of map B share a cell (one row per cell)")
        n_out = int(h[0])
        for name, shape, dt in (("cells", (n_out, 3), np.int32), ("members", (n_out, 8), np.int32), ("lam", (n_out, 8), np.float64)):
            dev[name] = DeviceArray(shape, dt)
        dev["occupied"] = DeviceArray((gs, gs, vh), np.int32) if want_occupied else None
        _lib.check(lib.avl_map_pull_fill(n_b, Pp, shift.ctypes.data, gs, cs, vh, mode, support, index.ptr, ib.value, scratch.ptr, si, head.ptr, n_out,
                                         dev["cells"].ptr, dev["members"].ptr, dev["lam"].ptr, dev["occupied"].ptr if want_occupied else None,
                                         counts.ptr, stream), "avl_map_pull_fill")
        c = counts.numpy(stream)
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")     # the stream is drained: the scratch may go
    except BaseException:
        for d in dev.values():
            if d is not None:
                d.free()
        raise
    finally:
        del keep, mask
        for d in work:
            d.free()
    return PullPlan(n_b, gs, vh, n_out, c, dev, stream)


def pull_rows(plan: PullPlan, feat_b, w_b, rgb_b, feat_out=None, device=False, stream=None):
    """(grid_feat (n_out, D) float32, weight (n_out,) float32, grid_rgb (n_out, 3) uint8) of a PullPlan (avl_map_pull_rows).  In
    float64, over the members of a voxel in corner order: omega = lambda * weight, grid_feat = sum(omega * f) / sum(omega) with every
    product and sum rounded once, weight = sum(omega) / sum(lambda), rgb like the features, truncated.  A voxel with one member of
    lambda 1 -- every voxel in nearest mode and without a transform -- comes back bit for bit.  The bytes do not depend on the
    alignment of the matrices.  feat_b (n_b, D) float32, w_b (n_b,) float32, rgb_b (n_b, 3) uint8; host arrays, DeviceArray /
    DeviceView or GPU tensors.  feat_out: a caller's (n_out, D) float32 device array to write the rows into."""
    if not isinstance(plan, PullPlan):
        raise TypeError(f"pull_rows: expected a PullPlan, got {type(plan).__name__}")
    n_b, n_out = plan.n_b, plan.n_out
    fb = _feat_shape(feat_b, "pull_rows: feat_b")
    if fb[0] != n_b:
        raise ValueError(f"pull_rows: the plan is of {n_b} rows, the features have {fb[0]}")
    D = fb[1]
    w_b = _typed(w_b, (n_b,), np.float32, "pull_rows: w_b")
    rgb_b = _typed(rgb_b, (n_b, 3), np.uint8, "pull_rows: rgb_b")
    if feat_out is not None:
        if not _is_dev(feat_out) or _image_shape(feat_out) != (n_out, D):
            raise ValueError(f"pull_rows: feat_out is a ({n_out}, {D}) float32 device array")
    lib = _lib.load()
    _lib.require_gpu()
    keep = [as_device(x, dt, stream) for x, dt in ((feat_b, np.float32), (w_b, np.float32), (rgb_b, np.uint8))]
    wout, rgb = DeviceArray((n_out,), np.float32), DeviceArray((n_out, 3), np.uint8)
    feat = feat_out if feat_out is not None else DeviceArray((n_out, D), np.float32)
    d = plan._dev
    _lib.check(lib.avl_map_pull_rows(n_out, d["members"].ptr, d["lam"].ptr, keep[0][0], keep[1][0], keep[2][0], n_b, D,
                                     as_device(feat, np.float32, stream)[0], wout.ptr, rgb.ptr, stream), "avl_map_pull_rows")
    outs = (feat, wout, rgb)
    if device:
        for o in outs:
            if isinstance(o, DeviceArray):
                o._keep = (keep, plan)
        return outs
    host = tuple(o.numpy(stream) if isinstance(o, DeviceArray) else o for o in outs)       # a caller's feat_out stays where it is
    _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    return host


class PulledMap:
    """pull_map's result: the arrays of the resampled map -- grid_pos (n, 3) int32 in ascending linear cell order, grid_feat (n, D)
    float32, weight (n,) float32, grid_rgb (n, 3) uint8, occupied_ids (gs, gs, vh) int32 or None; host arrays, or DeviceArrays with
    device=True -- and counts, a dict of PULL_COUNTS.  members (n, 8) int32 and lam (n, 8) float64 are host arrays read back from
    the plan on first use (96 bytes per voxel: a call that never asks for them does not pay for the copy); plan is the PullPlan."""

    def __init__(self, arrays, plan: PullPlan, device):
        self.grid_feat, self.weight, self.grid_rgb = arrays
        self.grid_pos = plan._dev["cells"] if device else plan.cells
        self.occupied_ids = plan._dev["occupied"] if device else plan.occupied_ids
        self.plan = plan
        self.counts = {k: int(v) for k, v in zip(PULL_COUNTS, plan.counts)}
        self.n_out = plan.n_out

    members = property(lambda self: self.plan.members)
    lam = property(lambda self: self.plan.lam)


def pull_map(pos_b, feat_b, w_b, rgb_b, gs, cs, vh, transform=None, shift=(0, 0, 0), use_b=None, interp="linear", min_support=0.5,
             want_occupied=True, device=False, stream=None) -> PulledMap:
    """Map B resampled onto the gs x gs x vh grid of cell size cs under `transform` (B's base frame -> the target's, None = identity)
    and the whole-cell `shift`, backward: pull_plan, then pull_rows.  No pinholes under a rotation, unlike the forward
    ops.fuse_maps.  interp="linear" blends the rows of up to eight neighbouring voxels of B, also across the border between two
    objects; interp="nearest" copies one row and keeps every feature as it was.  The voxels come out in ascending linear cell order.
    Inputs are host arrays, DeviceArray / DeviceView or GPU tensors; each host input is uploaded once."""
    gs, vh = _check_grid("pull_map", gs, vh)
    cs = _check_cell_size(cs, "pull_map")
    P = inverse_transform(transform, "pull_map")
    _shift3(shift, "pull_map")
    check_interp(interp, "pull_map")
    check_min_support(min_support, "pull_map")
    pos_b, n_b = _cells_i32(pos_b, "pull_map: pos_b")
    fb = _feat_shape(feat_b, "pull_map: feat_b")
    if fb[0] != n_b:
        raise ValueError(f"pull_map: {n_b} cells, {fb[0]} feature rows")
    w_b = _typed(w_b, (n_b,), np.float32, "pull_map: w_b")
    rgb_b = _typed(rgb_b, (n_b, 3), np.uint8, "pull_map: rgb_b")
    use_b = _use_mask(use_b, n_b, "pull_map: use_b")
    _lib.load()
    _lib.require_gpu()
    staged = []
    pos_b, w_b = _resident(pos_b, np.int32, stream, staged), _resident(w_b, np.float32, stream, staged)
    plan = pull_plan(pos_b, w_b, gs, cs, vh, transform, shift, use_b, interp, min_support, want_occupied, stream, _inverse=P)
    arrays = pull_rows(plan, feat_b, w_b, rgb_b, device=device, stream=stream)
    out = PulledMap(arrays, plan, device)
    if not device:
        for d in staged:
            d.free()
    return out
