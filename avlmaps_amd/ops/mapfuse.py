"""Fusing a revisit into the map: the cells of map B moved into map A's grid under a 4 x 4 transform, the join of both voxel lists by
cell and the weighted mean of the joined rows (csrc/avl_mapfuse.hip).  The arithmetic is the builder's running mean in
closed form, sum(w_i f_i) / sum(w_i); upstream has no counterpart for finished maps."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device, _is_torch
from ._args import _image_shape, _is_dev
from .audit import _cells_i32, _check_grid
from .mapdiff import _feat_shape, _shift3

FUSE_MAX_DIM = 8192
FUSE_COUNTS = ("dropped_a", "unselected_b", "outside_b", "merged_b", "new_cells", "shared_b")
FUSE_ERR_OUTSIDE, FUSE_ERR_SHARED = 1, 2


def check_transform(transform, who):
    """None, or the (4, 4) float64 rigid or affine transform as a contiguous array: finite, bottom row 0 0 0 1"""
    if transform is None:
        return None
    T = np.ascontiguousarray(np.asarray(transform, dtype=np.float64))
    if T.shape != (4, 4):
        raise ValueError(f"{who}: the transform is (4, 4), got shape {T.shape}")
    if not np.isfinite(T).all():
        raise ValueError(f"{who}: the transform is not finite")
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"{who}: the bottom row of the transform is {T[3].tolist()}, expected 0 0 0 1")
    return T


def check_gain(gain, who):
    g = float(gain)
    if not (g > 0.0 and np.isfinite(g)):
        raise ValueError(f"{who}: gain {gain!r} (a finite number greater than 0)")
    return g


def _check_cell_size(cs, who):
    c = float(cs)
    if not (c > 0.0 and np.isfinite(c)):
        raise ValueError(f"{who}: cs = {cs!r} (a finite cell size greater than 0)")
    return c


def _typed(x, n_shape, dtype, what, kinds=None):
    """`x` of exactly this shape and dtype (host arrays of a kind in `kinds` are converted), ready for as_device"""
    if _image_shape(x) != tuple(n_shape):
        raise ValueError(f"{what} has shape {_image_shape(x)}, expected {tuple(n_shape)}")
    dtype = np.dtype(dtype)
    if _is_torch(x):
        ok = str(x.dtype) == "torch." + dtype.name or (dtype == np.uint8 and str(x.dtype) == "torch.bool")
    elif _is_dev(x):
        ok = np.dtype(x.dtype) == dtype
    else:
        x = np.asarray(x)
        ok = x.dtype == dtype or (kinds is not None and x.dtype.kind in kinds)
    if not ok:
        raise TypeError(f"{what}: expected {dtype.name}, got {getattr(x, 'dtype', type(x).__name__)}")
    if _is_torch(x) and str(x.dtype) == "torch.bool":
        import torch
        x = x.to(torch.uint8)
    return x


def _use_mask(x, n, what):
    return None if x is None else _typed(x, (n,), np.uint8, what, kinds="b")


def _resident(x, dtype, stream, staged):
    """the argument on the device: itself when it is there already, else one upload that `staged` remembers"""
    if x is None or _is_dev(x):
        return x
    d = DeviceArray.from_numpy(np.ascontiguousarray(x, dtype=dtype), stream)
    staged.append(d)
    return d


def move_cells(cells, gs, cs, vh, transform=None, shift=(0, 0, 0), device=False, stream=None):
    """(cells (n, 3) int32, inside (n,) uint8): every cell (row, col, h) of a gs x gs x vh grid of cell size cs moved by the (4, 4)
    float64 `transform` of base coordinates (None = identity) and then by the whole-cell `shift` (avl_map_move_cells).  A cell stands
    for the centre of the base-coordinate interval that upstream's base_pos2grid_id_3d maps to it; the moved point goes back through
    that expression.  inside is 0, and the cell (-1, -1, -1), where the result leaves the grid.  With transform=None the call is
    integer only."""
    gs, vh = _check_grid("move_cells", gs, vh)
    cs = _check_cell_size(cs, "move_cells")
    T = check_transform(transform, "move_cells")
    shift = _shift3(shift, "move_cells")
    cells, n = _cells_i32(cells, "move_cells")
    lib = _lib.load()
    _lib.require_gpu()
    out, inside = DeviceArray((n, 3), np.int32), DeviceArray((n,), np.uint8)
    keep = None
    if n:
        cp, _, keep = as_device(cells, np.int32, stream)
        _lib.check(lib.avl_map_move_cells(cp, n, T.ctypes.data if T is not None else None, shift.ctypes.data, gs, cs, vh, out.ptr, inside.ptr,
                                          stream), "avl_map_move_cells")
    if device:
        out._keep = inside._keep = keep
        return out, inside
    return out.numpy(stream), inside.numpy(stream)


class FusePlan:
    """fuse_plan's result.  n_out output voxels: first the selected rows of A in row order, then the cells that only rows of B reach,
    ordered by their smallest row.  a_row (n_out,): the A row of a voxel or -1; b_start (n_out + 1,), b_rows: the CSR of the selected B
    rows of every voxel, ascending; out_of_a (n_a,), out_of_b (n_b,): the voxel of every input row or -1; counts (6,) int32 in the
    order of FUSE_COUNTS.  The arrays are read back from the device on first use; the device copies feed fuse_rows."""

    def __init__(self, n_a, n_b, gs, vh, head, counts, dev, cells_a, cells_b, stream):
        self.n_a, self.n_b, self.gs, self.vh = n_a, n_b, gs, vh
        self.n_out, self.n_sel_a, self.n_sel_b = int(head[0]), int(head[1]), int(head[2])
        self.counts = counts
        self._dev, self._cells_a, self._cells_b, self._stream, self._host = dev, cells_a, cells_b, stream, {}

    def _get(self, name, n):
        if name not in self._host:
            self._host[name] = self._dev[name].numpy(self._stream)[:n].copy()
        return self._host[name]

    a_row = property(lambda self: self._get("a_row", self.n_out))
    b_start = property(lambda self: self._get("b_start", self.n_out + 1))
    b_rows = property(lambda self: self._get("b_rows", self.n_sel_b))
    out_of_a = property(lambda self: self._get("out_of_a", self.n_a))
    out_of_b = property(lambda self: self._get("out_of_b", self.n_b))

    @property
    def b_count(self):
        return np.diff(self.b_start).astype(np.int32)


def fuse_plan(cells_a, w_a, cells_b, w_b, gs, vh, inside_b=None, use_a=None, use_b=None, stream=None) -> FusePlan:
    """Join map A's cells (n_a, 3) and map B's MOVED cells (n_b, 3) (move_cells) by cell (avl_map_fuse_plan).  A row is selected when
    its use mask (bool / uint8, None = all) is set, it lies inside the grid (inside_b: move_cells' second result) and its weight
    (float32) is finite and > 0.  ValueError when a selected row of A lies outside the grid or two of them share a cell."""
    gs, vh = _check_grid("fuse_plan", gs, vh)
    cells_a, n_a = _cells_i32(cells_a, "fuse_plan: cells_a")
    cells_b, n_b = _cells_i32(cells_b, "fuse_plan: cells_b")
    w_a = _typed(w_a, (n_a,), np.float32, "fuse_plan: w_a")
    w_b = _typed(w_b, (n_b,), np.float32, "fuse_plan: w_b")
    use_a, use_b = _use_mask(use_a, n_a, "fuse_plan: use_a"), _use_mask(use_b, n_b, "fuse_plan: use_b")
    inside_b = _use_mask(inside_b, n_b, "fuse_plan: inside_b")
    if n_a + n_b >= 2 ** 31 - 1:
        raise ValueError(f"fuse_plan: {n_a} + {n_b} rows (together below 2^31 - 1)")
    lib = _lib.load()
    m = max(n_a, n_b)
    ib, sb = C.c_size_t(0), C.c_size_t(0)
    _lib.check(lib.avl_cell_index_work_bytes(m, gs, vh, C.byref(ib)), "avl_cell_index_work_bytes")
    _lib.check(lib.avl_argsort_bits_work_bytes(n_b, 4, max(1, (n_a + n_b).bit_length()), C.byref(sb)), "avl_argsort_bits_work_bytes")
    _lib.require_gpu()
    staged = []
    cells_a, cells_b = _resident(cells_a, np.int32, stream, staged), _resident(cells_b, np.int32, stream, staged)
    index, sort_work = DeviceArray((ib.value,), np.uint8), DeviceArray((max(sb.value, 1),), np.uint8)
    scratch = DeviceArray((9 * m + 1024,), np.int32)
    head, counts = DeviceArray((4,), np.int32), DeviceArray((6,), np.int32)
    dev = dict(a_row=DeviceArray((n_a + n_b,), np.int32), b_start=DeviceArray((n_a + n_b + 1,), np.int32), b_rows=DeviceArray((n_b,), np.int32),
               out_of_a=DeviceArray((n_a,), np.int32), out_of_b=DeviceArray((n_b,), np.int32))
    keep = [as_device(x, dt, stream) for x, dt in ((cells_a, np.int32), (w_a, np.float32), (cells_b, np.int32), (w_b, np.float32))]
    masks = [None if x is None else as_device(x, np.uint8, stream) for x in (use_a, inside_b, use_b)]
    mp = [None if k is None else k[0] for k in masks]
    _lib.check(lib.avl_map_fuse_plan(keep[0][0], mp[0], keep[1][0], n_a, keep[2][0], mp[1], mp[2], keep[3][0], n_b, gs, vh, index.ptr, ib.value,
                                     sort_work.ptr, sb.value, scratch.ptr, 9 * m + 1024, head.ptr, dev["a_row"].ptr, dev["b_start"].ptr,
                                     dev["b_rows"].ptr, dev["out_of_a"].ptr, dev["out_of_b"].ptr, counts.ptr, stream), "avl_map_fuse_plan")
    h, c = head.numpy(stream), counts.numpy(stream)                 # the one read-back; the stream is drained: the scratch may go
    _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    del keep, masks
    for d in (index, sort_work, scratch, head, counts):
        d.free()
    if h[3] & FUSE_ERR_OUTSIDE:
        raise ValueError("fuse_plan: a selected row of map A lies outside the grid")
    if h[3] & FUSE_ERR_SHARED:
        raise ValueError("fuse_plan: two selected rows of map A share a cell (one row per cell)")
    return FusePlan(n_a, n_b, gs, vh, h, c, dev, cells_a, cells_b, stream)


def fuse_rows(plan: FusePlan, feat_a, w_a, rgb_a, feat_b, w_b, rgb_b, gain_a=1.0, gain_b=1.0, want_occupied=True, feat_out=None, device=False,
              stream=None):
    """(grid_pos (n_out, 3) int32, grid_feat (n_out, D) float32, weight (n_out,) float32, grid_rgb (n_out, 3) uint8, occupied_ids (gs,
    gs, vh) int32 or None) of a FusePlan (avl_map_fuse_rows).  The members of a voxel are its A row, then its B rows ascending; in
    float64 w_i = weight_i * gain, W = sum of w_i, and per element sum(w_i * f_i) / W in member order with every product and sum
    rounded once; rgb likewise, truncated.  A voxel with one member and gain 1 comes back bit for bit.  The bytes do not depend on
    the alignment of the matrices.  feat_* (n, D) float32, w_* (n,) float32, rgb_* (n, 3) uint8; host arrays, DeviceArray /
    DeviceView or GPU tensors.  feat_out: a caller's (n_out, D) float32 device array to write the rows into."""
    if not isinstance(plan, FusePlan):
        raise TypeError(f"fuse_rows: expected a FusePlan, got {type(plan).__name__}")
    g_a, g_b = check_gain(gain_a, "fuse_rows: gain_a"), check_gain(gain_b, "fuse_rows: gain_b")
    n_a, n_b, n_out = plan.n_a, plan.n_b, plan.n_out
    fa, fb = _feat_shape(feat_a, "fuse_rows: feat_a"), _feat_shape(feat_b, "fuse_rows: feat_b")
    if fa[0] != n_a or fb[0] != n_b:
        raise ValueError(f"fuse_rows: the plan is of {n_a} and {n_b} rows, the features have {fa[0]} and {fb[0]}")
    if fa[1] != fb[1]:
        raise ValueError(f"fuse_rows: feat_a has D = {fa[1]}, feat_b D = {fb[1]}")
    D = fa[1]
    w_a, w_b = _typed(w_a, (n_a,), np.float32, "fuse_rows: w_a"), _typed(w_b, (n_b,), np.float32, "fuse_rows: w_b")
    rgb_a, rgb_b = _typed(rgb_a, (n_a, 3), np.uint8, "fuse_rows: rgb_a"), _typed(rgb_b, (n_b, 3), np.uint8, "fuse_rows: rgb_b")
    if feat_out is not None:
        if not _is_dev(feat_out) or _image_shape(feat_out) != (n_out, D):
            raise ValueError(f"fuse_rows: feat_out is a ({n_out}, {D}) float32 device array")
    lib = _lib.load()
    _lib.require_gpu()
    keep = [as_device(x, dt, stream) for x, dt in ((feat_a, np.float32), (w_a, np.float32), (rgb_a, np.uint8), (plan._cells_a, np.int32),
                                                   (feat_b, np.float32), (w_b, np.float32), (rgb_b, np.uint8), (plan._cells_b, np.int32))]
    p = [k[0] for k in keep]
    pos, wout, rgb = DeviceArray((n_out, 3), np.int32), DeviceArray((n_out,), np.float32), DeviceArray((n_out, 3), np.uint8)
    feat = feat_out if feat_out is not None else DeviceArray((n_out, D), np.float32)
    occ = DeviceArray((plan.gs, plan.gs, plan.vh), np.int32) if want_occupied else None
    d = plan._dev
    _lib.check(lib.avl_map_fuse_rows(n_out, d["a_row"].ptr, d["b_start"].ptr, d["b_rows"].ptr, p[0], p[1], p[2], p[3], n_a, p[4], p[5], p[6], p[7],
                                     n_b, D, g_a, g_b, plan.gs, plan.vh, as_device(feat, np.float32, stream)[0], wout.ptr, rgb.ptr, pos.ptr,
                                     occ.ptr if occ is not None else None, stream), "avl_map_fuse_rows")
    outs = (pos, feat, wout, rgb, occ)
    if device:
        for o in outs:
            if isinstance(o, DeviceArray):
                o._keep = (keep, plan)
        return outs
    host = tuple(o.numpy(stream) if isinstance(o, DeviceArray) else o for o in outs)       # a caller's feat_out stays where it is
    _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    return host


class FusedMap:
    """fuse_maps' result: the arrays of the fused map -- grid_pos (n, 3) int32, grid_feat (n, D) float32, weight (n,) float32,
    grid_rgb (n, 3) uint8, occupied_ids (gs, gs, vh) int32 or None; host arrays, or DeviceArrays with device=True -- and, always on
    the host, the plan's bookkeeping: a_row (n,), b_count (n,), out_of_a (n_a,), out_of_b (n_b,) int32 and counts, a dict of
    FUSE_COUNTS."""

    def __init__(self, arrays, plan: FusePlan):
        self.grid_pos, self.grid_feat, self.weight, self.grid_rgb, self.occupied_ids = arrays
        self.a_row, self.b_count, self.out_of_a, self.out_of_b = plan.a_row, plan.b_count, plan.out_of_a, plan.out_of_b
        self.counts = {k: int(v) for k, v in zip(FUSE_COUNTS, plan.counts)}
        self.n_out = plan.n_out


def fuse_maps(pos_a, feat_a, w_a, rgb_a, pos_b, feat_b, w_b, rgb_b, gs, cs, vh, transform=None, shift=(0, 0, 0), use_a=None, use_b=None,
              gain_a=1.0, gain_b=1.0, want_occupied=True, device=False, stream=None) -> FusedMap:
    """One voxel map out of two on A's gs x gs x vh grid of cell size cs: B's cells are moved by `transform` (B's base frame -> A's,
    None = identity) and the whole-cell `shift` (move_cells), joined with A's by cell (fuse_plan) and every output voxel is the
    weighted mean of its members (fuse_rows).  use_a / use_b (bool, None = all) leave rows out; gain_a / gain_b scale the weights of
    a side.  Inputs are host arrays, DeviceArray / DeviceView or GPU tensors; each host input is uploaded once.  Forward, nearest
    cell: under a rotation some cells receive two or three rows of B and neighbouring cells none."""
    gs, vh = _check_grid("fuse_maps", gs, vh)
    cs = _check_cell_size(cs, "fuse_maps")
    check_transform(transform, "fuse_maps")
    _shift3(shift, "fuse_maps")
    check_gain(gain_a, "fuse_maps: gain_a"), check_gain(gain_b, "fuse_maps: gain_b")
    pos_a, n_a = _cells_i32(pos_a, "fuse_maps: pos_a")
    pos_b, n_b = _cells_i32(pos_b, "fuse_maps: pos_b")
    fa, fb = _feat_shape(feat_a, "fuse_maps: feat_a"), _feat_shape(feat_b, "fuse_maps: feat_b")
    if fa[0] != n_a or fb[0] != n_b:
        raise ValueError(f"fuse_maps: {n_a} and {n_b} cells, {fa[0]} and {fb[0]} feature rows")
    if fa[1] != fb[1]:
        raise ValueError(f"fuse_maps: feat_a has D = {fa[1]}, feat_b D = {fb[1]}")
    w_a, w_b = _typed(w_a, (n_a,), np.float32, "fuse_maps: w_a"), _typed(w_b, (n_b,), np.float32, "fuse_maps: w_b")
    rgb_a, rgb_b = _typed(rgb_a, (n_a, 3), np.uint8, "fuse_maps: rgb_a"), _typed(rgb_b, (n_b, 3), np.uint8, "fuse_maps: rgb_b")
    use_a, use_b = _use_mask(use_a, n_a, "fuse_maps: use_a"), _use_mask(use_b, n_b, "fuse_maps: use_b")
    _lib.load()
    _lib.require_gpu()
    staged = []
    pos_a, pos_b = _resident(pos_a, np.int32, stream, staged), _resident(pos_b, np.int32, stream, staged)
    w_a, w_b = _resident(w_a, np.float32, stream, staged), _resident(w_b, np.float32, stream, staged)
    moved, inside = move_cells(pos_b, gs, cs, vh, transform, shift, device=True, stream=stream)
    plan = fuse_plan(pos_a, w_a, moved, w_b, gs, vh, inside_b=inside, use_a=use_a, use_b=use_b, stream=stream)
    arrays = fuse_rows(plan, feat_a, w_a, rgb_a, feat_b, w_b, rgb_b, gain_a, gain_b, want_occupied, device=device, stream=stream)
    out = FusedMap(arrays, plan)
    if not device:
        for d in staged:
            d.free()
    return out
