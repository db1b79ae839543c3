"""Comparing two voxel maps of one place: the join of two voxel lists by cell, the dot products of the joined feature rows and the
status of every voxel (csrc/avl_mapdiff.hip).  Upstream has no counterpart: its maps are static."""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device, _is_torch
from ._args import _image_shape, _is_dev, _result
from .audit import _cells_i32, _check_grid, cell_index, CellIndex

DIFF_SAME, DIFF_CHANGED, DIFF_NO_MATCH, DIFF_UNSEEN = 0, 1, 2, 3
DIFF_MAX_RADIUS = 2
DIFF_MAX_DIM = 8192
DIFF_STREAM_ROWS = 1 << 16              # rows of a host feat_a that row_dots uploads at a time


def _shift3(shift, who):
    s = np.asarray(shift)
    if s.shape != (3,) or s.dtype.kind not in "iu" or np.abs(s.astype(np.int64)).max(initial=0) > 2 ** 31 - 1:
        raise ValueError(f"{who}: shift is three whole cells (row, col, h), got {shift!r}")
    return np.ascontiguousarray(s, dtype=np.int32)


def _check_radius(radius, who):
    if isinstance(radius, bool) or int(radius) != radius or not 0 <= int(radius) <= DIFF_MAX_RADIUS:
        raise ValueError(f"{who}: radius {radius!r} (a whole number of cells, 0 .. {DIFF_MAX_RADIUS})")
    return int(radius)


def _check_threshold(threshold, who):
    t = float(threshold)
    if not 0.0 < t <= 1.0:
        raise ValueError(f"{who}: threshold {threshold!r} (a cosine, 0 < threshold <= 1)")
    return t


def _feat_shape(x, what):
    """(rows, D) of a float32 feature matrix, host or device; TypeError for any other dtype"""
    shape = _image_shape(x)
    if len(shape) != 2:
        raise ValueError(f"{what}: expected (N, D) float32 rows, got shape {shape}")
    if _is_torch(x):
        ok = str(x.dtype) == "torch.float32"
    else:
        ok = np.dtype(getattr(x, "dtype", np.asarray(x).dtype)) == np.dtype(np.float32)
    if not ok:
        raise TypeError(f"{what}: feature rows are float32, got {getattr(x, 'dtype', type(x).__name__)}")
    if not 1 <= shape[1] <= DIFF_MAX_DIM:
        raise ValueError(f"{what}: D = {shape[1]} (1 .. {DIFF_MAX_DIM})")
    return shape


def _per_voxel_i32(x, n, what):
    """(n,) int32, host or device, ready for as_device"""
    if _image_shape(x) != (n,):
        raise ValueError(f"{what} has shape {_image_shape(x)}, expected ({n},)")
    if not _is_dev(x):
        x = np.asarray(x)
        if x.dtype.kind not in "iu":
            raise TypeError(f"{what}: expected integers, got {x.dtype}")
        x = np.minimum(x, 2 ** 31 - 1).astype(np.int32) if x.dtype != np.int32 else x      # a uint32 ray count saturates
    return x


def match_cells(index: CellIndex, cells, radius=1, shift=(0, 0, 0), device=False, stream=None):
    """(match, d2), each (n,) int32: for every cell (row, col, h) of `cells` (n, 3) int32, moved by the whole-cell `shift`, the row
    of the OTHER map -- the one `index` (ops.cell_index) was built from -- that owns the nearest occupied cell within Chebyshev
    `radius` 0 .. 2, and the squared cell distance to it; -1 in both where there is none or the moved cell lies outside the grid
    (avl_map_match_cells).  The winner minimises (squared distance, linear cell), in that order."""
    if not isinstance(index, CellIndex):
        raise TypeError(f"match_cells: expected a CellIndex, got {type(index).__name__}")
    radius = _check_radius(radius, "match_cells")
    shift = _shift3(shift, "match_cells")
    cells, n = _cells_i32(cells, "match_cells")
    lib = _lib.load()
    _lib.require_gpu()
    match, d2 = DeviceArray((n,), np.int32), DeviceArray((n,), np.int32)
    keep = None
    if n:
        cp, _, keep = as_device(cells, np.int32, stream)
        _lib.check(lib.avl_map_match_cells(index.ptr, index.nbytes, index.N, index.gs, index.vh, cp, n, shift.ctypes.data, radius, match.ptr,
                                           d2.ptr, stream), "avl_map_match_cells")
    if device:
        match._keep = d2._keep = (keep, index)
        return match, d2
    return match.numpy(stream), d2.numpy(stream)


def row_dots(feat_a, feat_b, match, device=False, stream=None):
    """(n_a, 3) float64: row i = (a.b, a.a, b.b) of a = feat_a[i] and b = feat_b[match[i]], float32 rows of 1 <= D <= 8192 elements;
    zeros where match[i] < 0 (avl_row_dots_f32).  The order of the additions is pinned (a lane of the wave owns the elements d with
    (d // 4) % 64 == lane, ascending d, then the xor butterfly 32 .. 1), nothing is fused: the same bytes on every run, for every
    alignment.  feat_b must be resident in one piece (its rows are gathered); a host feat_a is uploaded and read DIFF_STREAM_ROWS
    rows at a time."""
    n_a, D = _feat_shape(feat_a, "row_dots: feat_a")
    n_b, Db = _feat_shape(feat_b, "row_dots: feat_b")
    if D != Db:
        raise ValueError(f"row_dots: feat_a has D = {D}, feat_b D = {Db}")
    match = _per_voxel_i32(match, n_a, "row_dots: match")
    if not _is_dev(match) and match.size and int(match.max()) >= n_b:
        raise ValueError(f"row_dots: match names row {int(match.max())} of {n_b}")
    lib = _lib.load()
    _lib.require_gpu()
    sums = DeviceArray((n_a, 3), np.float64)
    keep = ()
    if n_a:
        bp, _, kb = as_device(feat_b, np.float32, stream)
        mp, _, km = as_device(match, np.int32, stream)
        if _is_dev(feat_a):
            ap, _, ka = as_device(feat_a, np.float32, stream)
            _lib.check(lib.avl_row_dots_f32(ap, n_a, bp, n_b, D, mp, sums.ptr, stream), "avl_row_dots_f32")
            keep = (ka, kb, km)
        else:
            feat_a = np.asarray(feat_a)
            for r0 in range(0, n_a, DIFF_STREAM_ROWS):
                r1 = min(n_a, r0 + DIFF_STREAM_ROWS)
                piece = DeviceArray.from_numpy(feat_a[r0:r1], stream)
                _lib.check(lib.avl_row_dots_f32(piece.ptr, r1 - r0, bp, n_b, D, mp + 4 * r0, sums.ptr + 24 * r0, stream), "avl_row_dots_f32")
                _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")          # the piece goes back to the pool
                piece.free()
            keep = (kb, km)
    return _result(sums, device, stream, keep=keep)


def diff_status(match, sums, threshold=0.8, through=None, min_rays=3, device=False, stream=None):
    """(status (n,) uint8, counts (4,) int32) from match (n,) int32 and sums (n, 3) float64 = (ab, aa, bb) (avl_map_diff_status):
    DIFF_NO_MATCH where match < 0 -- DIFF_UNSEEN instead where `through` (n,) integers is given and through < min_rays: the other
    session never looked there --; DIFF_SAME where aa > 0 and bb > 0 and ab > 0 and ab * ab >= threshold^2 * (aa * bb) in float64;
    DIFF_CHANGED otherwise.  counts[s] is the number of voxels of status s."""
    t = _check_threshold(threshold, "diff_status")
    shape = _image_shape(match)
    if len(shape) != 1:
        raise ValueError(f"diff_status: match has shape {shape}, expected (n,)")
    n = shape[0]
    match = _per_voxel_i32(match, n, "diff_status: match")
    if _image_shape(sums) != (n, 3):
        raise ValueError(f"diff_status: sums has shape {_image_shape(sums)}, expected ({n}, 3)")
    if through is not None:
        through = _per_voxel_i32(through, n, "diff_status: through")
    min_rays = int(min_rays)
    lib = _lib.load()
    _lib.require_gpu()
    status, counts = DeviceArray((n,), np.uint8), DeviceArray((4,), np.int32)
    mp, _, km = as_device(match, np.int32, stream)
    sp, _, ks = as_device(sums, np.float64, stream)
    tp, kt = None, None
    if through is not None:
        tp, _, kt = as_device(through, np.int32, stream)
    _lib.check(lib.avl_map_diff_status(mp, sp, n, t * t, tp, min_rays, status.ptr, counts.ptr, stream), "avl_map_diff_status")
    if device:
        status._keep = counts._keep = (km, ks, kt)
        return status, counts
    return status.numpy(stream), counts.numpy(stream)


class DiffSide:
    """One direction of a MapDiff: this map's voxels against the other map's index.  match, d2 (n,) int32; sums (n, 3) float64;
    status (n,) uint8; counts (4,) int32 -- host arrays, or DeviceArrays with device=True.  cosine: (n,) float64 on the host,
    ab / sqrt(aa * bb), NaN where unmatched or where a row is zero."""

    def __init__(self, match, d2, sums, status, counts, stream=None):
        self.match, self.d2, self.sums, self.status, self.counts, self._stream = match, d2, sums, status, counts, stream

    @staticmethod
    def _host(x, stream):
        return x.numpy(stream) if isinstance(x, DeviceArray) else x

    @property
    def cosine(self) -> np.ndarray:
        return cosine_of(self._host(self.match, self._stream), self._host(self.sums, self._stream))


def cosine_of(match, sums) -> np.ndarray:
    """(n,) float64 on the host: ab / sqrt(aa * bb), NaN where match < 0 or a row is zero"""
    match, sums = np.asarray(match), np.asarray(sums, np.float64).reshape(-1, 3)
    out = np.full(match.shape, np.nan)
    ok = (match >= 0) & (sums[:, 1] > 0) & (sums[:, 2] > 0)
    out[ok] = sums[ok, 0] / np.sqrt(sums[ok, 1] * sums[ok, 2])
    return out


class MapDiff:
    """map_diff's result: `a` is map A's voxels against map B (NO_MATCH = vanished), `b` map B's voxels against map A (NO_MATCH =
    appeared); each a DiffSide with its own nearest match."""

    def __init__(self, a: DiffSide, b: DiffSide, radius, threshold, shift, min_rays):
        self.a, self.b = a, b
        self.radius, self.threshold, self.shift, self.min_rays = int(radius), float(threshold), tuple(int(s) for s in shift), int(min_rays)


def map_diff(pos_a, feat_a, pos_b, feat_b, gs, vh, radius=1, threshold=0.8, shift=(0, 0, 0), through_a=None, through_b=None, min_rays=3,
             index_a=None, index_b=None, device=False, stream=None) -> MapDiff:
    """Compare two voxel maps of one place on one gs x gs x vh grid.  pos_* (N, 3) int32 cells, feat_* (N, D) float32 rows; host
    arrays, DeviceArray / DeviceView or GPU tensors.  Map A's cell c corresponds to map B's cell c + shift (whole cells).  Both
    directions run: A against B's cell index, and B against A's with the negated shift; each has its own nearest match within
    `radius`.  A matched pair is SAME when the cosine of its rows is at least `threshold`, CHANGED otherwise; an unmatched voxel is
    NO_MATCH, or UNSEEN where through_* (the other session's sight rays through this map's voxels, Map.audit_visibility) is given
    and below min_rays.  index_a / index_b: the maps' CellIndex when the caller has them (same grid), built and closed here
    otherwise.  Both feature matrices are made resident: each is the gathered side of one direction."""
    gs, vh = _check_grid("map_diff", gs, vh)
    radius = _check_radius(radius, "map_diff")
    _check_threshold(threshold, "map_diff")
    shift = _shift3(shift, "map_diff")
    pos_a, n_a = _cells_i32(pos_a, "map_diff: pos_a")
    pos_b, n_b = _cells_i32(pos_b, "map_diff: pos_b")
    fa, fb = _feat_shape(feat_a, "map_diff: feat_a"), _feat_shape(feat_b, "map_diff: feat_b")
    if fa[0] != n_a or fb[0] != n_b:
        raise ValueError(f"map_diff: {n_a} and {n_b} cells, {fa[0]} and {fb[0]} feature rows")
    if fa[1] != fb[1]:
        raise ValueError(f"map_diff: feat_a has D = {fa[1]}, feat_b D = {fb[1]}")
    for name, ix, n in (("index_a", index_a, n_a), ("index_b", index_b, n_b)):
        if ix is not None:
            if not isinstance(ix, CellIndex):
                raise TypeError(f"map_diff: {name} is a {type(ix).__name__}, expected a CellIndex")
            if (ix.gs, ix.vh, ix.N) != (gs, vh, n):
                raise ValueError(f"map_diff: {name} is of {ix.N} voxels on {ix.gs} x {ix.gs} x {ix.vh}, the map has {n} on {gs} x {gs} x {vh}")
    if through_a is not None:
        through_a = _per_voxel_i32(through_a, n_a, "map_diff: through_a")
    if through_b is not None:
        through_b = _per_voxel_i32(through_b, n_b, "map_diff: through_b")
    _lib.load()
    _lib.require_gpu()
    staged, dev = [], []                                # every input once on the device: each is read by both directions
    for x, dt in ((pos_a, np.int32), (feat_a, np.float32), (pos_b, np.int32), (feat_b, np.float32)):
        if _is_dev(x):
            dev.append(x)
        else:
            d = DeviceArray.from_numpy(np.ascontiguousarray(x, dtype=dt), stream)
            staged.append(d)
            dev.append(d)
    dpa, dfa, dpb, dfb = dev
    own_a = own_b = None
    try:
        if index_a is None:
            index_a = own_a = cell_index(dpa, gs, vh, stream)
        if index_b is None:
            index_b = own_b = cell_index(dpb, gs, vh, stream)
        sides = []
        for pos, feat, other_feat, index, sh, through in ((dpa, dfa, dfb, index_b, shift, through_a),
                                                          (dpb, dfb, dfa, index_a, -shift, through_b)):
            match, d2 = match_cells(index, pos, radius, sh, device=True, stream=stream)
            sums = row_dots(feat, other_feat, match, device=True, stream=stream)
            status, counts = diff_status(match, sums, threshold, through, min_rays, device=True, stream=stream)
            sides.append((match, d2, sums, status, counts))
        _lib.check(_lib.load().avl_stream_sync(stream), "avl_stream_sync")      # indices and staged inputs may go
    finally:
        for ix in (own_a, own_b):
            if ix is not None:
                ix.close()
    out = []
    for arrays in sides:
        for a in arrays:
            a._keep = None
        out.append(DiffSide(*(arrays if device else [a.numpy(stream) for a in arrays]), stream=stream))
    for d in staged:
        d.free()
    return MapDiff(out[0], out[1], radius, threshold, shift, min_rays)
