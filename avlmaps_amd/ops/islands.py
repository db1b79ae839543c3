"""Object islands of a 2-D mask, their contours and the nearest pair of two contours (csrc/avl_islands.hip)."""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device
from ._args import _image_shape, _image_u8, _workspace

ISLANDS_MAX_SIDE = 16384
ISLAND_TABLE_COLS = 8       # area, rmin, rmax, cmin, cmax, first_row, first_col, contour length (0 until trace_islands has run)
NEAREST_PAIR_MAX_COORD = 1 << 15


class Islands:
    """label_islands' result: n islands of an (H, W) mask.  labels: (H, W) int32, 0 = background, 1 .. n in raster order of the first
    pixel (host array, or the DeviceArray with device=True); table: (n, 8) int32 host array, one row per label (ISLAND_TABLE_COLS).
    The device copies of both live until close()."""

    def __init__(self, n, shape, labels_dev, table_dev, device, stream, keep):
        self.n, self.shape, self.stream = int(n), shape, stream
        self.labels_dev, self.table_dev, self._keep = labels_dev, table_dev, keep
        self.labels = labels_dev if device else labels_dev.numpy(stream)
        self._table = None

    @property
    def table(self) -> np.ndarray:
        if self._table is None:
            self._table = self.table_dev.numpy(self.stream) if self.n else np.zeros((0, ISLAND_TABLE_COLS), np.int32)
        return self._table

    def close(self):
        for a in (self.labels_dev, self.table_dev):
            if a is not None:
                a.free()
        self.labels_dev = self.table_dev = self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def label_islands(mask, device=False, stream=None) -> Islands:
    """8-connected islands of a 2-D mask (bool / uint8, host or DeviceArray; nonzero = foreground):
    scipy.ndimage.label(mask, structure=np.ones((3, 3))) with its numbering, plus the per-island table.  The island count is read
    back once to size the table."""
    lib = _lib.load()
    shape = _image_shape(mask)
    if len(shape) != 2:
        raise ValueError(f"expected a 2-D mask, got shape {shape}")
    H, W = shape
    ws, nws = _workspace(lib.avl_label_islands_work_bytes, "avl_label_islands", H, W)      # rejects a bad shape before any device work
    if isinstance(mask, np.ndarray) and mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        mask = mask != 0
    mp, _, keep = _image_u8(mask, stream)
    labels, n_dev = DeviceArray((H, W), np.int32), DeviceArray((1,), np.int32)
    _lib.check(lib.avl_label_islands(mp, W, H, W, labels.ptr, n_dev.ptr, ws.ptr, nws, stream), "avl_label_islands")
    n = int(n_dev.numpy(stream)[0])
    table = DeviceArray((n, ISLAND_TABLE_COLS), np.int32) if n else None
    if n:
        _lib.check(lib.avl_island_table(labels.ptr, H, W, n, table.ptr, stream), "avl_island_table")
    return Islands(n, (H, W), labels, table, device, stream, (keep, ws))


def trace_islands(islands: Islands):
    """The outer contour of every island, in label order: a list of (len, 2) int32 arrays of (row, col), each what
    utils.navigation_utils._trace_boundary returns for that island.  Two device passes: count, then write into one packed buffer."""
    lib = _lib.load()
    n, (H, W), stream = islands.n, islands.shape, islands.stream
    if n == 0:
        return []
    if islands.labels_dev is None:
        raise ValueError("trace_islands: the islands have been closed")
    lp, tp = islands.labels_dev.ptr, islands.table_dev.ptr
    _lib.check(lib.avl_trace_islands(lp, H, W, n, tp, None, None, 0, stream), "avl_trace_islands")
    islands._table = None
    lengths = islands.table[:, 7].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(offsets[-1])
    off_dev = DeviceArray.from_numpy(offsets[:-1], stream)
    points = DeviceArray((total, 2), np.int32)
    _lib.check(lib.avl_trace_islands(lp, H, W, n, tp, off_dev.ptr, points.ptr, total, stream), "avl_trace_islands")
    pts = points.numpy(stream)
    return [pts[offsets[k]:offsets[k + 1]] for k in range(n)]


def _points_i32(x, what, stream):
    """an (n, 2) list of integer points, host or int32 DeviceArray -> (ptr, n, keepalive)"""
    if isinstance(x, (DeviceArray, DeviceView)):
        ptr, shape, keep = as_device(x, np.int32, stream)
        if len(shape) != 2 or shape[1] != 2 or shape[0] < 1:
            raise ValueError(f"{what}: expected (n >= 1, 2) points, got shape {tuple(shape)}")
        return ptr, int(shape[0]), keep
    a = np.asarray(x)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError(f"{what}: expected (n >= 1, 2) points, got shape {a.shape}")
    if a.dtype.kind not in "iu":
        if a.dtype.kind != "f" or not np.array_equal(a, np.rint(a)):
            raise TypeError(f"{what}: contour points are integer cells, got {a.dtype}")
    if np.abs(a).max() > NEAREST_PAIR_MAX_COORD:
        raise ValueError(f"{what}: coordinates beyond +-{NEAREST_PAIR_MAX_COORD}")
    ptr, _, keep = as_device(np.ascontiguousarray(a, dtype=np.int32), np.int32, stream)
    return ptr, int(a.shape[0]), keep


def contour_nearest_pair(a, b, stream=None):
    """-> (i, j, d2): the points a[i], b[j] of two (n, 2) integer point lists with the smallest squared distance d2, the first in
    row-major (i, j) order among equals = np.unravel_index(np.argmin(np.linalg.norm(a[:, None] - b[None], axis=2)), (na, nb)),
    without the na x nb matrix (map.py:351-358)."""
    lib = _lib.load()
    _lib.require_gpu()
    ap, na, k1 = _points_i32(a, "contour_nearest_pair: a", stream)
    bp, nb, k2 = _points_i32(b, "contour_nearest_pair: b", stream)
    ws, nws = _workspace(lib.avl_nearest_pair_work_bytes, "avl_nearest_pair_work_bytes", na, nb)
    out = DeviceArray((3,), np.int64)
    _lib.check(lib.avl_nearest_pair_i32(ap, na, bp, nb, out.ptr, ws.ptr, nws, stream), "avl_nearest_pair_i32")
    i, j, d2 = (int(v) for v in out.numpy(stream))
    return i, j, d2
