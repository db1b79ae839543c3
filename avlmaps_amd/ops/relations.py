"""The relations between the objects of a voxel map: for every pair of objects that come within `radius` cells of each other, their
nearest gap, where it is, who rests on whom and how much they touch (csrc/avl_relations.hip).  Upstream has no
counterpart; map/map.py:183-240 relates the 2-D islands of one category's top-down mask."""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray, as_device
from ._args import _image_shape, _is_dev, _workspace
from .audit import _cells_i32, CellIndex

RELATIONS_MAX_RADIUS = 15       # kRelMaxRadius of csrc/avl_relations.hip: |d|^2 <= 225 fits the 8 bits of the packed minimum
RELATIONS_MAX_PAIRS = 1 << 28
RELATION_TABLE_COLS = 8         # lo, hi, d2, i, j, lo_on_hi, hi_on_lo, contacts


class ObjectRelations:
    """object_relations' result: P pairs among n objects at `radius` cells.  table (P, 8) int64, rows
    [lo, hi, d2, i, j, lo_on_hi, hi_on_lo, contacts] sorted by (lo, hi) -- a host array, or a DeviceArray with device=True (pair()
    then copies it back once)."""

    def __init__(self, P, table, radius, n, stream=None):
        self.P, self.table, self.radius, self.n, self.stream = int(P), table, int(radius), int(n), stream
        self._host = table if isinstance(table, np.ndarray) else None
        self._keys = None

    def host_table(self) -> np.ndarray:
        if self._host is None:
            self._host = self.table.numpy(self.stream)
        return self._host

    def pair(self, a, b):
        """the row of the pair of objects a and b (in either order), None when they are not related.  A binary search."""
        t = self.host_table()
        if self._keys is None:
            self._keys = t[:, 0] * (self.n + 1) + t[:, 1]
        lo, hi = min(int(a), int(b)), max(int(a), int(b))
        if lo == hi or lo < 1 or hi > self.n:
            return None
        key = lo * (self.n + 1) + hi
        k = int(np.searchsorted(self._keys, key))
        return t[k] if k < self.P and self._keys[k] == key else None


def object_relations(index: CellIndex, grid_pos, labels, n, radius, max_pairs=None, device=False, stream=None) -> ObjectRelations:
    """The table of the pairs of objects that come within `radius` cells (1 .. RELATIONS_MAX_RADIUS) of each other
    (avl_object_relations).  index: the cell_index of grid_pos (N, 3) int32 cells (row, col, height); labels (N,) int32, a value
    outside 1 .. n takes part in nothing; each a host array, a DeviceArray / DeviceView or a GPU tensor.  Every labelled voxel i
    inside the grid scans the offsets d with |d|^2 <= radius^2 (d = 0 included, cells outside the grid skipped); where the cell's
    owner j (the largest row of the cell) carries another label the pair (lo, hi) of the two labels gets an event.  A row of the
    table is [lo, hi, d2, i, j, lo_on_hi, hi_on_lo, contacts]: the smallest |d|^2, its witness (the smallest scanning row i, then
    the smallest offset code; j is what i saw), the voxels of lo with a cell of hi directly beneath them and the converse, and the
    events of the 26-neighbourhood from either side.  Rows that share a cell make the scan asymmetric: a row that does not own its
    cell scans but is never seen.  Rows are sorted by (lo, hi).
    The pair table holds max_pairs pairs.  max_pairs=None starts at max(1024, 16 n) and, while the count that comes back (read
    once per call) exceeds it, doubles it up to min(n (n - 1) / 2, 2^28); an explicit max_pairs that is too small, or more pairs
    than that bound, raises AvlError with the count seen.  Shapes, dtypes and ranges are checked before any device work."""
    if not isinstance(index, CellIndex):
        raise TypeError(f"object_relations: expected a CellIndex, got {type(index).__name__}")
    grid_pos, N = _cells_i32(grid_pos, "object_relations")
    if N != index.N:
        raise ValueError(f"object_relations: {N} voxel cells, the index was built over {index.N}")
    if _image_shape(labels) != (N,):
        raise ValueError(f"object_relations: labels has shape {_image_shape(labels)}, the map {N} voxels")
    if not _is_dev(labels):
        labels = np.asarray(labels)
        if labels.dtype.kind not in "iu" or (labels.size and np.abs(labels.astype(np.int64)).max() > np.iinfo(np.int32).max):
            raise TypeError(f"object_relations: labels are int32 values, got {labels.dtype}")
    n, radius = int(n), int(radius)
    if not 0 <= n <= np.iinfo(np.int32).max:
        raise ValueError(f"object_relations: n = {n} objects")
    if not 1 <= radius <= RELATIONS_MAX_RADIUS:
        raise ValueError(f"object_relations: radius {radius} cells (1 .. {RELATIONS_MAX_RADIUS})")
    explicit = max_pairs is not None
    bound = min(max(n * (n - 1) // 2, 1), RELATIONS_MAX_PAIRS)
    max_pairs = int(max_pairs) if explicit else min(max(1024, 16 * n), RELATIONS_MAX_PAIRS)
    if not 1 <= max_pairs <= RELATIONS_MAX_PAIRS:
        raise ValueError(f"object_relations: max_pairs = {max_pairs} (1 .. 2^28)")
    lib = _lib.load()
    _lib.require_gpu()
    ip = index.ptr                                      # a closed index raises here
    pp, _, k1 = as_device(grid_pos, np.int32, stream)
    lp, _, k2 = as_device(labels, np.int32, stream)
    count = DeviceArray((1,), np.int64)
    while True:
        ws, nws = _workspace(lib.avl_object_relations_work_bytes, "avl_object_relations", max_pairs)
        table = DeviceArray((max_pairs, RELATION_TABLE_COLS), np.int64)
        _lib.check(lib.avl_object_relations(ip, index.nbytes, N, index.gs, index.vh, pp, lp, n, radius, max_pairs, table.ptr, count.ptr,
                                            ws.ptr, nws, stream), "avl_object_relations")
        P = int(count.numpy(stream)[0])                 # (synchronous: the workspace may go)
        ws.free()
        if P <= max_pairs:
            break
        table.free()
        if explicit or max_pairs >= bound:
            raise _lib.AvlError(f"object_relations: {P} pairs were counted, more than max_pairs = {max_pairs}")
        max_pairs = min(2 * max_pairs, bound)
    del k1, k2
    out = DeviceArray((P, RELATION_TABLE_COLS), np.int64)
    if P:
        _lib.check(lib.avl_memcpy_d2d(out.ptr, table.ptr, out.nbytes, stream), "avl_memcpy_d2d")
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    table.free()
    if device:
        return ObjectRelations(P, out, radius, n, stream)
    host = out.numpy(stream)
    out.free()
    return ObjectRelations(P, host, radius, n, stream)
