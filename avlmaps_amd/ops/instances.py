"""Object instances in 3-D: the connected components of the masked voxels of a voxel list and their table
(csrc/avl_instances.hip).  Upstream has no counterpart; map/map.py:146-151 and map/vlmap_3d.py:75-100 stop at the category mask."""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _dev_u8, _image_shape, _workspace

INSTANCE_TABLE_COLS = 12        # count, rmin, rmax, cmin, cmax, hmin, hmax, sum_row, sum_col, sum_height, first, best
INSTANCES_MAX_BOX_SIDE = 1 << 20
_CONNECTIVITIES = (6, 18, 26)


class Instance3D(NamedTuple):
    """One object of a category (VLMap.get_instances_3d), in full-map cells.  label: its number among ALL instances of the category,
    1 .. n in (row, col, height) order of the first cell; bbox: (rmin, rmax, cmin, cmax, hmin, hmax), inclusive; center: the mean
    (row, col, height) of its voxels, float64; best_voxel / best_score: the voxel with the category's largest score and that score;
    cell: the centre's (row, col) rounded to the nearest cell (halves to even), what Navigator.plan_to takes as a goal."""
    label: int
    count: int
    bbox: Tuple[int, int, int, int, int, int]
    center: Tuple[float, float, float]
    best_voxel: int
    best_score: float
    cell: Tuple[int, int]

    @classmethod
    def from_row(cls, label, row, best_score=0.0):
        """row: one row of a VoxelInstances table (INSTANCE_TABLE_COLS integers)"""
        row = [int(v) for v in row]
        count = row[0]
        center = tuple(np.asarray(row[7:10], np.float64) / np.float64(count))
        cell = (int(np.rint(center[0])), int(np.rint(center[1])))
        return cls(int(label), count, tuple(row[1:7]), tuple(float(c) for c in center), row[11], float(best_score), cell)


class VoxelInstances:
    """label_voxels' result: n instances among N voxels.  labels: (N,) int32, 0 where the mask is 0, else 1 .. n (host array, or the
    DeviceArray with device=True); table: (n, 12) int64 host array, one row per label (INSTANCE_TABLE_COLS); best_score: (n,) float32;
    centers: (n, 3) float64 = sums / count.  The device copies live until close()."""

    def __init__(self, n, N, labels_dev, table_dev, best_dev, device, stream, keep):
        self.n, self.N, self.stream = int(n), int(N), stream
        self.labels_dev, self.table_dev, self.best_score_dev, self._keep = labels_dev, table_dev, best_dev, keep
        self.labels = labels_dev if device else labels_dev.numpy(stream)
        self._table = self._best_score = None

    @property
    def table(self) -> np.ndarray:
        if self._table is None:
            self._table = self.table_dev.numpy(self.stream) if self.n else np.zeros((0, INSTANCE_TABLE_COLS), np.int64)
        return self._table

    @property
    def best_score(self) -> np.ndarray:
        if self._best_score is None:
            self._best_score = self.best_score_dev.numpy(self.stream) if self.n else np.zeros((0,), np.float32)
        return self._best_score

    @property
    def centers(self) -> np.ndarray:
        t = self.table
        return t[:, 7:10].astype(np.float64) / t[:, 0:1].astype(np.float64)

    def mask_of(self, k: int) -> DeviceArray:
        """device (N,) uint8 mask of instance k (1 .. n)"""
        from .sim import mask_from_argmax
        if self.labels_dev is None:
            raise ValueError("mask_of: the instances have been closed")
        if not 1 <= int(k) <= self.n:
            raise IndexError(f"instance {k} of {self.n}")
        return mask_from_argmax(self.labels_dev, int(k), self.stream)       # the comparison labels == k is the same kernel's

    def close(self):
        for a in (self.labels_dev, self.table_dev, self.best_score_dev):
            if a is not None:
                a.free()
        self.labels_dev = self.table_dev = self.best_score_dev = self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _is_host(x):
    return not (isinstance(x, (DeviceArray, DeviceView)) or _is_torch(x))


def label_voxels(grid_pos, mask, connectivity=26, scores=None, device=False, stream=None) -> VoxelInstances:
    """The objects among the masked voxels of a map.  grid_pos (N, 3) int32 cells (row, col, height) in any order, mask (N,) bool /
    uint8, scores (N,) float32 or None; each a host array, a DeviceArray / DeviceView or a torch tensor.  Two masked voxels are
    adjacent when their cells differ by at most 1 on every axis and on at most 1 / 2 / 3 axes (connectivity 6 / 18 / 26); voxels of
    one cell belong together; unmasked voxels take part in nothing.  Labels, count and numbering are
    scipy.ndimage.label(dense, generate_binary_structure(3, 1 | 2 | 3)) of dense[row, col, height], read back at the voxels.
    Every side of the masked voxels' bounding box is at most INSTANCES_MAX_BOX_SIDE cells (AvlError otherwise).  `best` of the
    table is the voxel of an instance's largest score, the smallest index among equals, -1 without scores; a NaN among the scores
    of an instance leaves its `best` undefined.  The instance count is read back once to size the table."""
    lib = _lib.load()
    if connectivity not in _CONNECTIVITIES:
        raise ValueError(f"connectivity must be one of {_CONNECTIVITIES}, got {connectivity!r}")
    pshape = _image_shape(grid_pos)
    if len(pshape) != 2 or pshape[1] != 3:
        raise ValueError(f"expected (N, 3) voxel cells, got shape {pshape}")
    N = pshape[0]
    for name, x in (("mask", mask), ("scores", scores)):
        if x is not None and _image_shape(x) != (N,):
            raise ValueError(f"{name} has shape {_image_shape(x)}, the map {N} voxels")
    ws, nws = _workspace(lib.avl_label_voxels_work_bytes, "avl_label_voxels", N)       # rejects a bad N before any device work
    if _is_host(grid_pos):
        grid_pos = np.asarray(grid_pos)
        if grid_pos.dtype.kind not in "iu" or (grid_pos.size and np.abs(grid_pos.astype(np.int64)).max() > np.iinfo(np.int32).max):
            raise TypeError(f"voxel cells are int32 values, got {grid_pos.dtype}")
    if _is_host(mask):
        mask = np.asarray(mask)
        if mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
            mask = mask != 0
    pp, _, k1 = as_device(grid_pos, np.int32, stream)
    mp, _, k2 = _dev_u8(mask, stream)
    sp, k3 = None, None
    if scores is not None:
        sp, _, k3 = as_device(scores, np.float32, stream)
    labels, n_dev = DeviceArray((N,), np.int32), DeviceArray((1,), np.int32)
    _lib.check(lib.avl_label_voxels(pp, mp, N, int(connectivity), labels.ptr, n_dev.ptr, ws.ptr, nws, stream), "avl_label_voxels")
    n = int(n_dev.numpy(stream)[0])
    table = best = None
    if n:
        table, best = DeviceArray((n, INSTANCE_TABLE_COLS), np.int64), DeviceArray((n,), np.float32)
        _lib.check(lib.avl_voxel_instance_table(pp, labels.ptr, sp, N, n, table.ptr, best.ptr, stream), "avl_voxel_instance_table")
    return VoxelInstances(n, N, labels, table, best, device, stream, (k1, k2, k3, ws))
