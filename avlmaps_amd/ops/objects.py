"""The scene inventory: the objects of ALL classes of a voxel list in one labelling, the score of every voxel's own class, and the
score rows pooled per object in a pinned order (csrc/avl_objects.hip).  Upstream has no counterpart; map/map.py:146-151 and
map/vlmap_3d.py:75-100 stop at one category's mask."""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _image_shape, _is_dev, _result, _workspace
from .instances import Instance3D, INSTANCE_TABLE_COLS, VoxelInstances
from .select import _scores_matrix, _scores_shape

POOL_CHUNK = 256                # members per partial sum of pool_rows (kPoolChunk of csrc/avl_objects.hip): part of the result's definition
_CONNECTIVITIES = (6, 18, 26)


class Object3D(NamedTuple):
    """One object of a scene (VLMap.get_objects).  The first seven fields are Instance3D's, with `label` the object's number among
    ALL objects of the scene, 1 .. n in order of (first cell, category).  category / name: the class its voxels were labelled with
    (their row argmax) and its name; voted / voted_name: the column with the largest MEAN score over the object's voxels (the first
    one among equals) and its name; mean_score: the mean of `category`'s column; margin: the largest mean score minus the second
    largest, inf with one column."""
    label: int
    count: int
    bbox: Tuple[int, int, int, int, int, int]
    center: Tuple[float, float, float]
    best_voxel: int
    best_score: float
    cell: Tuple[int, int]
    category: int
    name: str
    voted: int
    voted_name: str
    mean_score: float
    margin: float

    @classmethod
    def from_row(cls, label, row, best_score, category, mean_row, names):
        """row: one row of a VoxelObjects table; mean_row: the object's (Q,) mean scores; names: the Q column names"""
        voted, margin = vote_rows(np.asarray(mean_row, np.float64)[None, :])
        category, voted = int(category), int(voted[0])
        return cls(*Instance3D.from_row(label, row, best_score), category, str(names[category]), voted, str(names[voted]),
                   float(mean_row[category]), float(margin[0]))


def vote_rows(mean_scores):
    """(voted (n,) int32, margin (n,) float64) of mean_scores (n, Q): the first maximum of every row, and the largest value minus
    the second largest (0 when the maximum is shared, inf for Q = 1).  Host NumPy."""
    m = np.asarray(mean_scores, np.float64)
    if m.ndim != 2 or m.shape[1] < 1:
        raise ValueError(f"expected (n, Q) mean scores with Q >= 1, got shape {m.shape}")
    voted = np.argmax(m, axis=1).astype(np.int32)
    if m.shape[1] == 1:
        return voted, np.full(m.shape[0], np.inf)
    top = np.sort(m, axis=1)[:, -2:]
    return voted, top[:, 1] - top[:, 0]


class VoxelObjects(VoxelInstances):
    """label_voxel_classes' result: n objects among N voxels.  labels, table, best_score, centers, mask_of(k) and close() are
    VoxelInstances'; classes_of: (n,) int32, the class of every object = classes[first].  classes: the classes as they were given,
    which classes_of reads on its first use; given on the device they are copied back then, once, unless the caller who has them
    on the host as well puts that array here first."""

    def __init__(self, n, N, labels_dev, table_dev, best_dev, device, stream, keep, classes):
        super().__init__(n, N, labels_dev, table_dev, best_dev, device, stream, keep)
        self.classes, self._classes_of = classes, None

    @property
    def classes_of(self) -> np.ndarray:
        if self._classes_of is None:
            c = self.classes
            if isinstance(c, DeviceArray):
                c = c.numpy(self.stream)
            elif _is_torch(c):
                c = c.cpu().numpy()
            elif isinstance(c, DeviceView):
                raise TypeError("classes_of: the classes of a DeviceView cannot be copied back, put a host array into `classes`")
            self._classes_of = np.asarray(c).astype(np.int32)[self.table[:, 10]] if self.n else np.zeros((0,), np.int32)
            self.classes = None
        return self._classes_of


def label_voxel_classes(grid_pos, classes, connectivity=26, scores=None, device=False, stream=None) -> VoxelObjects:
    """The objects of all classes among the voxels of a map, in one pass.  grid_pos (N, 3) int32 cells (row, col, height) in any
    order, classes (N,) int32 (any ids >= 0; a negative class: the voxel takes part in nothing), scores (N,) float32 or None; each
    a host array, a DeviceArray / DeviceView or a torch tensor.  Two voxels are adjacent when their cells are (as in label_voxels,
    connectivity 6 / 18 / 26) and their classes are equal; voxels of one cell belong together when their classes are equal.
    Objects are numbered 1 .. n in lexicographic order of (first cell, class): scipy.ndimage.label once per class on that class's
    dense array, all components then sorted by (first cell, class).  The table is label_voxels' (avl_voxel_instance_table on these
    labels), `best` the voxel of an object's largest score.  Every side of the participating voxels' bounding box is at most
    INSTANCES_MAX_BOX_SIDE cells (AvlError otherwise).  The object count is read back once to size the table."""
    lib = _lib.load()
    if connectivity not in _CONNECTIVITIES:
        raise ValueError(f"connectivity must be one of {_CONNECTIVITIES}, got {connectivity!r}")
    pshape = _image_shape(grid_pos)
    if len(pshape) != 2 or pshape[1] != 3:
        raise ValueError(f"expected (N, 3) voxel cells, got shape {pshape}")
    N = pshape[0]
    for name, x in (("classes", classes), ("scores", scores)):
        if (x is not None or name == "classes") and _image_shape(x) != (N,):
            raise ValueError(f"{name} has shape {_image_shape(x)}, the map {N} voxels")
    for name, x in (("voxel cells", grid_pos), ("classes", classes)):
        if not _is_dev(x):
            x = np.asarray(x)
            if x.dtype.kind not in "iu" or (x.size and np.abs(x.astype(np.int64)).max() > np.iinfo(np.int32).max):
                raise TypeError(f"{name} are int32 values, got {x.dtype}")
    ws, nws = _workspace(lib.avl_label_classes_work_bytes, "avl_label_classes", N)     # rejects a bad N before any device work
    pp, _, k1 = as_device(grid_pos, np.int32, stream)
    cp, _, k2 = as_device(classes, np.int32, stream)
    sp, k3 = None, None
    if scores is not None:
        sp, _, k3 = as_device(scores, np.float32, stream)
    labels, n_dev = DeviceArray((N,), np.int32), DeviceArray((1,), np.int32)
    _lib.check(lib.avl_label_classes(pp, cp, N, int(connectivity), labels.ptr, n_dev.ptr, ws.ptr, nws, stream), "avl_label_classes")
    n = int(n_dev.numpy(stream)[0])
    table = best = None
    if n:
        table, best = DeviceArray((n, INSTANCE_TABLE_COLS), np.int64), DeviceArray((n,), np.float32)
        _lib.check(lib.avl_voxel_instance_table(pp, labels.ptr, sp, N, n, table.ptr, best.ptr, stream), "avl_voxel_instance_table")
    return VoxelObjects(n, N, labels, table, best, device, stream, (k1, k2, k3, ws), classes if _is_dev(classes) else np.asarray(classes))


def pick_columns(rows, cols, device=False, stream=None):
    """(N,) float32: rows[i, cols[i]] of rows (N, C) float32 (host or device; a column slice of a wider matrix is read in place),
    0 where cols[i] (N,) int32 lies outside 0 .. C - 1.  With cols the row argmax: every voxel's score of its own class."""
    lib = _lib.load()
    N, C = _scores_shape(rows)
    if _image_shape(cols) != (N,):
        raise ValueError(f"cols has shape {_image_shape(cols)}, the matrix {N} rows")
    _lib.require_gpu()
    out = DeviceArray((N,), np.float32)
    keep = ()
    if N:
        rp, N, C, ld, k1 = _scores_matrix(rows, stream)
        cp, _, k2 = as_device(cols, np.int32, stream)
        _lib.check(lib.avl_pick_columns(rp, N, C, ld, cp, out.ptr, stream), "avl_pick_columns")
        keep = (k1, k2)
    return _result(out, device, stream, keep=keep)


def pool_rows(rows, labels, n, device=False, stream=None):
    """(n, C) float64: row k - 1 = the sum of the rows of `rows` (N, C) float32 whose label is k; labels (N,) int32 outside 1 .. n
    take part in nothing and an object without a member gets zeros.  The order of the additions is pinned, so the bytes are the
    same on every run: an object's members in ascending row index, cut into chunks of POOL_CHUNK consecutive members; a chunk's
    partial is the sequential float64 sum of its rows, from 0.0; the object's sum is the sequential float64 sum of its partials in
    chunk order, from 0.0.  Pools any per-voxel matrix: the scores, a stack of heats."""
    lib = _lib.load()
    N, C = _scores_shape(rows)
    n = int(n)
    if n < 0:
        raise ValueError(f"n = {n} objects")
    if _image_shape(labels) != (N,):
        raise ValueError(f"labels has shape {_image_shape(labels)}, the matrix {N} rows")
    if n == 0:
        if not device:
            return np.zeros((0, C), np.float64)
        _lib.require_gpu()
        return DeviceArray((0, C), np.float64)
    ws, nws = _workspace(lib.avl_pool_rows_work_bytes, "avl_pool_rows", N, C, n)       # rejects bad sizes before any device work
    rp, ld, k1 = None, C, None
    if N:
        rp, N, C, ld, k1 = _scores_matrix(rows, stream)
    lp, _, k2 = as_device(labels, np.int32, stream)
    out = DeviceArray((n, C), np.float64)
    _lib.check(lib.avl_pool_rows(rp, N, C, ld, lp, n, out.ptr, ws.ptr, nws, stream), "avl_pool_rows")
    return _result(out, device, stream, keep=(k1, k2, ws))
