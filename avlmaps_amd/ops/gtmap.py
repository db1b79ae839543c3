"""The ground-truth label map and the scores of a predicted map against it (csrc/avl_gtmap.hip)."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _is_dev, _result
from ._rays import frame_args
from .builder import _global_depth
from .explore import EXPLORE_MAX_SIDE

GT_MAX_CLASSES = 4096
GT_MAX_VOTES = 1 << 40        # n_voxels * n_classes
CONFUSION_MAX_CLASSES = 65536
CONFUSION_MAX_COUNTERS = 1 << 28
UNLABELLED = -1               # label of a voxel / cell no vote reached


def _dtype_of(x):
    return str(x.dtype) if _is_torch(x) else np.dtype(getattr(x, "dtype", object))


def _ids_i32(x, what):
    """object / class ids of any integer dtype -> int32 on the host (a device array must be int32 already); ids that do not fit raise"""
    if _is_dev(x):
        if _dtype_of(x) not in ("torch.int32", np.dtype(np.int32)):
            raise TypeError(f"{what} on the device must be int32, got {_dtype_of(x)}")
        return x
    a = np.asarray(x)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{what} must hold integers, got {a.dtype}")
    if a.size and (int(a.max()) >= 2 ** 31 or int(a.min()) < -2 ** 31):
        raise ValueError(f"{what}: ids must fit int32 (largest {int(a.max())}, smallest {int(a.min())})")
    return np.ascontiguousarray(a, dtype=np.int32)


def obj2cls_table(obj2cls):
    """-> int32 table (n_obj,) object id -> class id (-1 = no class), or None.  obj2cls: None, an integer array, a dict
    {object id: class id | (class id, name)} (the values of dataset/README.md:80-90's obj2cls, keys int or str) or a path to a .npy
    (array) or .json (dict or list) file.  Ids that do not fit int32 and negative object ids raise ValueError."""
    if obj2cls is None:
        return None
    if isinstance(obj2cls, (str, Path)):
        path = Path(obj2cls)
        if path.suffix == ".npy":
            obj2cls = np.load(path, allow_pickle=False)
        elif path.suffix == ".json":
            import json
            obj2cls = json.loads(path.read_text())
        else:
            raise ValueError(f"obj2cls: {path} is neither .npy nor .json")
    if isinstance(obj2cls, dict):
        items = []
        for k, v in obj2cls.items():
            v = v[0] if isinstance(v, (tuple, list)) else v
            items.append((int(k), int(v)))
        if any(k < 0 for k, _ in items):
            raise ValueError("obj2cls: negative object id")
        if any(k >= 2 ** 31 or not -2 ** 31 <= v < 2 ** 31 for k, v in items):
            raise ValueError("obj2cls: ids must fit int32")
        table = np.full((max((k for k, _ in items), default=-1) + 1,), -1, np.int32)
        for k, v in items:
            table[k] = v
        return table
    table = _ids_i32(np.asarray(obj2cls), "obj2cls")
    if table.ndim != 1:
        raise ValueError(f"obj2cls: expected a 1-D table, got shape {table.shape}")
    return table


def check_label_flag(err_flag, what, stream=None):
    """raise AvlError when a label kernel found data out of range (bit 0 of its device error flag)"""
    if int(err_flag.numpy(stream)[0]) != 0:
        raise _lib.AvlError(f"{what}: an id on the device is out of range (a voxel id >= n_voxels, or a label >= the number of classes)")


def _counter_check(x, shape, dtype, what):
    """the host-side checks of an in-place counter array (None, a host array or a DeviceArray), before any device work"""
    if x is None:
        return
    if not isinstance(x, (np.ndarray, DeviceArray)) or np.dtype(x.dtype) != np.dtype(dtype):
        raise TypeError(f"{what} must be a host array or DeviceArray of {np.dtype(dtype)}, got {getattr(x, 'dtype', type(x).__name__)}")
    if tuple(int(s) for s in x.shape) != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(x.shape)}")


def _counter_arg(x, shape, dtype, stream):
    """an in-place counter array that passed _counter_check: None (new, zero), a host array (updated in place) or a DeviceArray
    -> (ptr, owner, host)"""
    if x is None:
        d = DeviceArray(shape, dtype).zero_(stream)
        return d.ptr, d, None
    if isinstance(x, np.ndarray):
        d = DeviceArray.from_numpy(x, stream)
        return d.ptr, d, x
    return x.ptr, x, None


def _counter_result(owner, host, device, stream):
    if device:
        return owner
    out = owner.numpy(stream)
    if host is not None:
        np.copyto(host, out)
        return host
    return out


def gt_vote(votes, depth, semantic, calib, transforms, occupied_ids, n_voxels, n_classes, cs, stride=1, min_depth=0.1, max_depth=6.0,
            obj2cls=None, depth_div=1000.0, stats=None, err_flag=None, device=False, stream=None):
    """Fold the semantic frames of F views into per-voxel class counts (avl_gt_vote; the vote is defined at the top of
    csrc/avl_gtmap.hip).  -> (votes (n_voxels, n_classes) uint32, stats (4,) uint64: pixels dropped by depth or grid, by class,
    for want of a voxel, and votes cast).  votes / stats: None (new, zero), a host array (updated in place and returned) or a
    DeviceArray (updated in place; returned as it is with device=True).  depth: (F, H, W) or (H, W), uint16 (value / depth_div
    metres) or float32 metres; semantic: the same shape, object ids of any integer dtype (converted to int32 on the host; a device
    array must be int32), or class ids when obj2cls is None; obj2cls: an int table object id -> class id (see obj2cls_table), host
    or device; calib: the 3 x 3 camera matrix; transforms: (F, 4, 4) camera -> map (VLMapBuilder.frame_transforms); occupied_ids:
    the map's (gs, gs, vh) int32 voxel index, host or device.  err_flag: a zeroed (1,) int32 DeviceArray to collect the error bit
    of several calls (check it with check_label_flag); None: this call checks its own, which waits for the launch.  TypeError on
    other dtypes, ValueError on bad shapes or parameters, before any device work."""
    stride, n_voxels, n_classes = int(stride), int(n_voxels), int(n_classes)
    if not 1 <= n_classes <= GT_MAX_CLASSES:
        raise ValueError(f"gt_vote: {n_classes} classes (1 .. {GT_MAX_CLASSES})")
    if n_voxels < 0 or n_voxels * n_classes >= GT_MAX_VOTES:
        raise ValueError(f"gt_vote: {n_voxels} voxels x {n_classes} classes (N * C < 2^40)")
    F, H, W, Kinv, T, _ = frame_args("gt_vote", depth, calib, transforms, None, stride, cs, min_depth, max_depth)
    semantic = _ids_i32(semantic, "semantic")
    sshape = tuple(int(s) for s in semantic.shape)
    if (sshape if len(sshape) == 3 else (1,) + sshape) != (F, H, W):
        raise ValueError(f"gt_vote: depth frames of shape {(F, H, W)} but semantic frames of shape {sshape}")
    if _dtype_of(occupied_ids) not in ("torch.int32", np.dtype(np.int32)):
        raise TypeError(f"occupied_ids must be int32, got {_dtype_of(occupied_ids)}")
    oshape = tuple(int(s) for s in occupied_ids.shape)
    if len(oshape) != 3 or oshape[0] != oshape[1] or not 1 <= oshape[0] <= EXPLORE_MAX_SIDE or oshape[2] < 1:
        raise ValueError(f"gt_vote: occupied_ids must be (gs, gs, vh) with gs <= {EXPLORE_MAX_SIDE}, got shape {oshape}")
    gs, vh = oshape[0], oshape[2]
    if obj2cls is not None:
        obj2cls = _ids_i32(obj2cls, "obj2cls")
        if len(obj2cls.shape) != 1 or int(obj2cls.shape[0]) < 1:
            raise ValueError(f"gt_vote: obj2cls must be a non-empty 1-D table, got shape {tuple(obj2cls.shape)}")
    _counter_check(votes, (n_voxels, n_classes), np.uint32, "votes")
    _counter_check(stats, (4,), np.uint64, "stats")
    lib = _lib.load()
    _lib.require_gpu()
    vp, vown, vhost = _counter_arg(votes, (n_voxels, n_classes), np.uint32, stream)
    sp, sown, shost = _counter_arg(stats, (4,), np.uint64, stream)
    own_flag = err_flag is None
    if own_flag:
        err_flag = DeviceArray((1,), np.int32).zero_(stream)
    keep = []
    if F:
        dp, _, k1, is_u16 = _global_depth(depth, stream)
        mp, _, k2 = as_device(semantic, np.int32, stream)
        op, _, k3 = as_device(occupied_ids, np.int32, stream)
        tp, n_obj, k4 = None, 0, None
        if obj2cls is not None:
            tp, _, k4 = as_device(obj2cls, np.int32, stream)
            n_obj = int(obj2cls.shape[0])
        keep = [k1, k2, k3, k4]
        _lib.check(lib.avl_gt_vote(dp, int(is_u16), float(depth_div), mp, F, H, W, Kinv.ctypes.data, T.ctypes.data, gs, float(cs), vh, stride,
                                   float(min_depth), float(max_depth), tp, n_obj, n_classes, op, n_voxels, vp, sp, err_flag.ptr, stream),
                   "avl_gt_vote")
    if own_flag:
        check_label_flag(err_flag, "gt_vote", stream)
    elif device:
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")              # the staged frames may be released on return
    del keep
    return _counter_result(vown, vhost, device, stream), _counter_result(sown, shost, device, stream)


def gt_labels(votes, device=False, stream=None):
    """-> (label (N,) int32, support (N,) uint32) of a (N, C) uint32 vote array, host or device (avl_gt_labels): the lowest class
    whose count is the row's maximum, UNLABELLED (-1) for an all-zero row, and the row's sum (wrapping at 2^32)."""
    if not isinstance(votes, (np.ndarray, DeviceArray, DeviceView)) or np.dtype(votes.dtype) != np.dtype(np.uint32):
        raise TypeError(f"votes must be a host array or DeviceArray of uint32, got {getattr(votes, 'dtype', type(votes).__name__)}")
    shape = tuple(int(s) for s in votes.shape)
    if len(shape) != 2 or not 1 <= shape[1] <= GT_MAX_CLASSES or shape[0] * shape[1] >= GT_MAX_VOTES:
        raise ValueError(f"gt_labels: votes must be (N, C) with 1 <= C <= {GT_MAX_CLASSES} and N * C < 2^40, got shape {shape}")
    lib = _lib.load()
    _lib.require_gpu()
    N, C_ = shape
    if isinstance(votes, np.ndarray):
        keep = DeviceArray.from_numpy(votes, stream)
        vp = keep.ptr
    else:
        vp, keep = votes.ptr, votes
    label, support = DeviceArray((N,), np.int32), DeviceArray((N,), np.uint32)
    _lib.check(lib.avl_gt_labels(vp, N, C_, label.ptr, support.ptr, stream), "avl_gt_labels")
    if device:
        label._keep = support._keep = (keep,)
        return label, support
    return label.numpy(stream), support.numpy(stream)


def pool_labels_2d(labels, occupied_ids, window=None, err_flag=None, device=False, stream=None):
    """The label-valued top-down pool (avl_pool_labels_2d): (r1 - r0 + 1, c1 - c0 + 1) int32 over window = (r0, r1, c0, c1), both
    ends included (None: the whole grid); a cell holds the label of the highest voxel of its column that has one (label >= 0),
    UNLABELLED (-1) when none has.  labels: (N,) int32; occupied_ids: (gs, gs, vh) int32; host or device."""
    labels = _ids_i32(labels, "labels")
    if _dtype_of(occupied_ids) not in ("torch.int32", np.dtype(np.int32)):
        raise TypeError(f"occupied_ids must be int32, got {_dtype_of(occupied_ids)}")
    oshape = tuple(int(s) for s in occupied_ids.shape)
    if len(oshape) != 3 or oshape[0] != oshape[1] or not 1 <= oshape[0] <= EXPLORE_MAX_SIDE or oshape[2] < 1:
        raise ValueError(f"pool_labels_2d: occupied_ids must be (gs, gs, vh) with gs <= {EXPLORE_MAX_SIDE}, got shape {oshape}")
    if len(labels.shape) != 1:
        raise ValueError(f"pool_labels_2d: labels must be (N,), got shape {tuple(labels.shape)}")
    gs, vh = oshape[0], oshape[2]
    r0, r1, c0, c1 = (0, gs - 1, 0, gs - 1) if window is None else (int(w) for w in window)
    if not (0 <= r0 <= r1 < gs and 0 <= c0 <= c1 < gs):
        raise ValueError(f"pool_labels_2d: window rows {r0} .. {r1}, columns {c0} .. {c1} of a grid of {gs}")
    lib = _lib.load()
    _lib.require_gpu()
    lp, _, k1 = as_device(labels, np.int32, stream)
    op, _, k2 = as_device(occupied_ids, np.int32, stream)
    own_flag = err_flag is None
    if own_flag:
        err_flag = DeviceArray((1,), np.int32).zero_(stream)
    out = DeviceArray((r1 - r0 + 1, c1 - c0 + 1), np.int32)
    _lib.check(lib.avl_pool_labels_2d(lp, int(labels.shape[0]), op, gs, vh, r0, r1, c0, c1, out.ptr, err_flag.ptr, stream),
               "avl_pool_labels_2d")
    if own_flag:
        check_label_flag(err_flag, "pool_labels_2d", stream)
    return _result(out, device, stream, keep=(k1, k2))


def label_confusion_limits() -> int:
    """the largest n_gt_classes * n_pred_classes label_confusion counts in LDS; larger matrices take global atomics"""
    n = C.c_int(0)
    _lib.check(_lib.load().avl_label_confusion_limits(C.byref(n)), "avl_label_confusion_limits")
    return n.value


def label_confusion(gt, pred, n_gt_classes, n_pred_classes, conf=None, skipped=None, err_flag=None, device=False, stream=None):
    """-> (conf (n_gt_classes, n_pred_classes) uint64, skipped (2,) uint64) of two label arrays of one length (avl_label_confusion):
    gt < 0 counts in skipped[0]; otherwise pred < 0 counts in skipped[1]; otherwise conf[gt, pred] += 1.  A label at or above its
    number of classes raises AvlError.  conf / skipped: None (new, zero), a host array (updated in place and returned) or a
    DeviceArray (updated in place).  gt, pred: int32 on the device, any integer dtype on the host."""
    Cg, Cp = int(n_gt_classes), int(n_pred_classes)
    if not (1 <= Cg <= CONFUSION_MAX_CLASSES and 1 <= Cp <= CONFUSION_MAX_CLASSES and Cg * Cp <= CONFUSION_MAX_COUNTERS):
        raise ValueError(f"label_confusion: a {Cg} x {Cp} matrix (sides 1 .. {CONFUSION_MAX_CLASSES}, at most 2^28 counters)")
    gt, pred = _ids_i32(gt, "gt"), _ids_i32(pred, "pred")
    gshape, pshape = tuple(int(s) for s in gt.shape), tuple(int(s) for s in pred.shape)
    if gshape != pshape:
        raise ValueError(f"label_confusion: gt of shape {gshape} but pred of shape {pshape}")
    n = int(np.prod(gshape, dtype=np.int64))
    _counter_check(conf, (Cg, Cp), np.uint64, "conf")
    _counter_check(skipped, (2,), np.uint64, "skipped")
    lib = _lib.load()
    _lib.require_gpu()
    cp_, cown, chost = _counter_arg(conf, (Cg, Cp), np.uint64, stream)
    sp, sown, shost = _counter_arg(skipped, (2,), np.uint64, stream)
    own_flag = err_flag is None
    if own_flag:
        err_flag = DeviceArray((1,), np.int32).zero_(stream)
    k1 = k2 = None
    if n:
        gp, _, k1 = as_device(gt, np.int32, stream)
        pp, _, k2 = as_device(pred, np.int32, stream)
        _lib.check(lib.avl_label_confusion(gp, pp, n, Cg, Cp, cp_, sp, err_flag.ptr, stream), "avl_label_confusion")
    if own_flag:
        check_label_flag(err_flag, "label_confusion", stream)
    elif device:
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    del k1, k2
    return _counter_result(cown, chost, device, stream), _counter_result(sown, shost, device, stream)


class MapScores:
    """the scores of a predicted label map against the ground truth (map_scores): pixel_acc, mean_acc, miou, fwiou (float64), the
    per-class acc and iou ((Cg,) float64, NaN for a class without ground truth), support ((Cg,) int64, the row sums), the integer
    matrix conf they come from and, when known, skipped = (entries without ground truth, entries without a prediction)"""

    def __init__(self, pixel_acc, mean_acc, miou, fwiou, acc, iou, support, conf, skipped=None, categories=None):
        self.pixel_acc, self.mean_acc, self.miou, self.fwiou = pixel_acc, mean_acc, miou, fwiou
        self.acc, self.iou, self.support, self.conf, self.skipped, self.categories = acc, iou, support, conf, skipped, categories

    def as_dict(self) -> dict:
        names = list(self.categories) if self.categories is not None else [str(k) for k in range(len(self.acc))]
        nan = lambda x: None if np.isnan(x) else float(x)      # noqa: E731
        return dict(pixel_acc=nan(self.pixel_acc), mean_acc=nan(self.mean_acc), miou=nan(self.miou), fwiou=nan(self.fwiou),
                    total=int(self.support.sum()), skipped=None if self.skipped is None else [int(s) for s in self.skipped],
                    classes=[dict(id=k, name=names[k] if k < len(names) else str(k), support=int(self.support[k]), acc=nan(self.acc[k]),
                                  iou=nan(self.iou[k])) for k in range(len(self.acc))])

    def __repr__(self):
        return (f"MapScores(pixel_acc={self.pixel_acc:.4f}, mean_acc={self.mean_acc:.4f}, miou={self.miou:.4f}, fwiou={self.fwiou:.4f}, "
                f"total={int(self.support.sum())})")


def map_scores(conf, skipped=None, categories=None) -> MapScores:
    """Pixel accuracy, mean accuracy, mIoU and frequency-weighted IoU of a (Cg, Cp) integer confusion matrix (rows = ground truth),
    host-side in float64:  pixel_acc = trace / total;  acc[k] = conf[k, k] / row_sum[k];  iou[k] = conf[k, k] / (row_sum[k] +
    col_sum[k] - conf[k, k]) with col_sum[k] = conf[k, k] = 0 for k >= Cp;  mean_acc, miou = np.mean over the classes with
    row_sum > 0 in class order;  fwiou = (sum of row_sum[k] * iou[k] over those classes, added in class order) / total.  Cp may
    exceed Cg (init_categories appends "other": a voxel predicted "other" is simply wrong).  An empty matrix gives NaN scores."""
    m = np.asarray(conf)
    if m.ndim != 2 or m.dtype.kind not in "iu":
        raise ValueError(f"map_scores: expected a 2-D integer matrix, got {m.dtype}{m.shape}")
    m = m.astype(np.int64)
    Cg, Cp = m.shape
    row_sum = m.sum(axis=1)
    col_sum, diag = np.zeros(Cg, np.int64), np.zeros(Cg, np.int64)
    k = min(Cg, Cp)
    col_sum[:k] = m.sum(axis=0)[:k]
    diag[:k] = np.diagonal(m)[:k]
    total = int(row_sum.sum())
    valid = row_sum > 0
    acc, iou = np.full(Cg, np.nan), np.full(Cg, np.nan)
    acc[valid] = diag[valid] / row_sum[valid]
    iou[valid] = diag[valid] / (row_sum[valid] + col_sum[valid] - diag[valid])
    if total == 0:
        return MapScores(np.nan, np.nan, np.nan, np.nan, acc, iou, row_sum, m, skipped, categories)
    weighted = 0.0
    for c in np.flatnonzero(valid):
        weighted += float(row_sum[c]) * float(iou[c])
    return MapScores(int(diag.sum()) / total, float(np.mean(acc[valid])), float(np.mean(iou[valid])), weighted / total, acc, iou, row_sum,
                     m, skipped, categories)
