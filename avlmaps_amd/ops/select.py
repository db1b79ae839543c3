"""Open-set queries: exact order statistics and quantiles of the columns of a score matrix, and the voxels above a column's own
threshold (csrc/avl_colselect.hip).  Replaces upstream's map/clip_map.py:62-75 (CLIPMap.load_categories: np.percentile and the
comparison per category on a host copy), which cannot be imported upstream."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, _is_torch
from ._args import _is_dev, _workspace

COLSELECT_SLOTS = 64            # (column, k) pairs of one group of passes: 64 x 256 LDS counters


class ColumnOrderStats(NamedTuple):
    """column_order_stats' result, one entry per slot (column, k).  v_k: the k-th smallest value of the column (float32, k = 0 the
    minimum) in np.sort's order, where every NaN is one largest value and -0 = +0 (a zero comes back as +0); v_next: the (k+1)-th
    smallest, v_k itself for k = N - 1; count_lt / count_le: the number of elements before / up to the run of values equal to v_k
    in the sorted column (int64; for a finite or infinite v_k these are (column < v_k).sum() and (column <= v_k).sum());
    nan_count: the column's NaNs (int64)."""
    v_k: np.ndarray
    v_next: np.ndarray
    count_lt: np.ndarray
    count_le: np.ndarray
    nan_count: np.ndarray


def _scores_matrix(scores, stream):
    """(N, Q) float32 scores, host or device -> (ptr, N, Q, ld, keepalive).  A view of a wider row-major matrix (a NumPy or torch
    column slice with unit column stride) is taken as it lies, with the wider row stride ld; anything else is made contiguous."""
    if isinstance(scores, (DeviceArray, DeviceView)):
        if scores.dtype != np.float32:
            raise TypeError(f"expected float32 scores, got {scores.dtype}")
        shape, ld, ptr, keep = scores.shape, None, scores.ptr, scores
    elif _is_torch(scores):
        import torch
        if not scores.is_cuda:
            raise TypeError("torch tensors passed to avlmaps_amd must live on the GPU")
        if scores.dtype != torch.float32:
            raise TypeError(f"expected torch.float32 scores, got {scores.dtype}")
        shape, ld = tuple(scores.shape), None
        if len(shape) == 2 and shape[0] > 1 and shape[1] >= 1:
            if scores.stride(1) == 1 and scores.stride(0) >= shape[1]:
                ld = int(scores.stride(0))
            else:
                scores = scores.contiguous()
        ptr, keep = scores.data_ptr(), scores
    else:
        a = np.asarray(scores)
        if a.dtype != np.float32:
            raise TypeError(f"expected float32 scores, got {a.dtype}")
        shape, ld = a.shape, None
        if a.ndim == 2 and a.shape[0] > 1 and a.shape[1] >= 1 and a.strides[1] == 4 and a.strides[0] % 4 == 0 and a.strides[0] > 4 * a.shape[1]:
            ld = a.strides[0] // 4                       # upload the rows as they lie, from the view's first to its last element
            a = np.lib.stride_tricks.as_strided(a, shape=((a.shape[0] - 1) * ld + a.shape[1],), strides=(4,), writeable=False)
        _lib.require_gpu()
        keep = DeviceArray.from_numpy(np.ascontiguousarray(a), stream)
        ptr = keep.ptr
    if len(shape) != 2 or shape[1] < 1:
        raise ValueError(f"expected an (N, Q) score matrix with Q >= 1, got shape {tuple(shape)}")
    N, Q = int(shape[0]), int(shape[1])
    return ptr, N, Q, (Q if ld is None else ld), keep


def _scores_shape(scores):
    shape = tuple(int(s) for s in (scores.shape if hasattr(scores, "shape") else np.asarray(scores).shape))
    if len(shape) != 2 or shape[1] < 1:
        raise ValueError(f"expected an (N, Q) score matrix with Q >= 1, got shape {shape}")
    return shape


def column_order_stats(scores, columns, ks, stream=None) -> ColumnOrderStats:
    """Exact order statistics of columns of `scores` (N, Q) float32 -- a host array, a DeviceArray / DeviceView or a torch tensor; a
    column slice of a wider matrix is read in place.  Slot s asks for the ks[s]-th smallest value (0 <= k < N) of column columns[s];
    a column may appear in several slots, and more than COLSELECT_SLOTS slots go in groups of that many.  A radix select on the
    device (avl_colselect_f32): nothing but the five small tables comes back.  See ColumnOrderStats for the order and the counts."""
    lib = _lib.load()
    columns = np.ascontiguousarray(np.atleast_1d(columns), dtype=np.int64)
    ks = np.ascontiguousarray(np.atleast_1d(ks), dtype=np.int64)
    if columns.ndim != 1 or columns.shape != ks.shape:
        raise ValueError(f"columns and ks must be two 1-D tables of one length, got {columns.shape} and {ks.shape}")
    N, Q = _scores_shape(scores)
    if N < 1:
        raise ValueError("a matrix without rows has no order statistics")
    if columns.size and (columns.min() < 0 or columns.max() >= Q):
        raise IndexError(f"columns must lie in [0, {Q}), got {int(columns.min())} .. {int(columns.max())}")
    if ks.size and (ks.min() < 0 or ks.max() >= N):
        raise IndexError(f"ks must lie in [0, {N}), got {int(ks.min())} .. {int(ks.max())}")
    S = int(columns.size)
    if S == 0:
        return ColumnOrderStats(np.zeros(0, np.float32), np.zeros(0, np.float32), *(np.zeros(0, np.int64) for _ in range(3)))
    cols32 = columns.astype(np.int32)
    ws, nws = _workspace(lib.avl_colselect_workspace_bytes, "avl_colselect_workspace_bytes", S)
    ptr, N, Q, ld, keep = _scores_matrix(scores, stream)
    floats, counts = DeviceArray((2, S), np.float32), DeviceArray((3, S), np.int64)
    _lib.check(lib.avl_colselect_f32(ptr, N, Q, ld, cols32.ctypes.data, ks.ctypes.data, S, floats.ptr, floats.ptr + 4 * S, counts.ptr,
                                     counts.ptr + 8 * S, counts.ptr + 16 * S, ws.ptr, nws, stream), "avl_colselect_f32")
    f, c = floats.numpy(stream), counts.numpy(stream)
    del keep
    return ColumnOrderStats(f[0], f[1], c[0], c[1], c[2])


def quantile_lerp(v_k, v_next, t):
    """NumPy's _lerp in float64: v_k + d * t, or v_next - d * (1 - t) where t >= 0.5, with d = v_next - v_k"""
    a, b, t = np.asarray(v_k, np.float64), np.asarray(v_next, np.float64), np.asarray(t, np.float64)
    with np.errstate(invalid="ignore"):
        d = b - a
        return np.where(t >= 0.5, b - d * (1 - t), a + d * t)


def quantile_index(q, N):
    """(k, t) of the q-th percentile of N sorted values with linear interpolation: h = (q / 100) * (N - 1), k = floor(h), t = h - k"""
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"percentiles lie in [0, 100], got {q!r}")
    h = np.float64(q) / np.float64(100) * np.float64(N - 1)
    k = np.floor(h)
    return int(k), np.float64(h - k)


def column_quantiles(scores, q, columns=None, stream=None) -> np.ndarray:
    """The q-th percentile (0 .. 100) of every column of `scores` (N, Q) float32 -- or of `columns` -- as float64, from two exact order
    statistics of the device's radix select and NumPy's linear interpolation between them in float64 on the host:
    np.percentile(column.astype(np.float64), q) bit for bit; a column with a NaN gives NaN, as NumPy does.  NOT np.percentile of the
    float32 column, which since NumPy 2.0 computes the position h in float32 (a spacing of 0.125 at two million rows)."""
    N, Q = _scores_shape(scores)
    if N < 1:
        raise ValueError("a matrix without rows has no quantiles")
    columns = np.arange(Q, dtype=np.int64) if columns is None else np.ascontiguousarray(np.atleast_1d(columns), dtype=np.int64)
    k, t = quantile_index(q, N)
    st = column_order_stats(scores, columns, np.full(columns.shape, k, np.int64), stream)
    out = quantile_lerp(st.v_k, st.v_next, t)
    out[st.nan_count > 0] = np.nan
    return out


def cols_above(scores, thresholds, column=None, device=False, stream=None):
    """Which scores lie above their column's threshold: scores (N, Q) float32 as for column_order_stats, thresholds (Q,) float64
    (host or device).  -> (bits, counts) or, with `column`, (bits, counts, mask): bits (N, ceil(Q / 64)) uint64 with bit c % 64 of word
    c / 64 of row r set iff float64(scores[r, c]) > thresholds[c] (a NaN on either side is not above); counts (Q,) int64, the set
    bits of every column, always a host array; mask (N,) uint8, the chosen column's bits as the 0 / 1 voxel mask that pool_label_2d,
    label_voxels and heatmap_from_mask take.  device=True leaves bits and mask on the device.  One pass (avl_cols_above_f32)."""
    lib = _lib.load()
    N, Q = _scores_shape(scores)
    if column is not None and not 0 <= int(column) < Q:
        raise IndexError(f"column {column} of {Q}")
    if _is_dev(thresholds):
        from ..device import as_device
        tp, tshape, tkeep = as_device(thresholds, np.float64, stream)
    else:
        thresholds = np.ascontiguousarray(thresholds, dtype=np.float64)
        tshape, tp, tkeep = thresholds.shape, None, None
    if tuple(tshape) != (Q,):
        raise ValueError(f"thresholds have shape {tuple(tshape)}, the scores {Q} columns")
    _lib.require_gpu()
    if tp is None:
        tkeep = DeviceArray.from_numpy(thresholds, stream)
        tp = tkeep.ptr
    ptr, N, Q, ld, keep = _scores_matrix(scores, stream) if N else (None, N, Q, Q, None)
    groups = (Q + 63) // 64
    bits, counts = DeviceArray((N, groups), np.uint64), DeviceArray((Q,), np.int64)
    mask = DeviceArray((N,), np.uint8) if column is not None else None
    _lib.check(lib.avl_cols_above_f32(ptr, N, Q, ld, tp, -1 if column is None else int(column), bits.ptr, counts.ptr,
                                      None if mask is None else mask.ptr, stream), "avl_cols_above_f32")
    counts = counts.numpy(stream)                     # (synchronises: the inputs of the launch may go)
    if not device:
        bits = bits.numpy(stream)
        mask = None if mask is None else mask.numpy(stream)
    del keep, tkeep
    return (bits, counts) if column is None else (bits, counts, mask)
