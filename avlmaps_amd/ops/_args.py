"""The marshalling the kernel families share: the device predicate, the image coercers, the workspace query and the result hand-back.
Coercers that belong to one family (their checks and messages differ on purpose) live in that family's module."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch


def _is_dev(x):
    return isinstance(x, (DeviceArray, DeviceView)) or _is_torch(x)


def _workspace(work_bytes, what, *dims):
    """(workspace DeviceArray, its size in bytes) for `dims`: `work_bytes` is the kernel's avl_*_work_bytes, which also rejects bad
    dimensions -- a host-side query, so a caller that runs this first rejects them before any device work; `what` names the caller
    in the error.  The buffer is allocated only once a GPU is known to be there."""
    n = C.c_size_t(0)
    _lib.check(work_bytes(*dims, C.byref(n)), what)
    _lib.require_gpu()
    return DeviceArray((n.value,), np.uint8), n.value


def _dev_u8(x, stream):
    """bool / uint8 host array, DeviceArray or torch tensor -> uint8 device pointer"""
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x).astype(np.uint8, copy=False)
    elif _is_torch(x):
        import torch
        if x.dtype == torch.bool:
            x = x.to(torch.uint8)
    return as_device(x, np.uint8, stream)


def _image_u8(x, stream):
    """2-D bool / uint8 image, host or device -> (ptr, (H, W), keepalive)"""
    ptr, shape, keep = _dev_u8(x, stream)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D image, got shape {tuple(shape)}")
    return ptr, (int(shape[0]), int(shape[1])), keep


def _image_any(x, stream):
    """2-D image -> (ptr, (H, W), is_u8, keepalive): float64 stays float64, everything else becomes uint8 (nonzero = true)"""
    dt = np.dtype(x.dtype) if isinstance(x, (np.ndarray, DeviceArray, DeviceView)) else None
    if dt is None and not _is_torch(x):
        x = np.asarray(x)
        dt = x.dtype
    if dt is not None and dt == np.float64:
        ptr, shape, keep = as_device(x, np.float64, stream)
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"expected a non-empty 2-D image, got shape {tuple(shape)}")
        return ptr, (int(shape[0]), int(shape[1])), 0, keep
    if _is_torch(x):
        import torch
        if x.dtype == torch.float64:
            ptr, shape, keep = as_device(x, np.float64, stream)
            return ptr, (int(shape[0]), int(shape[1])), 0, keep
    if isinstance(x, np.ndarray) and x.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        x = x != 0
    ptr, shape, keep = _image_u8(x, stream)
    return ptr, shape, 1, keep


def _image_shape(x):
    """shape of a host or device image without touching the device"""
    return tuple(int(s) for s in (x.shape if hasattr(x, "shape") else np.asarray(x).shape))


def _result(out, device, stream, as_bool=False, keep=()):
    if device:
        out._keep = keep          # inputs and workspaces of the queued launches live as long as their result
        return out
    a = out.numpy(stream)
    return a.astype(bool) if as_bool else a
