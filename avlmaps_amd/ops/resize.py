"""Pillow's 8-bit image resize and CLIP's preprocess for batches of frames (csrc/avl_resize.hip): the coefficient tables and the
normalisation table are built here on the host, every pixel is touched on the GPU only."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _is_dev, _result, _workspace

RESIZE_MAX_SIDE = 16384         # 1 <= H, W and both sides of the resized image
RESIZE_MAX_BATCH = 65535
RESIZE_MAX_CHANNELS = 4
RESIZE_TILE_W = 64              # output columns per workgroup of the horizontal pass
RESIZE_LDS_COEFS = 4096         # such a tile's coefficients are staged in LDS up to this many (ksize <= 64), read from global memory beyond
RESIZE_LDS_SPAN = 4096          # the bytes of an input row such a tile reads are staged in LDS up to this many
RESIZE_PRECISION_BITS = 22      # Pillow's PRECISION_BITS: 32 - 8 - 2
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_RESIZE_SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0}
_RESIZE_KEPT = 16
_RESIZE_TABLES = {}             # (device, in_size, out_size, filter) -> (k, bounds) DeviceArrays, most recent last
_CLIP_TABLES = {}               # (device, mean, std, dtype) -> the (256, 3) table's DeviceArray, most recent last


def resize_limits():
    """(tile_w, lds_coefs, lds_span) as the library was compiled; RESIZE_TILE_W, RESIZE_LDS_COEFS and RESIZE_LDS_SPAN state them"""
    t, a, w = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().avl_resize_limits(C.byref(t), C.byref(a), C.byref(w)), "avl_resize_limits")
    return t.value, a.value, w.value


def _resize_filter(name, x):
    """Pillow's box_filter, bilinear_filter and bicubic_filter (a = -0.5) on a float64 array, operation for operation"""
    if name == "box":
        return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resize_coeffs(in_size, out_size, filter="bicubic"):
    """Host code: Pillow's precompute_coeffs and normalize_coeffs_8bpc for one axis -> (k int32 (out_size, ksize), bounds int32
    (out_size, 2)): output xx reads the bounds[xx, 1] inputs from bounds[xx, 0] on with the weights k[xx] / 2^22 (zero beyond).
    The window sums run in ascending order in float64, as Pillow's do."""
    in_size, out_size = int(in_size), int(out_size)
    if filter not in _RESIZE_SUPPORT:
        raise ValueError(f"filter={filter!r}: one of {sorted(_RESIZE_SUPPORT)} (lanczos and hamming are not built)")
    if not (1 <= in_size <= RESIZE_MAX_SIDE and 1 <= out_size <= RESIZE_MAX_SIDE):
        raise ValueError(f"resizing {in_size} to {out_size}: both must lie in 1 .. {RESIZE_MAX_SIDE}")
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = _RESIZE_SUPPORT[filter] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                 # C's (int): towards zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize)
    w = _resize_filter(filter, (x[None, :] + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where(x[None, :] < xmax[:, None], w, 0.0)
    ww = np.zeros(out_size)
    for i in range(ksize):                                                          # ascending, one add per tap (np.sum adds pairwise)
        ww = np.where(i < xmax, ww + w[:, i], ww)
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = np.where(w < 0, -0.5 + w * (1 << RESIZE_PRECISION_BITS), 0.5 + w * (1 << RESIZE_PRECISION_BITS)).astype(np.int64)
    k = np.where(x[None, :] < xmax[:, None], k, 0).astype(np.int32)
    return np.ascontiguousarray(k), np.ascontiguousarray(np.stack([xmin, xmax], axis=1).astype(np.int32))


def _resize_tables(in_size, out_size, filter, stream):
    """the tables of one axis on the device, kept per (device, sizes, filter); None when the axis keeps its size.  Raises when a
    row of coefficients could overflow the kernel's (and Pillow's) int32 accumulator."""
    if in_size == out_size:
        return None
    key = (_lib.current_device(), in_size, out_size, filter)
    t = _RESIZE_TABLES.pop(key, None)
    if t is None:
        k, b = resize_coeffs(in_size, out_size, filter)
        worst = int(np.abs(k.astype(np.int64)).sum(axis=1).max())
        if 255 * worst + (1 << (RESIZE_PRECISION_BITS - 1)) >= 1 << 31:
            raise ValueError(f"resizing {in_size} to {out_size} ({filter}): 255 * sum|k| = 255 * {worst} overflows the int32 accumulator")
        t = (DeviceArray.from_numpy(k, stream), DeviceArray.from_numpy(b, stream))
    _RESIZE_TABLES[key] = t
    while len(_RESIZE_TABLES) > _RESIZE_KEPT:
        del _RESIZE_TABLES[next(iter(_RESIZE_TABLES))]
    return t


def clip_preprocess_plan(h, w, n_px=224):
    """(oh, ow, top, left): torchvision's Resize(n_px) (the short side becomes n_px, the long one int(n_px * long / short)) and
    CenterCrop(n_px) (int(round((side - n_px) / 2.0)), Python's round: half to even) for an h x w image"""
    h, w, n_px = int(h), int(w), int(n_px)
    if min(h, w, n_px) < 1:
        raise ValueError(f"an image of {h} x {w} and n_px={n_px}: all must be at least 1")
    if h <= w:
        oh, ow = n_px, int(n_px * w / h)
    else:
        oh, ow = int(n_px * h / w), n_px
    return oh, ow, int(round((oh - n_px) / 2.0)), int(round((ow - n_px) / 2.0))


def clip_table(mean=CLIP_MEAN, std=CLIP_STD, dtype=np.float32):
    """Host code: (256, 3) table[v, c] = (float32(v) / float32(255) - float32(mean[c])) / float32(std[c]), torchvision's ToTensor
    and Normalize in float32; a float16 table is that one rounded to nearest even"""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError(f"dtype={dtype}: float32 or float16")
    m, s = np.asarray(mean, np.float32).reshape(-1), np.asarray(std, np.float32).reshape(-1)
    if m.shape != (3,) or s.shape != (3,) or not (s != 0).all():
        raise ValueError("mean and std are three numbers each, std non-zero")
    t = (np.arange(256, dtype=np.float32)[:, None] / np.float32(255) - m[None, :]) / s[None, :]
    return np.ascontiguousarray(t.astype(dtype))


def _clip_device_table(mean, std, dtype, stream):
    key = (_lib.current_device(), tuple(float(v) for v in mean), tuple(float(v) for v in std), np.dtype(dtype).str)
    t = _CLIP_TABLES.pop(key, None)
    if t is None:
        t = DeviceArray.from_numpy(clip_table(mean, std, dtype), stream)
    _CLIP_TABLES[key] = t
    while len(_CLIP_TABLES) > _RESIZE_KEPT:
        del _CLIP_TABLES[next(iter(_CLIP_TABLES))]
    return t


def _images_shape(images):
    """(B, H, W, C, ndim) of a uint8 image or batch, host or device, checked without any device work"""
    if isinstance(images, (DeviceArray, DeviceView)):
        shape, ok = tuple(images.shape), images.dtype == np.uint8
    elif _is_torch(images):
        shape, ok = tuple(int(s) for s in images.shape), str(images.dtype) == "torch.uint8"
    else:
        shape, ok = np.shape(images), np.asarray(images).dtype == np.uint8
    if not ok:
        raise TypeError("expected uint8 pixels")
    if len(shape) == 2:
        B, H, W, Cn = 1, shape[0], shape[1], 1
    elif len(shape) == 3:
        B, (H, W, Cn) = 1, shape
    elif len(shape) == 4:
        B, H, W, Cn = shape
    else:
        raise ValueError(f"expected (H, W), (H, W, C) or (B, H, W, C) images, got shape {shape}")
    if not (1 <= B <= RESIZE_MAX_BATCH and 1 <= H <= RESIZE_MAX_SIDE and 1 <= W <= RESIZE_MAX_SIDE and 1 <= Cn <= RESIZE_MAX_CHANNELS):
        raise ValueError(f"images of shape {shape}: 1 .. {RESIZE_MAX_BATCH} images, sides 1 .. {RESIZE_MAX_SIDE}, 1 .. {RESIZE_MAX_CHANNELS} channels")
    return int(B), int(H), int(W), int(Cn), len(shape)


def _images_dev(images, stream):
    """-> (device pointer, keepalive) of the contiguous uint8 pixels"""
    if _is_dev(images):
        ptr, _, keep = as_device(images, np.uint8, stream)
        return ptr, keep
    _lib.require_gpu()
    d = DeviceArray.from_numpy(np.ascontiguousarray(images, dtype=np.uint8), stream)
    return d.ptr, d


def _table_args(t):
    """(k pointer, bounds pointer, ksize) of a pass, nulls for a skipped one"""
    return (t[0].ptr, t[1].ptr, t[0].shape[1]) if t is not None else (None, None, 0)


def resize_u8(images, size, filter="bicubic", window=None, device=False, stream=None):
    """PIL.Image.resize((ow, oh), filter) with size = (oh, ow) and filter "box", "bilinear" or "bicubic", bit for bit, for every
    image of a batch: (H, W), (H, W, C) or (B, H, W, C) uint8 with C <= 4, host array, DeviceArray, DeviceView or torch tensor
    (every channel is resized on its own, as Pillow does in modes L and RGB; RGBA's premultiplication is not applied).  window =
    (top, left, h, w) computes that part of the resized image only.  The result has the input's number of axes; a host array, or
    (device=True) a DeviceArray."""
    B, H, W, Cn, nd = _images_shape(images)
    oh, ow = (int(s) for s in size)
    top, left, h, w = (int(v) for v in window) if window is not None else (0, 0, oh, ow)
    if not (1 <= oh <= RESIZE_MAX_SIDE and 1 <= ow <= RESIZE_MAX_SIDE):
        raise ValueError(f"size={tuple(size)}: both sides must lie in 1 .. {RESIZE_MAX_SIDE}")
    if top < 0 or left < 0 or h < 1 or w < 1 or top + h > oh or left + w > ow:
        raise ValueError(f"window={window} leaves the resized image of {oh} x {ow}")
    if filter not in _RESIZE_SUPPORT:
        raise ValueError(f"filter={filter!r}: one of {sorted(_RESIZE_SUPPORT)} (lanczos and hamming are not built)")
    lib = _lib.load()
    ws, nws = _workspace(lib.avl_resize_work_bytes, "avl_resize_work_bytes", B, H, Cn, w, int(oh != H))
    th, tv = _resize_tables(W, ow, filter, stream), _resize_tables(H, oh, filter, stream)
    ptr, keep = _images_dev(images, stream)
    out = DeviceArray({2: (h, w), 3: (h, w, Cn), 4: (B, h, w, Cn)}[nd], np.uint8)
    _lib.check(lib.avl_resize_u8(ptr, B, H, W, Cn, *_table_args(th), ow, *_table_args(tv), oh, top, left, h, w, out.ptr, ws.ptr, nws,
                                 stream), "avl_resize_u8")
    return _result(out, device, stream, keep=(keep, ws, th, tv))


def clip_preprocess(images, n_px=224, mean=CLIP_MEAN, std=CLIP_STD, dtype=np.float32, device=True, stream=None, as_torch=False):
    """OpenAI CLIP's preprocess (_transform(n_px): bicubic Resize of the short side to n_px as Pillow does it, CenterCrop, ToTensor,
    Normalize) of (H, W, 3) or (B, H, W, 3) uint8 frames of one size, host or device, in one call: (B, 3, n_px, n_px) float32 or
    float16, a DeviceArray (device=True), a host array, or (as_torch=True) a torch CUDA tensor the kernel wrote into, queued on
    torch's current stream unless `stream` says otherwise.  Only the pixels inside the crop are computed."""
    B, H, W, Cn, nd = _images_shape(images)
    if nd < 3 or Cn != 3:
        raise ValueError("expected (H, W, 3) or (B, H, W, 3) RGB frames")
    n_px = int(n_px)
    oh, ow, top, left = clip_preprocess_plan(H, W, n_px)
    if max(oh, ow) > RESIZE_MAX_SIDE:
        raise ValueError(f"frames of {H} x {W} resize to {oh} x {ow}: a side above {RESIZE_MAX_SIDE}")
    dtype = np.dtype(dtype)
    table_host = clip_table(mean, std, dtype)                 # rejects a bad mean, std or dtype before any device work
    lib = _lib.load()
    if as_torch and stream is None:
        from ..device import torch_stream_ptr
        stream = torch_stream_ptr()
    ws, nws = _workspace(lib.avl_resize_work_bytes, "avl_resize_work_bytes", B, H, 3, n_px, int(oh != H))
    th, tv = _resize_tables(W, ow, "bicubic", stream), _resize_tables(H, oh, "bicubic", stream)
    table = _clip_device_table(mean, std, dtype, stream)
    assert table.shape == table_host.shape
    ptr, keep = _images_dev(images, stream)
    if as_torch:
        import torch
        res = torch.empty((B, 3, n_px, n_px), dtype=torch.float16 if dtype == np.float16 else torch.float32,
                          device=torch.device("cuda", torch.cuda.current_device()))
        out_ptr = res.data_ptr()
    else:
        res = DeviceArray((B, 3, n_px, n_px), dtype)
        out_ptr = res.ptr
    _lib.check(lib.avl_clip_preprocess(ptr, B, H, W, *_table_args(th), ow, *_table_args(tv), oh, top, left, n_px, n_px, table.ptr,
                                       int(dtype == np.float16), out_ptr, ws.ptr, nws, stream), "avl_clip_preprocess")
    if as_torch:
        # the inputs and the workspace of the queued launches must outlive them: the tensor is handed out once they have run
        _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
        return res
    return _result(res, device, stream, keep=(keep, ws, th, tv, table))
