"""2-D image operations: morphology, Gaussian filters and resizing (csrc/avl_morph2d.hip), the exact distance transform, the decay
map of a mask and the product of 2-D maps (csrc/avl_edt2d.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _image_any, _image_shape, _image_u8, _result, _workspace
from .fields import GOAL_MAX_TERMS, _check_decay


# ---------------------------------------------------------------------------------------- 2-D image morphology (csrc/avl_morph2d.hip)
_MORPH_OPS = {"dilate": _lib.MORPH_DILATE, "erode": _lib.MORPH_ERODE}
_MORPH_STRUCTURES = {"cross": _lib.MORPH_CROSS, "box": _lib.MORPH_BOX}


def gaussian_weights(sigma, truncate=4.0):
    """(weights (2 * radius + 1,) float64, radius): scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius) with
    gaussian_filter1d's radius = int(truncate * sigma + 0.5), operation for operation"""
    sd = float(sigma)
    radius = int(float(truncate) * sd + 0.5)
    sigma2 = sd * sd
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum(), radius


def binary_morph(image, op, structure="cross", iterations=1, device=False, stream=None):
    """scipy.ndimage.binary_dilation / binary_erosion(image, structure, iterations) with border_value 0: op 'dilate' | 'erode',
    structure 'cross' (SciPy's default) | 'box' (np.ones((3, 3))).  -> (H, W) bool, or the uint8 DeviceArray (device=True)."""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H, W), keep = _image_u8(image, stream)
    out = DeviceArray((H, W), np.uint8)
    tmp = DeviceArray((H, W), np.uint8) if iterations > 4 else None
    _lib.check(lib.avl_morph_binary(ip, H, W, _MORPH_OPS[op], _MORPH_STRUCTURES[structure], int(iterations), out.ptr,
                                    tmp.ptr if tmp is not None else None, stream), "avl_morph_binary")
    return _result(out, device, stream, as_bool=True, keep=(keep, tmp))


def gaussian_filter2d(image, sigma, truncate=4.0, threshold=None, device=False, stream=None):
    """scipy.ndimage.gaussian_filter(image.astype(float), sigma, truncate=truncate) (mode 'reflect'), SciPy's bits: (H, W) float64.
    With `threshold` the mask `value > threshold` is returned as well: (values, mask)."""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H, W), is_u8, keep = _image_any(image, stream)
    w, radius = gaussian_weights(sigma, truncate)
    out = DeviceArray((H, W), np.float64)
    tmp = DeviceArray((H, W), np.float64)
    gt = DeviceArray((H, W), np.uint8) if threshold is not None else None
    _lib.check(lib.avl_gauss2d_f64(ip, is_u8, H, W, w.ctypes.data, radius, out.ptr, gt.ptr if gt is not None else None,
                                   float(threshold if threshold is not None else 0.0), tmp.ptr, stream), "avl_gauss2d_f64")
    vals = _result(out, device, stream, keep=(keep, tmp))
    if gt is None:
        return vals
    return vals, _result(gt, device, stream, as_bool=True, keep=(keep, tmp))


def resize2x_up(image, device=False, stream=None):
    """cv2.resize(image.astype(float), (2 * W, 2 * H)) with the default INTER_LINEAR: (2 * H, 2 * W) float64"""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H, W), is_u8, keep = _image_any(image, stream)
    out = DeviceArray((2 * H, 2 * W), np.float64)
    _lib.check(lib.avl_resize2x_up_f64(ip, is_u8, H, W, out.ptr, stream), "avl_resize2x_up_f64")
    return _result(out, device, stream, keep=(keep,))


def resize2x_down(image, device=False, stream=None):
    """cv2.resize(image.astype(float), (W // 2, H // 2)) of an image with even sides: the 2 x 2 block means, float64"""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H2, W2), is_u8, keep = _image_any(image, stream)
    if H2 % 2 or W2 % 2:
        raise ValueError(f"resize2x_down needs even sides, got {(H2, W2)}")
    out = DeviceArray((H2 // 2, W2 // 2), np.float64)
    _lib.check(lib.avl_resize2x_down_f64(ip, is_u8, H2 // 2, W2 // 2, out.ptr, stream), "avl_resize2x_down_f64")
    return _result(out, device, stream, keep=(keep,))


def dilate_map(binary_map, dilate_iter=0, gaussian_sigma=1.0, want_values=True, want_zero=True, device=False, stream=None):
    """Map._dilate_map (map.py:169-181) on the GPU -> (values (H, W) float64, zero (H, W) bool = values == 0); an output that is
    not wanted is None.  binary_map: bool / uint8 image, host or device."""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (H, W), keep = _image_u8(binary_map, stream)
    ws, n = _workspace(lib.avl_dilate_map_work_bytes, "avl_dilate_map_work_bytes", H, W)
    vals = DeviceArray((H, W), np.float64) if want_values else None
    zero = DeviceArray((H, W), np.uint8) if want_zero else None
    _lib.check(lib.avl_dilate_map(ip, H, W, int(dilate_iter), float(gaussian_sigma), vals.ptr if vals is not None else None,
                                  zero.ptr if zero is not None else None, ws.ptr, n, stream), "avl_dilate_map")
    return (None if vals is None else _result(vals, device, stream, keep=(keep, ws)),
            None if zero is None else _result(zero, device, stream, as_bool=True, keep=(keep, ws)))


def mask_foreground(mask_2d, r0=0, r1=None, c0=0, c1=None, device=False, stream=None):
    """The mask chain of VLMap.get_pos (vlmap.py:166-171) on the crop [r0:r1, c0:c1] of mask_2d: binary_closing(iterations=3),
    gaussian_filter(0.8, truncate=3), > 0.5, binary_dilation -> (r1 - r0, c1 - c0) bool, or the uint8 DeviceArray."""
    lib = _lib.load()
    _lib.require_gpu()
    ip, (Hf, Wf), keep = _image_u8(mask_2d, stream)
    r1 = Hf if r1 is None else int(r1)
    c1 = Wf if c1 is None else int(c1)
    r0, c0 = int(r0), int(c0)
    if not (0 <= r0 < r1 <= Hf and 0 <= c0 < c1 <= Wf):
        raise ValueError(f"crop [{r0}:{r1}, {c0}:{c1}] is not inside the {(Hf, Wf)} mask")
    H, W = r1 - r0, c1 - c0
    ws, n = _workspace(lib.avl_mask_foreground_work_bytes, "avl_mask_foreground_work_bytes", H, W)
    out = DeviceArray((H, W), np.uint8)
    _lib.check(lib.avl_mask_foreground(ip, Wf, r0, r1, c0, c1, out.ptr, ws.ptr, n, stream), "avl_mask_foreground")
    return _result(out, device, stream, as_bool=True, keep=(keep, ws))


# ---------------------------------------------------------------------------------------- 2-D distance transform (csrc/avl_edt2d.hip)
EDT_MAX_SIDE = 16384


def _edt_workspace(lib, H, W, what):
    """(workspace, its size, the `found` flag): avl_edt2d_work_bytes rejects a side above EDT_MAX_SIDE before any device work"""
    ws, n = _workspace(lib.avl_edt2d_work_bytes, what, int(H), int(W))
    return ws, n, DeviceArray((1,), np.int32)


def distance_transform_edt(image, device=False, stream=None):
    """scipy.ndimage.distance_transform_edt(image) for a 2-D image, SciPy's bits: per non-zero cell the float64 distance to the nearest
    zero cell, 0 on zero cells.  image: bool / uint8 / numeric host array (nonzero = true) or a uint8 DeviceArray.  -> (H, W)
    float64, or the DeviceArray (device=True; the check below then synchronises the stream all the same).
    An image without a zero cell raises ValueError (SciPy measures to an imaginary cell at (-1, 0) there); a side above
    EDT_MAX_SIDE raises AvlError before any device work.  return_indices is not supported."""
    lib = _lib.load()
    shape = _image_shape(image)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D image, got shape {shape}")
    H, W = shape
    ws, nws, found = _edt_workspace(lib, H, W, "avl_edt2d")
    if isinstance(image, np.ndarray) and image.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        image = image != 0
    ip, _, keep = _image_u8(image, stream)
    out = DeviceArray((H, W), np.float64)
    _lib.check(lib.avl_edt2d(ip, W, H, W, 0, out.ptr, found.ptr, ws.ptr, nws, stream), "avl_edt2d")
    if not int(found.numpy(stream)[0]):
        raise ValueError("distance_transform_edt: the image has no zero cell to measure to")
    return _result(out, device, stream, keep=(keep, ws))


def _smooth_mask_window(lib, mp, ld, H, W, sigma, stream):
    """gaussian_filter(mask.astype(np.float32), sigma) > 0.5 in float32 storage (habitat_lang_robot.py:231-232) of the (H, W) window
    at device pointer mp with rows of ld cells -> (the (H, W) uint8 mask, the float32 temporary it must outlive the launch with)"""
    w, radius = gaussian_weights(sigma)
    gt, tmp = DeviceArray((H, W), np.uint8), DeviceArray((H, W), np.float32)
    _lib.check(lib.avl_gauss2d_f32(mp, 1, ld, H, W, w.ctypes.data, radius, None, gt.ptr, 0.5, tmp.ptr, stream), "avl_gauss2d_f32")
    return gt, tmp


def mask_smooth_2d(mask, sigma=1, window=None, device=False, stream=None):
    """The mask step of mask_decay_2d(smooth_sigma=sigma) on its own: gaussian_filter(mask.astype(np.float32), sigma) > 0.5 of
    mask[r0:r1, c0:c1] (window, default the whole mask) -> (H, W) bool, or the uint8 DeviceArray."""
    lib = _lib.load()
    shape = _image_shape(mask)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D mask, got shape {shape}")
    r0, r1, c0, c1 = (0, shape[0], 0, shape[1]) if window is None else (int(v) for v in window)
    if not (0 <= r0 < r1 <= shape[0] and 0 <= c0 < c1 <= shape[1]):
        raise ValueError(f"window [{r0}:{r1}, {c0}:{c1}] is not inside the {shape} mask")
    _lib.require_gpu()
    if isinstance(mask, np.ndarray) and mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        mask = mask != 0
    mp, _, keep = _image_u8(mask, stream)
    gt, tmp = _smooth_mask_window(lib, mp + r0 * shape[1] + c0, shape[1], r1 - r0, c1 - c0, sigma, stream)
    return _result(gt, device, stream, as_bool=True, keep=(keep, tmp))


def mask_decay_2d(mask, decay_rate, cell_size=1.0, normalize=False, smooth_sigma=None, device=False, stream=None, window=None):
    """The decay map of a 2-D mask (nonzero = target), NumPy's float64 bits:
        d = distance_transform_edt(mask == 0);  t = 1 - (d / cell_size) * decay_rate;  t[t < 0] = 0
        normalize:  (t - t.min()) / (t.max() - t.min())
    cell_size=1, normalize=True is habitat_lang_robot.py:233-236; cell_size=cs, normalize=False is get_heatmap_from_mask_2d
    (visualize_utils.py:97-102).  smooth_sigma: first mask = gaussian_filter(mask.astype(np.float32), smooth_sigma) > 0.5 in float32
    storage (habitat_lang_robot.py:231-232).  window=(r0, r1, c0, c1): work on mask[r0:r1, c0:c1] without copying it.
    -> (H, W) float64 or the DeviceArray.  ValueError: a mask without a target (after the smoothing), or normalize on a constant map."""
    lib = _lib.load()
    shape = _image_shape(mask)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"expected a non-empty 2-D mask, got shape {shape}")
    r0, r1, c0, c1 = (0, shape[0], 0, shape[1]) if window is None else (int(v) for v in window)
    if not (0 <= r0 < r1 <= shape[0] and 0 <= c0 < c1 <= shape[1]):
        raise ValueError(f"window [{r0}:{r1}, {c0}:{c1}] is not inside the {shape} mask")
    H, W, ld = r1 - r0, c1 - c0, shape[1]
    decay = _check_decay(decay_rate)
    cs = float(cell_size)
    if not (np.isfinite(cs) and cs > 0.0):
        raise ValueError(f"cell_size must be finite and > 0, got {cell_size!r}")
    ws, nws, found = _edt_workspace(lib, H, W, "avl_mask_decay_2d")
    if isinstance(mask, np.ndarray) and mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        mask = mask != 0
    mp, _, keep = _image_u8(mask, stream)
    mp += r0 * ld + c0
    keep = [keep, ws]
    if smooth_sigma is not None:
        gt, tmp = _smooth_mask_window(lib, mp, ld, H, W, smooth_sigma, stream)
        keep += [gt, tmp]
        mp, ld = gt.ptr, W
    out, mm = DeviceArray((H, W), np.float64), DeviceArray((2,), np.float64)
    _lib.check(lib.avl_mask_decay_2d(mp, ld, H, W, cs, decay, int(bool(normalize)), out.ptr, mm.ptr, found.ptr, ws.ptr, nws, stream),
               "avl_mask_decay_2d")
    if not int(found.numpy(stream)[0]):
        raise ValueError("mask_decay_2d: the mask has no target cell" + (" after the smoothing" if smooth_sigma is not None else ""))
    if normalize:
        lo, hi = mm.numpy(stream)
        if not hi > lo:
            raise ValueError(f"mask_decay_2d: the 2-D map is constant ({lo}), its min-max normalisation is undefined")
    return _result(out, device, stream, keep=tuple(keep))


def gaussian_filter2d_f32(image, sigma, truncate=4.0, threshold=None, device=False, stream=None):
    """scipy.ndimage.gaussian_filter(image.astype(np.float32), sigma, truncate=truncate), SciPy's float32 bits: (H, W) float32 -- every
    line accumulated in double, the intermediate and the result rounded to float32.  image: bool / uint8 (nonzero = 1) or float32.
    With `threshold` the mask `value > threshold` is returned as well: (values, mask)."""
    lib = _lib.load()
    _lib.require_gpu()
    dt = np.dtype(image.dtype) if hasattr(image, "dtype") and not _is_torch(image) else None
    if dt is not None and dt == np.float32:
        ip, shape, keep = as_device(image, np.float32, stream)
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"expected a non-empty 2-D image, got shape {tuple(shape)}")
        (H, W), is_u8 = (int(shape[0]), int(shape[1])), 0
    else:
        if isinstance(image, np.ndarray) and image.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
            raise TypeError(f"gaussian_filter2d_f32 takes a bool, uint8 or float32 image, got {image.dtype}")
        ip, (H, W), keep = _image_u8(image, stream)
        is_u8 = 1
    w, radius = gaussian_weights(sigma, truncate)
    out, tmp = DeviceArray((H, W), np.float32), DeviceArray((H, W), np.float32)
    gt = DeviceArray((H, W), np.uint8) if threshold is not None else None
    _lib.check(lib.avl_gauss2d_f32(ip, is_u8, W, H, W, w.ctypes.data, radius, out.ptr, gt.ptr if gt is not None else None,
                                   float(threshold if threshold is not None else 0.0), tmp.ptr, stream), "avl_gauss2d_f32")
    vals = _result(out, device, stream, keep=(keep, tmp))
    if gt is None:
        return vals
    return vals, _result(gt, device, stream, as_bool=True, keep=(keep, tmp))


class _WindowTermC(C.Structure):
    """avl_window_term of include/avlmaps_hip.h"""
    _fields_ = [("d_data", C.c_void_p), ("ld", C.c_int64), ("is_f64", C.c_int32), ("reserved", C.c_int32)]


class Window:
    """The window [r0:r1, c0:c1] of a 2-D float32 / float64 image (host array or DeviceArray) as a term of product_argmax_2d: a
    device image is read in place."""

    def __init__(self, image, r0, r1, c0, c1):
        self.image, self.r0, self.r1, self.c0, self.c1 = image, int(r0), int(r1), int(c0), int(c1)
        shape = _image_shape(image)
        if len(shape) != 2 or not (0 <= self.r0 < self.r1 <= shape[0] and 0 <= self.c0 < self.c1 <= shape[1]):
            raise ValueError(f"window [{r0}:{r1}, {c0}:{c1}] is not inside an image of shape {shape}")
        self.shape = (self.r1 - self.r0, self.c1 - self.c0)


class ProductResult:
    """product_argmax_2d's result: heat (h, w) float64 DeviceArray or None, cell = (row, col) of the first maximum in raster order
    within the window, value = the product there"""
    __slots__ = ("heat", "cell", "value")

    def __init__(self, heat, cell, value):
        self.heat, self.cell, self.value = heat, cell, value


def product_argmax_2d(terms, want_heat=True, stream=None) -> ProductResult:
    """habitat_lang_robot.py:357-375 + 419-425: heat = ((t0 * t1) * t2) ... in float64 over 1 to 8 (h, w) maps, and np.argmax +
    np.unravel_index of it, in one pass.  terms: float32 / float64 2-D host arrays or DeviceArrays, or ops.Window views of them, all
    of one (h, w); anything else is converted to float64 first.  want_heat=False stores nothing of size h * w."""
    lib = _lib.load()
    terms = list(terms)
    if not 1 <= len(terms) <= GOAL_MAX_TERMS:
        raise ValueError(f"a product has 1 to {GOAL_MAX_TERMS} terms, got {len(terms)}")
    wins = []
    for t in terms:
        if not isinstance(t, Window):
            shape = _image_shape(t)
            if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
                raise ValueError(f"a term is a non-empty 2-D map, got shape {shape}")
            t = Window(t, 0, shape[0], 0, shape[1])
        wins.append(t)
    h, w = wins[0].shape
    if any(t.shape != (h, w) for t in wins):
        raise ValueError(f"the terms differ in shape: {[t.shape for t in wins]}")
    _lib.require_gpu()
    arr, keep = (_WindowTermC * len(wins))(), []
    for k, t in enumerate(wins):
        img = t.image
        if isinstance(img, (DeviceArray, DeviceView)):
            dt = img.dtype
        else:
            img = np.asarray(img)
            dt = img.dtype if img.dtype in (np.float32, np.float64) else np.dtype(np.float64)
        if dt not in (np.float32, np.float64):
            raise TypeError(f"a term is float32 or float64, got {dt}")
        ptr, shape, kp = as_device(img, dt, stream)
        keep.append(kp)
        ld = int(shape[1])
        arr[k] = _WindowTermC(ptr + (t.r0 * ld + t.c0) * dt.itemsize, ld, int(dt == np.float64), 0)
    heat = DeviceArray((h, w), np.float64) if want_heat else None
    idx, val = C.c_int64(), C.c_double()
    _lib.check(lib.avl_product_argmax_2d(arr, len(wins), h, w, heat.ptr if want_heat else None, C.byref(idx), C.byref(val), stream),
               "avl_product_argmax_2d")
    return ProductResult(heat, (int(idx.value) // w, int(idx.value) % w), float(val.value))
