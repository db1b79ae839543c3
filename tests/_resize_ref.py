"""NumPy twin of Pillow's 8-bit ImagingResample (box, bilinear, bicubic) and of OpenAI CLIP's _transform(n_px), written from their
definitions and independent of avlmaps_amd: coefficients, one pass, a resize with an output window, the crop plan, the
normalisation table and clip_preprocess_ref.  No GPU, no Pillow."""
import math

import numpy as np

PRECISION_BITS = 22
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}


def coeffs_ref(in_size, out_size, filter="bicubic"):
    """(k int32 (out_size, ksize), bounds int32 (out_size, 2)): precompute_coeffs + normalize_coeffs_8bpc, one output at a time"""
    f, s = FILTERS[filter]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = s * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        bounds[xx] = (xmin, xmax)
    return k, bounds


def pass_ref(img, k, bounds, axis, lo=0, hi=None):
    """one pass over `axis` (0 or 1) of an (H, W, C) uint8 image for the outputs lo .. hi - 1; int32 accumulator, arithmetic shift"""
    hi = len(k) if hi is None else hi
    img = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((hi - lo,) + img.shape[1:], np.uint8)
    for xx in range(lo, hi):
        xmin, xmax = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
        for x in range(xmax):
            acc = acc + img[xmin + x] * k[xx, x]
        out[xx - lo] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_ref(img, size, filter="bicubic", window=None):
    """PIL.Image.resize((ow, oh), filter) of an (H, W) or (H, W, C) uint8 image; window = (top, left, h, w) of the resized image"""
    a = np.asarray(img, np.uint8)
    squeeze = a.ndim == 2
    a = a[:, :, None] if squeeze else a
    H, W = a.shape[:2]
    oh, ow = size
    top, left, h, w = window if window is not None else (0, 0, oh, ow)
    assert 0 <= top and 0 <= left and h >= 1 and w >= 1 and top + h <= oh and left + w <= ow
    if ow != W:
        a = pass_ref(a, *coeffs_ref(W, ow, filter), axis=1, lo=left, hi=left + w)
    else:
        a = a[:, left:left + w]
    if oh != H:
        a = pass_ref(a, *coeffs_ref(H, oh, filter), axis=0, lo=top, hi=top + h)
    else:
        a = a[top:top + h]
    a = np.ascontiguousarray(a)
    return a[:, :, 0] if squeeze else a


def plan_ref(h, w, n_px=224):
    """(oh, ow, top, left) of CLIP's Resize(n_px) and CenterCrop(n_px) for an h x w image"""
    if h <= w:
        oh, ow = n_px, int(n_px * w / h)
    else:
        oh, ow = int(n_px * h / w), n_px
    return oh, ow, int(round((oh - n_px) / 2.0)), int(round((ow - n_px) / 2.0))


def table_ref(mean=CLIP_MEAN, std=CLIP_STD, dtype=np.float32):
    """(256, 3): ToTensor and Normalize of every byte value per channel, each operation a correctly rounded float32 one"""
    v = np.arange(256, dtype=np.float32)[:, None] / np.float32(255)
    t = (v - np.asarray(mean, np.float32)[None, :]) / np.asarray(std, np.float32)[None, :]
    assert t.dtype == np.float32
    return t.astype(dtype)


def clip_preprocess_ref(img, n_px=224, mean=CLIP_MEAN, std=CLIP_STD, dtype=np.float32):
    """(3, n_px, n_px): CLIP's preprocess of one (H, W, 3) uint8 image"""
    a = np.asarray(img, np.uint8)
    oh, ow, top, left = plan_ref(a.shape[0], a.shape[1], n_px)
    u8 = resize_ref(a, (oh, ow), "bicubic", (top, left, n_px, n_px))
    t = table_ref(mean, std, dtype)
    return np.ascontiguousarray(np.stack([t[u8[:, :, c], c] for c in range(3)]))


# ---------------------------------------------------------------------------------------- the cases the host and the GPU tests share
# H, W of a frame for CLIP's preprocess (short side to 224, bicubic): an upscale whose filterscale clamps to 1, its portrait, both
# passes skipped, the two pure crops with a half-way offset (left 0 and 2), a downscale
CLIP_CASES = ((37, 53), (53, 37), (224, 224), (224, 225), (224, 227), (100, 151), (1, 1))
WORKLOAD = (720, 1080)          # 13 taps per axis, used once
# (H, W, oh, ow, filters): two passes, horizontal only, vertical only, a tiny one, and about 260 taps (beyond any LDS budget)
RESIZE_CASES = ((64, 48, 17, 64, ("box", "bilinear", "bicubic")), (9, 200, 9, 31, ("bicubic",)), (200, 9, 31, 9, ("bicubic",)),
                (5, 7, 3, 2, ("bicubic",)), (9, 2000, 9, 31, ("bicubic",)))


def make_images(seed, shape):
    """a random uint8 image and one of 0 / 255 only: bicubic overshoots on the second and reaches both ends of the clamp"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8), (rng.integers(0, 2, shape) * 255).astype(np.uint8)


def inner_window(oh, ow):
    """a window of an oh x ow image that starts and ends inside a tile of 64 columns and 4 rows where the image is large enough"""
    top, left = min(1, oh - 1), min(3, ow - 1)
    return top, left, max(1, min(oh - top - 1, 9)), max(1, min(ow - left - 2, 70))
