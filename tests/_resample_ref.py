"""NumPy restatements of csrc/avl_resample.hip, used by the resampling tests and tools/probe_resample.py.

resample_ref is the kernel's sum, operation for operation: for output m the terms h[m * down + half - k * up] * float64(x[k]) over
every 0 <= k < n whose tap index lies in [0, len(h)), added in ascending k, the product and the sum separate float64 operations,
one rounding to float32.  That is scipy.signal.resample_poly(x, up, down) (upfirdn with zero padding) with a float64 accumulator;
test_resample_host.py ties the two together."""
import numpy as np

from avlmaps_amd import ops

TILE = ops.RESAMPLE_TILE                  # outputs per tile of the kernel
LDS_TAPS = ops.RESAMPLE_LDS_TAPS          # taps beyond this count are read from global memory
LDS_WINDOW = ops.RESAMPLE_LDS_WINDOW      # a tile whose inputs exceed this count reads them from global memory

# (up, down) of 44 100 <-> 48 000, 44 100 -> 16 000, 11 025 <-> 48 000, 22 050 -> 44 100 and 44 100 -> 32 000
RATIOS = ((147, 160), (160, 147), (160, 441), (640, 147), (147, 640), (2, 1), (441, 320))


def taps(up, down):
    """scipy.signal.resample_poly's default filter from NumPy alone (the product's own design is ops.resample_taps: the same
    expression, restated here so that a test of the product does not check it against itself)"""
    M = max(up, down)
    half = 10 * M
    i = np.arange(2 * half + 1) - half
    t = np.sinc(i / M) / M * np.kaiser(2 * half + 1, 5.0)
    return t / t.sum() * up


def n_out(n, up, down):
    return -(-n * up // down)


def window_bound(up, down):
    """the most input samples one tile of the kernel reads"""
    return ((TILE - 1) * down + 20 * max(up, down)) // up + 1


def resample_ref(x, up, down, m_lo=0, m_hi=None, h=None):
    """outputs m_lo <= m < m_hi (all of them by default) of the resampled recording, float32; vectorised over the outputs, a loop
    over the term index"""
    x = np.asarray(x, dtype=np.float32)
    h = taps(up, down) if h is None else np.asarray(h, dtype=np.float64)
    n, half = len(x), (len(h) - 1) // 2
    m_hi = n_out(n, up, down) if m_hi is None else m_hi
    m = np.arange(m_lo, m_hi, dtype=np.int64)
    a = m * down + half
    q, p = a // up, a % up
    room = len(h) - 1 - p
    k_lo = np.where(room < 0, q + 1, np.maximum(q - room // up, 0))
    k_hi = np.minimum(q, n - 1)
    acc = np.zeros(len(m), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(int(max((k_hi - k_lo).max() + 1, 0)) if len(m) else 0):
            k = k_lo + i
            ok = k <= k_hi
            kk = np.where(ok, k, 0)
            t = np.where(ok, a - kk * up, 0)
            acc = np.where(ok, acc + h[t] * x[kk].astype(np.float64), acc)
        return acc.astype(np.float32)


def decode_ref(s, width):
    """(n, channels) integer samples of `width` bytes (width 4 also: 24-bit left-justified) -> mono float32"""
    s = np.asarray(s)
    s = s.reshape(len(s), -1)
    return ((s.astype(np.float64) / 2.0 ** (8 * width - 1)).sum(axis=1) / s.shape[1]).astype(np.float32)


def pack24(v):
    """int32 values in [-2^23, 2^23) of any shape -> their packed little-endian 3-byte samples, shape + (3,) uint8"""
    v = np.ascontiguousarray(v, dtype="<i4")
    return v.view(np.uint8).reshape(v.shape + (4,))[..., :3].copy()


def ulps(got, want):
    """|got - want| in units of float32 spacing at want (NaN where either is not finite)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    with np.errstate(invalid="ignore"):
        return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
