"""Sound-map audio: PCM decoding, silence segmentation and track packing (csrc/avl_audio.hip), resampling between any two rates
(csrc/avl_resample.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device, _is_torch
from ._args import _is_dev, _result, _workspace

AUDIO_MAX_SAMPLES = 2 ** 31 - 1
AUDIO_MAX_CHANNELS = 8


def _audio_f32(audio, stream):
    """a mono float32 recording, host or device -> (ptr, n, DeviceArray / view that keeps it alive)"""
    if _is_dev(audio):
        ptr, shape, keep = as_device(audio, np.float32, stream)
        if len(shape) != 1:
            raise ValueError(f"expected a mono recording of shape (n,), got {tuple(shape)}")
        return ptr, int(shape[0]), keep
    a = np.asarray(audio)
    if a.ndim != 1:
        raise ValueError(f"expected a mono recording of shape (n,), got {a.shape}")
    if a.dtype != np.float32:
        raise TypeError(f"expected float32 samples, got {a.dtype} (decode_pcm16 converts int16 PCM)")
    if not 1 <= a.shape[0] <= AUDIO_MAX_SAMPLES:
        raise ValueError(f"a recording of {a.shape[0]} samples is outside 1 .. 2^31 - 1")
    _lib.require_gpu()
    d = DeviceArray.from_numpy(a, stream)
    return d.ptr, int(a.shape[0]), d


def decode_pcm16(pcm, device=True, stream=None):
    """Interleaved int16 PCM, (n,) or (n, channels) with channels <= 8, host or int16 DeviceArray -> the mono float32 recording
    np.mean(pcm.astype(np.float32) / 32768, axis=1), the documented meaning of librosa.load(..., mono=True) for PCM16 input
    (never compared with librosa or libsndfile, which this project does not have).  A DeviceArray (n,) with device=True."""
    lib = _lib.load()
    if isinstance(pcm, (DeviceArray, DeviceView)):
        ptr, shape, keep = as_device(pcm, np.int16, stream)
    else:
        a = np.asarray(pcm)
        if a.dtype != np.int16:
            raise TypeError(f"expected int16 PCM, got {a.dtype}")
        shape, ptr, keep = a.shape, None, a
    if len(shape) not in (1, 2):
        raise ValueError(f"expected PCM of shape (n,) or (n, channels), got {tuple(shape)}")
    n, ch = int(shape[0]), int(shape[1]) if len(shape) == 2 else 1
    if not 1 <= n <= AUDIO_MAX_SAMPLES or not 1 <= ch <= AUDIO_MAX_CHANNELS:
        raise ValueError(f"{n} frames of {ch} channels: outside 1 .. 2^31 - 1 frames, 1 .. {AUDIO_MAX_CHANNELS} channels")
    _lib.require_gpu()
    if ptr is None:
        keep = DeviceArray.from_numpy(np.ascontiguousarray(keep), stream)
        ptr = keep.ptr
    out = DeviceArray((n,), np.float32)
    _lib.check(lib.avl_audio_decode_pcm16(ptr, n, ch, out.ptr, stream), "avl_audio_decode_pcm16")
    return _result(out, device, stream, keep=(keep,))


class AudioSegments:
    """segment_audio's result.  segments: (S, 2) int64 (l, r) per segment, host array (a DeviceArray with device=True;
    segments_host always holds the host copy); time_ranges: (S, 2) float64 = segments / float(sample_rate), librosa's samples_to_time;
    audio: the recording on the device, (n,) float32, alive as long as this object."""

    def __init__(self, segments_dev, segments_host, sample_rate, audio, n, device):
        self.segments_dev, self.segments_host = segments_dev, segments_host
        self.segments = segments_dev if device else segments_host
        self.sample_rate, self.audio, self.n = sample_rate, audio, n
        self.time_ranges = segments_host / float(sample_rate)

    def __len__(self):
        return len(self.segments_host)


def segment_audio(audio, sample_rate, silence_duration_s=1.0, silence_thres=0.0, device=False, stream=None) -> AudioSegments:
    """audio_utils.py:515-546 segment_audio_with_silence on a mono float32 recording (host array or DeviceArray): sample i is loud
    iff audio[i] > silence_thres; a loud sample starts a segment iff it is the first one or follows the previous loud sample by
    gap = int(silence_duration_s * sample_rate) samples or more; a segment is (l, r), the track upstream cuts audio[l:r].
    Departures: a recording without a loud sample returns zero segments (upstream: IndexError); gap must be at least 1 (upstream's
    loop then emits an extra leading (l, l)); a threshold that float32 cannot hold exactly raises ValueError, because the compare
    runs in float32."""
    lib = _lib.load()
    thr = float(silence_thres)
    if thr != thr or float(np.float32(thr)) != thr:
        raise ValueError(f"silence_thres={silence_thres!r} is not exactly representable in float32")
    gap = int(silence_duration_s * sample_rate)
    if gap < 1:
        raise ValueError(f"silence_duration_s * sample_rate = {silence_duration_s * sample_rate}: the gap must be at least one sample")
    ap, n, keep = _audio_f32(audio, stream)
    ws, nws = _workspace(lib.avl_audio_segment_work_bytes, "avl_audio_segment_work_bytes", n)
    cap = (n - 1) // gap + 1                      # two starts are at least gap samples apart
    cnt = DeviceArray((1,), np.int64)
    seg = DeviceArray((cap, 2), np.int64)
    _lib.check(lib.avl_audio_segment(ap, n, thr, gap, seg.ptr, cap, cnt.ptr, ws.ptr, nws, stream), "avl_audio_segment")
    S = int(cnt.numpy(stream)[0])
    if S > cap:
        raise _lib.AvlError(f"avl_audio_segment: {S} segments for a capacity of {cap}")
    host = seg.numpy(stream)[:S].copy() if S else np.zeros((0, 2), np.int64)
    dev = None
    if device:                                    # an exact-size copy: the capacity buffer goes back to the pool
        dev = DeviceArray((S, 2), np.int64)
        if S:
            _lib.check(lib.avl_memcpy_d2d(dev.ptr, seg.ptr, S * 16, stream), "avl_memcpy_d2d")
            _lib.check(lib.avl_stream_sync(stream), "avl_stream_sync")
    res = AudioSegments(dev, host, sample_rate, keep if isinstance(keep, (DeviceArray, DeviceView)) else DeviceView(ap, (n,), np.float32),
                        n, device)
    res._keep = keep
    return res


def _check_ranges(ranges, n):
    r = np.asarray(ranges)
    if r.size == 0:
        return np.zeros((0, 2), np.int64)
    if r.ndim != 2 or r.shape[1] != 2 or r.dtype.kind not in "iu":
        raise ValueError(f"expected (S, 2) integer (start, stop) ranges, got shape {r.shape} of {r.dtype}")
    r = np.ascontiguousarray(r, dtype=np.int64)
    if (r[:, 0] < 0).any() or (r[:, 0] > r[:, 1]).any() or (r[:, 1] > n).any():
        raise ValueError(f"ranges must satisfy 0 <= start <= stop <= {n}")
    return r


def pack_tracks(audio, ranges, length, scale=32768.0, device=False, stream=None):
    """(S, length) float32: row k is audio[start_k:stop_k] * scale cut or zero-padded to `length` samples.  With scale = 32768 and
    length = 5 * sample_rate this is audio_mapping_utils.py:85 followed by get_five_second_contexts_audio(track, [2.5], sr) for all
    segments at once (the same numbers as upstream's float64 buffers: the scale is a power of two).  ranges: (S, 2) host integers,
    0 <= start <= stop <= n, checked here."""
    lib = _lib.load()
    length, scale = int(length), float(scale)
    if not 1 <= length <= AUDIO_MAX_SAMPLES:
        raise ValueError(f"length={length} outside 1 .. 2^31 - 1")
    if float(np.float32(scale)) != scale:
        raise ValueError(f"scale={scale!r} is not exactly representable in float32")
    ap, n, keep = _audio_f32(audio, stream)
    r = _check_ranges(ranges, n)
    S = len(r)
    _lib.require_gpu()
    out = DeviceArray((S, length), np.float32)
    if S:
        rd = DeviceArray.from_numpy(r, stream)
        _lib.check(lib.avl_audio_pack(ap, n, rd.ptr, S, length, scale, out.ptr, stream), "avl_audio_pack")
        keep = (keep, rd)
    return _result(out, device, stream, keep=(keep,))


def context_ranges(n, times, sample_rate, seconds=5.0):
    """Host code: the (start, stop) slices audio_utils.py:569-583 get_five_second_contexts_audio takes of an n-sample recording,
    one per kept time, as (S, 2) int64 with 0 <= start <= stop <= n, ready for pack_tracks.  A time is skipped when
    t - seconds / 2 > (n - 1) / sample_rate; the bounds are (np.asarray([t - 2.5, t + 2.5]) * sr).astype(int) (librosa's
    time_to_samples); Python's slice rules then apply: a negative bound counts from the end, both are clipped to [0, n], and
    start >= stop is an empty slice (stop = start here)."""
    n, half = int(n), seconds / 2
    out = []
    for t in times:
        if t - half > (n - 1) / sample_rate:
            continue
        b = (np.asarray([t - half, t + half]) * sample_rate).astype(int)
        start, stop, _ = slice(int(b[0]), int(b[1])).indices(n)
        out.append((start, max(start, stop)))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


# ---------------------------------------------------------------------------------------- any rate, any PCM width (csrc/avl_resample.hip)
RESAMPLE_MAX_RATIO = 4096       # 1 <= up, down; every pair of the rates 8 000 .. 192 000 Hz needs at most 2 560 (11 025 <-> 192 000)
RESAMPLE_TILE = 1024            # outputs per tile of the kernel
RESAMPLE_LDS_TAPS = 9216        # the tap table is staged in LDS up to this many taps, read from global memory beyond
RESAMPLE_LDS_WINDOW = 8192      # a tile's input window is staged in LDS up to this many samples
_RESAMPLE_TAPS_KEPT = 8
_RESAMPLE_TAPS = {}             # (device, up, down) -> the taps' DeviceArray, most recent last


def resample_limits():
    """(tile, lds_taps, lds_window) as the library was compiled; RESAMPLE_TILE, RESAMPLE_LDS_TAPS and RESAMPLE_LDS_WINDOW state them"""
    t, a, w = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().avl_audio_resample_limits(C.byref(t), C.byref(a), C.byref(w)), "avl_audio_resample_limits")
    return t.value, a.value, w.value


def resample_ratio(sr_in, sr_out):
    """(up, down) = (sr_out, sr_in) / gcd; ValueError unless both rates are positive integers and 1 <= up, down <= 4096"""
    import math
    if int(sr_in) != sr_in or int(sr_out) != sr_out or sr_in < 1 or sr_out < 1:
        raise ValueError(f"sample rates must be positive integers, got {sr_in!r} and {sr_out!r}")
    sr_in, sr_out = int(sr_in), int(sr_out)
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    if max(up, down) > RESAMPLE_MAX_RATIO:
        raise ValueError(f"{sr_in} Hz -> {sr_out} Hz is the ratio {up} / {down}: both terms must be at most {RESAMPLE_MAX_RATIO}")
    return up, down


def resample_taps(up, down) -> np.ndarray:
    """Host code: the float64 taps of scipy.signal.resample_poly(x, up, down)'s default filter,
    firwin(2 * half + 1, 1 / M, window=("kaiser", 5.0)) * up with M = max(up, down) and half = 10 * M, from NumPy alone: the
    windowed sinc, normalised to unit gain at 0 Hz, times up.  Within 5.6e-16 of SciPy's for the ratios the tests list."""
    up, down = int(up), int(down)
    if not (1 <= up <= RESAMPLE_MAX_RATIO and 1 <= down <= RESAMPLE_MAX_RATIO):
        raise ValueError(f"ratio {up} / {down}: both terms must lie in 1 .. {RESAMPLE_MAX_RATIO}")
    M = max(up, down)
    half = 10 * M
    L = 2 * half + 1
    i = np.arange(L) - half
    t = np.sinc(i / M) / M * np.kaiser(L, 5.0)
    return t / t.sum() * up


def _device_taps(up, down, stream):
    key = (_lib.current_device(), up, down)
    d = _RESAMPLE_TAPS.pop(key, None)
    if d is None:
        d = DeviceArray.from_numpy(resample_taps(up, down), stream)
    _RESAMPLE_TAPS[key] = d
    while len(_RESAMPLE_TAPS) > _RESAMPLE_TAPS_KEPT:
        del _RESAMPLE_TAPS[next(iter(_RESAMPLE_TAPS))]
    return d


def _audio_len(audio):
    """the length of a mono float32 recording, host or device, checked without any device work"""
    if isinstance(audio, (DeviceArray, DeviceView)):
        shape, dt = audio.shape, audio.dtype
    elif _is_torch(audio):
        shape, dt = tuple(audio.shape), np.dtype(np.float32) if str(audio.dtype) == "torch.float32" else str(audio.dtype)
    else:
        a = np.asarray(audio)
        shape, dt = a.shape, a.dtype
    if len(shape) != 1:
        raise ValueError(f"expected a mono recording of shape (n,), got {tuple(shape)}")
    if dt != np.float32:
        raise TypeError(f"expected float32 samples, got {dt} (decode_pcm converts PCM)")
    if not 1 <= int(shape[0]) <= AUDIO_MAX_SAMPLES:
        raise ValueError(f"a recording of {shape[0]} samples is outside 1 .. 2^31 - 1")
    return int(shape[0])


def resample_audio(audio, sr_in, sr_out, device=False, stream=None):
    """scipy.signal.resample_poly(audio, up, down) with its default filter, a float64 accumulator and one rounding to float32, where
    up / down is sr_out / sr_in reduced: stands in for the resampling of librosa.load(path, sr=sr_out) (audio_mapping_utils.py:238),
    whose own filter (soxr_hq) this is NOT.  audio: a mono float32 host array, DeviceArray or DeviceView; the result has
    ceil(n * up / down) samples, a host array or (device=True) a DeviceArray.  sr_in == sr_out returns `audio` itself.  The taps
    (resample_taps) are kept on the device per (up, down)."""
    up, down = resample_ratio(sr_in, sr_out)
    n = _audio_len(audio)
    if up == down:
        return audio
    n_out = -(-n * up // down)
    if n_out > AUDIO_MAX_SAMPLES:
        raise ValueError(f"{n} samples at {up} / {down} are {n_out} samples, more than 2^31 - 1")
    lib = _lib.load()
    ap, n, keep = _audio_f32(audio, stream)
    taps = _device_taps(up, down, stream)
    out = DeviceArray((n_out,), np.float32)
    _lib.check(lib.avl_audio_resample(ap, n, up, down, taps.ptr, taps.shape[0], out.ptr, n_out, stream), "avl_audio_resample")
    return _result(out, device, stream, keep=(keep, taps))


def decode_pcm(data, width=None, channels=None, device=True, stream=None):
    """Interleaved PCM of any of the widths a WAV file has -> the mono float32 recording (a DeviceArray (n,) with device=True):
      int16  (n,) or (n, channels)   decode_pcm16, unchanged
      int32  (n,) or (n, channels)   32-bit PCM, or 24-bit left-justified in 32 bits (scipy.io.wavfile's convention): width 4
      uint8  with width=3            the raw little-endian 3-byte samples of a 24-bit file, any shape of n * channels * 3 bytes
                                     (channels defaults to 1, or to shape[1] of an (n, channels, 3) array)
    host arrays, DeviceArrays or DeviceViews.  Widths 3 and 4: float32((sum_c float64(s[i, c]) / 2^(8 width - 1)) / channels), the
    NumPy expression ((s.astype(np.float64) / 2.0 ** (8 * width - 1)).sum(axis=1) / channels).astype(np.float32)."""
    dev = isinstance(data, (DeviceArray, DeviceView))
    a = data if dev else np.asarray(data)
    dt, shape = np.dtype(a.dtype), tuple(a.shape)
    if dt == np.int16 and width in (None, 2):
        if channels not in (None, shape[1] if len(shape) == 2 else 1):
            raise ValueError(f"channels={channels} does not match PCM of shape {shape}")
        return decode_pcm16(data, device=device, stream=stream)
    if dt == np.int32 and width in (None, 4):
        width = 4
        if len(shape) not in (1, 2):
            raise ValueError(f"expected PCM of shape (n,) or (n, channels), got {shape}")
        n, ch = shape[0], shape[1] if len(shape) == 2 else 1
        if channels not in (None, ch):
            raise ValueError(f"channels={channels} does not match PCM of shape {shape}")
    elif dt == np.uint8 and width == 3:
        ch = int(channels) if channels is not None else (shape[1] if len(shape) == 3 and shape[2] == 3 else 1)
        size = int(np.prod(shape, dtype=np.int64))
        if ch < 1 or size % (3 * ch):
            raise ValueError(f"{size} bytes are not whole frames of {ch} channels of 3 bytes")
        n = size // (3 * ch)
    else:
        raise ValueError(f"{dt} samples with width={width}: int16, int32, or uint8 bytes with width=3 are decoded")
    if not 1 <= n <= AUDIO_MAX_SAMPLES or not 1 <= ch <= AUDIO_MAX_CHANNELS:
        raise ValueError(f"{n} frames of {ch} channels: outside 1 .. 2^31 - 1 frames, 1 .. {AUDIO_MAX_CHANNELS} channels")
    lib = _lib.load()
    _lib.require_gpu()
    keep = a if dev else DeviceArray.from_numpy(np.ascontiguousarray(a), stream)
    out = DeviceArray((n,), np.float32)
    _lib.check(lib.avl_audio_decode_pcm(keep.ptr, n, ch, width, out.ptr, stream), "avl_audio_decode_pcm")
    return _result(out, device, stream, keep=(keep,))
