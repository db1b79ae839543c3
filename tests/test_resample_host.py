"""Host side of loading a recording at any rate and PCM width: the filter design and the NumPy twin of the resampling kernel
against SciPy, the argument checks of ops and of the C entry points (which happen before any device work), and WAV reading.
No GPU."""
import ctypes as C
import sys
import wave
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _resample_ref as R  # noqa: E402


def write_pcm_wav(path, samples, rate, width):
    """samples: (n,) or (n, channels) integers in the range of `width` bytes, written with the standard wave module"""
    s = np.asarray(samples)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if s.ndim == 1 else s.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(R.pack24(s).tobytes() if width == 3 else s.astype({2: "<i2", 4: "<i4"}[width]).tobytes())


# ------------------------------------------------------------------ the filter and the sum against SciPy
@pytest.mark.parametrize("up,down", R.RATIOS)
def test_taps_equal_scipys_default_filter(up, down):
    """Bound 1e-12 absolute: at most 81 921 taps times |x| <= 1 then move an output by less than 1e-7 of a float32 ulp at 1.
    Observed: at most 5.6e-16 over these ratios."""
    from scipy.signal import firwin
    from avlmaps_amd import ops
    M = max(up, down)
    want = firwin(20 * M + 1, 1.0 / M, window=("kaiser", 5.0)) * up
    for h in (R.taps(up, down), ops.resample_taps(up, down)):
        assert h.dtype == np.float64 and h.shape == want.shape
        err = np.abs(h - want).max()
        print(f"taps {up}/{down}: max |twin - firwin * up| = {err:.3g}")
        assert err <= 1e-12
    assert np.array_equal(R.taps(up, down), ops.resample_taps(up, down))


@pytest.mark.parametrize("up,down", R.RATIOS)
def test_twin_equals_resample_poly(up, down):
    """At most 1 float32 ulp per element, derived and not measured: the twin and resample_poly add the same float64 terms (in
    another order at most), so they differ by far less than 1e-13 relative to the terms' magnitude, and two float64 values that
    close round to the same or to adjacent float32 values.  Observed: 0 unequal elements in every ratio."""
    from scipy.signal import resample_poly
    rng = np.random.default_rng(up * 10000 + down)
    x = rng.uniform(-1, 1, 5000).astype(np.float32)
    got = R.resample_ref(x, up, down)
    want = resample_poly(x.astype(np.float64), up, down).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape == (R.n_out(len(x), up, down),)
    u = R.ulps(got, want)
    print(f"twin {up}/{down}: {int((got != want).sum())} of {len(want)} elements unequal, max {u.max():.3g} ulp")
    assert u.max() <= 1.0
    # a sub-range of the outputs is the same numbers
    lo = len(want) // 3
    assert np.array_equal(R.resample_ref(x, up, down, m_lo=lo, m_hi=lo + 77), got[lo:lo + 77])


@pytest.mark.parametrize("n", [1, 3, 20, 21])
def test_twin_on_inputs_shorter_than_the_filter(n):
    from scipy.signal import resample_poly
    x = np.random.default_rng(n).uniform(-1, 1, n).astype(np.float32)
    for up, down in ((2, 1), (1, 2), (147, 160), (160, 441)):
        want = resample_poly(x.astype(np.float64), up, down).astype(np.float32)
        got = R.resample_ref(x, up, down)
        assert got.shape == want.shape and R.ulps(got, want).max() <= 1.0


def test_exported_limits_are_the_librarys():
    from avlmaps_amd import ops
    from avlmaps_amd.build import build
    build()
    assert ops.resample_limits() == (ops.RESAMPLE_TILE, ops.RESAMPLE_LDS_TAPS, ops.RESAMPLE_LDS_WINDOW) == (R.TILE, R.LDS_TAPS, R.LDS_WINDOW)
    # the ratios the GPU tests use to reach every variant of the kernel lie where they are meant to
    assert 20 * 160 + 1 <= R.LDS_TAPS < 20 * 640 + 1 and R.window_bound(147, 160) <= R.LDS_WINDOW < R.window_bound(1, 16)
    assert 20 * 16 + 1 <= R.LDS_TAPS and R.window_bound(2560, 147) <= R.LDS_WINDOW < R.window_bound(147, 2560)


# ------------------------------------------------------------------ argument checks without a GPU
def test_ops_check_their_arguments_before_any_device_work():
    from avlmaps_amd import ops
    a = np.zeros(100, np.float32)
    for sr_in, sr_out in ((4097, 1), (1, 4097), (8000, 44101), (44100, 0), (0, 44100), (44100.5, 48000)):
        with pytest.raises(ValueError):
            ops.resample_audio(a, sr_in, sr_out)
    assert ops.resample_ratio(11025, 192000) == (2560, 147) and ops.resample_ratio(48000, 44100) == (147, 160)
    assert ops.resample_ratio(4096, 1) == (1, 4096)
    with pytest.raises(ValueError):
        ops.resample_taps(4097, 1)
    with pytest.raises(TypeError, match="float32"):
        ops.resample_audio(a.astype(np.float64), 48000, 44100)
    with pytest.raises(ValueError, match="mono"):
        ops.resample_audio(a.reshape(10, 10), 48000, 44100)
    with pytest.raises(ValueError, match="samples"):
        ops.resample_audio(a[:0], 48000, 44100)
    assert ops.resample_audio(a, 44100, 44100) is a                        # the same rate: the input itself, no launch
    s = np.zeros((10, 2), np.int32)
    with pytest.raises(ValueError, match="width"):
        ops.decode_pcm(s, width=5)
    with pytest.raises(ValueError, match="channels"):
        ops.decode_pcm(np.zeros((10, 9), np.int32))
    with pytest.raises(ValueError, match="channels"):
        ops.decode_pcm(np.zeros(10 * 9 * 3, np.uint8), width=3, channels=9)
    with pytest.raises(ValueError):
        ops.decode_pcm(np.zeros((10, 9), np.int16))
    with pytest.raises(ValueError, match="frames"):
        ops.decode_pcm(np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="whole frames"):
        ops.decode_pcm(np.zeros(10, np.uint8), width=3, channels=2)
    with pytest.raises(ValueError):
        ops.decode_pcm(np.zeros(12, np.uint8))                             # bytes without a width
    with pytest.raises(ValueError):
        ops.decode_pcm(np.zeros(12, np.float32))
    with pytest.raises(ValueError, match="channels"):
        ops.decode_pcm(s, channels=3)


def test_entry_points_check_their_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    build()
    lib = _lib.load()
    fake = C.c_void_p(4096)                          # never dereferenced: every call below fails its checks first

    def err():
        return lib.avl_last_error()
    assert lib.avl_audio_resample(None, 10, 1, 2, fake, 41, fake, 5, None) != 0 and b"null" in err()
    assert lib.avl_audio_resample(fake, 10, 1, 2, None, 41, fake, 5, None) != 0 and b"null" in err()
    assert lib.avl_audio_resample(fake, 0, 1, 2, fake, 41, fake, 0, None) == 1 and b"outside" in err()
    assert lib.avl_audio_resample(fake, 2 ** 31, 1, 2, fake, 41, fake, 2 ** 30, None) == 1
    assert lib.avl_audio_resample(fake, 10, 4097, 1, fake, 81941, fake, 40970, None) == 1 and b"ratio" in err()
    assert lib.avl_audio_resample(fake, 10, 1, 4097, fake, 81941, fake, 1, None) == 1 and b"ratio" in err()
    assert lib.avl_audio_resample(fake, 10, 0, 1, fake, 41, fake, 1, None) == 1
    assert lib.avl_audio_resample(fake, 10, 1, 2, fake, 40, fake, 5, None) == 1 and b"odd" in err()
    assert lib.avl_audio_resample(fake, 10, 1, 2, fake, 0, fake, 5, None) == 1
    assert lib.avl_audio_resample(fake, 10, 1, 2, fake, 81923, fake, 5, None) == 1
    assert lib.avl_audio_resample(fake, 10, 1, 2, fake, 41, fake, 6, None) == 1 and b"ceil" in err()
    assert lib.avl_audio_resample(fake, 11, 1, 2, fake, 41, fake, 5, None) == 1 and b"ceil" in err()
    assert lib.avl_audio_resample(fake, 2 ** 31 - 1, 2, 1, fake, 41, fake, 2 ** 32 - 2, None) == 1 and b"n_out" in err()
    assert lib.avl_audio_resample(C.c_void_p(4098), 10, 1, 2, fake, 41, fake, 5, None) == 1 and b"aligned" in err()
    assert lib.avl_audio_resample(fake, 10, 1, 2, C.c_void_p(4100), 41, fake, 5, None) == 1 and b"aligned" in err()
    assert lib.avl_audio_decode_pcm(None, 10, 1, 3, fake, None) != 0 and b"null" in err()
    assert lib.avl_audio_decode_pcm(fake, 0, 1, 3, fake, None) == 1
    assert lib.avl_audio_decode_pcm(fake, 10, 9, 3, fake, None) == 1 and b"channels" in err()
    assert lib.avl_audio_decode_pcm(fake, 10, 0, 4, fake, None) == 1
    for width in (0, 1, 2, 5, 8):
        assert lib.avl_audio_decode_pcm(fake, 10, 1, width, fake, None) == 1 and b"width" in err()
    assert lib.avl_audio_decode_pcm(C.c_void_p(4097), 10, 1, 4, fake, None) == 1 and b"aligned" in err()
    assert lib.avl_audio_resample_limits(None, None, None) != 0 and b"null" in err()


# ------------------------------------------------------------------ WAV files
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("width", [3, 4])
def test_read_wav_round_trips_24_and_32_bit_pcm(tmp_path, width, channels):
    from avlmaps_amd.utils import audio_utils as U
    rng = np.random.default_rng(10 * width + channels)
    lim = 2 ** (8 * width - 1)
    s = rng.integers(-lim, lim, (301, channels)).astype(np.int32)
    s[:2] = [[-lim], [lim - 1]]
    s = s if channels > 1 else s[:, 0]
    write_pcm_wav(tmp_path / "a.wav", s, 48000, width)
    rate, data = U.read_wav(tmp_path / "a.wav")
    assert rate == 48000 and data.dtype == np.int32 and data.shape == s.shape
    assert np.array_equal(data, s * 256 if width == 3 else s)              # 24 bits: left-justified, SciPy's convention
    from scipy.io import wavfile
    rate2, data2 = wavfile.read(str(tmp_path / "a.wav"))
    assert rate2 == rate and np.array_equal(data2, data)
    if width == 3:
        _, raw = U.read_wav(tmp_path / "a.wav", raw24=True)
        assert raw.dtype == np.uint8 and raw.shape == (301, channels, 3) and np.array_equal(raw, R.pack24(s).reshape(301, channels, 3))
        assert np.array_equal(R.decode_ref(data, 4), R.decode_ref(s, 3))   # v * 2^8 / 2^31 == v / 2^23


def test_read_wav_keeps_its_other_answers(tmp_path):
    from scipy.io import wavfile
    from avlmaps_amd.utils import audio_utils as U
    rng = np.random.default_rng(4)
    mono = rng.integers(-32768, 32768, 200).astype(np.int16)
    write_pcm_wav(tmp_path / "m.wav", mono, 8000, 2)
    rate, data = U.read_wav(tmp_path / "m.wav")
    assert rate == 8000 and data.dtype == np.int16 and data.shape == (200,) and np.array_equal(data, mono)
    wavfile.write(tmp_path / "u8.wav", 8000, rng.integers(0, 256, 100).astype(np.uint8))
    wavfile.write(tmp_path / "f64.wav", 8000, rng.uniform(-1, 1, 100))
    for name in ("u8.wav", "f64.wav"):
        with pytest.raises(ValueError, match="only"):
            U.read_wav(tmp_path / name)


def test_load_wav_without_resample_still_raises(tmp_path):
    from avlmaps_amd.utils import audio_utils as U
    s = np.random.default_rng(2).integers(-2 ** 23, 2 ** 23, 100)
    write_pcm_wav(tmp_path / "a.wav", s, 48000, 3)
    for kw in ({}, {"resample": False}, {"device": True}):
        with pytest.raises(ValueError, match="resampl.*resample=True"):
            U.load_wav(tmp_path / "a.wav", 44100, **kw)
    write_pcm_wav(tmp_path / "empty.wav", s[:0], 48000, 3)
    with pytest.raises(ValueError, match="no samples"):
        U.load_wav(tmp_path / "empty.wav", 44100, resample=True)
