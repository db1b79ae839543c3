"""Loading a recording at any rate and PCM width on the GPU (csrc/avl_resample.hip through ops.resample_audio and ops.decode_pcm,
utils/audio_utils.load_wav(resample=True), and the sound map on top of them).

Oracle: the NumPy twins of _resample_ref.py, which add the kernel's terms in the kernel's order, so every comparison with them is
np.array_equal; test_resample_host.py ties the twins to scipy.signal.resample_poly, and one test here compares with SciPy itself
(at most 1 float32 ulp, see there).  Shapes are the smallest at which the kernel can go wrong: around one tile of T outputs, inputs
shorter than the filter, both sources of the taps and of the input window, more tiles than the grid has workgroups, and one
recording long enough for m * down and k * up to pass 2^31."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import _resample_ref as R  # noqa: E402
import _sound_ref as S  # noqa: E402
from test_resample_host import write_pcm_wav  # noqa: E402
from test_sound_host import SEQS, write_wav  # noqa: E402

T = R.TILE
EDGE_RATIOS = ((2, 1), (1, 2), (147, 160), (160, 147), (160, 441))


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


def n_for(target, up, down):
    """the shortest input with at least `target` outputs"""
    n = max(1, (target - 1) * down // up)
    while R.n_out(n, up, down) < target:
        n += 1
    return n


def check(ops, x, up, down):
    """resample at the rates (down, up) Hz and compare with the twin, bit for bit"""
    x = np.asarray(x, np.float32)
    got = ops.resample_audio(x, down, up)
    want = R.resample_ref(x, up, down)
    assert got.dtype == np.float32 and got.shape == want.shape == (R.n_out(len(x), up, down),)
    assert np.array_equal(got, want, equal_nan=True), (up, down, len(x), np.flatnonzero(got != want)[:5])
    return got


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("target", [1, T - 1, T, T + 1, 3 * T + 5])
@pytest.mark.parametrize("up,down", EDGE_RATIOS)
def test_output_counts_around_a_tile(ops, up, down, target):
    n = n_for(target, up, down)
    assert target <= R.n_out(n, up, down) < target + max(1, -(-up // down))
    check(ops, np.random.default_rng(target + up).uniform(-1, 1, n), up, down)


@pytest.mark.parametrize("up,down", EDGE_RATIOS)
def test_inputs_shorter_than_the_filter_and_impulses_at_both_ends(ops, up, down):
    rng = np.random.default_rng(down)
    for n in (1, 3):
        check(ops, rng.uniform(-1, 1, n), up, down)
    n = n_for(2 * T + 77, up, down)
    for at in (0, n - 1):                                   # the truncated taps of either end
        x = np.zeros(n, np.float32)
        x[at] = 1.0
        got = check(ops, x, up, down)
        assert np.count_nonzero(got) >= 5


@pytest.mark.parametrize("up,down", EDGE_RATIOS)
def test_nan_and_inf_propagate_like_numpys(ops, up, down):
    rng = np.random.default_rng(up)
    x = rng.uniform(-1, 1, n_for(T + 300, up, down)).astype(np.float32)
    x[[0, 7, len(x) // 2, len(x) - 1]] = [np.inf, -np.inf, np.nan, np.inf]
    x[len(x) // 3: len(x) // 3 + 2] = [np.inf, -np.inf]     # inf - inf inside one sum
    got = check(ops, x, up, down)
    assert np.isnan(got).any() and np.isfinite(got).any()


# ------------------------------------------------------------------ both sources of the taps and of the window
@pytest.mark.parametrize("up,down,n,taps_lds,win_lds", [
    (147, 160, 2500, True, True),             # 48 000 -> 44 100: everything in LDS
    (160, 441, 7000, True, True),             # 44 100 -> 16 000: 8 821 taps, the largest usual table under the budget
    (459, 460, 2500, True, True),             # 9 201 taps: the last table that fits
    (460, 461, 2500, False, True),            # 9 221 taps: the first that does not
    (147, 640, 11000, False, True),           # 48 000 -> 11 025: 12 801 taps
    (2560, 147, 300, False, True),            # 11 025 -> 192 000: 51 201 taps, more than any LDS
    (147, 2560, 60000, False, False),         # 192 000 -> 11 025: the window of a tile exceeds its budget too
    (1, 16, 16 * (2 * T + 9), True, False),   # a small table and a window beyond the budget
])
def test_every_variant_of_the_kernel(ops, up, down, n, taps_lds, win_lds):
    assert (20 * max(up, down) + 1 <= R.LDS_TAPS) == taps_lds and (R.window_bound(up, down) <= R.LDS_WINDOW) == win_lds
    check(ops, np.random.default_rng(n).uniform(-1, 1, n), up, down)


def test_more_tiles_than_workgroups_with_the_taps_in_lds(ops):
    """2 051 tiles for a grid of at most 2 048 workgroups: the first three workgroups take a second tile and stage a second
    window.  Compared: their first tiles, their second tiles and the tiles before those (the twin of all 2.1 M outputs takes
    seconds)."""
    n_out = 2051 * T - 3
    x = np.random.default_rng(9).uniform(-1, 1, 2 * n_out).astype(np.float32)
    got = ops.resample_audio(x, 2, 1)
    assert got.shape == (n_out,)
    for lo, hi in ((0, 4 * T), (2045 * T, n_out)):
        assert np.array_equal(got[lo:hi], R.resample_ref(x, 1, 2, m_lo=lo, m_hi=hi))
    assert np.abs(got).max() < 1.5 and np.count_nonzero(got) > n_out - 100


def test_products_past_2_to_the_31(ops):
    """48 000 -> 11 025 on 14 700 000 samples (59 MB): m * down and k * up pass 2^31; 3 299 tiles of global-memory taps"""
    from avlmaps_amd.device import DeviceArray
    up, down, n = 147, 640, 14_700_000
    n_out = R.n_out(n, up, down)
    assert (n_out - 1) * down > 2 ** 31 and (n - 1) * up > 2 ** 31
    x = np.zeros(n, np.float32)
    x[-100_000:] = np.random.default_rng(31).uniform(-1, 1, 100_000)
    d = DeviceArray.from_numpy(x)
    out = ops.resample_audio(d, 48000, 11025, device=True)
    assert out.shape == (n_out,)
    got = out.numpy()
    assert np.array_equal(got[-4096:], R.resample_ref(x, up, down, m_lo=n_out - 4096))
    first = ((n - 100_000) * up - 10 * down) // down         # outputs before this one see only zeros
    assert not got[:first].any() and got[first:first + 64].any()


def test_tables_shorter_than_the_ratio_through_the_c_abi(ops):
    """the taps are data of the C entry point: a table with fewer taps than phases leaves some outputs without any term (they are
    +0), and one with an arbitrary odd length and values is the same sum"""
    from avlmaps_amd import _lib
    from avlmaps_amd.device import DeviceArray
    lib = _lib.load()
    rng = np.random.default_rng(12)
    n = 2 * T + 50
    x = rng.uniform(-1, 1, n).astype(np.float32)
    d = DeviceArray.from_numpy(x)
    for up, down, n_taps in ((4, 3, 3), (2, 1, 1), (7, 2, 5), (3, 5, 1), (5, 3, 21), (1, 1, 9)):
        h = rng.uniform(-1, 1, n_taps)
        n_out = R.n_out(n, up, down)
        dh, out = DeviceArray.from_numpy(h), DeviceArray((n_out,), np.float32)
        _lib.check(lib.avl_audio_resample(d.ptr, n, up, down, dh.ptr, n_taps, out.ptr, n_out, None), "avl_audio_resample")
        want = R.resample_ref(x, up, down, h=h)
        assert np.array_equal(out.numpy(), want), (up, down, n_taps)
        if n_taps < up:
            assert (want == 0).sum() >= n_out // up


# ------------------------------------------------------------------ pointers and residency
def test_views_device_results_and_streams(ops):
    from avlmaps_amd import _lib
    from avlmaps_amd.device import DeviceArray, DeviceView
    lib = _lib.load()
    x = np.random.default_rng(5).uniform(-1, 1, 3 * T + 11).astype(np.float32)
    d = DeviceArray.from_numpy(x)
    for off in (1, 3):                                       # 4-byte but not 16-byte aligned
        got = ops.resample_audio(DeviceView(d.ptr + 4 * off, (len(x) - off,), np.float32), 48000, 44100)
        assert np.array_equal(got, R.resample_ref(x[off:], 147, 160))
    # device in, device out, and on again without a host copy in between
    a = ops.resample_audio(d, 22050, 44100, device=True)
    b = ops.resample_audio(a, 44100, 16000, device=True)
    assert isinstance(a, DeviceArray) and isinstance(b, DeviceArray) and a.dtype == b.dtype == np.float32
    want_a = R.resample_ref(x, 2, 1)
    assert np.array_equal(a.numpy(), want_a) and np.array_equal(b.numpy(), R.resample_ref(want_a, 160, 441))
    assert ops.resample_audio(d, 44100, 44100, device=True) is d
    # a stream of the caller's
    st = C.c_void_p()
    _lib.check(lib.avl_stream_create(C.byref(st)), "avl_stream_create")
    try:
        for up, down in ((147, 160), (147, 640)):
            got = ops.resample_audio(x, down, up, stream=st)
            assert np.array_equal(got, R.resample_ref(x, up, down))
        dev = ops.resample_audio(d, 2, 1, device=True, stream=st)
        _lib.check(lib.avl_stream_sync(st), "avl_stream_sync")
        assert np.array_equal(dev.numpy(), R.resample_ref(x, 1, 2))
        pcm = np.random.default_rng(6).integers(-2 ** 23, 2 ** 23, (T + 1, 2)).astype(np.int32)
        assert np.array_equal(ops.decode_pcm(R.pack24(pcm), width=3, device=False, stream=st), R.decode_ref(pcm, 3))
    finally:
        _lib.check(lib.avl_stream_destroy(st), "avl_stream_destroy")


# ------------------------------------------------------------------ against SciPy itself
@pytest.mark.parametrize("up,down", R.RATIOS)
def test_against_resample_poly(ops, up, down):
    """at most 1 float32 ulp: the kernel and resample_poly add the same float64 terms, each to within a few float64 ulps of the
    exact sum, and two float64 values that close round to the same float32 value or to adjacent ones.  Observed on an MI355X:
    0 elements differ in every ratio here; 1 of 225 M in the long recordings of tools/probe_resample.py, by 1 ulp."""
    from scipy.signal import resample_poly
    x = np.random.default_rng(up + down).uniform(-1, 1, 5000).astype(np.float32)
    got = ops.resample_audio(x, down, up)
    want = resample_poly(x.astype(np.float64), up, down).astype(np.float32)
    u = R.ulps(got, want)
    print(f"{up}/{down}: {int((got != want).sum())} of {len(want)} elements differ from resample_poly, max {u.max():.3g} ulp")
    assert got.shape == want.shape and u.max() <= 1.0


# ------------------------------------------------------------------ decode
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("width", [3, 4])
def test_decode_pcm(ops, width, channels):
    from avlmaps_amd.device import DeviceArray, DeviceView
    lim = 2 ** (8 * width - 1)
    rng = np.random.default_rng(10 * width + channels)
    for n in (1, 255, 256, 257, 70001):
        s = rng.integers(-lim, lim, (n, channels)).astype(np.int32)
        ext = np.array([lim - 1, -lim, -(lim - 1), 0, 1, -1], np.int64)
        s[:6] = ext[:len(s[:6]), None]                                       # every channel at an extreme
        if n > 8:
            s[6] = np.resize([lim - 1, -lim], channels)
            s[7] = np.resize([-lim, -lim, lim - 1], channels)
        want = R.decode_ref(s, width)
        if width == 4:
            got = ops.decode_pcm(s if channels > 1 else s[:, 0], device=False)
        else:
            raw = R.pack24(s)
            got = ops.decode_pcm(raw, width=3, device=False)                 # (n, channels, 3): the channels are read off the shape
            assert np.array_equal(ops.decode_pcm(raw.reshape(-1), width=3, channels=channels, device=False), want)
            left = ops.decode_pcm(s * 256 if channels > 1 else s[:, 0] * 256, device=False)      # left-justified in 32 bits
            assert np.array_equal(left, want)
        assert got.dtype == np.float32 and got.shape == (n,)
        assert np.array_equal(got, want)
    if channels == 1:
        assert got[0] == np.float32((lim - 1) / lim) and got[1] == -1.0
    if width == 3:                                                            # packed frames at an odd address
        buf = DeviceArray.from_numpy(np.concatenate([np.zeros(1, np.uint8), raw.reshape(-1)]))
        dev = ops.decode_pcm(DeviceView(buf.ptr + 1, raw.shape, np.uint8), width=3, device=True)
        assert isinstance(dev, DeviceArray) and np.array_equal(dev.numpy(), want)


# ------------------------------------------------------------------ end to end
def test_load_wav_decodes_24_bit_stereo_and_resamples(ops, tmp_path):
    from avlmaps_amd.device import DeviceArray
    from avlmaps_amd.utils import audio_utils as U
    rng = np.random.default_rng(48)
    s = rng.integers(-2 ** 23, 2 ** 23, (2 * T + 123, 2)).astype(np.int32)
    write_pcm_wav(tmp_path / "field.wav", s, 48000, 3)
    want = R.resample_ref(R.decode_ref(s, 3), 147, 160)
    got = U.load_wav(tmp_path / "field.wav", 44100, resample=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want)
    dev = U.load_wav(tmp_path / "field.wav", 44100, device=True, resample=True)
    assert isinstance(dev, DeviceArray) and np.array_equal(dev.numpy(), want)
    assert np.array_equal(U.load_wav(tmp_path / "field.wav", 48000), R.decode_ref(s, 3))           # its own rate: decoded only
    # 32-bit PCM, 16-bit PCM and float32 files at another rate
    write_pcm_wav(tmp_path / "i32.wav", s * 256, 48000, 4)
    assert np.array_equal(U.load_wav(tmp_path / "i32.wav", 44100, resample=True), want)
    p16 = rng.integers(-32768, 32768, 3000).astype(np.int16)
    write_wav(tmp_path / "i16.wav", p16, 22050)
    assert np.array_equal(U.load_wav(tmp_path / "i16.wav", 44100, resample=True), R.resample_ref(S.decode_ref(p16), 2, 1))
    from scipy.io import wavfile
    f = rng.uniform(-1, 1, 3000).astype(np.float32)
    wavfile.write(tmp_path / "f32.wav", 44100, f)
    assert np.array_equal(U.load_wav(tmp_path / "f32.wav", 16000, resample=True), R.resample_ref(f, 160, 441))
    # segment_audio_with_silence on a path at another rate
    tr, tracks = U.segment_audio_with_silence(tmp_path / "i16.wav", 0.01, 0, 44100)
    audio = R.resample_ref(S.decode_ref(p16), 2, 1)
    segs = S.segment_closed_form(audio, 0.0, 441)
    assert len(segs) >= 1 and np.array_equal(np.asarray(tr), segs / 44100.0)
    assert all(np.array_equal(t, audio[l:r]) for t, (l, r) in zip(tracks, segs))


FILE_RATE, MAP_RATE = 22050, 44100
SILENCE_S = 400.5 / MAP_RATE            # a gap of 400 samples at the map's rate: the fixture's 200 at the rate of its files
MAP_FPS = MAP_RATE / 16.0               # the fixture's eight samples per video frame, after the doubling


@pytest.fixture(scope="module")
def g(golden):
    return golden("g13_sound_map.npz")


@pytest.fixture(scope="module")
def built(tmp_path_factory, g, ops):
    """the fixture's recordings written as 22 050 Hz files, and a sound map configured for 44 100 Hz built from them"""
    from avlmaps_amd.apps.common import DEFAULTS, HashAudioEncoder, HashAudioText, to_cfg
    from avlmaps_amd.map.sound_map import SoundMap
    root = tmp_path_factory.mktemp("sound_rates")
    level = str(g["level"])
    for seq in SEQS:
        d = root / "audio_video" / seq
        d.mkdir(parents=True)
        write_wav(d / f"output_with_audio_{level}.wav", g[f"{seq}_pcm"], FILE_RATE)
        np.savetxt(d / "poses.txt", g[f"{seq}_poses"])
        (d / f"range_and_audio_meta_{level}.txt").write_text(f"0,10,dog,{seq}.wav\n")
    params = dict(DEFAULTS["sound_data_collect_params"], sample_rate=MAP_RATE, fps=MAP_FPS, silence_duration_s=SILENCE_S,
                  silence_threshold=int(g["silence_thres"]), difficulty=level)
    sm = SoundMap(str(root), to_cfg(DEFAULTS["sound_config"]), to_cfg(params), audio_text_model=HashAudioText(),
                  audio_encoder=HashAudioEncoder())
    sm.create_sound_map(str(root))
    return root, sm


def test_create_sound_map_resamples_its_recordings(built, g):
    from avlmaps_amd.apps.common import HashAudioEncoder
    from avlmaps_amd.utils.audio_mapping_utils import create_audio_map_batch
    root, sm = built
    db = sm.load_sound_map(str(root))
    enc, gap = HashAudioEncoder(), int(SILENCE_S * MAP_RATE)
    assert gap == 400
    details = {}
    create_audio_map_batch(str(root), enc, sample_rate=MAP_RATE, silence_duration_s=SILENCE_S, silence_thres=0, fps=MAP_FPS,
                           difficulty_level=str(g["level"]), details=details)
    assert sorted(details) == list(SEQS)
    i = 0
    for seq in SEQS:
        audio = R.resample_ref(S.decode_ref(g[f"{seq}_pcm"]), 2, 1)
        segs = S.segment_closed_form(audio, 0.0, gap)
        assert len(segs) >= 3 and np.array_equal(details[seq]["segments"], segs)
        assert np.array_equal(details[seq]["time_ranges"], segs / float(MAP_RATE))
        packed = S.pack_ref(audio, segs, 5 * MAP_RATE, 32768.0)
        feats = enc(packed)
        for k in range(len(segs)):
            assert db[i]["audio_features"].shape == (enc.D,) and np.array_equal(db[i]["audio_features"], feats[k])
            i += 1
    assert sorted(db) == list(range(i))


def test_get_pos_with_audio_accepts_a_clip_at_another_rate(built, ops, tmp_path):
    from avlmaps_amd.apps.common import HashAudioEncoder
    root, sm = built
    sm.load_sound_map(str(root))
    feats, locs = sm.get_all_audio_features_and_locations()
    # a 16 kHz clip: the database holds no equal track, so the answer is the nearest feature of the twin-resampled clip
    clip = np.random.default_rng(16).integers(-20000, 20000, 1600).astype(np.int16)
    write_wav(tmp_path / "query.wav", clip, 16000)
    audio = R.resample_ref(S.decode_ref(clip), 441, 160)
    q = HashAudioEncoder()(S.pack_ref(audio, [(0, len(audio))], 5 * MAP_RATE, 32768.0))[0]
    idx, _ = ops.retrieve_frame(np.ascontiguousarray(feats, dtype=np.float32), q)
    got = sm.get_pos_with_audio(str(tmp_path / "query.wav"), MAP_RATE)
    assert len(got) == len(locs[idx]) and all(np.array_equal(a, b) for a, b in zip(got, locs[idx]))
