"""The sound map's audio kernels (csrc/avl_audio.hip through ops.decode_pcm16, segment_audio, pack_tracks) and the builder on top of
them (SoundMap.create_sound_map, get_pos, get_pos_with_audio, AVLMap.create_map(audio_encoder=)).

Oracles: the reference's own results recorded in golden g13 (tools/gen_golden_sound.py) and the NumPy closed forms of _sound_ref.py,
which test_sound_host.py ties to the same file.  Every comparison is np.array_equal: segments are integers, packed and decoded
samples are exact products and quotients.  Shapes are the smallest at which the scans can go wrong: around one tile (4096 samples),
a few tiles, and one recording with more tiles than the summary workgroup has threads."""
import ctypes as C
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import _sound_ref as R  # noqa: E402
from test_sound_host import SEQS, write_wav  # noqa: E402

T = R.TILE


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


@pytest.fixture(scope="module")
def g(golden):
    return golden("g13_sound_map.npz")


def check(ops, audio, gap, thr=0.0, sr=1):
    """segment with gap samples (sample_rate 1 makes silence_duration_s the gap) and compare with the closed form"""
    audio = np.asarray(audio, np.float32)
    seg = ops.segment_audio(audio, sr, float(gap) / sr, thr)
    want = R.segment_closed_form(audio, thr, gap)
    assert seg.segments.dtype == np.int64 and seg.segments.shape == want.shape, (seg.segments.shape, want.shape)
    assert np.array_equal(seg.segments, want)
    assert np.array_equal(seg.time_ranges, want / float(sr))
    return want


def spikes(n, at, value=1.0, fill=0.0):
    a = np.full(n, fill, np.float32)
    a[list(at)] = value
    return a


# ------------------------------------------------------------------ segmentation
@pytest.mark.parametrize("seq", SEQS)
def test_segments_equal_the_reference(ops, g, seq):
    sr = int(g["sample_rate"])
    audio = ops.decode_pcm16(g[f"{seq}_pcm"])
    seg = ops.segment_audio(audio, sr, float(g["silence_duration_s"]), float(g["silence_thres"]))
    assert np.array_equal(seg.segments, g[f"{seq}_segments"])
    assert np.array_equal(seg.time_ranges, g[f"{seq}_time_ranges"])
    assert seg.audio is audio and seg.n == len(g[f"{seq}_pcm"])
    assert np.array_equal(seg.segments, R.segment_closed_form(R.decode_ref(g[f"{seq}_pcm"]), 0.0, sr))
    # the tracks the reference's encoder received, cut or padded to five seconds
    L = 5 * sr
    packed = ops.pack_tracks(seg.audio, seg.segments, L)
    lens, flat = g[f"{seq}_track_lengths"], g[f"{seq}_tracks"]
    want = np.zeros((len(lens), L), np.float32)
    for k, (o, m) in enumerate(zip(np.cumsum(lens) - lens, lens)):
        want[k, :min(m, L)] = flat[o:o + min(m, L)]
    assert np.array_equal(packed, want)
    dev = ops.segment_audio(audio, sr, 1.0, 0.0, device=True)
    assert np.array_equal(dev.segments.numpy(), seg.segments) and np.array_equal(dev.segments_host, seg.segments)


@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 3 * T + 5])
def test_sizes_around_a_tile(ops, n):
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n).astype(np.float32)
    a[rng.random(n) < 0.9] = 0
    for gap in (1, 2, 7, 300, n, n + 1):
        check(ops, a, gap)
    check(ops, spikes(n, [n - 1]), 3)                      # a loud last sample only
    check(ops, spikes(n, [0]), 3)
    assert len(check(ops, np.zeros(n, np.float32), 3)) == 0          # no loud sample: no segment, no error
    assert len(check(ops, np.ones(n, np.float32), 2)) == 1           # every sample loud: one segment (0, n - 1)
    assert len(check(ops, np.ones(n, np.float32), 1)) == n           # gap 1: every loud sample is its own segment (l == r)


def test_a_single_loud_sample_gives_l_equal_r(ops):
    for at in (0, 15, 16, 4095, 4096, 9000):
        want = check(ops, spikes(2 * T + 999, [at]), 50)
        assert want.tolist() == [[at, at]]


@pytest.mark.parametrize("d", [-1, 0, 1])
@pytest.mark.parametrize("silent_tiles", [0, 1, 3])
def test_gaps_across_tile_boundaries(ops, d, silent_tiles):
    """two loud samples exactly gap + d apart: the first is the last sample of a tile (or a few before it), the second the first
    of a later tile (or a few after), with whole silent tiles in between, so the carried value passes through several summaries"""
    for back, fwd in ((0, 0), (3, 0), (0, 5), (17, 33)):
        p = T - 1 - back
        q = (1 + silent_tiles) * T + fwd
        gap = q - p - d
        if gap < 1:                                         # neighbours one sample apart have no gap + 1 case
            continue
        a = spikes((2 + silent_tiles) * T + 100, [p, q])
        want = check(ops, a, gap)
        assert len(want) == (1 if d == -1 else 2)
        b = a.copy()
        b[[5, 6, 7, q + 40]] = 2.0                          # neighbours that must not change where the split falls
        check(ops, b, gap)
    # loud on the last sample of a tile and the first of the next
    check(ops, spikes(2 * T, [T - 1, T]), 1)
    check(ops, spikes(2 * T, [T - 1, T]), 2)
    # thread and wave boundaries inside a tile
    for p, q in ((15, 16), (63 * 16 + 15, 64 * 16), (1023, 1024), (100, 2000)):
        for dd in (-1, 0, 1):
            check(ops, spikes(T, [p, q]), max(1, q - p - dd))


def test_nan_and_negative_threshold(ops):
    rng = np.random.default_rng(7)
    a = rng.standard_normal(2 * T + 77).astype(np.float32)
    a[rng.random(len(a)) < 0.3] = np.nan
    a[T - 1] = np.nan
    a[T] = np.inf
    for thr in (0.0, -0.5, 0.75, -np.inf):
        for gap in (2, 9):
            check(ops, a, gap, thr)
    assert len(check(ops, np.full(T + 3, np.nan, np.float32), 4)) == 0
    assert len(check(ops, np.zeros(T + 3, np.float32), 4, thr=-1.0)) == 1          # silence is loud above a negative threshold
    assert len(check(ops, np.full(10, -1.0, np.float32), 4, thr=-1.0)) == 0         # strictly greater


def test_more_tiles_than_the_summary_workgroup_has_threads(ops):
    n = 4 * 1024 * 1024 + 12345                              # 1028 tiles: the summary workgroup loops five times over its 256 threads
    assert -(-n // T) > 4 * R.SUMMARY_THREADS
    rng = np.random.default_rng(3)
    a = np.zeros(n, np.float32)
    for s in rng.integers(0, n - 5000, 60):
        a[s:s + int(rng.integers(1, 5000))] = 1.0
    a[[0, n - 1]] = 1.0
    a[rng.integers(0, n, 200)] = -1.0
    gap = 30000                                              # more than seven tiles
    want = check(ops, a, gap)
    assert 10 < len(want) < 70
    # an unaligned view of the same device buffer takes the scalar loads
    from avlmaps_amd.device import DeviceArray, DeviceView
    d = DeviceArray.from_numpy(a)
    for off in (1, 3):
        seg = ops.segment_audio(DeviceView(d.ptr + 4 * off, (n - off,), np.float32), 1, float(gap), 0.0)
        assert np.array_equal(seg.segments, R.segment_closed_form(a[off:], 0.0, gap))


def test_capacity_smaller_than_the_count_through_the_c_abi(ops):
    from avlmaps_amd import _lib
    from avlmaps_amd.device import DeviceArray
    lib = _lib.load()
    n = T + 50
    a = spikes(n, [3, 100, 101, 900, T - 1, T + 49])
    want = R.segment_closed_form(a, 0.0, 50)
    assert len(want) == 5
    d = DeviceArray.from_numpy(a)
    nb = C.c_size_t(0)
    _lib.check(lib.avl_audio_segment_work_bytes(n, C.byref(nb)))
    ws, cnt = DeviceArray((nb.value,), np.uint8), DeviceArray((1,), np.int64)
    for cap in (0, 1, 3, 5, 8):
        seg = DeviceArray.from_numpy(np.full((cap + 2, 2), -7, np.int64))
        _lib.check(lib.avl_audio_segment(d.ptr, n, 0.0, 50, seg.ptr, cap, cnt.ptr, ws.ptr, nb.value, None), "avl_audio_segment")
        got = seg.numpy()
        assert int(cnt.numpy()[0]) == 5
        k = min(cap, 5)
        assert np.array_equal(got[:k], want[:k]) and (got[k:] == -7).all()          # nothing written past the capacity


# ------------------------------------------------------------------ pack
@pytest.mark.parametrize("L", [1000, 1001, 7, 4096 + 4, 5000])
def test_pack_rows(ops, L):
    rng = np.random.default_rng(L)
    n = 3 * L + 13
    a = rng.standard_normal(n).astype(np.float32)
    ranges = np.array([[0, L], [5, 5 + L - 1], [3, 3 + L + 9], [17, 17], [n - 10, n], [n, n], [0, n], [1, 2], [n - L, n]], np.int64)
    for scale in (32768.0, 1.0):
        out = ops.pack_tracks(a, ranges, L, scale=scale)
        assert out.dtype == np.float32 and out.shape == (len(ranges), L)
        assert np.array_equal(out, R.pack_ref(a, ranges, L, scale))
    assert ops.pack_tracks(a, np.zeros((0, 2), np.int64), L).shape == (0, L)
    dev = ops.pack_tracks(a, ranges[:2], L, device=True)
    assert np.array_equal(dev.numpy(), R.pack_ref(a, ranges[:2], L, 32768.0))
    with pytest.raises(ValueError):
        ops.pack_tracks(a, [[0, n + 1]], L)


def test_contexts_equal_the_reference(ops, g):
    from avlmaps_amd.utils.audio_utils import get_five_second_contexts_audio
    sr = int(g["sample_rate"])
    for key in "ac":
        got = get_five_second_contexts_audio(g[f"ctx_{key}_audio"], g[f"ctx_{key}_times"].tolist(), sr)
        assert got.dtype == np.float64 and np.array_equal(got, g[f"ctx_{key}_out"])


# ------------------------------------------------------------------ decode
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
def test_decode_pcm16(ops, channels):
    rng = np.random.default_rng(channels)
    n = 1000 + channels
    pcm = rng.integers(-32768, 32768, (n, channels)).astype(np.int16)
    pcm[:6] = np.array([32767, -32768, 32767, -32768, 0, 1])[:, None]
    pcm[6] = np.resize([32767, -32768], channels)
    pcm[7] = np.resize([-32768, -32768, 32767], channels)
    got = ops.decode_pcm16(pcm if channels > 1 else pcm[:, 0], device=False)
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.array_equal(got, R.decode_ref(pcm))
    if channels == 1:
        assert got[0] == np.float32(32767 / 32768) and got[1] == -1.0


# ------------------------------------------------------------------ end to end
def write_sequences(root, g, with_skipped=True):
    sr, level = int(g["sample_rate"]), str(g["level"])
    for seq in SEQS:
        d = root / "audio_video" / seq
        d.mkdir(parents=True)
        write_wav(d / f"output_with_audio_{level}.wav", g[f"{seq}_pcm"], sr)
        np.savetxt(d / "poses.txt", g[f"{seq}_poses"])
        (d / f"range_and_audio_meta_{level}.txt").write_text(f"0,10,dog,{seq}.wav\n")
    if with_skipped:
        (root / "audio_video" / "000001").mkdir()          # no meta file: skipped


def sound_cfg(g):
    from avlmaps_amd.apps.common import DEFAULTS, to_cfg
    params = dict(DEFAULTS["sound_data_collect_params"], sample_rate=int(g["sample_rate"]), fps=float(g["fps"]),
                  silence_duration_s=float(g["silence_duration_s"]), silence_threshold=int(g["silence_thres"]), difficulty=str(g["level"]))
    return to_cfg(DEFAULTS["sound_config"]), to_cfg(params)


@pytest.fixture(scope="module")
def built(tmp_path_factory, g):
    from avlmaps_amd.apps.common import HashAudioEncoder, HashAudioText
    from avlmaps_amd.map.sound_map import SoundMap
    root = tmp_path_factory.mktemp("sound")
    write_sequences(root, g)
    sc, sp = sound_cfg(g)
    sm = SoundMap(str(root), sc, sp, audio_text_model=HashAudioText(), audio_encoder=HashAudioEncoder())
    path = sm.create_sound_map(str(root))
    return root, sm, Path(path)


def test_create_sound_map_reproduces_the_reference(built, g, ops):
    from avlmaps_amd.apps.common import HashAudioEncoder
    from avlmaps_amd.utils.audio_mapping_utils import create_audio_map_batch
    root, sm, path = built
    assert path == sm.sound_map_path(root) and path.exists()
    assert (root / "audio_video" / f"audio_map_statistics_{g['level']}.pkl").exists()
    db = sm.load_sound_map(str(root))
    counts = g["db_counts"]
    assert sorted(db) == list(range(len(counts)))
    assert [len(db[i]["locations"]) for i in db] == counts.tolist()
    got = np.concatenate([np.reshape(db[i]["locations"], (-1, 3)) for i in db])
    assert np.array_equal(got, g["db_locations"])
    # the features are the encoder's of the reference's recorded tracks, cut or padded to five seconds
    sr = int(g["sample_rate"])
    enc, i = HashAudioEncoder(), 0
    for seq in SEQS:
        lens, flat = g[f"{seq}_track_lengths"], g[f"{seq}_tracks"]
        for o, m in zip(np.cumsum(lens) - lens, lens):
            row = np.zeros(5 * sr, np.float32)
            row[:min(m, 5 * sr)] = flat[o:o + min(m, 5 * sr)]
            assert db[i]["audio_features"].shape == (enc.D,) and np.array_equal(db[i]["audio_features"], enc(row[None])[0])
            i += 1
    # segments, time and frame ranges per sequence
    details = {}
    create_audio_map_batch(str(root), enc, sample_rate=sr, silence_duration_s=1.0, silence_thres=0, fps=float(g["fps"]),
                           difficulty_level=str(g["level"]), details=details)
    assert sorted(details) == list(SEQS)
    for seq in SEQS:
        assert np.array_equal(details[seq]["segments"], g[f"{seq}_segments"])
        assert np.array_equal(details[seq]["time_ranges"], g[f"{seq}_time_ranges"])
        assert np.array_equal(details[seq]["frame_ranges"], g[f"{seq}_frame_ranges"])


def test_segment_audio_with_silence_returns_upstreams_pair(built, g):
    from avlmaps_amd.utils.audio_utils import segment_audio_with_silence
    root, _, _ = built
    seq, sr = SEQS[0], int(g["sample_rate"])
    tr, tracks = segment_audio_with_silence(str(root / "audio_video" / seq / f"output_with_audio_{g['level']}.wav"), 1.0, 0, sr)
    assert np.array_equal(np.asarray(tr), g[f"{seq}_time_ranges"])
    assert np.array_equal(np.concatenate(tracks) * np.float32(32768), g[f"{seq}_tracks"])
    assert [len(t) for t in tracks] == g[f"{seq}_track_lengths"].tolist()


def test_get_pos_and_get_pos_with_audio(built, g, tmp_path):
    root, sm, _ = built
    sm.load_sound_map(str(root))
    feats, locs = sm.get_all_audio_features_and_locations()
    # get_pos: the segment with the largest logit of the category
    cats = sm.sound_categories
    text = sm.aclp.encode_text(cats)
    logits = (sm.logit_scale() * feats) @ text.T
    for name in ("dog", "clock tick"):
        col = logits[:, cats.index(name)]
        order = np.unique(col)                                 # (the two empty tracks share one feature: equal logits, the first wins)
        assert order[-1] - order[-2] > 1e-3                    # the winner is not a rounding matter
        want = locs[int(np.argmax(col))]
        got = sm.get_pos(name)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    # get_pos_with_audio: a segment's own track finds that segment
    sr = int(g["sample_rate"])
    seq = SEQS[1]
    k = 1
    l, r = g[f"{seq}_segments"][k]
    write_wav(tmp_path / "query.wav", g[f"{seq}_pcm"][l:r], sr)
    got = sm.get_pos_with_audio(str(tmp_path / "query.wav"), sr)
    want = locs[len(g[f"{SEQS[0]}_segments"]) + k]
    assert len(got) == len(want) > 0 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert sm.get_pos_with_audio(str(tmp_path / "missing.wav"), sr) == ([], [])


def test_avlmap_builds_loads_and_indexes_the_sound_map(tmp_path, g):
    """AVLMap.create_map(audio_encoder=) on the first 1 300 samples of the fixture's second sequence (two segments, both with
    locations: index_sound rejects a database entry without any, as it did before), then load_map and index_sound"""
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps.common import HashAudioEncoder, HashAudioText, HashFeatureExtractor, load_config
    from avlmaps_amd.map import AVLMap
    sc = make(tmp_path / "scene", frames=3, H=48, W=64)
    sr, level, seq = int(g["sample_rate"]), str(g["level"]), SEQS[1]
    d = sc / "audio_video" / "000000"
    d.mkdir(parents=True)
    pcm = g[f"{seq}_pcm"][:1300]
    write_wav(d / f"output_with_audio_{level}.wav", pcm, sr)
    np.savetxt(d / "poses.txt", g[f"{seq}_poses"])
    (d / f"range_and_audio_meta_{level}.txt").write_text("0,10,dog,a.wav\n")
    _, sp = sound_cfg(g)
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [32, 0, 32, 0, 32, 24, 0, 0, 1], "depth_sample_rate": 3,
                                                       "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05},
                                        "sound_data_collect_params": dict(sp)}))
    cfg = load_config(str(cfg_path))
    av = AVLMap(cfg, data_dir=str(sc), audio_text_model=HashAudioText())
    np.random.seed(3)
    assert av.create_map(str(sc), feat_extractor=HashFeatureExtractor(64), audio_encoder=HashAudioEncoder())
    db = pickle.loads(av.sound_map.sound_map_path(sc).read_bytes())
    segs = R.segment_closed_form(R.decode_ref(pcm), 0.0, sr)
    assert np.array_equal(segs, g[f"{seq}_segments"][:2])
    frames = (segs / float(sr) * float(g["fps"])).astype(int)
    assert [len(db[i]["locations"]) for i in db] == (frames[:, 1] - frames[:, 0]).tolist() and min(len(db[i]["locations"]) for i in db) > 0
    assert np.array_equal(db[1]["locations"][0], g[f"{seq}_poses"][frames[1, 0], :3])
    av2 = AVLMap(cfg, data_dir=str(sc), audio_text_model=HashAudioText())
    assert av2.load_map(str(sc))
    heat = av2.index_sound("dog")
    assert heat.dtype == np.float32 and heat.shape == (len(av2.vlmap.grid_pos),) and np.isfinite(heat).all() and heat.max() > 0


def test_cli_chain_create_map_sound_then_index_map(tmp_path):
    """tools/make_synth_dataset.py --audio, create_map --sound, index_map --modality sound on the defaults (44.1 kHz, 25 fps)"""
    import yaml
    from make_synth_dataset import make, make_audio
    from avlmaps_amd.apps import create_map, index_map
    sc = make(tmp_path / "scene", frames=3, H=48, W=64)
    make_audio(sc, bursts=2)
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [32, 0, 32, 0, 32, 24, 0, 0, 1], "depth_sample_rate": 3,
                                                       "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(sc), "--config", str(cfg_path), "--features", "hash", "--feat-dim", "64", "--seed", "3", "--sound"])
    db = pickle.loads((sc / "audio_video" / "audio_data_level_3.pkl").read_bytes())
    assert len(db) == 2 and all(len(db[i]["locations"]) == 37 for i in db)          # 1.5 s bursts at 25 fps: frames 25..62, 112..149
    assert (sc / "audio_video" / "audio_map_statistics_level_3.pkl").exists()
    heat = index_map.main(["--data-dir", str(sc), "--config", str(cfg_path), "--text-model", "hash", "--modality", "sound", "--query", "dog"])
    assert heat.dtype == np.float32 and np.isfinite(heat).all() and heat.max() > 0
