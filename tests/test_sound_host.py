"""Host side of the sound-map builder: the closed forms against the reference's recorded results (golden g13, made by
tools/gen_golden_sound.py), WAV loading, the file layout, the frame and location arithmetic, and the argument checks of the three
C entry points, which happen before any device work.  No GPU."""
import ctypes as C
import pickle
import sys
import wave
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _sound_ref as R  # noqa: E402

SEQS = ("000000", "000002")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g13_sound_map.npz")


def write_wav(path, pcm, rate):
    pcm = np.asarray(pcm, np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


# ------------------------------------------------------------------ closed forms == the reference's recorded results
@pytest.mark.parametrize("seq", SEQS)
def test_closed_form_equals_the_reference(g, seq):
    sr, gap = int(g["sample_rate"]), int(float(g["silence_duration_s"]) * int(g["sample_rate"]))
    audio = R.decode_ref(g[f"{seq}_pcm"])
    want = g[f"{seq}_segments"]
    assert len(want) >= 3
    for fn in (R.segment_closed_form, R.segment_walk):
        assert np.array_equal(fn(audio, float(g["silence_thres"]), gap), want)
    assert np.array_equal(want / float(sr), g[f"{seq}_time_ranges"])
    # the tracks the reference handed to its encoder: audio[l:r] * 32768 in float32, uncropped
    lens = g[f"{seq}_track_lengths"]
    assert np.array_equal(lens, want[:, 1] - want[:, 0])
    assert np.array_equal(np.concatenate([audio[l:r] * np.float32(32768) for l, r in want]), g[f"{seq}_tracks"])


def test_the_fixture_holds_the_edge_cases(g):
    s = g["000000_segments"]
    assert (s[:, 0] == s[:, 1]).sum() >= 2                       # lone loud samples: empty tracks
    assert s[-1, 1] == len(g["000000_pcm"]) - 1                  # the recording ends loud
    assert (s[:, 1] - s[:, 0]).max() > 5 * int(g["sample_rate"])  # a track longer than the encoder's five seconds
    assert g["000002_segments"][0, 0] == 0                       # a loud first sample
    gaps = s[1:, 0] - s[:-1, 1]
    assert 200 in gaps and 201 in gaps                           # (199 does not split: samples 299 -> 498 stay in one segment)


@pytest.mark.parametrize("key", ["a", "c"])
def test_context_ranges_equal_the_reference(g, key):
    from avlmaps_amd import ops
    sr = int(g["sample_rate"])
    audio, times, want = g[f"ctx_{key}_audio"], g[f"ctx_{key}_times"].tolist(), g[f"ctx_{key}_out"]
    assert np.array_equal(R.context_ref(audio, times, sr), want)
    ranges = ops.context_ranges(len(audio), times, sr)
    assert ranges.dtype == np.int64 and ranges.shape == (len(want), 2) and len(want) < len(times)       # a time was skipped
    assert (ranges[:, 0] >= 0).all() and (ranges[:, 0] <= ranges[:, 1]).all() and (ranges[:, 1] <= len(audio)).all()
    assert np.array_equal(R.pack_ref(audio, ranges, 5 * sr, 1.0).astype(np.float64).reshape(len(want), 1, -1), want)
    if key == "c":
        assert ranges[0].tolist() == [300, 600]                 # t = 1.0: audio[-300:700] counts from the end
    else:
        assert ranges[0, 0] == ranges[0, 1]                     # the same bounds on a long recording: empty


def test_context_ranges_random_against_slicing():
    from avlmaps_amd import ops
    rng = np.random.default_rng(5)
    for _ in range(50):
        n, sr = int(rng.integers(1, 900)), int(rng.integers(20, 90))
        audio = rng.standard_normal(n).astype(np.float32)
        times = [t for t in rng.uniform(-3, n / sr + 4, 6).tolist()
                 if np.diff((np.asarray([t - 2.5, t + 2.5]) * sr).astype(int))[0] <= 5 * sr]          # (upstream raises on 5 sr + 1)
        want = R.context_ref(audio, times, sr)
        ranges = ops.context_ranges(n, times, sr)
        assert len(ranges) == len(want)
        if len(want):
            assert np.array_equal(R.pack_ref(audio, ranges, 5 * sr, 1.0).astype(np.float64).reshape(len(want), 1, -1), want)


# ------------------------------------------------------------------ WAV files
def test_load_wav_reads_pcm16_and_rejects_a_wrong_rate(tmp_path):
    from avlmaps_amd.utils import audio_utils as U
    rng = np.random.default_rng(1)
    mono = rng.integers(-32768, 32768, 500).astype(np.int16)
    stereo = rng.integers(-32768, 32768, (300, 2)).astype(np.int16)
    write_wav(tmp_path / "m.wav", mono, 8000)
    write_wav(tmp_path / "s.wav", stereo, 22050)
    rate, data = U.read_wav(tmp_path / "m.wav")
    assert rate == 8000 and data.dtype == np.int16 and np.array_equal(data, mono)
    rate, data = U.read_wav(tmp_path / "s.wav")
    assert rate == 22050 and np.array_equal(data, stereo)
    with pytest.raises(ValueError, match="resampl"):
        U.load_wav(tmp_path / "m.wav", 44100)
    # a float32 file passes through unchanged
    from scipy.io import wavfile
    f = rng.uniform(-1, 1, 400).astype(np.float32)
    wavfile.write(tmp_path / "f.wav", 16000, f)
    out = U.load_wav(tmp_path / "f.wav", 16000)
    assert out.dtype == np.float32 and np.array_equal(out, f)
    assert U.segment_audio_with_silence(tmp_path / "missing.wav", 1, 0, 8000) == ([], [])


# ------------------------------------------------------------------ layout and arithmetic
def test_file_names_and_dictionary_layout(tmp_path):
    from avlmaps_amd.apps.common import DEFAULTS, to_cfg
    from avlmaps_amd.map.sound_map import SoundMap
    from avlmaps_amd.utils import audio_mapping_utils as M
    from avlmaps_amd.utils import audio_utils as U
    assert M.sound_file_names("level_2") == ("range_and_audio_meta_level_2.txt", "output_with_audio_level_2.mp4",
                                             "audio_data_level_2.pkl", "audio_map_statistics_level_2.pkl")
    assert M.sound_file_names("level_1", manual_mode=True)[2] == "audio_data_manual_level_1.pkl"
    sm = SoundMap(str(tmp_path), to_cfg(DEFAULTS["sound_config"]), to_cfg(DEFAULTS["sound_data_collect_params"]))
    assert sm.sound_map_path(tmp_path) == tmp_path / "audio_video" / M.sound_file_names("level_3")[2]
    p = DEFAULTS["sound_data_collect_params"]
    assert (p["fps"], p["sample_rate"], p["silence_duration_s"], p["silence_threshold"], p["considered_seq_num_per_scene"]) == \
        (25, 44100, 1, 0, 20)
    d = U.create_audio_dictionary([np.ones(4, np.float32), np.zeros(4, np.float32)], [[np.zeros(3)], []])
    assert sorted(d) == [0, 1] and sorted(d[0]) == ["audio_features", "locations"] and d[1]["locations"] == []
    (tmp_path / "audio_video" / "b").mkdir(parents=True)
    (tmp_path / "audio_video" / "a").mkdir()
    (tmp_path / "audio_video" / "audio_data_level_3.pkl").write_bytes(b"")
    av, seqs = U.setup_audio_paths(str(tmp_path))
    assert av == str(tmp_path / "audio_video") and [Path(s).name for s in seqs] == ["a", "b"]
    # statistics: the last two fields of every meta line
    (tmp_path / "audio_video" / "a" / "range_and_audio_meta_level_3.txt").write_text("3,9,dog,1-100.wav\n12,20,cat,2-7.wav\n")
    path = M.create_audio_map_statistics(str(tmp_path), "level_3")
    assert Path(path).name == "audio_map_statistics_level_3.pkl"
    assert pickle.loads(Path(path).read_bytes()) == [["dog", "1-100.wav"], ["cat", "2-7.wav"]]
    with pytest.raises(FileNotFoundError, match="output_with_audio_level_3"):
        M.find_audio(tmp_path / "audio_video" / "a" / "output_with_audio_level_3.mp4", 44100, tmp_path)
    with pytest.raises(RuntimeError, match="audio encoder"):
        sm.create_sound_map(str(tmp_path))


@pytest.mark.parametrize("seq", SEQS)
def test_frame_ranges_and_locations_equal_the_reference(g, seq):
    from avlmaps_amd.utils import audio_mapping_utils as M
    from avlmaps_amd.utils import audio_utils as U
    from avlmaps_amd.utils.mapping_utils import cvt_pose_vec2tf
    tr = [tuple(t) for t in g[f"{seq}_time_ranges"]]
    fr = U.convert_time_ranges_to_frame_ranges(tr, float(g["fps"]))
    assert np.array_equal(np.asarray(fr, np.int64), g[f"{seq}_frame_ranges"])
    poses = g[f"{seq}_poses"]
    locs = M.segment_locations(poses, fr)
    first = 0 if seq == SEQS[0] else len(g[f"{SEQS[0]}_segments"])
    counts = g["db_counts"][first:first + len(fr)]
    assert [len(l) for l in locs] == counts.tolist()
    off = int(g["db_counts"][:first].sum())
    assert np.array_equal(np.concatenate([np.reshape(l, (-1, 3)) for l in locs]), g["db_locations"][off:off + int(counts.sum())])
    assert np.array_equal(locs[0][0], cvt_pose_vec2tf(poses[fr[0][0]])[:3, 3])
    if seq == SEQS[1]:
        assert counts[-1] < fr[-1][1] - fr[-1][0]                # the poses end before the last segment does


# ------------------------------------------------------------------ argument checks without a GPU
def test_entry_points_check_their_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    build()
    lib = _lib.load()
    fake = C.c_void_p(4096)                          # never dereferenced: every call below fails its checks first

    def err():
        return lib.avl_last_error()
    nb = C.c_size_t(0)
    assert lib.avl_audio_segment_work_bytes(10, None) != 0 and b"null" in err()
    assert lib.avl_audio_segment_work_bytes(0, C.byref(nb)) != 0 and b"outside" in err()
    assert lib.avl_audio_segment_work_bytes(2 ** 31, C.byref(nb)) != 0
    assert lib.avl_audio_segment_work_bytes(2 ** 31 - 1, C.byref(nb)) == 0 and nb.value >= (2 ** 31 // R.TILE) * 20
    assert lib.avl_audio_segment_work_bytes(R.TILE + 1, C.byref(nb)) == 0 and nb.value >= 2 * 20
    assert lib.avl_audio_segment(None, 10, 0.0, 1, fake, 4, fake, fake, 1 << 20, None) != 0 and b"null" in err()
    assert lib.avl_audio_segment(fake, 10, 0.0, 0, fake, 4, fake, fake, 1 << 20, None) == 1 and b"gap" in err()
    assert lib.avl_audio_segment(fake, 0, 0.0, 1, fake, 4, fake, fake, 1 << 20, None) == 1
    assert lib.avl_audio_segment(fake, 10, float("nan"), 1, fake, 4, fake, fake, 1 << 20, None) == 1 and b"NaN" in err()
    assert lib.avl_audio_segment(fake, 10, 0.0, 1, None, 4, fake, fake, 1 << 20, None) == 1
    assert lib.avl_audio_segment(fake, 10, 0.0, 1, fake, -1, fake, fake, 1 << 20, None) == 1
    assert lib.avl_audio_segment(fake, 10, 0.0, 1, fake, 4, fake, fake, 8, None) == 1 and b"workspace" in err()
    assert lib.avl_audio_pack(None, 10, fake, 1, 8, 1.0, fake, None) != 0 and b"null" in err()
    assert lib.avl_audio_pack(fake, 10, fake, 1, 0, 1.0, fake, None) == 1
    assert lib.avl_audio_pack(fake, 10, fake, -1, 8, 1.0, fake, None) == 1
    assert lib.avl_audio_pack(fake, 10, fake, 2 ** 40, 8, 1.0, fake, None) == 1
    assert lib.avl_audio_pack(fake, 10, None, 0, 8, 1.0, fake, None) == 0            # no rows: nothing to do
    assert lib.avl_audio_decode_pcm16(None, 10, 1, fake, None) != 0 and b"null" in err()
    assert lib.avl_audio_decode_pcm16(fake, 10, 9, fake, None) == 1 and b"channels" in err()
    assert lib.avl_audio_decode_pcm16(fake, 10, 0, fake, None) == 1
    assert lib.avl_audio_decode_pcm16(fake, 0, 1, fake, None) == 1


def test_ops_check_their_arguments():
    from avlmaps_amd import ops
    a = np.zeros(100, np.float32)
    with pytest.raises(ValueError, match="float32"):
        ops.segment_audio(a, 100, 1.0, 0.1)                      # 0.1 is not a float32
    with pytest.raises(ValueError, match="gap"):
        ops.segment_audio(a, 100, 0.001, 0.0)
    with pytest.raises(TypeError):
        ops.segment_audio(a.astype(np.float64), 100, 1.0, 0.0)
    with pytest.raises(ValueError):
        ops.segment_audio(a.reshape(10, 10), 100, 1.0, 0.0)
    with pytest.raises(TypeError):
        ops.decode_pcm16(a)
    with pytest.raises(ValueError):
        ops.decode_pcm16(np.zeros((10, 9), np.int16))
    for bad in ([[-1, 5]], [[5, 4]], [[0, 101]]):
        with pytest.raises(ValueError, match="start"):
            ops._check_ranges(bad, 100)
    assert ops._check_ranges([[0, 0], [100, 100], [3, 100]], 100).dtype == np.int64
    assert hasattr(ops, "pack_tracks") and hasattr(ops, "context_ranges")
