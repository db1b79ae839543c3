#!/usr/bin/env python3
"""G13: the reference's sound-map builder (avlmaps/utils/audio_utils.py:515-583, audio_mapping_utils.py:26-122), EXECUTED on two
small sequences.

Run:  python tools/gen_golden_sound.py        (needs the reference checkout, see tools/ref_import.py; never runs on the GPU box)
Writes tests/golden/g13_sound_map.npz: arrays only.  The reference's modules are imported from where they lie, with what this
container lacks replaced: librosa, soundfile, wav2clip, torchvision, clip, omegaconf, the AudioCLIP package, esc50_utils,
category_assigner and the dataloader are stubs; lb.load returns the test track of the path it is given, lb.samples_to_time is
samples / sr and lb.time_to_samples is (t * sr).astype(int) (their documented meaning); extract_audio_from_video does nothing
(upstream's shells out to rm and ffmpeg); encode_audio_batch records the tracks it is handed and returns hashed features.  Then the
real segment_audio_with_silence, convert_time_ranges_to_frame_ranges, get_five_second_contexts_audio and the whole
create_audio_map_batch run.

Data: sample rate 200 Hz, 25 frames per second, one second of silence (gap 200 samples), threshold 0.  The tracks are int16 PCM / 32768,
what a PCM16 WAV file decodes to.
  seq 000000  3400 samples: bursts of mixed-sign noise (so most loud samples have quiet neighbours), pauses of 199, 200 and 201
              samples between loud samples, a lone loud sample (l == r, an empty track), a burst longer than five seconds, and a loud
              last sample
  seq 000001  no meta file: skipped
  seq 000002  2100 samples, the poses end before the recording does (the location slices are clipped)
Contexts: times with a negative start (counted from the end, on a 600-sample track it is not empty), a clipped end and a skipped time.
"""
import contextlib
import importlib
import io
import os
import sys
import tempfile
import types
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from ref_import import import_reference  # noqa: E402

OUT = HERE.parent / "tests" / "golden"
SR, FPS, SILENCE_S, THRES, LEVEL, D = 200, 25, 1.0, 0, "level_3", 16
SCENE = "g13scene_1"


def burst(rng, n):
    return rng.integers(-20000, 20000, n).astype(np.int16)


def tracks(rng):
    a = np.zeros(3400, np.int16)
    a[40:300] = burst(rng, 260)
    a[40], a[299] = 5, 7
    a[300:498] = -3                                  # quiet but not zero
    a[498] = 11                                      # 199 samples after 299: same segment
    a[698] = 1                                       # 200 after 498: a new segment, a lone loud sample -> (698, 698)
    a[899] = 32767                                   # 201 after 698: a new segment ...
    a[899:2150] = np.where(np.arange(1251) % 3 == 0, burst(rng, 1251), -1)     # ... longer than five seconds
    a[899] = 32767
    a[2149] = 9
    a[2600:2900] = burst(rng, 300)
    a[2600] = -32768                                 # not loud: the segment starts at the first positive sample after it
    a[3399] = 1                                      # the recording ends loud, 500 or so after the burst: a last lone sample
    b = np.zeros(2100, np.int16)
    b[0] = 3                                         # loud first sample
    b[1:150] = burst(rng, 149)
    b[500:1200] = burst(rng, 700)
    b[1650:1900] = burst(rng, 250)
    return a, b


def main():
    rng = np.random.default_rng(1313)
    pcm = dict(zip(("000000", "000002"), tracks(rng)))
    audio = {k: (v.astype(np.float32) / 32768).astype(np.float32) for k, v in pcm.items()}
    poses = {"000000": np.round(rng.uniform(-3, 3, (int(3400 / SR * FPS) + 2, 7)), 4),
             "000002": np.round(rng.uniform(-3, 3, (200, 7)), 4)}           # 2100 samples are 262 frames: the last segment is clipped

    class Tqdm:
        def __init__(self, it=None, **k):
            self.it = it

        def __iter__(self):
            return iter(self.it)

        def set_description(self, *a, **k):
            pass

    by_path, sample_log = {}, []
    lb = types.ModuleType("librosa")
    lb.load = lambda path, sr=None: (by_path[path], sr)

    def samples_to_time(samples, sr):
        sample_log.append([int(samples[0]), int(samples[1])])
        return np.asarray(samples) / sr
    lb.samples_to_time = samples_to_time
    lb.time_to_samples = lambda t, sr: (np.asarray(t) * sr).astype(int)
    sys.modules["librosa"] = lb
    tq = types.ModuleType("tqdm")
    tq.tqdm = Tqdm
    real_tqdm = sys.modules.get("tqdm")
    sys.modules["tqdm"] = tq
    for name in ["soundfile", "wav2clip", "avlmaps.utils.esc50_utils", "avlmaps.utils.category_assigner",
                 "avlmaps.dataloader", "avlmaps.dataloader.habitat_dataloader", "avlmaps.audioclip", "avlmaps.audioclip.model",
                 "avlmaps.audioclip.model.audioclip", "avlmaps.audioclip.utils", "avlmaps.audioclip.utils.transforms", "noisereduce"]:
        sys.modules[name] = MagicMock(name=name)
    import_reference()
    au = importlib.import_module("avlmaps.utils.audio_utils")
    amu = importlib.import_module("avlmaps.utils.audio_mapping_utils")
    if real_tqdm is not None:
        sys.modules["tqdm"] = real_tqdm

    out = dict(sample_rate=np.int64(SR), fps=np.float64(FPS), silence_duration_s=np.float64(SILENCE_S), silence_thres=np.int64(THRES),
               level=np.array(LEVEL), seqs=np.array(sorted(pcm)), feat_dim=np.int64(D))
    recorded = []

    def record(tracks_, aclp, audio_transforms, sample_rate):
        recorded.append([np.asarray(t).copy() for t in tracks_])
        feats = []
        for t in tracks_:
            seed = int.from_bytes(np.asarray(t, np.float32).tobytes()[:8].ljust(8, b"\0"), "little") % (2 ** 32)
            feats.append(np.random.default_rng(seed).standard_normal(D).astype(np.float32))
        return np.stack(feats)

    sink = io.StringIO()
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(sink):
        data_dir = os.path.join(tmp, SCENE)
        touched = []
        for i, seq in enumerate(("000000", "000001", "000002")):
            d = Path(data_dir) / "audio_video" / seq
            d.mkdir(parents=True)
            if seq in pcm:
                (d / f"range_and_audio_meta_{LEVEL}.txt").write_text(f"0,10,dog,{seq}.wav\n")
                np.savetxt(d / "poses.txt", poses[seq])
                wav = f"/tmp/{SCENE.split('_')[0]}_{i}.wav"          # where upstream expects the extracted sound track
                Path(wav).touch()
                touched.append(wav)
                by_path[wav] = audio[seq]
        try:
            # the stand-alone functions, per sequence
            for seq, wav in zip(sorted(pcm), touched):
                del sample_log[:]
                time_ranges, seg_tracks = au.segment_audio_with_silence(wav, silence_duration_s=SILENCE_S, silence_thres=THRES,
                                                                        sample_rate=SR)
                out[f"{seq}_pcm"], out[f"{seq}_poses"] = pcm[seq], poses[seq]
                out[f"{seq}_segments"] = np.asarray(sample_log, np.int64).reshape(-1, 2)
                out[f"{seq}_time_ranges"] = np.asarray(time_ranges, np.float64).reshape(-1, 2)
                out[f"{seq}_frame_ranges"] = np.asarray(au.convert_time_ranges_to_frame_ranges(time_ranges, FPS), np.int64).reshape(-1, 2)
                assert all(np.array_equal(t, audio[seq][l:r]) for t, (l, r) in zip(seg_tracks, sample_log))
            # the whole builder
            amu.extract_audio_from_video = lambda video_path, output_audio_path: None
            amu.encode_audio_batch = record
            amu.tqdm = Tqdm
            amu.create_audio_map_batch(data_dir, aclp=object(), audio_transforms=None, sample_rate=SR, silence_duration_s=SILENCE_S,
                                       silence_thres=THRES, fps=FPS, difficulty_level=LEVEL, manual_mode=False, seq_num=None)
            import pickle
            with open(os.path.join(data_dir, "audio_video", f"audio_data_{LEVEL}.pkl"), "rb") as f:
                db = pickle.load(f)
        finally:
            for wav in touched:
                os.unlink(wav)
    assert len(recorded) == 2
    for seq, rec in zip(sorted(pcm), recorded):
        out[f"{seq}_track_lengths"] = np.array([len(t) for t in rec], np.int64)
        out[f"{seq}_tracks"] = np.concatenate(rec).astype(np.float32) if rec else np.zeros(0, np.float32)
        assert all(t.dtype == np.float32 for t in rec)
    out["db_counts"] = np.array([len(db[i]["locations"]) for i in range(len(db))], np.int64)
    out["db_locations"] = np.concatenate([np.asarray(db[i]["locations"], np.float64).reshape(-1, 3) for i in range(len(db))])

    # five-second contexts
    ctx_audio = {"a": audio["000000"], "c": audio["000002"][500:1100].copy()}
    times = [1.0, 2.5, 2.7, 5.4, 5.5, 9.0, 16.0, 19.4, 19.6]       # (2.9 would span 1001 samples by rounding: upstream raises there)
    for k, a in ctx_audio.items():
        out[f"ctx_{k}_audio"], out[f"ctx_{k}_times"] = a, np.asarray(times)
        out[f"ctx_{k}_out"] = np.asarray(au.get_five_second_contexts_audio(a, times, SR), np.float64)
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT / "g13_sound_map.npz", **out)
    for k, v in out.items():
        print(k, getattr(v, "shape", None), getattr(v, "dtype", None))
    print("segments", {s: out[f"{s}_segments"].tolist() for s in sorted(pcm)})
    print("wrote", OUT / "g13_sound_map.npz", (OUT / "g13_sound_map.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
