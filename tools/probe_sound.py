"""GPU box: time the audio steps of the sound-map builder (csrc/avl_audio.hip) against NumPy on the same machine.  Prints one JSON
object (and writes it to --out).

    probe_sound.py [--reps 30] [--warmup 3] [--minutes 1 5 30] [--out profiles/sound_probe.txt]

Recordings of 1, 5 and 30 minutes at 44.1 kHz, mono PCM16: four seconds of noise every ten seconds, silence in between, so about one
segment per ten seconds; one second of silence splits (gap 44100), threshold 0, five-second contexts scaled by 32768.
  device_all       the host PCM uploaded, ops.decode_pcm16, ops.segment_audio, ops.pack_tracks(device=True): what
                   create_audio_map_batch runs per sequence before the encoder, the packed batch left in device memory
  device_upload    DeviceArray.from_numpy of the int16 PCM alone
  device_decode    ops.decode_pcm16 on the resident PCM
  device_segment   ops.segment_audio on the resident recording (five launches, the count and the segments read back)
  device_pack      ops.pack_tracks on the resident recording (the ranges uploaded, one launch)
  numpy_all        the same three steps with the vectorised NumPy closed forms of tests/_sound_ref.py (decode_ref,
                   segment_closed_form, pack_ref); numpy_decode / numpy_segment / numpy_pack are its parts
  python_walk      segment only, one Python iteration per loud sample (tests/_sound_ref.segment_walk: the cost structure of upstream's
                   loop, audio_utils.py:530-539).  Timed on the one-minute recording only.
Every path ends synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it.  `same` says that the device and NumPy paths returned equal results."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import _sound_ref as R  # noqa: E402
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402

SR, THR, SCALE = 44100, 0.0, 32768.0


def recording(minutes, seed=0):
    rng = np.random.default_rng(seed)
    n = int(minutes * 60 * SR)
    pcm = np.zeros(n, np.int16)
    for s in range(3 * SR, n - 4 * SR, 10 * SR):
        pcm[s:s + 4 * SR] = rng.integers(-12000, 12000, 4 * SR)
    return pcm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--minutes", type=float, nargs="+", default=[1, 5, 30])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    L, gap = 5 * SR, SR
    res = {"sample_rate": SR, "gap": gap, "context": L, "method": "host clock around synchronised calls, median of reps", "cases": {}}
    for minutes in a.minutes:
        pcm = recording(minutes)
        n = len(pcm)

        def dev_all():
            audio = ops.decode_pcm16(pcm)
            seg = ops.segment_audio(audio, SR, 1.0, THR)
            return seg, ops.pack_tracks(seg.audio, seg.segments_host, L, SCALE, device=True)

        def np_all():
            audio = R.decode_ref(pcm)
            seg = R.segment_closed_form(audio, THR, gap)
            return seg, R.pack_ref(audio, seg, L, SCALE)
        (dseg, dpack), (hseg, hpack) = dev_all(), np_all()
        same = np.array_equal(dseg.segments_host, hseg) and np.array_equal(dpack.numpy(), hpack)
        dpcm = DeviceArray.from_numpy(pcm)
        daudio = ops.decode_pcm16(dpcm)
        haudio = R.decode_ref(pcm)
        case = {"samples": n, "segments": int(len(hseg)), "same": bool(same)}
        case["device_all"] = stats(lib, dev_all, a.reps, a.warmup)
        case["device_upload"] = stats(lib, lambda: DeviceArray.from_numpy(pcm), a.reps, a.warmup)
        case["device_decode"] = stats(lib, lambda: ops.decode_pcm16(dpcm), a.reps, a.warmup)
        case["device_segment"] = stats(lib, lambda: ops.segment_audio(daudio, SR, 1.0, THR), a.reps, a.warmup)
        case["device_pack"] = stats(lib, lambda: ops.pack_tracks(daudio, hseg, L, SCALE, device=True), a.reps, a.warmup)
        print(f"# {minutes} min: device done", file=sys.stderr, flush=True)
        case["numpy_all"] = stats(lib, np_all, a.reps, a.warmup)
        case["numpy_decode"] = stats(lib, lambda: R.decode_ref(pcm), a.reps, a.warmup)
        case["numpy_segment"] = stats(lib, lambda: R.segment_closed_form(haudio, THR, gap), a.reps, a.warmup)
        case["numpy_pack"] = stats(lib, lambda: R.pack_ref(haudio, hseg, L, SCALE), a.reps, a.warmup)
        if minutes == min(a.minutes):
            assert np.array_equal(R.segment_walk(haudio, THR, gap), hseg)
            case["python_walk"] = dict(stats(lib, lambda: R.segment_walk(haudio, THR, gap), a.reps, a.warmup),
                                       note="one-minute recording only")
        print(f"# {minutes} min: host done", file=sys.stderr, flush=True)
        res["cases"][f"{minutes:g}_min"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
