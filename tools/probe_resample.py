"""GPU box: time loading a recording at another rate (csrc/avl_resample.hip) against scipy.signal.resample_poly on the same machine.
Prints one JSON object (and writes it to --out).

    probe_resample.py [--reps 30] [--warmup 3] [--scipy-reps 5] [--minutes 1 5 30] [--out profiles/resample_probe.txt]

Mono 24-bit recordings of 1, 5 and 30 minutes (uniform noise, packed 3-byte samples as a field recorder writes them), for each of
48 000 -> 44 100, 22 050 -> 44 100 and 44 100 -> 16 000 Hz:
  device_all        the host bytes uploaded, ops.decode_pcm(width=3), ops.resample_audio(device=True): what load_wav(...,
                    resample=True) runs after reading the file, the result left in device memory
  device_upload     DeviceArray.from_numpy of the packed bytes alone
  device_decode     ops.decode_pcm on the resident bytes
  device_resample   ops.resample_audio on the resident recording (one launch; the taps are resident after the first call)
  scipy_f64         resample_poly on the float64 copy of the decoded recording: the definition the kernel follows
  scipy_f32         resample_poly on the float32 recording itself (SciPy then filters in float32)
Every device path ends synchronised, so a host clock around each call is a valid time; every device figure is the median of
`reps` calls after `warmup`, the SciPy figures of `scipy-reps` calls after one, with the minimum and maximum next to them.
`unequal_f64` / `max_ulp_f64` compare the device result with float32(scipy_f64), `unequal_f32` / `max_ulp_f32` with scipy_f32."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import _resample_ref as R  # noqa: E402
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402

RATES = ((48000, 44100), (22050, 44100), (44100, 16000))


def recording(minutes, rate, seed=0):
    """mono 24-bit samples: their values (n, 1) int32 and their packed little-endian bytes (n, 1, 3) uint8"""
    n = int(minutes * 60 * rate)
    vals = np.random.default_rng(seed).integers(-2 ** 23, 2 ** 23, (n, 1), dtype=np.int32)
    return vals, R.pack24(vals)


def main():
    from scipy.signal import resample_poly
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scipy-reps", type=int, default=5)
    ap.add_argument("--minutes", type=float, nargs="+", default=[1, 5, 30])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    res = {"method": "host clock around synchronised calls, median of reps", "tile": ops.RESAMPLE_TILE, "lds_taps": ops.RESAMPLE_LDS_TAPS,
           "lds_window": ops.RESAMPLE_LDS_WINDOW, "cases": {}}
    for sr_in, sr_out in RATES:
        up, down = ops.resample_ratio(sr_in, sr_out)
        for minutes in a.minutes:
            vals, raw = recording(minutes, sr_in)
            n = len(raw)

            def dev_all():
                return ops.resample_audio(ops.decode_pcm(raw, width=3), sr_in, sr_out, device=True)
            draw = DeviceArray.from_numpy(raw)
            daudio = ops.decode_pcm(draw, width=3)
            haudio = daudio.numpy()
            got = dev_all().numpy()
            case = {"samples_in": n, "samples_out": int(len(got)), "up": up, "down": down, "taps": 20 * max(up, down) + 1,
                    "decode_same": bool(np.array_equal(haudio, R.decode_ref(vals, 3)))}
            case["device_all"] = stats(lib, dev_all, a.reps, a.warmup)
            case["device_upload"] = stats(lib, lambda: DeviceArray.from_numpy(raw), a.reps, a.warmup)
            case["device_decode"] = stats(lib, lambda: ops.decode_pcm(draw, width=3), a.reps, a.warmup)
            case["device_resample"] = stats(lib, lambda: ops.resample_audio(daudio, sr_in, sr_out, device=True), a.reps, a.warmup)
            print(f"# {sr_in} -> {sr_out}, {minutes:g} min: device done", file=sys.stderr, flush=True)
            h64 = haudio.astype(np.float64)
            want64 = resample_poly(h64, up, down).astype(np.float32)
            want32 = resample_poly(haudio, up, down)
            for name, want in (("f64", want64), ("f32", want32)):
                case[f"unequal_{name}"] = int((got != want).sum())
                case[f"max_ulp_{name}"] = float(R.ulps(got, want).max())
            case["scipy_f64"] = stats(lib, lambda: resample_poly(h64, up, down), a.scipy_reps, 1)
            case["scipy_f32"] = stats(lib, lambda: resample_poly(haudio, up, down), a.scipy_reps, 1)
            print(f"# {sr_in} -> {sr_out}, {minutes:g} min: host done", file=sys.stderr, flush=True)
            res["cases"][f"{sr_in}_to_{sr_out}_{minutes:g}_min"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
