"""GPU box: time the open-set quantile query (csrc/avl_colselect.hip: ops.column_quantiles + ops.cols_above) against the host path it
replaces.  Prints one JSON object (and writes it to --out).

    probe_quantile.py [--rows 2000000] [--columns 1 16 64] [--reps 30] [--host-reps 30] [--warmup 3] [--out profiles/quantile_<date>.txt]

Scores of `rows` voxels x 1 / 16 / 64 categories, float32, resident on the device as the similarity kernel leaves them (values like
cosine similarities: normal around 0.2, so the first digit of the radix select is nearly constant, the worst case for its
LDS counters).  Per width:
  device           ops.column_quantiles(scores, 95) + ops.cols_above(scores, thresholds, column=0, device=True) on the resident matrix:
                   five streaming passes per 64 columns for the two order statistics, the float64 interpolation on the host, one
                   pass for words, counts and mask; the (Q,) tables come back, words and mask stay on the device
  quantiles, above the two halves of that, each alone
  host             what upstream's rule costs without the kernels: the matrix copied back (scores.numpy()), np.percentile(scores, 95,
                   axis=0) and scores > thresholds
All paths end synchronised, so a host clock around each call is a valid time; every figure is the median of its reps after `warmup`
calls, with the minimum and maximum next to it.  `bytes_per_pass` is rows x Q x 4, `passes` what the device path streams (6 per
64 columns), `stream_TBps` their product over the device time and `of_spec` that over the 8 TB/s of the data sheet: the launches'
gaps, the picks and the host's part are inside the time, so it is a whole-call rate, not a kernel's.  `same` says that the device
thresholds are np.percentile of the float64 columns bit for bit and the counts and mask those of the float64 comparison.
--host-reps 0 leaves the host path out: the form to run under rocprofv3 --kernel-trace --stats for the kernels' own times."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402

SPEC_TBPS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--columns", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    res = {"rows": a.rows, "percentile": 95, "method": "host clock around synchronised calls, median of reps", "numpy": np.__version__,
           "cases": {}}
    for Q in a.columns:
        scores = (rng.standard_normal((a.rows, Q), dtype=np.float32) * np.float32(0.03) + np.float32(0.2))
        dev = DeviceArray.from_numpy(scores)

        def quantiles():
            return ops.column_quantiles(dev, 95)

        thr = quantiles()

        def above():
            return ops.cols_above(dev, thr, column=0, device=True)

        def device():
            return ops.cols_above(dev, ops.column_quantiles(dev, 95), column=0, device=True)

        def host():
            m = dev.numpy()
            t = np.percentile(m, 95, axis=0)
            return t, m > t

        _, counts, mask = device()
        want = np.percentile(scores.astype(np.float64), 95, axis=0)
        hit = scores.astype(np.float64) > want
        case = {"columns": Q, "same": bool(thr.tobytes() == want.tobytes() and np.array_equal(counts, hit.sum(axis=0))
                                          and np.array_equal(mask.numpy(), hit[:, 0].astype(np.uint8)))}
        del hit, mask
        case["device"] = stats(lib, device, a.reps, a.warmup)
        case["quantiles"] = stats(lib, quantiles, a.reps, a.warmup)
        case["above"] = stats(lib, above, a.reps, a.warmup)
        if a.host_reps:
            case["host"] = stats(lib, host, a.host_reps, 1)
            case["host_over_device"] = case["host"]["median_ms"] / case["device"]["median_ms"]
        groups = (Q + ops.COLSELECT_SLOTS - 1) // ops.COLSELECT_SLOTS
        case["bytes_per_pass"] = int(a.rows) * Q * 4
        case["passes"] = 5 * groups + 1
        case["stream_TBps"] = case["bytes_per_pass"] * case["passes"] / (case["device"]["median_ms"] * 1e-3) / 1e12
        case["of_spec"] = case["stream_TBps"] / SPEC_TBPS
        res["cases"][f"columns_{Q}"] = case
        dev.free()
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
