"""GPU box: time the correlative pose search (csrc/avl_match.hip, ops.match_frames) against a vectorised NumPy restatement of the
same search on the same box.  Prints one JSON object (and writes it to --out).

    probe_match.py [--reps 30] [--warmup 3] [--out profiles/match_probe.txt]

720 x 1080 float32 depth frames of probe_explored.py's synthetic room at stride 4 (48 600 lattice pixels per frame), gs = 1000,
cs = 0.05, vh = 30, probe_audit.py's synthetic map of 2.0 M voxels in distinct cells drawn uniformly from the grid, K = 41 angles
(-10 .. 10 degrees in steps of 0.5), R = 10 and 20 cells (441 and 1681 shifts), 1, 16 and 32 frames in one joint volume, the height
band [2, 29]:
  resident     ops.match_frames with the depth frames and the results on the device: memsets, rasterise, correlate, finish
  from_host    the same call on host frames with the results copied back
  numpy        the host path, for one frame only: the points with the kernel's fma chains (an error-free product and sum), the
               rotation and the cells for all points at once, then one gather of the padded dense occupancy per angle and shift;
               scores, best and valid equal the device's: `same` is asserted, after the JSON line has been printed
Every device figure is the median of `reps` synchronised calls after `warmup` (host clock), minimum and maximum next to it.  A
random map gives the search nothing to find: the scores are what chance gives, the work per point and shift is the real map's."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_audit import N_VOXELS, VH, fma  # noqa: E402
from probe_explored import CS, GS, H, K, STRIDE, W, frames  # noqa: E402
from probe_morph2d import stats  # noqa: E402

ANGLES = ops.match_angles(10.0, 0.5)
PARAMS = dict(stride=STRIDE, min_depth=0.1, max_depth=6.0, h_band=(2, VH - 1))


def numpy_match(occ, depth, Ts, R, pivot):
    """ops.match_frames(joint=True) for whole frames at a time -> (scores (1, K, S, S) uint32, best (1, 4) int32, valid (1,) uint32)"""
    Kinv = np.linalg.inv(K)
    v, u = np.meshgrid(np.arange(STRIDE // 2, H, STRIDE), np.arange(STRIDE // 2, W, STRIDE), indexing="ij")
    x, y = u.ravel() + 0.5, v.ravel() + 0.5
    dirs = [fma(Kinv[i, 2], 1.0, fma(Kinv[i, 1], y, Kinv[i, 0] * x)) for i in range(3)]
    pts = []
    for f in range(len(depth)):
        T = Ts[f]
        z = depth[f][v.ravel(), u.ravel()].astype(np.float64)
        p = [d * z for d in dirs]
        with np.errstate(all="ignore"):
            ok = (p[2] > PARAMS["min_depth"]) & (p[2] < PARAMS["max_depth"])
            P = [fma(T[i, 3], 1.0, fma(T[i, 2], p[2], fma(T[i, 1], p[1], T[i, 0] * p[0]))) for i in range(3)]
            ok &= np.isfinite(P[0]) & np.isfinite(P[1]) & np.isfinite(P[2])
            h = np.trunc(np.where(ok, P[2], 0.0) / CS).astype(np.int64)
        ok &= (h >= PARAMS["h_band"][0]) & (h <= PARAMS["h_band"][1])
        pts.append(np.stack([P[0][ok], P[1][ok], h[ok].astype(np.float64)]))
    X, Y, Hh = np.concatenate(pts, axis=1)
    Hh = Hh.astype(np.int64)
    S, half = 2 * R + 1, GS / 2
    padded = np.pad(occ, ((2 * R, 2 * R), (2 * R, 2 * R), (0, 0)))
    scores = np.zeros((1, len(ANGLES), S, S), np.uint32)
    px, py = pivot
    for k, (c, s) in enumerate(ANGLES):
        if c == 1.0 and s == 0.0:
            qx, qy = X, Y
        else:
            dx, dy = X - px, Y - py
            qx, qy = px + (c * dx - s * dy), py + (s * dx + c * dy)
        row = (half - np.trunc(qx / CS)).astype(np.int64)
        col = (half - np.trunc(qy / CS)).astype(np.int64)
        keep = (row >= -R) & (row <= GS - 1 + R) & (col >= -R) & (col <= GS - 1 + R)
        r, cc, hh = row[keep] + 2 * R, col[keep] + 2 * R, Hh[keep]
        for a in range(S):
            for b in range(S):
                scores[0, k, a, b] = np.count_nonzero(padded[r + (a - R), cc + (b - R), hh])
    kk, aa, bb = (w.reshape(-1) for w in np.meshgrid(np.arange(len(ANGLES)), np.arange(S), np.arange(S), indexing="ij"))
    di, dj, sc, k0 = aa - R, bb - R, scores.reshape(-1).astype(np.int64), len(ANGLES) // 2
    i = np.lexsort((dj, di, kk, np.abs(kk - k0), di * di + dj * dj, -sc))[0]
    return scores, np.array([[kk[i], di[i], dj[i], sc[i]]], np.int32), np.array([X.shape[0]], np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    depth, Ts = frames(32)
    rng = np.random.default_rng(1)
    lin = rng.choice(GS * GS * VH, N_VOXELS, replace=False)
    grid_pos = np.stack(np.unravel_index(lin, (GS, GS, VH)), axis=1).astype(np.int32)
    occ = np.zeros(GS * GS * VH, bool)
    occ[lin] = True
    occ = occ.reshape(GS, GS, VH)
    index = ops.cell_index(DeviceArray.from_numpy(grid_pos), GS, VH)
    pivot = (float(Ts[0, 0, 3]), float(Ts[0, 1, 3]))
    res = {"frame": [H, W], "gs": GS, "cs": CS, "vh": VH, "stride": STRIDE, "voxels": N_VOXELS, "angles": len(ANGLES), "h_band": list(PARAMS["h_band"]),
           "pixels_per_frame": len(range(2, H, 4)) * len(range(2, W, 4)), "method": "host clock around synchronised calls, median of reps",
           "cases": {}}
    ok = True
    for R in (10, 20):
        for F in (1, 16, 32):
            d, T = depth[:F], Ts[:F]
            ddepth = DeviceArray.from_numpy(d)

            def resident():
                r = ops.match_frames(index, ddepth, K, T, CS, ANGLES, R, joint=True, pivot=pivot, device=True, **PARAMS)
                _lib.check(lib.avl_device_sync())
                r.free()

            def from_host():
                ops.match_frames(index, d, K, T, CS, ANGLES, R, joint=True, pivot=pivot, **PARAMS)
            got = ops.match_frames(index, ddepth, K, T, CS, ANGLES, R, joint=True, pivot=pivot, **PARAMS)
            case = {"valid": int(got.valid[0]), "best": got.best[0].tolist(), "shifts": (2 * R + 1) ** 2,
                    "probes": int(got.valid[0]) * len(ANGLES) * (2 * R + 1) ** 2}
            if F == 1:
                t0 = time.perf_counter()
                want = numpy_match(occ, d, T, R, pivot)
                case["numpy"] = {"mean_ms": (time.perf_counter() - t0) * 1e3, "reps": 1}
                case["same"] = bool(np.array_equal(got.scores, want[0]) and np.array_equal(got.best, want[1]) and np.array_equal(got.valid, want[2]))
                ok &= case["same"]
            case["resident"] = stats(lib, resident, a.reps, a.warmup)
            case["from_host"] = stats(lib, from_host, a.reps, a.warmup)
            res["cases"][f"radius_{R}_frames_{F}"] = case
            ddepth.free()
    index.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    assert ok, "the device search and the NumPy restatement differ"


if __name__ == "__main__":
    main()
