"""GPU box: time ops.label_voxels (csrc/avl_instances.hip) against the host path it replaces.  Prints one JSON object (and writes it
to --out).

    probe_instances.py [--reps 30] [--warmup 3] [--out profiles/instances_<date>.txt]

A synthetic map of about 2 M voxels in a 1000 x 1000 x 30 grid: a floor and a smooth height field above it (gaussian-filtered noise),
in shuffled order like a map's insertion order.  A category's mask is the voxels whose column lies in one of a set of random discs
-- blobs, not noise -- sized to hold about 1 %, 10 % and 50 % of the voxels.  Per mask:
  device_resident  ops.label_voxels(device=True) with grid_pos, mask and scores already on the device, and the table read back: the
                   sort, the union-find, the count read back, the three table passes -- what VLMap.get_instances_3d runs
  device_host      the same from host arrays: the uploads of positions (24 MB), mask and scores and the read-back of the labels are part
                   of it
  host             what a user would do today, on the same bounding box: dense[...] = 1 into the box of the masked voxels,
                   scipy.ndimage.label with the 26-connected structure, the labels read back at the voxels
Both paths end synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it.  `same` says that both paths returned the same labels and count."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
from scipy import ndimage

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402

GS, VH = 1000, 30


def synthetic_map(seed=0):
    """(N, 3) int32 cells: the floor and one surface voxel per column where the height field is above it, shuffled"""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.random((GS, GS)), 8)
    h = np.clip(np.rint((f - f.min()) / (f.max() - f.min()) * (VH + 6) - 3), 0, VH - 1).astype(np.int32)
    r, c = np.mgrid[0:GS, 0:GS]
    up = h > 0
    pos = np.concatenate([np.stack([r.ravel(), c.ravel(), np.zeros(GS * GS, np.int64)], 1), np.stack([r[up], c[up], h[up]], 1)])
    return pos[rng.permutation(len(pos))].astype(np.int32)


def disc_mask(pos, fraction, seed):
    """the voxels whose column lies in one of a set of random discs of radius 6 .. 40 cells, added until `fraction` of them are in"""
    rng = np.random.default_rng(seed)
    img = np.zeros((GS, GS), bool)
    rr, cc = np.ogrid[0:GS, 0:GS]
    while img.mean() < fraction:
        r0, c0, rad = rng.integers(0, GS), rng.integers(0, GS), rng.integers(6, 41)
        img |= (rr - r0) ** 2 + (cc - c0) ** 2 <= rad * rad
    return img[pos[:, 0], pos[:, 1]].astype(np.uint8)


def host_labels(pos, mask):
    m = mask.astype(bool)
    p = pos[m]
    lo = p.min(0)
    q = p - lo
    dense = np.zeros(q.max(0) + 1, np.uint8)
    dense[q[:, 0], q[:, 1], q[:, 2]] = 1
    lab, n = ndimage.label(dense, ndimage.generate_binary_structure(3, 3))
    labels = np.zeros(len(pos), np.int32)
    labels[m] = lab[q[:, 0], q[:, 1], q[:, 2]]
    return labels, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    pos = synthetic_map()
    scores = np.random.default_rng(1).random(len(pos)).astype(np.float32)
    dpos, dscores = DeviceArray.from_numpy(pos), DeviceArray.from_numpy(scores)
    res = {"voxels": int(len(pos)), "grid": [GS, GS, VH], "connectivity": 26,
           "method": "host clock around synchronised calls, median of reps", "cases": {}}
    for k, fraction in enumerate((0.01, 0.1, 0.5)):
        mask = disc_mask(pos, fraction, 10 + k)
        dmask = DeviceArray.from_numpy(mask)

        def resident():
            with ops.label_voxels(dpos, dmask, 26, scores=dscores, device=True) as inst:
                return inst.table

        def from_host():
            with ops.label_voxels(pos, mask, 26, scores=scores) as inst:
                return inst.labels, inst.n, inst.table

        def host():
            return host_labels(pos, mask)
        got, want = from_host(), host()
        case = {"masked": int(mask.sum()), "fraction": float(mask.mean()), "instances": int(want[1]),
                "largest": int(got[2][:, 0].max()) if got[1] else 0, "same": bool(got[1] == want[1] and np.array_equal(got[0], want[0]))}
        case["device_resident"] = stats(lib, resident, a.reps, a.warmup)
        case["device_host"] = stats(lib, from_host, a.reps, a.warmup)
        case["host"] = stats(lib, host, a.reps, a.warmup)
        res["cases"][f"mask_{int(fraction * 100)}pct"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
