"""GPU box: time the cell-to-cell line of sight (csrc/avl_sight.hip, ops.visible_counts) against a vectorised NumPy restatement of
the same walk on the same box.  Prints one JSON object (and writes it to --out).

    probe_sight.py [--reps 30] [--warmup 3] [--out profiles/sight_probe.txt]

A synthetic map of about 2.0 M voxels at gs = 1000, cs = 0.05, vh = 30: a floor, full-height walls every 100 cells with door gaps,
clutter below 0.5 m in 8 % of the columns, and a 12 x 12 x 16-cell object in the middle of a room whose voxels are the targets
(T = 256 and T = 1024 of them, evenly spaced rows) and `transparent`.  The eyes are the cells without a voxel between 0.05 m and 1 m within 3 m and within 6 m of the
object's centre in the plane (roughly 11 k and 45 k cells), at 1 m (height cell 20); the 3-D range is the same 3 m or 6 m.
  resident     ops.visible_counts with the index, eyes, targets and transparent on the device and device=True: the launch alone
  from_host    the same call on host arrays, results copied back: two uploads of cells, one of the mask, two downloads
  numpy        the walk stepped for a block of 512 eyes x T targets at once (one NumPy pass per step) against a dense occupancy
               grid; timed ONCE, and for cases of more than 4 M pairs only on every k-th eye (4 M pairs) and scaled by the eye count
               (`numpy_scaled`: true)
`same` compares the device result with NumPy's on the eyes NumPy walked; it is asserted after the JSON line has been printed.  Every
device figure is the median of `reps` synchronised calls after `warmup` (host clock), minimum and maximum next to it."""
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
from probe_morph2d import stats  # noqa: E402

GS, VH, CS = 1000, 30, 0.05
EYE_H = 20
CENTRE = (550, 550)


def synthetic_map(seed=0):
    """(grid_pos (N, 3) int32 in distinct cells, object mask (N,) bool)"""
    rng = np.random.default_rng(seed)
    occ = np.zeros((GS, GS, VH), bool)
    occ[:, :, 0] = True                                                     # the floor: 1.0 M
    lines = np.arange(0, GS, 100)
    wall = np.zeros((GS, GS), bool)
    wall[lines, :] = wall[:, lines] = True
    for r in lines:                                                         # a door in every wall segment
        for c in lines:
            wall[r, c + 45:c + 55] = wall[r + 45:r + 55, c] = False
    occ[wall] = True                                                        # ~ 0.5 M
    columns = rng.random((GS, GS)) < 0.08                                   # clutter: 8 % of the columns, 60 % full below 0.5 m: ~ 0.4 M
    occ[:, :, 1:10] |= columns[:, :, None] & (rng.random((GS, GS, 9)) < 0.6)
    obj = np.zeros_like(occ)
    obj[CENTRE[0] - 6:CENTRE[0] + 6, CENTRE[1] - 6:CENTRE[1] + 6, 1:17] = True
    occ |= obj
    pos = np.argwhere(occ).astype(np.int32)
    pos = pos[rng.permutation(len(pos))]
    return pos, obj[tuple(pos.T)], occ


def eyes_within(occ, metres):
    free = ~occ[:, :, 1:EYE_H + 1].any(axis=2)
    r, c = np.nonzero(free)
    near = (r - CENTRE[0]) ** 2 + (c - CENTRE[1]) ** 2 <= (metres / CS) ** 2
    return np.stack([r[near], c[near], np.full(int(near.sum()), EYE_H)], axis=1).astype(np.int32)


def numpy_counts(blocking, eyes, targets, max_range2, block=512):
    """visible and first of ops.visible_counts (end_margin 0, every cell inside the grid): `blocking` is the dense grid of the cells
    whose owner is not transparent"""
    T = len(targets)
    flat = blocking.ravel()
    visible, first = np.zeros(len(eyes), np.uint32), np.full(len(eyes), -1, np.int32)
    t = targets.astype(np.int64)
    for lo in range(0, len(eyes), block):
        e = eyes[lo:lo + block].astype(np.int64)
        a = np.repeat(e, T, axis=0)
        b = np.tile(t, (len(e), 1))
        d = np.abs(b - a)
        s = np.where(b > a, 1, -1)
        n = d.max(axis=1)
        ok = (d * d).sum(axis=1) <= max_range2
        err = 2 * d - n[:, None]
        x = a.copy()
        for k in range(1, int(n.max(initial=0))):
            step = err > 0
            x += np.where(step, s, 0)
            err += 2 * d - np.where(step, 2 * n[:, None], 0)
            live = ok & (k < n)
            hit = flat[np.where(live, (x[:, 0] * GS + x[:, 1]) * VH + x[:, 2], 0)]      # (a finished pair keeps stepping, unread)
            ok &= ~(live & hit)
        ok = ok.reshape(len(e), T)
        visible[lo:lo + len(e)] = ok.sum(axis=1)
        first[lo:lo + len(e)] = np.where(ok.any(axis=1), ok.argmax(axis=1), -1)
    return visible, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    pos, mask, occ = synthetic_map()
    blocking = occ.copy()
    blocking[tuple(pos[mask].T)] = False
    rows = np.flatnonzero(mask)
    tr = mask.astype(np.uint8)
    out = {"voxels": int(len(pos)), "gs": GS, "vh": VH, "object_voxels": int(len(rows)), "cases": []}
    d_pos, d_tr = DeviceArray.from_numpy(pos), DeviceArray.from_numpy(tr)
    same = True
    with ops.cell_index(d_pos, GS, VH) as index:
        out["index_bytes"] = index.nbytes
        for metres in (3.0, 6.0):
            eyes = eyes_within(occ, metres)
            d_eyes = DeviceArray.from_numpy(eyes)
            for T in (256, 1024):
                targets = np.ascontiguousarray(pos[rows[np.linspace(0, len(rows) - 1, T).astype(np.int64)]])
                d_targets = DeviceArray.from_numpy(targets)
                rng_cells = metres / CS
                case = {"range_m": metres, "eyes": int(len(eyes)), "targets": int(len(targets)), "pairs": int(len(eyes) * len(targets))}
                case["resident"] = stats(lib, lambda: ops.visible_counts(index, d_eyes, d_targets, d_tr, max_range=rng_cells, device=True),
                                         args.reps, args.warmup)
                case["from_host"] = stats(lib, lambda: ops.visible_counts(index, eyes, targets, tr, max_range=rng_cells), args.reps, args.warmup)
                got_v, got_f = ops.visible_counts(index, d_eyes, d_targets, d_tr, max_range=rng_cells)
                n_np = len(eyes) if case["pairs"] <= 4_000_000 else max(512, 4_000_000 // len(targets) // 512 * 512)
                sel = np.arange(len(eyes))[::len(eyes) // n_np][:n_np]          # every k-th eye: near and far ones alike
                t0 = time.perf_counter()
                ref_v, ref_f = numpy_counts(blocking, eyes[sel], targets, int(np.floor(rng_cells ** 2)))
                took = (time.perf_counter() - t0) * 1e3
                case["numpy_scaled"] = n_np < len(eyes)
                case["numpy_eyes"] = int(n_np)
                case["numpy_ms"] = took * len(eyes) / n_np
                case["speedup_resident"] = case["numpy_ms"] / case["resident"]["median_ms"]
                case["speedup_from_host"] = case["numpy_ms"] / case["from_host"]["median_ms"]
                case["visible_mean"] = float(got_v.mean())
                case["same"] = bool(np.array_equal(got_v[sel], ref_v) and np.array_equal(got_f[sel], ref_f))
                same = same and case["same"]
                out["cases"].append(case)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")
    assert same, "the device result differs from the NumPy restatement"


if __name__ == "__main__":
    main()
