"""GPU box: time the fusion of two voxel maps (csrc/avl_mapfuse.hip through ops.move_cells, fuse_plan, fuse_rows, fuse_maps) on two
synthetic maps of 2 M voxels x 512 features at three overlaps and under one rotation, against two yardsticks from the same run: a
NumPy host fuse, asserted equal, and the project's own avl_gather_rows moving the same number of feature bytes.  Prints one JSON
object (and writes it to --out).

    probe_mapfuse.py [--voxels 2000000] [--dim 512] [--reps 30] [--warmup 3] [--numpy-reps 1] [--out PATH]

Map A: `voxels` distinct cells of a 1000 x 1000 x 30 grid, seeded float32 rows, weights in [1, 30), colours.  Map B: as many cells, of
which 0 %, 50 % or 100 % are cells of A and the others free cells, shuffled.  All inputs are resident (DeviceArrays), the fused rows are
written into a resident matrix made once, the other results stay on the device.  Per case:
  move          ops.move_cells under the identity transform (the float64 path); in the rotated case under 3 degrees about the vertical
                axis plus (0.013, -0.02, 0) m
  plan          ops.fuse_plan: two cell indices, three scans, one stable argsort, one read-back of four integers
  rows          ops.fuse_rows without occupied_ids.  `bytes` = (members + n_out) * D * 4, what it must read and write of feature rows;
                `share_of_8TBps` = bytes / time / 8e12; `share_of_gather` = the gather's time / this time
  rows_occupied the same with occupied_ids (a 120 MB fill and one scattered store per voxel more)
  gather        avl_gather_rows of bytes / (2 * D * 4) rows of 4 * D bytes, random rows of map B: reads and writes as many feature bytes
                in all.  The copy floor: whole rows gathered, whole rows written, no arithmetic
  fuse_maps     the whole call on resident inputs, results on the device
  numpy         (the 50 % case only) a stable sort of the concatenated linear cells, group starts from the sorted keys, np.add.reduceat
                over float64 products in pieces of 2^17 rows, the division; grid_feat, weight and grid_rgb are asserted equal to the
                device's after bringing them into the device's voxel order
Every path ends synchronised, so a host clock around each call is a valid time; every device figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it.  Kernel times were not collected with rocprofv3 --kernel-trace --stats: the figures
include the launches, the plan's read-back and the synchronisation (tens of microseconds each)."""
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
from probe_mapdiff import rows  # noqa: E402
from probe_morph2d import stats  # noqa: E402

GS, VH, CS = 1000, 30, 0.05


def cells_of(lin):
    return np.stack(np.unravel_index(lin, (GS, GS, VH)), axis=1).astype(np.int32)


def numpy_fuse(pos_a, feat_a, w_a, rgb_a, pos_b, feat_b, w_b, rgb_b):
    """-> (linear cell, feat, weight, rgb) of every output voxel, in ascending linear cell"""
    lin = np.concatenate([(p[:, 0].astype(np.int64) * GS + p[:, 1]) * VH + p[:, 2] for p in (pos_a, pos_b)])
    order = np.argsort(lin, kind="stable")                              # A's row before B's rows, B's ascending: the member order
    key = lin[order]
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    w = np.concatenate([w_a, w_b]).astype(np.float64)[order]
    n_a, D = len(pos_a), feat_a.shape[1]
    W = np.add.reduceat(w, starts)
    col = np.add.reduceat(w[:, None] * np.concatenate([rgb_a, rgb_b]).astype(np.float64)[order], starts, axis=0)
    feat = np.empty((len(starts), D), np.float32)
    piece = 1 << 17
    for g0 in range(0, len(starts), piece):
        g1 = min(len(starts), g0 + piece)
        r0, r1 = starts[g0], starts[g1] if g1 < len(starts) else len(order)
        idx = order[r0:r1]
        f = np.where((idx < n_a)[:, None], feat_a[np.minimum(idx, n_a - 1)], feat_b[np.maximum(idx - n_a, 0)]).astype(np.float64)
        acc = np.add.reduceat(w[r0:r1, None] * f, starts[g0:g1] - r0, axis=0)
        feat[g0:g1] = (acc / W[g0:g1, None]).astype(np.float32)
    return key[starts], feat, W.astype(np.float32), np.trunc(col / W[:, None]).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    n, D = a.voxels, a.dim
    rng = np.random.default_rng(0)
    lin = rng.choice(GS * GS * VH, 2 * n, replace=False)
    pos_a, free = cells_of(lin[:n]), lin[n:]
    feat_a, feat_b = rows(rng, n, D), rows(rng, n, D)
    w_a, w_b = rng.uniform(1, 30, n).astype(np.float32), rng.uniform(1, 30, n).astype(np.float32)
    rgb_a, rgb_b = rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.integers(0, 256, (n, 3)).astype(np.uint8)
    print(f"maps made: 2 x {n} voxels x {D}", file=sys.stderr, flush=True)
    dfa, dfb, dwa, dwb, dra, drb, dpa = (DeviceArray.from_numpy(x) for x in (feat_a, feat_b, w_a, w_b, rgb_a, rgb_b, pos_a))
    out = DeviceArray((2 * n, D), np.float32)
    res = {"voxels": n, "dim": D, "grid": [GS, GS, VH], "cases": {},
           "method": "host clock around synchronised calls, median of reps; inputs resident, results on the device",
           "kernel_times": "not collected (no rocprofv3 --kernel-trace --stats run)"}
    turn = np.eye(4)
    turn[:2, :2] = [[np.cos(np.radians(3.0)), -np.sin(np.radians(3.0))], [np.sin(np.radians(3.0)), np.cos(np.radians(3.0))]]
    turn[:3, 3] = (0.013, -0.02, 0.0)
    for name, share, T in (("overlap_0", 0.0, np.eye(4)), ("overlap_50", 0.5, np.eye(4)), ("overlap_100", 1.0, np.eye(4)), ("rotated_3deg", 1.0, turn)):
        k = int(round(share * n))
        lin_b = np.concatenate([lin[:n][rng.permutation(n)[:k]], free[:n - k]])[rng.permutation(n)]
        pos_b = cells_of(lin_b)
        dpb = DeviceArray.from_numpy(pos_b)
        case = {"shared_cells": k}
        case["move"] = stats(lib, lambda: ops.move_cells(dpb, GS, CS, VH, transform=T, device=True), a.reps, a.warmup)
        moved, inside = ops.move_cells(dpb, GS, CS, VH, transform=T, device=True)
        case["plan"] = stats(lib, lambda: ops.fuse_plan(dpa, dwa, moved, dwb, GS, VH, inside_b=inside), a.reps, a.warmup)
        plan = ops.fuse_plan(dpa, dwa, moved, dwb, GS, VH, inside_b=inside)
        view = ops.DeviceView(out.ptr, (plan.n_out, D), np.float32)
        case["rows"] = stats(lib, lambda: ops.fuse_rows(plan, dfa, dwa, dra, dfb, dwb, drb, feat_out=view, want_occupied=False, device=True),
                             a.reps, a.warmup)
        case["rows_occupied"] = stats(lib, lambda: ops.fuse_rows(plan, dfa, dwa, dra, dfb, dwb, drb, feat_out=view, device=True), a.reps, a.warmup)
        members = plan.n_sel_a + plan.n_sel_b
        nbytes = (members + plan.n_out) * D * 4
        k_rows = nbytes // (2 * D * 4)
        picks = DeviceArray.from_numpy(rng.integers(0, n, k_rows).astype(np.int64))
        dst = DeviceArray((k_rows, D), np.float32)
        case["gather"] = stats(lib, lambda: _lib.check(lib.avl_gather_rows(dfb.ptr, 4 * D, picks.ptr, k_rows, dst.ptr, None), "avl_gather_rows"),
                               a.reps, a.warmup)
        dst.free(), picks.free()
        case["rows"].update(n_out=plan.n_out, members=members, bytes=nbytes, TBps=nbytes / (case["rows"]["median_ms"] * 1e-3) / 1e12)
        case["rows"]["share_of_8TBps"] = case["rows"]["TBps"] / 8.0
        case["rows"]["share_of_gather"] = case["gather"]["median_ms"] / case["rows"]["median_ms"]
        case["gather"].update(rows=k_rows, TBps=nbytes / (case["gather"]["median_ms"] * 1e-3) / 1e12)
        case["counts"] = {key: int(v) for key, v in zip(ops.FUSE_COUNTS, plan.counts)}
        case["fuse_maps"] = stats(lib, lambda: ops.fuse_maps(dpa, dfa, dwa, dra, dpb, dfb, dwb, drb, GS, CS, VH, transform=T, want_occupied=False,
                                                             device=True), max(a.reps // 3, 1), 1)
        print(f"{name}: device side done", file=sys.stderr, flush=True)
        if name == "overlap_50" and a.numpy_reps > 0:
            got = ops.fuse_rows(plan, dfa, dwa, dra, dfb, dwb, drb, want_occupied=False)
            ts = []
            for _ in range(a.numpy_reps):
                t0 = time.perf_counter()
                want = numpy_fuse(pos_a, feat_a, w_a, rgb_a, pos_b, feat_b, w_b, rgb_b)
                ts.append((time.perf_counter() - t0) * 1e3)
                print(f"numpy run: {ts[-1]:.0f} ms", file=sys.stderr, flush=True)
            lin_out = (got[0][:, 0].astype(np.int64) * GS + got[0][:, 1]) * VH + got[0][:, 2]
            at = np.searchsorted(want[0], lin_out)
            same = bool(np.array_equal(want[0][at], lin_out) and len(lin_out) == len(want[0]) and np.array_equal(want[1][at], got[1])
                        and np.array_equal(want[2][at], got[2]) and np.array_equal(want[3][at], got[3]))
            assert same, "the NumPy fuse and the device disagree"
            case["numpy"] = {"median_ms": float(np.median(ts)), "reps": len(ts), "equal": same}
            device_ms = case["move"]["median_ms"] + case["plan"]["median_ms"] + case["rows"]["median_ms"]
            case["numpy"]["speedup_over_move_plan_rows"] = case["numpy"]["median_ms"] / device_ms
            del got, want
        res["cases"][name] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
