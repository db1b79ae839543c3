"""GPU box: time the free-space carver and the frontier mask (csrc/avl_explore.hip) against a vectorised NumPy restatement of the same
walk on the same box.  Prints one JSON object (and writes it to --out).

    probe_explored.py [--reps 30] [--warmup 3] [--host-reps 3] [--out profiles/explored_probe.txt]

720 x 1080 float32 depth frames of a synthetic room (walls 2 - 5.5 m away, a band of pixels beyond max_depth), gs = 1000, cs = 0.05,
stride 4 (48 600 rays per frame), poses turning on the spot, batches of 1, 16 and 64 resident frames:
  carve_resident   ops.carve_free_space on depth, poses' map and frames already on the device: the kernel launches alone
  carve_fresh_map  the same into a map reset to "never seen" before every call (the reset is inside the time): every cell's first
                   visit pays its atomic, where carve_resident mostly ends at the read
  carve_upload     the same with the batch uploaded from a host array first (what Map.create_explored_map pays per batch)
  frontier_device  ops.frontier_mask on device-resident (1000, 1000) masks
  numpy_walk       the host path: back-projection, slab and end cells for all rays of a frame at once, then the Bresenham stepped for all
                   rays together (one NumPy pass per step), frame by frame; --host-reps calls only, it takes seconds
  frontier_numpy   the NumPy expression of the frontier on the host masks
`same` says the device map equals the NumPy walk's (the NumPy path multiplies and adds where the kernel has K1's fma chain: a last-bit
difference in a point can move an end cell, so `cells_differing` is reported rather than assumed zero).  Every device figure is the
median of `reps` synchronised calls after `warmup` (host clock), minimum and maximum next to it.
Run it a second time with AVLMAPS_HIP_LIB pointing at a variant built with -DAVL_CARVE_ALWAYS_ATOMIC (tools/build_variant.py
always_atomic --src avl_explore.hip -DAVL_CARVE_ALWAYS_ATOMIC) for the other side of the read-before-atomic A/B."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402

H, W, GS, CS, STRIDE = 720, 1080, 1000, 0.05, 4
PARAMS = dict(stride=STRIDE, h_min=0.0, h_max=1.5, min_depth=0.1, max_depth=6.0)
K = np.array([[540.0, 0, 540.0], [0, 540.0, 360.0], [0, 0, 1.0]])


def frames(n, seed=0):
    """(depth (n, H, W) float32, transforms (n, 4, 4)): a camera at 1.5 m turning 3 degrees per frame while drifting, in a room whose
    walls are 2 - 5.5 m away; the top rows see through a window (beyond max_depth)"""
    rng = np.random.default_rng(seed)
    u = (np.arange(W) + 0.5 - 540.0) / 540.0
    depth = np.empty((n, H, W), np.float32)
    Ts = np.zeros((n, 4, 4))
    for i in range(n):
        base = 3.75 + 1.75 * np.sin(3.0 * u + 0.4 * i)
        depth[i] = (base[None, :] + rng.uniform(-0.05, 0.05, (H, W))).astype(np.float32)
        depth[i, :40] = 9.0
        yaw = np.deg2rad(3.0 * i)
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])
        Ts[i, :3, :3] = R @ np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])
        Ts[i, :3, 3] = (0.02 * i, 0.01 * i, 1.5)
        Ts[i, 3, 3] = 1.0
    return depth, Ts


def numpy_walk(first_seen, depth, Ts, ids):
    """the walk of csrc/avl_explore.hip for whole frames at a time (plain products and sums where the kernel has fma)"""
    Kinv = np.linalg.inv(K)
    v, u = np.meshgrid(np.arange(STRIDE // 2, H, STRIDE), np.arange(STRIDE // 2, W, STRIDE), indexing="ij")
    pix = np.stack([u.ravel() + 0.5, v.ravel() + 0.5, np.ones(u.size)])
    dirs = Kinv @ pix
    flat = first_seen.reshape(-1).view(np.uint32)
    half = GS / 2
    cell = lambda x: (half - np.trunc(x / CS)).astype(np.int64)       # noqa: E731
    for f in range(len(depth)):
        T, fid = Ts[f], np.uint32(ids[f])
        O = T[:3, 3]
        orow, ocol = int(half - int(O[0] / CS)), int(half - int(O[1] / CS))
        if 0 <= orow < GS and 0 <= ocol < GS:
            flat[orow * GS + ocol] = min(flat[orow * GS + ocol], fid)
        p = dirs * depth[f][v.ravel(), u.ravel()].astype(np.float64)
        ok = p[2] > PARAMS["min_depth"]
        far = p[2] >= PARAMS["max_depth"]
        with np.errstate(all="ignore"):
            p = np.where(far, p * (PARAMS["max_depth"] / p[2]), p)
            P = T[:3, :3] @ p + O[:, None]
            dz = P[2] - O[2]
            ta, tb = (PARAMS["h_min"] - O[2]) / dz, (PARAMS["h_max"] - O[2]) / dz
            level = dz == 0
            t0 = np.where(level, 0.0, np.maximum(0.0, np.minimum(ta, tb)))
            t1 = np.where(level, 1.0, np.minimum(1.0, np.maximum(ta, tb)))
            ok &= np.where(level, (O[2] >= PARAMS["h_min"]) & (O[2] <= PARAMS["h_max"]), t0 <= t1) & np.all(np.isfinite(P), axis=0)
            ax, ay = np.where(t0 == 0, O[0], O[0] + t0 * (P[0] - O[0])), np.where(t0 == 0, O[1], O[1] + t0 * (P[1] - O[1]))
            bx, by = np.where(t1 == 1, P[0], O[0] + t1 * (P[0] - O[0])), np.where(t1 == 1, P[1], O[1] + t1 * (P[1] - O[1]))
            ok &= np.isfinite(ax) & np.isfinite(ay) & np.isfinite(bx) & np.isfinite(by)
        ax, ay, bx, by = (np.where(ok, w, 0.0) for w in (ax, ay, bx, by))
        r, c, br, bc = cell(ax), cell(ay), cell(bx), cell(by)
        ok &= (r >= 0) & (r < GS) & (c >= 0) & (c < GS)
        skip_end = ~far & (t1 == 1)
        dr, dc = np.abs(br - r), np.abs(bc - c)
        sr, sc = np.where(br > r, 1, -1), np.where(bc > c, 1, -1)
        err = dc - dr
        live = ok.copy()
        while live.any():
            live &= (r >= 0) & (r < GS) & (c >= 0) & (c < GS)
            at_end = (r == br) & (c == bc)
            mark = live & ~(at_end & skip_end)
            idx = r[mark] * GS + c[mark]
            flat[idx] = np.minimum(flat[idx], fid)
            live &= ~at_end
            e2 = 2 * err
            mc, mr = live & (e2 > -dr), live & (e2 < dc)
            err = err - np.where(mc, dr, 0) + np.where(mr, dc, 0)
            c = c + np.where(mc, sc, 0)
            r = r + np.where(mr, sr, 0)
    return first_seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    depth, Ts = frames(64)
    res = {"frame": [H, W], "gs": GS, "cs": CS, "stride": STRIDE, "rays_per_frame": len(range(2, H, 4)) * len(range(2, W, 4)),
           "library": os.environ.get("AVLMAPS_HIP_LIB") or "stock", "method": "host clock around synchronised calls, median of reps",
           "cases": {}}
    never = np.full((GS, GS), -1, np.int32)
    for F in (1, 16, 64):
        d, T, ids = depth[:F], Ts[:F], np.arange(F)
        ddepth = DeviceArray.from_numpy(d)
        dmap = DeviceArray.from_numpy(never)

        def carve_resident():
            ops.carve_free_space(dmap, ddepth, K, T, ids, GS, CS, device=True, **PARAMS)

        def carve_fresh_map():
            _lib.check(lib.avl_memset(dmap.ptr, 0xFF, dmap.nbytes, None), "avl_memset")
            ops.carve_free_space(dmap, ddepth, K, T, ids, GS, CS, device=True, **PARAMS)

        def carve_upload():
            ops.carve_free_space(dmap, DeviceArray.from_numpy(d), K, T, ids, GS, CS, device=True, **PARAMS)
        carve_resident()
        got = dmap.numpy()
        host_reps = a.host_reps if F == 1 else 1                         # seconds per frame: the longer batches are walked once
        t0 = time.perf_counter()
        for _ in range(host_reps):
            want = numpy_walk(never.copy(), d, T, ids)
        host_ms = (time.perf_counter() - t0) * 1e3 / host_reps
        case = {"cells_seen": int((got >= 0).sum()), "cells_differing": int((got != want).sum()), "same": bool(np.array_equal(got, want)),
                "numpy_walk": {"mean_ms": host_ms, "reps": host_reps}}
        case["carve_fresh_map"] = stats(lib, carve_fresh_map, a.reps, a.warmup)
        case["carve_resident"] = stats(lib, carve_resident, a.reps, a.warmup)
        case["carve_upload"] = stats(lib, carve_upload, a.reps, a.warmup)
        res["cases"][f"frames_{F}"] = case
        if F == 64:
            explored = got >= 0
            free = np.random.default_rng(1).random((GS, GS)) < 0.9
            dfree, dexp = DeviceArray.from_numpy(free.astype(np.uint8)), DeviceArray.from_numpy(explored.astype(np.uint8))

            def frontier_numpy():
                unknown = np.pad(~explored & free, 1)
                return free & explored & (unknown[:-2, 1:-1] | unknown[2:, 1:-1] | unknown[1:-1, :-2] | unknown[1:-1, 2:])
            fr = ops.frontier_mask(dfree, dexp)
            res["cases"]["frontier_1000x1000"] = {
                "frontier_cells": int(fr.sum()), "same": bool(np.array_equal(fr.astype(bool), frontier_numpy())),
                "frontier_device": stats(lib, lambda: ops.frontier_mask(dfree, dexp, device=True), a.reps, a.warmup),
                "frontier_numpy": stats(lib, frontier_numpy, a.reps, a.warmup)}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
