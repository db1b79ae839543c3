"""GPU box: time the visibility audit (csrc/avl_audit.hip) -- the cell index build and the two ray passes -- against a vectorised NumPy
restatement of the same walk on the same box.  Prints one JSON object (and writes it to --out).

    probe_audit.py [--reps 30] [--warmup 3] [--out profiles/audit_probe.txt]

720 x 1080 float32 depth frames of probe_explored.py's synthetic room, gs = 1000, cs = 0.05, vh = 30, stride 4 (48 600 rays per
frame), a synthetic map of 2.0 M voxels in distinct cells drawn uniformly from the grid (6.7 % of the cells: far denser along a ray
than a real map's surfaces, so more probes end in the prefix and permutation reads), batches of 1, 16 and 64 resident frames:
  index_build      ops.cell_index of the device-resident voxel list (memsets, bit set, count, scan, prefix, permutation)
  pass_a           ops.audit_rays with last_hit only, depth and outputs on the device: the kernel launches alone
  pass_b           ops.audit_rays with through and after = last_hit
  numpy_walk       the host path, both passes: back-projection, slab and end cells for all rays of a frame at once, then the 3-D walk
                   stepped for all rays together (one NumPy pass per step) against a dense id grid, frame by frame; once per batch
The NumPy path reproduces the kernel's explicit fma chains with an error-free product and sum (two_prod / two_sum), so the points
and with them every cell are the kernel's: `same` is asserted, after the JSON line has been printed.  Every device figure is the
median of `reps` synchronised calls after `warmup` (host clock), minimum and maximum next to it.
Run it a second time with AVLMAPS_HIP_LIB pointing at a variant built with -DAVL_AUDIT_PLAIN_ADD (tools/build_variant.py plain_add
--src avl_audit.hip -DAVL_AUDIT_PLAIN_ADD) for the other side of the through-add's A/B: a plain atomicAdd per lane."""
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
from probe_explored import CS, GS, H, K, STRIDE, W, frames  # noqa: E402
from probe_morph2d import stats  # noqa: E402

VH, N_VOXELS, END_MARGIN = 30, 2_000_000, 2
PARAMS = dict(stride=STRIDE, h_min=-CS, h_max=VH * CS, min_depth=0.1, max_depth=6.0)


def fma(a, b, c):
    """round(a * b + c) from an error-free product (Veltkamp / Dekker) and an error-free sum (Knuth)"""
    p = a * b
    sa, sb = 134217729.0 * a, 134217729.0 * b
    ah, bh = sa - (sa - a), sb - (sb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def numpy_walk(ids_grid, depth, Ts, ids, last_hit, through, after):
    """the walk of csrc/avl_audit.hip for whole frames at a time"""
    Kinv = np.linalg.inv(K)
    v, u = np.meshgrid(np.arange(STRIDE // 2, H, STRIDE), np.arange(STRIDE // 2, W, STRIDE), indexing="ij")
    x, y = u.ravel() + 0.5, v.ravel() + 0.5
    dirs = [fma(Kinv[i, 2], 1.0, fma(Kinv[i, 1], y, Kinv[i, 0] * x)) for i in range(3)]
    half = GS / 2
    cell = lambda w: (half - np.trunc(w / CS)).astype(np.int64)        # noqa: E731
    for f in range(len(depth)):
        T, fid = Ts[f], int(ids[f])
        O = T[:3, 3]
        z = depth[f][v.ravel(), u.ravel()].astype(np.float64)
        p = [d * z for d in dirs]
        ok = p[2] > PARAMS["min_depth"]
        far = p[2] >= PARAMS["max_depth"]
        with np.errstate(all="ignore"):
            s = PARAMS["max_depth"] / p[2]
            p = [np.where(far, q * s, q) for q in p]
            P = [fma(T[i, 3], 1.0, fma(T[i, 2], p[2], fma(T[i, 1], p[1], T[i, 0] * p[0]))) for i in range(3)]
            dz = P[2] - O[2]
            ta, tb = (PARAMS["h_min"] - O[2]) / dz, (PARAMS["h_max"] - O[2]) / dz
            level = dz == 0
            t0 = np.where(level, 0.0, np.maximum(0.0, np.minimum(ta, tb)))
            t1 = np.where(level, 1.0, np.minimum(1.0, np.maximum(ta, tb)))
            ok &= np.where(level, (O[2] >= PARAMS["h_min"]) & (O[2] <= PARAMS["h_max"]), t0 <= t1)
            ok &= np.isfinite(P[0]) & np.isfinite(P[1]) & np.isfinite(P[2])
            A = [np.where(t0 == 0, O[i], O[i] + t0 * (P[i] - O[i])) for i in range(3)]
            B = [np.where(t1 == 1, P[i], O[i] + t1 * (P[i] - O[i])) for i in range(3)]
            for w in A + B:
                ok &= np.isfinite(w)
        A, B = [np.where(ok, w, 0.0) for w in A], [np.where(ok, w, 0.0) for w in B]
        r, c, br, bc = cell(A[0]), cell(A[1]), cell(B[0]), cell(B[1])
        bhu = np.trunc(B[2] / CS).astype(np.int64)
        h, bh = np.clip(np.trunc(A[2] / CS).astype(np.int64), 0, VH - 1), np.clip(bhu, 0, VH - 1)
        ok &= (r >= 0) & (r < GS) & (c >= 0) & (c < GS) & (np.abs(br) <= 1 << 28) & (np.abs(bc) <= 1 << 28)
        has_end = ~far & (t1 == 1)
        is_hit = has_end & (bhu >= 0) & (bhu < VH) & (br >= 0) & (br < GS) & (bc >= 0) & (bc < GS)
        pos, end = [r, c, h], [br, bc, bh]
        d = [np.abs(end[i] - pos[i]) for i in range(3)]
        sg = [np.where(end[i] > pos[i], 1, -1) for i in range(3)]
        n = np.maximum(d[0], np.maximum(d[1], d[2]))
        e = [2 * d[i] - n for i in range(3)]
        below = np.where(has_end, n - END_MARGIN, np.iinfo(np.int64).max)
        live = ok.copy()
        k = 0
        while True:
            live &= (k <= n) & (pos[0] >= 0) & (pos[0] < GS) & (pos[1] >= 0) & (pos[1] < GS)
            if not live.any():
                break
            vox = np.full(live.shape, -1, np.int64)
            vox[live] = ids_grid[(pos[0][live] * GS + pos[1][live]) * VH + pos[2][live]]
            found = vox >= 0
            if last_hit is not None:
                hit = found & (k == n) & is_hit
                np.maximum.at(last_hit, vox[hit], fid)
            if through is not None:
                thr = found & (k < below)
                if after is not None:
                    thr[thr] = fid > after[vox[thr]]
                np.add.at(through, vox[thr], 1)
            for i in range(3):                                          # an axis with d == n steps every time under the one rule
                step = e[i] > 0
                pos[i] = pos[i] + np.where(step, sg[i], 0)
                e[i] = e[i] - np.where(step, 2 * n, 0) + 2 * d[i]
            k += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    depth, Ts = frames(64)
    rng = np.random.default_rng(1)
    lin = rng.choice(GS * GS * VH, N_VOXELS, replace=False)
    grid_pos = np.stack(np.unravel_index(lin, (GS, GS, VH)), axis=1).astype(np.int32)
    ids_grid = np.full(GS * GS * VH, -1, np.int32)
    ids_grid[lin] = np.arange(N_VOXELS, dtype=np.int32)
    dpos = DeviceArray.from_numpy(grid_pos)
    index = ops.cell_index(dpos, GS, VH)
    res = {"frame": [H, W], "gs": GS, "cs": CS, "vh": VH, "stride": STRIDE, "end_margin": END_MARGIN, "voxels": N_VOXELS,
           "index_bytes": index.nbytes, "rays_per_frame": len(range(2, H, 4)) * len(range(2, W, 4)),
           "library": os.environ.get("AVLMAPS_HIP_LIB") or "stock", "method": "host clock around synchronised calls, median of reps",
           "cases": {}}

    def build():
        ops.cell_index(dpos, GS, VH).close()
    res["cases"]["index_build"] = stats(lib, build, a.reps, a.warmup)
    ok = True
    for F in (1, 16, 64):
        d, T, ids = depth[:F], Ts[:F], np.arange(F)
        ddepth = DeviceArray.from_numpy(d)
        lh = DeviceArray.from_numpy(np.full(N_VOXELS, -1, np.int32))
        th = DeviceArray((N_VOXELS,), np.uint32).zero_()

        def pass_a():
            ops.audit_rays(index, ddepth, K, T, ids, CS, end_margin=END_MARGIN, last_hit=lh, **PARAMS)

        def pass_b():
            ops.audit_rays(index, ddepth, K, T, ids, CS, end_margin=END_MARGIN, through=th, after=lh, **PARAMS)
        pass_a()
        pass_b()
        got_lh, got_th = lh.numpy(), th.numpy()
        want_lh, want_th = np.full(N_VOXELS, -1, np.int32), np.zeros(N_VOXELS, np.uint32)
        t0 = time.perf_counter()
        numpy_walk(ids_grid, d, T, ids, want_lh, None, None)
        numpy_walk(ids_grid, d, T, ids, None, want_th, want_lh)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(got_lh, want_lh) and np.array_equal(got_th, want_th))
        ok &= same
        case = {"voxels_hit": int((got_lh >= 0).sum()), "voxels_seen_through": int((got_th > 0).sum()), "through_total": int(got_th.sum(dtype=np.int64)),
                "voxels_differing": int((got_lh != want_lh).sum() + (got_th != want_th).sum()), "same": same,
                "numpy_walk": {"mean_ms": host_ms, "reps": 1}}
        case["pass_a"] = stats(lib, pass_a, a.reps, a.warmup)
        case["pass_b"] = stats(lib, pass_b, a.reps, a.warmup)
        res["cases"][f"frames_{F}"] = case
        for x in (ddepth, lh, th):
            x.free()
    index.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    assert ok, "the device audit and the NumPy walk differ"


if __name__ == "__main__":
    main()
