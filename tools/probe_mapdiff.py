"""GPU box: time the comparison of two voxel maps (csrc/avl_mapdiff.hip through ops.map_diff) on two synthetic maps of 2 M voxels x
512 features, and a NumPy restatement of it (a dict join plus einsum) on the same box.  Prints one JSON object (and writes it to
--out).

    probe_mapdiff.py [--voxels 2000000] [--dim 512] [--reps 30] [--warmup 3] [--numpy-reps 3] [--radius 1] [--out PATH]

Map A: `voxels` distinct cells of a 1000 x 1000 x 30 grid with seeded float32 rows.  Map B: A with 5 % of the voxels moved by one
cell along one axis (rows kept), 2 % of the rows replaced by fresh ones, 2 % of the voxels removed and as many added in free cells,
then shuffled.  All inputs are resident (DeviceArrays) and the results stay on the device.
  index_a, index_b     ops.cell_index of either map
  match_ab             ops.match_cells, A against B's index
  row_dots_ab          ops.row_dots on that match: `share_of_8TBps` = 2 N D 4 bytes / time / 8e12 (unmatched rows read nothing, so the
                       bytes actually read are a few per cent fewer)
  status_ab            ops.diff_status
  map_diff             the whole call, both directions, indices given
  map_diff_with_index  the whole call building and closing both indices itself
  numpy                both directions of: a Python dict from linear cell to row, the centre cell first and the offsets ordered by
                       (d2, linear cell) for the rest, np.einsum for the three sums in float64, the predicate in NumPy -- the join
                       and the status are checked against the device's; the sums differ in their order of additions and are compared
                       to 1e-12 relative
Every path ends synchronised, so a host clock around each call is a valid time; every device figure is the median of `reps` calls
after `warmup`, with the minimum and maximum next to it; the NumPy figure is the median of --numpy-reps runs.  Kernel times were not
collected with rocprofv3 --kernel-trace --stats: the figures include the launch and the synchronisation (tens of microseconds)."""
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

GS, VH = 1000, 30


def rows(rng, n, D):
    out = np.empty((n, D), np.float32)
    for r0 in range(0, n, 1 << 16):                     # in pieces: no float64 temporary of the whole matrix
        out[r0:r0 + (1 << 16)] = rng.random((min(1 << 16, n - r0), D), dtype=np.float32) - np.float32(0.5)
    return out


def make_maps(n, D, seed=0):
    rng = np.random.default_rng(seed)
    n_add = n // 50
    lin = rng.choice(GS * GS * VH, n + n_add, replace=False)
    cells = np.stack(np.unravel_index(lin, (GS, GS, VH)), axis=1).astype(np.int32)
    pos_a, fresh = cells[:n], cells[n:]
    feat_a = rows(rng, n, D)
    who = rng.permutation(n)
    moved, replaced, removed = who[:n // 20], who[n // 20:n // 20 + n // 50], who[n // 20 + n // 50:n // 20 + 2 * (n // 50)]
    pos_b, feat_b = pos_a.copy(), feat_a.copy()
    axis, step = rng.integers(0, 3, len(moved)), rng.choice(np.array([-1, 1], np.int32), len(moved))
    pos_b[moved, axis] += step
    pos_b[:, :2] = np.clip(pos_b[:, :2], 0, GS - 1)
    pos_b[:, 2] = np.clip(pos_b[:, 2], 0, VH - 1)
    feat_b[replaced] = rows(rng, len(replaced), D)
    keep = np.ones(n, bool)
    keep[removed] = False
    pos_b, feat_b = np.concatenate([pos_b[keep], fresh]), np.concatenate([feat_b[keep], rows(rng, n_add, D)])
    perm = rng.permutation(len(pos_b))
    return pos_a, feat_a, np.ascontiguousarray(pos_b[perm]), np.ascontiguousarray(feat_b[perm])


def numpy_side(pos, feat, pos_o, feat_o, radius, t2):
    """one direction of the NumPy restatement -> (match, status, sums)"""
    lin_o = (pos_o[:, 0].astype(np.int64) * GS + pos_o[:, 1]) * VH + pos_o[:, 2]
    owner = dict(zip(lin_o.tolist(), range(len(lin_o))))                # ascending rows: the largest stays
    lin = ((pos[:, 0].astype(np.int64) * GS + pos[:, 1]) * VH + pos[:, 2]).tolist()
    match = np.fromiter((owner.get(c, -1) for c in lin), np.int32, len(lin))
    offs = sorted((dr * dr + dc * dc + dh * dh, (dr * GS + dc) * VH + dh, dr, dc, dh) for dr in range(-radius, radius + 1)
                  for dc in range(-radius, radius + 1) for dh in range(-radius, radius + 1) if (dr, dc, dh) != (0, 0, 0))
    for i in np.flatnonzero(match < 0).tolist():
        r, c, h = pos[i].tolist()
        for _, dl, dr, dc, dh in offs:                                  # ordered by (d2, linear cell): the first hit wins
            if 0 <= r + dr < GS and 0 <= c + dc < GS and 0 <= h + dh < VH:
                m = owner.get(lin[i] + dl, -1)
                if m >= 0:
                    match[i] = m
                    break
    ok = match >= 0
    sums = np.zeros((len(pos), 3))
    a, b = feat[ok], feat_o[match[ok]]
    sums[ok, 0] = np.einsum("ij,ij->i", a, b, dtype=np.float64)
    sums[ok, 1] = np.einsum("ij,ij->i", a, a, dtype=np.float64)
    sums[ok, 2] = np.einsum("ij,ij->i", b, b, dtype=np.float64)
    ab, aa, bb = sums.T
    status = np.where((aa > 0) & (bb > 0) & (ab > 0) & (ab * ab >= t2 * (aa * bb)), 0, 1).astype(np.uint8)
    status[~ok] = 2
    return match, status, sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-reps", type=int, default=3)
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    pos_a, feat_a, pos_b, feat_b = make_maps(a.voxels, a.dim)
    print(f"maps made: {len(pos_a)} and {len(pos_b)} voxels x {a.dim}", file=sys.stderr, flush=True)
    dpa, dfa, dpb, dfb = (DeviceArray.from_numpy(x) for x in (pos_a, feat_a, pos_b, feat_b))
    res = {"voxels_a": len(pos_a), "voxels_b": len(pos_b), "dim": a.dim, "grid": [GS, GS, VH], "radius": a.radius, "threshold": a.threshold,
           "method": "host clock around synchronised calls, median of reps; inputs resident, results on the device",
           "kernel_times": "not collected (no rocprofv3 --kernel-trace --stats run)"}
    res["index_a"] = stats(lib, lambda: ops.cell_index(dpa, GS, VH).close(), a.reps, a.warmup)
    res["index_b"] = stats(lib, lambda: ops.cell_index(dpb, GS, VH).close(), a.reps, a.warmup)
    with ops.cell_index(dpa, GS, VH) as ia, ops.cell_index(dpb, GS, VH) as ib:
        res["match_ab"] = stats(lib, lambda: ops.match_cells(ib, dpa, a.radius, device=True), a.reps, a.warmup)
        match, d2 = ops.match_cells(ib, dpa, a.radius, device=True)
        res["row_dots_ab"] = stats(lib, lambda: ops.row_dots(dfa, dfb, match, device=True), a.reps, a.warmup)
        nbytes = 2 * len(pos_a) * a.dim * 4
        res["row_dots_ab"]["bytes_2ND4"] = nbytes
        res["row_dots_ab"]["TBps"] = nbytes / (res["row_dots_ab"]["median_ms"] * 1e-3) / 1e12
        res["row_dots_ab"]["share_of_8TBps"] = res["row_dots_ab"]["TBps"] / 8.0
        sums = ops.row_dots(dfa, dfb, match, device=True)
        res["status_ab"] = stats(lib, lambda: ops.diff_status(match, sums, a.threshold, device=True), a.reps, a.warmup)
        res["map_diff"] = stats(lib, lambda: ops.map_diff(dpa, dfa, dpb, dfb, GS, VH, radius=a.radius, threshold=a.threshold, index_a=ia,
                                                          index_b=ib, device=True), a.reps, a.warmup)
        diff = ops.map_diff(dpa, dfa, dpb, dfb, GS, VH, radius=a.radius, threshold=a.threshold, index_a=ia, index_b=ib)
    res["map_diff_with_index"] = stats(lib, lambda: ops.map_diff(dpa, dfa, dpb, dfb, GS, VH, radius=a.radius, threshold=a.threshold, device=True),
                                       a.reps, a.warmup)
    res["counts_a"] = [int(c) for c in diff.a.counts]
    res["counts_b"] = [int(c) for c in diff.b.counts]
    print("device side done", file=sys.stderr, flush=True)
    ts, t2 = [], a.threshold * a.threshold
    for _ in range(max(a.numpy_reps, 0)):
        t0 = time.perf_counter()
        side_a = numpy_side(pos_a, feat_a, pos_b, feat_b, a.radius, t2)
        side_b = numpy_side(pos_b, feat_b, pos_a, feat_a, a.radius, t2)
        ts.append((time.perf_counter() - t0) * 1e3)
        print(f"numpy run: {ts[-1]:.0f} ms", file=sys.stderr, flush=True)
    if ts:
        res["numpy"] = {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "reps": len(ts)}
        res["numpy"]["speedup"] = res["numpy"]["median_ms"] / res["map_diff_with_index"]["median_ms"]
        same = True
        for side, (m, s, sums_np) in ((diff.a, side_a), (diff.b, side_b)):
            same = same and np.array_equal(side.match, m)
            ok = m >= 0
            close = np.allclose(side.sums[ok], sums_np[ok], rtol=1e-12, atol=0)
            # the status may differ only where the predicate sits within the sums' rounding of the threshold: count them
            res.setdefault("numpy_status_differs", []).append(int(np.count_nonzero(side.status != s)))
            same = same and bool(close)
        res["numpy_join_equal_and_sums_close"] = bool(same)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
