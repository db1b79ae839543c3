"""GPU box: time the backward resampling of a voxel map (csrc/avl_mappull.hip through ops.pull_plan, pull_rows, pull_map) on synthetic
maps of 2 M voxels x 512 features turned by 3 and by 45 degrees, against three yardsticks from the same run: the forward path on the
same inputs (ops.move_cells + fuse_plan + fuse_rows), the project's own avl_gather_rows moving as many output bytes, and a NumPy host
version on a smaller map, asserted equal.  Prints one JSON object (and writes it to --out).

    probe_mappull.py [--voxels 2000000] [--dim 512] [--reps 30] [--warmup 3] [--check-side 200] [--out PATH]

Two maps on the 1000 x 1000 x 30 grid share their rows, weights and colours.  `random`: probe_mapfuse.py's map, `voxels` distinct cells
drawn from the whole grid (7 % of the cells, no surfaces: in linear mode few cells reach the support and a voxel has one or two
members).  `slab`: a solid floor four cells thick, voxels / 4 cells per layer in a centred square (surfaces as a built map has them: a
voxel has up to eight members and neighbouring voxels share them).  All inputs are resident (DeviceArrays), the gathered rows are
written into a resident matrix made once.  Per map, angle (about the vertical axis, plus (0.013, -0.02, 0) m) and mode:
  plan_call     avl_map_pull_plan alone on buffers made once: the index of B, the dense marking pass over 30 M cells, the prefix
  fill_call     avl_map_pull_fill alone (with occupied_ids): the second dense pass
  pull_plan     ops.pull_plan: both calls, the read-back of n_out between them, the allocation of the plan's arrays
  rows          ops.pull_rows.  `bytes_once` = (rows of B that are a member of some voxel + n_out) * D * 4: what must be read once and
                written once; `share_of_8TBps` = bytes_once / time / 8e12.  `bytes_gathered` = (members + n_out) * D * 4: what the kernel
                asks for, the re-reads of shared members included; `gathered_TBps` is that over the time
  gather        avl_gather_rows of n_out random rows of map B: as many output bytes written, as many read.  The copy floor
  pull_map      the whole call on resident inputs, results on the device
and per map and angle `forward`: move_cells, fuse_plan (an empty map A) and fuse_rows of the same inputs, each timed.
Every path ends synchronised, so a host clock around each call is a valid time; every device figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it.  Kernel times and counters were not collected (no rocprofv3 run): the figures
include the launches, the read-back and the synchronisation."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from avlmaps_amd.ops.mappull import _scratch_i32  # noqa: E402
from probe_mapdiff import rows  # noqa: E402
from probe_morph2d import stats  # noqa: E402

GS, VH, CS = 1000, 30, 0.05


def turn(deg):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(np.radians(deg)), -np.sin(np.radians(deg))], [np.sin(np.radians(deg)), np.cos(np.radians(deg))]]
    T[:3, 3] = (0.013, -0.02, 0.0)
    return T


def _bracket(s):
    a = np.abs(s)
    small = a < 1.5
    b = a - 0.5
    f = np.floor(b)
    j0, u = np.where(small, 0.0, f), np.where(small, a / 1.5, b - f)
    k0 = np.where(s >= 0.0, j0, np.where(u == 0.0, -j0, -(j0 + 1.0)))
    return k0.astype(np.int64), np.where(s >= 0.0, u, np.where(u == 0.0, 0.0, 1.0 - u))


def numpy_pull(pos, feat, w, rgb, gs, cs, vh, P, interp, min_support):
    """-> (cells, members, lam, feat, weight, rgb) of the definition (include/avlmaps_hip.h section 32) in elementwise float64 NumPy, every
    row of the map selected and inside the grid"""
    owner = np.full(gs * gs * vh, -1, np.int64)
    owner[(pos[:, 0].astype(np.int64) * gs + pos[:, 1]) * vh + pos[:, 2]] = np.arange(len(pos))
    r, c, h = (v.ravel() for v in np.indices((gs, gs, vh)))
    kr, kc = gs // 2 - r, gs // 2 - c
    x, y, z = (kr + 0.5 * np.sign(kr)) * cs, (kc + 0.5 * np.sign(kc)) * cs, (h + 0.5) * cs
    qx, qy, qz = ((((P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z) + P[k, 3]) / cs for k in range(3))

    def probe(rr, cc, hh):
        ok = (rr >= 0) & (rr < gs) & (cc >= 0) & (cc < gs) & (hh >= 0) & (hh < vh)
        return np.where(ok, owner[np.where(ok, (rr * gs + cc) * vh + hh, 0)], -1)
    members, lam = np.full((len(r), 8), -1, np.int64), np.zeros((len(r), 8))
    if interp == "nearest":
        members[:, 0] = probe(np.trunc(gs / 2 - np.trunc(qx)).astype(np.int64), np.trunc(gs / 2 - np.trunc(qy)).astype(np.int64), np.trunc(qz).astype(np.int64))
        lam[:, 0] = members[:, 0] >= 0
    else:
        (kx, tx), (ky, ty) = _bracket(qx), _bracket(qy)
        sz = qz - 0.5
        h0, tz = np.floor(sz).astype(np.int64), sz - np.floor(sz)
        for j in range(8):
            dz, dy, dx = j & 1, j >> 1 & 1, j >> 2 & 1
            l = ((tx if dx else 1.0 - tx) * (ty if dy else 1.0 - ty)) * (tz if dz else 1.0 - tz)
            m = np.where(l > 0.0, probe(gs // 2 - (kx + dx), gs // 2 - (ky + dy), h0 + dz), -1)
            members[:, j], lam[:, j] = m, np.where(m >= 0, l, 0.0)
    support = np.zeros(len(r))
    for j in range(8):
        support = support + lam[:, j]                                   # + 0.0 for a corner that is no member
    keep = (support > 0.0) & (support >= min_support)
    members, lam, support = members[keep], lam[keep], support[keep]
    n = len(members)
    out_f, out_rgb, W = np.empty((n, feat.shape[1]), np.float32), np.empty((n, 3), np.uint8), np.zeros(n)
    om = lam * np.where(members >= 0, w.astype(np.float64)[np.maximum(members, 0)], 0.0)
    for j in range(8):
        W = W + om[:, j]
    for v0 in range(0, n, 8192):
        sl = slice(v0, min(n, v0 + 8192))
        acc, col, first = None, None, np.ones(sl.stop - sl.start, bool)
        for j in range(8):
            has = members[sl, j] >= 0
            rows_j = np.maximum(members[sl, j], 0)
            p, pc = om[sl, j, None] * feat[rows_j].astype(np.float64), om[sl, j, None] * rgb[rows_j].astype(np.float64)
            if acc is None:
                acc, col = np.where(has[:, None], p, 0.0), np.where(has[:, None], pc, 0.0)
            else:
                acc = np.where(has[:, None], np.where(first[:, None], p, acc + p), acc)
                col = np.where(has[:, None], np.where(first[:, None], pc, col + pc), col)
            first &= ~has
        out_f[sl], out_rgb[sl] = (acc / W[sl, None]).astype(np.float32), np.trunc(col / W[sl, None]).astype(np.uint8)
    cells = np.stack([r[keep], c[keep], h[keep]], axis=1).astype(np.int32)
    return cells, members.astype(np.int32), lam, out_f, (W / support).astype(np.float32), out_rgb


def check_against_numpy(side, D, rng):
    """both modes under both angles on a side x side x 10 grid: a slab and scattered voxels above it; -> the voxel counts"""
    vh = 10
    lo, hi = side // 5, side - side // 5
    slab = np.stack(np.meshgrid(np.arange(lo, hi), np.arange(lo, hi), np.arange(3, 5), indexing="ij"), -1).reshape(-1, 3)
    above = rng.choice(side * side * 4, side * side // 4, replace=False)
    above = np.stack(np.unravel_index(above, (side, side, 4)), axis=1) + [0, 0, 6]
    pos = np.concatenate([slab, above]).astype(np.int32)[rng.permutation(len(slab) + len(above))]
    n = len(pos)
    feat, w, rgb = rows(rng, n, D), rng.uniform(1, 30, n).astype(np.float32), rng.integers(0, 256, (n, 3)).astype(np.uint8)
    sizes = {}
    for deg in (3.0, 45.0):
        for interp in ops.PULL_INTERP:
            got = ops.pull_map(pos, feat, w, rgb, side, CS, vh, transform=turn(deg), interp=interp)
            want = numpy_pull(pos, feat, w, rgb, side, CS, vh, ops.inverse_transform(turn(deg), "probe"), interp, 0.5)
            for name, g, x in zip(("cells", "members", "lam", "feat", "weight", "rgb"),
                                  (got.grid_pos, got.members, got.lam, got.grid_feat, got.weight, got.grid_rgb), want):
                assert g.shape == x.shape and np.array_equal(g, x), f"the NumPy version and the device disagree: {deg} degrees, {interp}, {name}"
            sizes[f"{interp}_{deg:g}deg"] = int(got.n_out)
    return {"voxels": n, "grid": [side, side, vh], "n_out": sizes, "equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check-side", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    n, D = a.voxels, a.dim
    rng = np.random.default_rng(0)
    res = {"voxels": n, "dim": D, "grid": [GS, GS, VH], "maps": {},
           "method": "host clock around synchronised calls, median of reps; inputs resident, results on the device",
           "kernel_times": "not collected (no rocprofv3 run, no counters)"}
    if a.check_side > 0:
        res["numpy_check"] = check_against_numpy(a.check_side, D, rng)
        print(f"numpy check done: {res['numpy_check']}", file=sys.stderr, flush=True)
    feat, w, rgb = rows(rng, n, D), rng.uniform(1, 30, n).astype(np.float32), rng.integers(0, 256, (n, 3)).astype(np.uint8)
    dfb, dwb, drb = (DeviceArray.from_numpy(x) for x in (feat, w, rgb))
    del feat
    side = int(np.sqrt(n // 4))
    lo = (GS - side) // 2
    slab = np.stack(np.meshgrid(np.arange(lo, lo + side), np.arange(lo, lo + side), np.arange(2, 6), indexing="ij"), -1).reshape(-1, 3)
    strip = np.stack(np.unravel_index(np.arange(n - len(slab)), (GS, GS, 1)), axis=1) + [0, 0, 20]      # the remainder, high above the floor
    slab = np.concatenate([slab, strip])
    random = np.stack(np.unravel_index(rng.choice(GS * GS * VH, n, replace=False), (GS, GS, VH)), axis=1)
    empty = (np.zeros((0, 3), np.int32), np.zeros((0, D), np.float32), np.zeros((0,), np.float32), np.zeros((0, 3), np.uint8))
    ib = C.c_size_t(0)
    _lib.check(lib.avl_cell_index_work_bytes(n, GS, VH, C.byref(ib)), "avl_cell_index_work_bytes")
    si = _scratch_i32(n, GS, VH)
    index, scratch, head, counts = DeviceArray((ib.value,), np.uint8), DeviceArray((si,), np.int32), DeviceArray((8,), np.int32), DeviceArray((4,), np.int32)
    occ = DeviceArray((GS, GS, VH), np.int32)
    out = DeviceArray((int(2.2 * n), D), np.float32)
    shift = np.zeros(3, np.int32)
    for name, pos in (("random", random), ("slab", slab)):
        dpb = DeviceArray.from_numpy(pos.astype(np.int32)[rng.permutation(n)])
        res["maps"][name] = {}
        for deg in (3.0, 45.0):
            T = turn(deg)
            P = ops.inverse_transform(T, "probe")
            case = {}
            fwd = {"move": stats(lib, lambda: ops.move_cells(dpb, GS, CS, VH, transform=T, device=True), a.reps, a.warmup)}
            moved, inside = ops.move_cells(dpb, GS, CS, VH, transform=T, device=True)
            fwd["plan"] = stats(lib, lambda: ops.fuse_plan(empty[0], empty[2], moved, dwb, GS, VH, inside_b=inside), a.reps, a.warmup)
            fplan = ops.fuse_plan(empty[0], empty[2], moved, dwb, GS, VH, inside_b=inside)
            view = ops.DeviceView(out.ptr, (fplan.n_out, D), np.float32)
            fwd["rows"] = stats(lib, lambda: ops.fuse_rows(fplan, empty[1], empty[2], empty[3], dfb, dwb, drb, feat_out=view, want_occupied=False,
                                                           device=True), a.reps, a.warmup)
            fwd.update(n_out=fplan.n_out, total_ms=fwd["move"]["median_ms"] + fwd["plan"]["median_ms"] + fwd["rows"]["median_ms"])
            case["forward"] = fwd
            del fplan, moved, inside
            for mode, interp in enumerate(ops.PULL_INTERP):
                m = {}

                def plan_call():
                    _lib.check(lib.avl_map_pull_plan(dpb.ptr, None, dwb.ptr, n, P.ctypes.data, shift.ctypes.data, GS, CS, VH, mode, 0.5, index.ptr,
                                                     ib.value, scratch.ptr, si, head.ptr, None), "avl_map_pull_plan")
                m["plan_call"] = stats(lib, plan_call, a.reps, a.warmup)
                n_out = int(head.numpy()[0])
                cells, members, lam = DeviceArray((n_out, 3), np.int32), DeviceArray((n_out, 8), np.int32), DeviceArray((n_out, 8), np.float64)

                def fill_call():
                    _lib.check(lib.avl_map_pull_fill(n, P.ctypes.data, shift.ctypes.data, GS, CS, VH, mode, 0.5, index.ptr, ib.value, scratch.ptr, si,
                                                     head.ptr, n_out, cells.ptr, members.ptr, lam.ptr, occ.ptr, counts.ptr, None), "avl_map_pull_fill")
                m["fill_call"] = stats(lib, fill_call, a.reps, a.warmup)
                for d in (cells, members, lam):
                    d.free()
                m["pull_plan"] = stats(lib, lambda: ops.pull_plan(dpb, dwb, GS, CS, VH, transform=T, interp=interp), max(a.reps // 3, 1), 1)
                plan = ops.pull_plan(dpb, dwb, GS, CS, VH, transform=T, interp=interp, want_occupied=False)
                assert plan.n_out == n_out and plan.n_out <= int(2.2 * n)
                view = ops.DeviceView(out.ptr, (n_out, D), np.float32)
                m["rows"] = stats(lib, lambda: ops.pull_rows(plan, dfb, dwb, drb, feat_out=view, device=True), a.reps, a.warmup)
                k = int((plan.members >= 0).sum())
                used = n - int(plan.counts[0]) - int(plan.counts[1]) - int(plan.counts[3])
                once, asked = (used + n_out) * D * 4, (k + n_out) * D * 4
                picks = DeviceArray.from_numpy(rng.integers(0, n, max(n_out, 1)).astype(np.int64))
                m["gather"] = stats(lib, lambda: _lib.check(lib.avl_gather_rows(dfb.ptr, 4 * D, picks.ptr, n_out, out.ptr, None), "avl_gather_rows"),
                                    a.reps, a.warmup)
                picks.free()
                sec = m["rows"]["median_ms"] * 1e-3
                m["rows"].update(n_out=n_out, members=k, members_per_voxel=k / max(n_out, 1), rows_of_b_used=used, bytes_once=once, bytes_gathered=asked,
                                 once_TBps=once / sec / 1e12, share_of_8TBps=once / sec / 8e12, gathered_TBps=asked / sec / 1e12,
                                 share_of_gather=m["gather"]["median_ms"] / m["rows"]["median_ms"])
                m["gather"].update(rows=n_out, TBps=2 * n_out * D * 4 / (m["gather"]["median_ms"] * 1e-3) / 1e12)
                m["counts"] = {key: int(v) for key, v in zip(ops.PULL_COUNTS, plan.counts)}
                m["pull_map"] = stats(lib, lambda: ops.pull_map(dpb, dfb, dwb, drb, GS, CS, VH, transform=T, interp=interp, want_occupied=False,
                                                                device=True), max(a.reps // 3, 1), 1)
                case[interp] = m
                del plan
                print(f"{name} {deg:g} degrees {interp}: n_out {n_out}, rows {m['rows']['median_ms']:.3f} ms", file=sys.stderr, flush=True)
            res["maps"][name][f"{deg:g}deg"] = case
        dpb.free()
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
