"""GPU box: time ops.object_relations (csrc/avl_relations.hip) on the inventory of a 2 M-voxel map against the host path on the same
box, and count the atomics a voxel issues.  Prints one JSON object (and writes it to --out).

    probe_relations.py [--reps 30] [--warmup 3] [--radii 2 5 10] [--classes 40] [--host-pairs 20000000] [--out profiles/relations_<date>.txt]

probe_objects.py's synthetic map (about 2 M voxels in a 1000 x 1000 x 30 grid, shuffled, one voxel per cell) and its inventory: the
classes are the Voronoi regions of 600 sites, the objects ops.label_voxel_classes' at connectivity 26.  Positions, labels and the
cell index are resident on the device before any clock starts.  Per radius R (cells):
  gpu         ops.object_relations(index, pos, labels, n, R): the scan, the finish, the count read back and the (P, 8) table read
              back; the median of `reps` calls after `warmup`, host clock around synchronised calls
  index       ops.cell_index(pos, gs, vh) alone, which get_scene_graph pays once per call
  host        labels and cells copied back (timed apart: copy_back), scipy.spatial.cKDTree.query_pairs(R) on the labelled cells and
              a NumPy reduction per pair (minimum d2, contacts, the two support counts); one run, not a median.  When the pairs of
              the whole map would exceed --host-pairs (estimated from 2 000 sampled voxels), the tree of every k-th object's
              voxels is matched against the tree of all of them (sparse_distance_matrix) and the time is scaled by
              labelled voxels / matched voxels: host_scaled says so, and host_voxels how many were matched
  same        the host's P, d2 and counts equal the GPU's table (for a scaled run: on the pairs of the matched objects)
  atomics     counted on the host for every 64th labelled voxel, by walking the kernel's offset order (dr, dc, then dh upwards):
              flushes = the times a lane hands a pair's registers to the table (one 64-bit atomicMin at most, issued only when it
              lowers the slot), counter_atomics = the integer atomicAdds of those flushes (a counter that is zero is skipped),
              both per labelled voxel; floor_wall gives the same two figures for the voxels of the pair with the most contacts"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_instances import GS, VH, synthetic_map  # noqa: E402
from probe_morph2d import stats  # noqa: E402
from probe_objects import region_classes  # noqa: E402


def reduce_pairs(pos, labels, n, i, j, both_sides):
    """{(lo, hi): [d2, lo_on_hi, hi_on_lo, contacts]} of the voxel pairs (i, j); both_sides: every unordered voxel pair is listed once
    (query_pairs) and stands for the two events of the definition"""
    a, b = labels[i], labels[j]
    keep = a != b
    i, j, a, b = i[keep], j[keep], a[keep], b[keep]
    d = pos[j].astype(np.int64) - pos[i]
    d2 = (d * d).sum(1)
    lo, hi = np.minimum(a, b).astype(np.int64), np.maximum(a, b)
    key = lo * (n + 1) + hi
    uniq, inv = np.unique(key, return_inverse=True)
    best = np.full(len(uniq), 1 << 60, np.int64)
    np.minimum.at(best, inv, d2)
    w = 2 if both_sides else 1
    contacts = np.bincount(inv, weights=(d2 <= 3) * w, minlength=len(uniq)).astype(np.int64)
    column = (d[:, 0] == 0) & (d[:, 1] == 0)
    # i above j (dh = -1 from i): i's object lies on j's; with both_sides the pair also stands for j scanning upwards, which is no event
    i_on_j, j_on_i = column & (d[:, 2] == -1), column & (d[:, 2] == 1) & both_sides
    lo_on_hi = np.bincount(inv, weights=(i_on_j & (a < b)) | (j_on_i & (b < a)), minlength=len(uniq)).astype(np.int64)
    hi_on_lo = np.bincount(inv, weights=(i_on_j & (a > b)) | (j_on_i & (b > a)), minlength=len(uniq)).astype(np.int64)
    return {(int(k // (n + 1)), int(k % (n + 1))): [int(best[t]), int(lo_on_hi[t]), int(hi_on_lo[t]), int(contacts[t])] for t, k in enumerate(uniq)}


def host_path(pos_all, labels_all, n, R, budget, rng):
    """-> (pairs dict, seconds, scaled, matched voxels, matched objects or None)"""
    part = np.flatnonzero((labels_all >= 1) & (labels_all <= n))
    pos, labels = pos_all[part], labels_all[part]
    t0 = time.perf_counter()
    tree = cKDTree(pos)
    sample = rng.choice(len(pos), min(2000, len(pos)), replace=False)
    per_voxel = float(np.mean(tree.query_ball_point(pos[sample], R, return_length=True))) - 1.0
    estimate = per_voxel * len(pos) / 2
    if estimate <= budget:
        ij = tree.query_pairs(R + 1e-6, output_type="ndarray")              # (|d|^2 is an integer: nothing lies between R and R + 1e-6)
        pairs = reduce_pairs(pos, labels, n, ij[:, 0], ij[:, 1], True)
        return pairs, time.perf_counter() - t0, False, len(pos), None
    k = int(np.ceil(2 * estimate / budget))
    chosen = np.arange(1, n + 1, k)
    t0 = time.perf_counter()                                                 # the tree of all voxels is built inside the clock again
    tree = cKDTree(pos)
    sub = np.flatnonzero(np.isin(labels, chosen))
    m = cKDTree(pos[sub]).sparse_distance_matrix(tree, R + 1e-6, output_type="coo_matrix")
    pairs = reduce_pairs(pos, labels, n, sub[m.row], m.col.astype(np.int64), False)
    seconds = (time.perf_counter() - t0) * len(pos) / max(len(sub), 1)
    return pairs, seconds, True, len(sub), set(chosen.tolist())


def count_atomics(pos, labels, n, R, rows):
    """(flushes, counter atomics) of every voxel of `rows`, by the kernel's walk"""
    owner = np.full((GS + 2 * R, GS + 2 * R, VH + 2 * R), -1, np.int32)
    owner[pos[:, 0] + R, pos[:, 1] + R, pos[:, 2] + R] = np.arange(len(pos), dtype=np.int32)       # one voxel per cell
    p, a = pos[rows].astype(np.int64) + R, labels[rows]
    last = np.zeros(len(rows), np.int64)
    on, contacts = np.zeros(len(rows), bool), np.zeros(len(rows), bool)
    flushes, adds = np.zeros(len(rows), np.int64), np.zeros(len(rows), np.int64)
    for dr in range(-R, R + 1):
        for dc in range(-R, R + 1):
            for dh in range(-R, R + 1):
                d2 = dr * dr + dc * dc + dh * dh
                if d2 > R * R:
                    continue
                j = owner[p[:, 0] + dr, p[:, 1] + dc, p[:, 2] + dh]
                b = np.where(j >= 0, labels[np.maximum(j, 0)], 0)
                ev = (b >= 1) & (b <= n) & (b != a)
                change = ev & (b != last)
                out = change & (last != 0)
                flushes += out
                adds += out * (on.astype(np.int64) + contacts)
                on[change], contacts[change] = False, False
                last[change] = b[change]
                if (dr, dc, dh) == (0, 0, -1):
                    on |= ev
                if 1 <= d2 <= 3:
                    contacts |= ev
    end = last != 0
    return flushes + end, adds + end * (on.astype(np.int64) + contacts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radii", type=int, nargs="+", default=[2, 5, 10])
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--host-pairs", type=int, default=20_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    pos = synthetic_map()
    N = len(pos)
    classes = region_classes(pos, a.classes, 100 + a.classes)
    dpos = DeviceArray.from_numpy(pos)
    vo = ops.label_voxel_classes(dpos, DeviceArray.from_numpy(classes), 26, device=True)
    n = vo.n
    res = {"voxels": int(N), "gs": GS, "vh": VH, "classes": a.classes, "objects": int(n),
           "method": "host clock around synchronised calls, median of reps; the host path is one run", "cases": {}}

    def build_index():
        ops.cell_index(dpos, GS, VH).close()

    res["index"] = stats(lib, build_index, a.reps, a.warmup)
    t0 = time.perf_counter()
    labels, cells = vo.labels_dev.numpy(), dpos.numpy()
    res["copy_back_ms"] = (time.perf_counter() - t0) * 1e3
    labelled = np.flatnonzero((labels >= 1) & (labels <= n))
    rng = np.random.default_rng(1)
    with ops.cell_index(dpos, GS, VH) as index:
        for R in a.radii:
            def gpu():
                return ops.object_relations(index, dpos, vo.labels_dev, n, R)

            rel = gpu()
            case = {"pairs": int(rel.P), "gpu": stats(lib, gpu, a.reps, a.warmup)}
            print(f"R = {R}: P = {rel.P}, gpu {case['gpu']['median_ms']:.3f} ms", file=sys.stderr, flush=True)
            pairs, seconds, scaled, matched, chosen = host_path(cells, labels, n, R, a.host_pairs, rng)
            case.update(host_ms=seconds * 1e3, host_scaled=bool(scaled), host_voxels=int(matched), labelled_voxels=int(len(labelled)))
            table = rel.table if chosen is None else rel.table[np.isin(rel.table[:, 0], list(chosen)) | np.isin(rel.table[:, 1], list(chosen))]
            if chosen is not None:                       # the matched objects scanned, the others were only seen: the counts are one side's
                got = {(int(r[0]), int(r[1])): [int(r[2])] for r in table}
                pairs = {k: v[:1] for k, v in pairs.items()}
            else:
                got = {(int(r[0]), int(r[1])): [int(r[2]), int(r[5]), int(r[6]), int(r[7])] for r in table}
            case["same"] = bool(got == pairs)
            case["speedup"] = case["host_ms"] / case["gpu"]["median_ms"]
            print(f"R = {R}: host {case['host_ms']:.0f} ms (scaled: {scaled}), same: {case['same']}", file=sys.stderr, flush=True)
            rows = labelled[::64]
            flushes, adds = count_atomics(cells, labels, n, R, rows)
            case["atomics"] = {"sampled_voxels": int(len(rows)), "flushes_per_voxel": float(flushes.mean()),
                               "counter_atomics_per_voxel": float(adds.mean()), "voxels_without_a_flush": float((flushes == 0).mean())}
            top = rel.table[np.argmax(rel.table[:, 7])] if rel.P else None
            if top is not None:
                mine = np.isin(labels[rows], top[:2])
                case["atomics"]["floor_wall"] = {"pair": [int(top[0]), int(top[1])], "contacts": int(top[7]), "sampled_voxels": int(mine.sum()),
                                                 "flushes_per_voxel": float(flushes[mine].mean()) if mine.any() else 0.0,
                                                 "counter_atomics_per_voxel": float(adds[mine].mean()) if mine.any() else 0.0}
            print(f"R = {R}: atomics {case['atomics']}", file=sys.stderr, flush=True)
            res["cases"][f"radius_{R}"] = case
    vo.close()
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
