"""GPU box: time the three device steps of VLMap.get_objects (csrc/avl_objects.hip) against what the library could do before them: one
ops.label_voxels call per category.  Prints one JSON object (and writes it to --out).

    probe_objects.py [--reps 30] [--warmup 3] [--classes 16 40 64] [--out profiles/objects_<date>.txt]

probe_instances.py's synthetic map of about 2 M voxels in a 1000 x 1000 x 30 grid, in shuffled order.  The Q classes lie in compact
regions: the plane is cut into the Voronoi cells of 600 random sites, every site has a class, and a voxel's class is its column's.
scores (N, Q) float32 is noise below 0.5 plus 1 in the voxel's own class, so the row argmax is the class.  Positions, scores and
argmax are resident on the device before any clock starts.  Per Q:
  pick        ops.pick_columns(scores, argmax, device=True)
  label       ops.label_voxel_classes(pos, argmax, 26, scores=pick, device=True) and its table read back: two sorts, the union-find,
              the count read back, the three table passes
  pool        ops.pool_rows(scores, labels, n, device=True).  bytes = 4 N Q + 4 N (every score and every label once); hbm_fraction
              = bytes / time / 8 TB/s, the data-sheet bandwidth: a fraction, not a target
  one_pass    the three together, as get_objects runs them, and the sums read back
  per_class   for every class c: ops.mask_from_argmax(argmax, c), ops.label_voxels(pos, mask, 26, scores=column c, device=True) and
              its table read back, the columns resident as Q contiguous arrays -- Q box passes, sorts, union-finds and read-backs
`same` says that, class by class, the rows of the one-pass table in label order equal the per-class tables and best scores.
Every path ends synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_instances import GS, synthetic_map  # noqa: E402
from probe_morph2d import stats  # noqa: E402

SITES = 600
HBM_BYTES_PER_S = 8e12          # data sheet


def region_classes(pos, Q, seed):
    """(N,) int32: the class of the Voronoi cell (of SITES random sites, classes dealt in turn) that the voxel's column lies in"""
    rng = np.random.default_rng(seed)
    sites = rng.integers(0, GS, (SITES, 2))
    cls = (np.arange(SITES) % Q).astype(np.int32)
    _, nearest = cKDTree(sites).query(pos[:, :2])
    return cls[nearest]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--classes", type=int, nargs="+", default=[16, 40, 64])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    pos = synthetic_map()
    N = len(pos)
    dpos = DeviceArray.from_numpy(pos)
    res = {"voxels": int(N), "connectivity": 26, "sites": SITES, "pool_chunk": ops.POOL_CHUNK,
           "method": "host clock around synchronised calls, median of reps", "cases": {}}
    for Q in a.classes:
        rng = np.random.default_rng(Q)
        classes = region_classes(pos, Q, 100 + Q)
        scores = (rng.random((N, Q), dtype=np.float32) * np.float32(0.5))
        scores[np.arange(N), classes] += 1
        assert np.array_equal(np.argmax(scores, axis=1), classes)
        dscores, dam = DeviceArray.from_numpy(scores), DeviceArray.from_numpy(classes)
        dcols = [DeviceArray.from_numpy(np.ascontiguousarray(scores[:, c])) for c in range(Q)]

        def pick():
            return ops.pick_columns(dscores, dam, device=True)

        own = pick()

        def label():
            with ops.label_voxel_classes(dpos, dam, 26, scores=own, device=True) as vo:
                return vo.table

        keep = ops.label_voxel_classes(dpos, dam, 26, scores=own, device=True)

        def pool():
            return ops.pool_rows(dscores, keep.labels_dev, keep.n, device=True)

        def one_pass():
            with ops.label_voxel_classes(dpos, dam, 26, scores=pick(), device=True) as vo:
                return vo.table, vo.best_score, ops.pool_rows(dscores, vo.labels_dev, vo.n)

        def per_class():
            out = []
            for c in range(Q):
                with ops.label_voxels(dpos, ops.mask_from_argmax(dam, c), 26, scores=dcols[c], device=True) as inst:
                    out.append((inst.table, inst.best_score))
            return out

        table, best, _ = one_pass()
        owner = classes[table[:, 10]]
        same = all(np.array_equal(table[owner == c], t) and np.array_equal(best[owner == c], b) for c, (t, b) in enumerate(per_class()))
        assert same, "the one-pass objects differ from the per-class ones"
        case = {"objects": int(keep.n), "largest": int(table[:, 0].max()), "same": bool(same)}
        for name, fn in (("pick", pick), ("label", label), ("pool", pool), ("one_pass", one_pass), ("per_class", per_class)):
            case[name] = stats(lib, fn, a.reps, a.warmup)
        nbytes = 4 * N * Q + 4 * N
        case["pool"]["bytes"] = nbytes
        case["pool"]["hbm_fraction"] = nbytes / (case["pool"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S
        case["speedup"] = case["per_class"]["median_ms"] / case["one_pass"]["median_ms"]
        res["cases"][f"classes_{Q}"] = case
        keep.close()
        for d in [dscores, dam, own] + dcols:
            d.free()
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
