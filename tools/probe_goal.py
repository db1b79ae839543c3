"""GPU box: time the cross-modal goal (csrc/avl_goal.hip) at the benchmark map's size against the composition it replaces.
Prints one JSON object (and writes it to --out).

    probe_goal.py [--reps 30] [--warmup 3] [--out profiles/goal_probe.json]

Workload: 2 M voxels, gs = 1000, the four-term goal -- object heat (nearest-target decay of a 1 % mask, ops.HeatPlan), area field
from 10 000 poses, sound field from 300 segments, image cone -- on the synthetic inputs of probe_multimodal_index.py.
  host path   the four stand-alone queries as the public API returns them: each (N,) heat copied to the host, the float64 product
              and np.argmax in NumPy, grid_pos[argmax]
  fused path  the same term kernels, their outputs left on the device, one ops.goal_fuse; with want_heat the (N,) float64 product
              is also copied to the host, as AVLMap.index_goal returns it
Both paths start from the same device-resident inputs and end synchronised, so a host clock around each call is a valid time; every
figure is the median of `reps` calls after `warmup`, with the minimum and maximum next to it.  The text towers and the object score
matmul run before either path in the same way and are not part of this probe.  Run under rocprofv3 --kernel-trace --stats for the
per-kernel times."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_multimodal_index import trajectory  # noqa: E402

HBM_PEAK_BPS = 8.0e12


def stats(lib, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        _lib.check(lib.avl_device_sync())
        t0 = time.perf_counter()
        fn()
        _lib.check(lib.avl_device_sync())
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--voxels", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    gs, vh, F, N, S = 1000, 30, 10_000, a.voxels, 300
    res = {"gs": gs, "voxels": N, "frames": F, "sound_segments": S, "method": "host clock around synchronised calls, median of reps"}

    lin = rng.choice(gs * gs * vh, size=N, replace=False)
    gp = np.stack([lin // (gs * vh), (lin // vh) % gs, lin % vh], 1).astype(np.int32)
    pos = DeviceArray.from_numpy(gp)
    cells = trajectory(rng, F, gs)
    peaks = rng.random(F)
    dcells, dpeaks = DeviceArray.from_numpy(cells), DeviceArray.from_numpy(peaks)
    seg_cells, counts = [], []
    for _ in range(S):
        n = int(rng.integers(1, 21))
        start = int(rng.integers(0, F - 60))
        seg_cells.append(cells[start:start + 3 * n:3])
        counts.append(n)
    offsets, seg = np.concatenate([[0], np.cumsum(counts)]), np.concatenate(seg_cells)
    probs = rng.random(S).astype(np.float32)
    mask = DeviceArray.from_numpy((rng.random(N) < 0.01).astype(np.uint8))
    plan = ops.HeatPlan(pos)
    img_cell = (480, 512)

    def terms_on_device():
        obj = plan(mask, 0.05, 0.1)
        area = ops.area_field(dcells, dpeaks, gs, 0.1)
        sound = ops.sound_field(offsets, seg, probs, gs, 0.01)
        return obj, area, sound

    def goal_terms(obj, area, sound):
        return [ops.GoalTerm.dense(obj), ops.GoalTerm.field(area, vh), ops.GoalTerm.field(sound, vh),
                ops.GoalTerm.cones(np.array([img_cell], np.int32), np.ones(1), 0.01)]

    def host_path():
        obj, area, sound = terms_on_device()
        parts = [obj.numpy(), ops.field_lift(area, pos, vh).numpy(), ops.field_lift(sound, pos, vh).numpy(),
                 ops.planar_decay(pos, img_cell[0], img_cell[1], 0.01).numpy()]
        heat = parts[0].astype(np.float64)
        for p in parts[1:]:
            heat = heat * p.astype(np.float64)
        idx = int(np.argmax(heat))
        return heat, idx, gp[idx]

    def fused_path(want_heat):
        r = ops.goal_fuse(goal_terms(*terms_on_device()), pos, want_heat=want_heat)
        return (r.heat.numpy() if want_heat else None), r.index, r.pos

    # the two paths give the same answer, bit for bit
    h0, i0, p0 = host_path()
    h1, i1, p1 = fused_path(True)
    _, i2, p2 = fused_path(False)
    res["same_answer"] = bool(np.array_equal(h0, h1) and i0 == i1 == i2 and p0.tolist() == p1.tolist() == p2.tolist())
    res["goal_voxel"], res["goal_value"] = i1, float(h1[i1])

    res["host_path"] = stats(lib, host_path, a.reps, a.warmup)
    res["fused_path_with_heat_copy"] = stats(lib, lambda: fused_path(True), a.reps, a.warmup)
    res["fused_path_no_heat"] = stats(lib, lambda: fused_path(False), a.reps, a.warmup)

    # where the time goes
    obj, area, sound = terms_on_device()
    terms = goal_terms(obj, area, sound)
    res["object_heat"] = stats(lib, lambda: plan(mask, 0.05, 0.1), a.reps, a.warmup)
    res["area_field"] = stats(lib, lambda: ops.area_field(dcells, dpeaks, gs, 0.1), a.reps, a.warmup)
    res["sound_field"] = stats(lib, lambda: ops.sound_field(offsets, seg, probs, gs, 0.01), a.reps, a.warmup)
    res["fuse_with_heat"] = stats(lib, lambda: ops.goal_fuse(terms, pos, want_heat=True), a.reps, a.warmup)
    res["fuse_no_heat"] = stats(lib, lambda: ops.goal_fuse(terms, pos, want_heat=False), a.reps, a.warmup)
    res["host_lifts_and_image_kernels"] = stats(lib, lambda: (ops.field_lift(area, pos, vh), ops.field_lift(sound, pos, vh),
                                                               ops.planar_decay(pos, img_cell[0], img_cell[1], 0.01)), a.reps, a.warmup)
    d32, d64 = DeviceArray((N,), np.float32), DeviceArray((N,), np.float64)
    res["host_copies_3xf32_1xf64"] = stats(lib, lambda: (d32.numpy(), d32.numpy(), d32.numpy(), d64.numpy()), a.reps, a.warmup)
    res["heat_copy_f64"] = stats(lib, lambda: d64.numpy(), a.reps, a.warmup)
    parts = [np.asarray(rng.random(N), np.float32) for _ in range(3)] + [rng.random(N)]

    def numpy_product():
        heat = parts[0].astype(np.float64)
        for p in parts[1:]:
            heat = heat * p.astype(np.float64)
        return int(np.argmax(heat))
    res["host_numpy_product_argmax"] = stats(lib, numpy_product, a.reps, a.warmup)

    # bytes the fused kernel must move through HBM (the fields are L2 traffic); rates against the kernel time come from the trace
    res["fuse_bytes_no_heat"] = N * (12 + 4)
    res["fuse_bytes_with_heat"] = N * (12 + 4 + 8)
    res["hbm_peak_bytes_per_s"] = HBM_PEAK_BPS
    res["fuse_floor_us_no_heat"] = res["fuse_bytes_no_heat"] / HBM_PEAK_BPS * 1e6
    res["fuse_floor_us_with_heat"] = res["fuse_bytes_with_heat"] / HBM_PEAK_BPS * 1e6
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
