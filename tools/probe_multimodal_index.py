"""GPU box: time the area / sound / image goal queries at the benchmark map's size (csrc/avl_field2d.hip), and the reference's
CPU loop for a few poses / segments, extrapolated.  Prints one JSON object (and writes it to --out).

    probe_multimodal_index.py [--reps 20] [--out profiles/multimodal_probe.json] [--cpu-samples 4]

area:  gs = 1000, F = 10 000 frame poses on a random-walk trajectory (a robot's path), 2 M voxels, decay 0.1 and 0.01 --
       the field kernel, the lift, and the (F x 768) @ (768,) score matmul (ops.sim_scores, float32-exact form)
sound: 300 segments x 1..20 locations along the same trajectory, decay 0.01
image: planar decay over 2 M voxels (float64)
Device time comes from events around `reps` back-to-back calls after a warm-up; run under rocprofv3 --kernel-trace --stats for
the per-kernel split."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402


def trajectory(rng, n, gs):
    """n cells of a random walk with 0.05 m steps at a 0.05 m grid: ~1 cell per frame, reflected at a 200-cell margin"""
    pts = np.empty((n, 2), np.float64)
    p = np.array([gs / 2, gs / 2], np.float64)
    heading = 0.0
    for i in range(n):
        heading += rng.normal(0, 0.15)
        p += [np.cos(heading), np.sin(heading)]
        for k in range(2):
            if p[k] < 200 or p[k] > gs - 200:
                heading += np.pi
                p[k] = min(max(p[k], 200), gs - 200)
        pts[i] = p
    return np.floor(pts).astype(np.int32)


def timed(lib, fn, reps):
    fn()
    _lib.check(lib.avl_device_sync())
    e0, e1 = _lib.C.c_void_p(), _lib.C.c_void_p()
    _lib.check(lib.avl_event_create(_lib.C.byref(e0)))
    _lib.check(lib.avl_event_create(_lib.C.byref(e1)))
    _lib.check(lib.avl_event_record(e0, None))
    for _ in range(reps):
        fn()
    _lib.check(lib.avl_event_record(e1, None))
    _lib.check(lib.avl_event_sync(e1))
    ms = _lib.C.c_float()
    _lib.check(lib.avl_event_elapsed_ms(e0, e1, _lib.C.byref(ms)))
    lib.avl_event_destroy(e0)
    lib.avl_event_destroy(e1)
    return ms.value / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-samples", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    gs, F, N, D = 1000, 10_000, 2_000_000, 768
    res = {"gs": gs, "frames": F, "voxels": N}

    lin = rng.choice(gs * gs * 30, size=N, replace=False)
    pos = DeviceArray.from_numpy(np.stack([lin // 30000, (lin // 30) % 1000, lin % 30], 1).astype(np.int32))
    cells = trajectory(rng, F, gs)
    feat = rng.standard_normal((F, D)).astype(np.float32)
    feat /= np.linalg.norm(feat, axis=1, keepdims=True)
    dfeat = DeviceArray.from_numpy(feat)
    q = rng.standard_normal((1, D)).astype(np.float32)
    scores = (feat @ q.T).ravel()
    peaks = ((scores - scores.min()) / (scores.max() - scores.min())).astype(np.float64)
    dcells, dpeaks = DeviceArray.from_numpy(cells), DeviceArray.from_numpy(peaks)

    res["area_scores_matmul_ms"] = timed(lib, lambda: ops.sim_scores(dfeat, q, want_scores=True, want_argmax=False, precision="exact"),
                                         a.reps)
    for decay in (0.1, 0.01):
        holder = {}

        def field():
            holder["gf"] = ops.area_field(dcells, dpeaks, gs, decay)
        res[f"area_field_ms_decay{decay}"] = timed(lib, field, a.reps)
        gf = holder["gf"]
        res[f"area_lift_ms_decay{decay}"] = timed(lib, lambda: ops.field_lift(gf, pos, 30), a.reps)
        res[f"area_field_plus_lift_ms_decay{decay}"] = res[f"area_field_ms_decay{decay}"] + res[f"area_lift_ms_decay{decay}"]

    S = 300
    seg_cells, counts = [], []
    for i in range(S):
        n = int(rng.integers(1, 21))
        start = int(rng.integers(0, F - 60))
        seg_cells.append(cells[start:start + 3 * n:3])
        counts.append(n)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    seg = np.concatenate(seg_cells)
    probs = rng.random(S).astype(np.float32)
    holder = {}

    def sfield():
        holder["gf"] = ops.sound_field(offsets, seg, probs, gs, 0.01)
    res["sound_segments"], res["sound_locations"] = S, int(len(seg))
    res["sound_field_ms_decay0.01"] = timed(lib, sfield, a.reps)
    sgf = holder["gf"]
    res["sound_lift_ms"] = timed(lib, lambda: ops.field_lift(sgf, pos, 30), a.reps)
    res["image_planar_decay_ms"] = timed(lib, lambda: ops.planar_decay(pos, 480, 512, 0.01), a.reps)

    # the reference's CPU loop, a few poses / segments, extrapolated (one EDT each on the full grid)
    from scipy.ndimage import distance_transform_edt
    k = a.cpu_samples
    D2 = np.zeros((gs, gs), np.float32)
    t0 = time.perf_counter()
    for i in range(k):
        tmp = np.zeros((gs, gs), np.float32)
        tmp[cells[i, 0], cells[i, 1]] = peaks[i]
        t = np.clip(np.ones((gs, gs)) * peaks[i] - distance_transform_edt(tmp == 0) * 0.1, 0, 1)
        D2 = np.where(D2 > t, D2, t)
    per_pose = (time.perf_counter() - t0) / k
    res["cpu_ref_area_s_per_pose"] = per_pose
    res["cpu_ref_area_s_extrapolated_10000_poses"] = per_pose * F
    t0 = time.perf_counter()
    for i in range(k):
        tmp = np.zeros((gs, gs), np.float32)
        for r, c in seg_cells[i]:
            tmp[r, c] = probs[i]
        d = distance_transform_edt(tmp == 0)
        t = np.ones((gs, gs), np.float32) * probs[i] - probs[i] * d * 0.01
        D2 += np.where(t < 0, 0, t)
    res["cpu_ref_sound_s_extrapolated_300_segments"] = (time.perf_counter() - t0) / k * S
    gp = np.stack([lin // 30000, (lin // 30) % 1000, lin % 30], 1).astype(np.int32)
    t0 = time.perf_counter()
    occ_rows = 200_000
    heat = np.zeros(occ_rows, np.float32)
    for i in range(occ_rows):                                         # the occupied_ids lift loop, 200 k voxels of it
        heat[i] = D2[gp[i, 0], gp[i, 1]]
    res["cpu_ref_lift_s_extrapolated_2M_voxels"] = (time.perf_counter() - t0) * (N / occ_rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
