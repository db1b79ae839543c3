"""GPU box: time the 2-D viewshed (csrc/avl_viewshed.hip, ops.viewshed_gain / ops.viewshed_seen, Map.plan_exploration) against a
vectorised NumPy walk of the same pairs on the same box.  Prints one JSON object (and writes it to --out).

    probe_viewshed.py [--reps 30] [--warmup 3] [--host-eyes 8] [--gain-only] [--out profiles/viewshed_probe.txt]

Crops of 300 x 400, 600 x 700 and 1000 x 1000 cells of probe_travel.py's (1000, 1000) indoor-like obstacle map; explored is the half
of the crop above its anti-diagonal (row / H + col / W < 1).  The eyes are the known-free cells whose row and column are multiples
of 4 (Map.get_exploration_views' lattice, without frontier centres and without the reachability filter).  R = 60 and 127 cells.
  gain_resident   ops.viewshed_gain(device=True) on device-resident masks and eyes: the launch alone
  gain_host       the same call on host arrays, the (E, 8) table copied back
  seen_1, seen_64 ops.viewshed_seen(device=True) on resident masks for the first eye and for 64 eyes spread over the list
  tour_5          Map.plan_exploration(k=5) end to end on a Map whose obstacle crop is this crop, from the free cell nearest to its
                  centre, with max_range = R cells (R = 60 only: 127 cells at 5 cm exceed no limit, but one tour is enough)
  numpy           the walk stepped for all unknown in-range cells of one eye at once (one NumPy pass per step), on --host-eyes eyes
                  spread over the list, timed ONCE and scaled by the eye count (`numpy_scaled`: true)
`same` compares the device's gain rows with NumPy's on the eyes NumPy walked; it is asserted after the JSON line has been printed.
`walked_share` is, over those eyes, the share of window cells that were targets (unknown and in range).  Every device figure is the
median of `reps` synchronised calls after `warmup` (host clock), minimum and maximum next to it.  --gain-only times gain_resident
alone: the A/B of the LDS-staged walk against the walk that probes free / explored in global memory runs it twice,
    python tools/build_variant.py viewglobal --src avl_viewshed.hip -DAVL_VIEWSHED_GLOBAL_PROBE
    AVLMAPS_HIP_LIB=variants/libavlmaps_hip_viewglobal.so python tools/probe_viewshed.py --gain-only
Kernel times and counters are not collected here (that needs a separate rocprofv3 --kernel-trace --stats run)."""
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
from probe_travel import indoor_map  # noqa: E402

GS, CS = 1000, 0.05


def numpy_gain(free, explored, eye, radius):
    """(the gain row of one eye inside the image, its targets, its window cells): every unknown in-range cell walked at once"""
    H, W = free.shape
    er, ec = int(eye[0]), int(eye[1])
    r0, r1, c0, c1 = max(er - radius, 0), min(er + radius, H - 1), max(ec - radius, 0), min(ec + radius, W - 1)
    rr, cc = np.mgrid[r0:r1 + 1, c0:c1 + 1]
    unknown = free[r0:r1 + 1, c0:c1 + 1] & ~explored[r0:r1 + 1, c0:c1 + 1]
    pick = unknown & ((rr - er) ** 2 + (cc - ec) ** 2 <= radius * radius) & ((rr != er) | (cc != ec))
    tr, tc = rr[pick].astype(np.int64), cc[pick].astype(np.int64)
    dr, dc = np.abs(tr - er), np.abs(tc - ec)
    sr, sc = np.where(tr > er, 1, -1), np.where(tc > ec, 1, -1)
    n = np.maximum(dr, dc)
    e_r, e_c = 2 * dr - n, 2 * dc - n
    r, c = np.full(len(tr), er, np.int64), np.full(len(tr), ec, np.int64)
    alive = np.ones(len(tr), bool)
    blocking = ~free
    for k in range(1, int(n.max()) if len(n) else 0):
        step = e_r > 0
        r += np.where(step, sr, 0)
        e_r += 2 * dr - np.where(step, 2 * n, 0)
        step = e_c > 0
        c += np.where(step, sc, 0)
        e_c += 2 * dc - np.where(step, 2 * n, 0)
        inner = k < n
        alive &= ~(inner & blocking[np.where(inner, r, er), np.where(inner, c, ec)])
    sectors = ops.octant_of(tr[alive] - er, tc[alive] - ec)
    return np.bincount(sectors, minlength=8).astype(np.int32), int(pick.sum()), int(pick.size)


def synthetic_map(free, explored, r0, c0):
    """a VLMap without a scene directory whose obstacle crop is `free` placed at (r0, c0) of the (GS, GS) grid"""
    from avlmaps_amd.apps.common import load_config
    from avlmaps_amd.map import VLMap
    vm = VLMap(load_config(overrides={"map_config.grid_size": GS, "map_config.cell_size": CS}).map_config)
    occupied = -np.ones((GS, GS, 6), np.int32)
    H, W = free.shape
    wall = np.zeros((GS, GS), bool)
    wall[r0:r0 + H, c0:c0 + W] = ~free
    wall[r0, c0] = wall[r0 + H - 1, c0 + W - 1] = True                 # the crop is the bounding box of the obstacles
    occupied[wall, 2] = 1 + np.arange(int(wall.sum()))
    vm.occupied_ids = occupied
    seen = np.zeros((GS, GS), bool)
    seen[r0:r0 + H, c0:c0 + W] = explored
    vm.first_seen = np.where(seen, 0, -1).astype(np.int32)
    vm.generate_obstacle_map()
    return vm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-eyes", type=int, default=8)
    ap.add_argument("--gain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    obstacles = indoor_map(GS)
    res = {"gs": GS, "method": "host clock around synchronised calls, median of reps", "library": str(_lib.LIB_PATH.name),
           "stride": 4, "kernel_times": "not collected", "cases": {}}
    checks = []
    for H, W in ((300, 400), (600, 700), (1000, 1000)):
        r0, c0 = (GS - H) // 2, (GS - W) // 2
        free = ~obstacles[r0:r0 + H, c0:c0 + W]
        rr, cc = np.mgrid[0:H, 0:W]
        explored = rr / H + cc / W < 1.0
        known = free & explored
        lattice = np.zeros((H, W), bool)
        lattice[::4, ::4] = known[::4, ::4]
        eyes = np.argwhere(lattice).astype(np.int32)
        f8, x8 = free.astype(np.uint8), explored.astype(np.uint8)
        dfree, dexp, deyes = DeviceArray.from_numpy(f8), DeviceArray.from_numpy(x8), DeviceArray.from_numpy(eyes)
        spread = eyes[np.linspace(0, len(eyes) - 1, 64).astype(np.int64)]
        d1, d64 = DeviceArray.from_numpy(spread[:1]), DeviceArray.from_numpy(spread)
        vm = None if a.gain_only else synthetic_map(free, explored, r0, c0)
        for radius in (60, 127):
            case = {"eyes": int(len(eyes)), "explored_share": float(explored.mean()), "free_share": float(free.mean())}
            case["gain_resident"] = stats(lib, lambda: ops.viewshed_gain(dfree, dexp, deyes, radius, device=True), a.reps, a.warmup)
            if not a.gain_only:
                got = ops.viewshed_gain(dfree, dexp, deyes, radius)
                case["gain_sum"], case["gain_max"] = int(got.sum()), int(got.sum(1).max())
                case["gain_host"] = stats(lib, lambda: ops.viewshed_gain(f8, x8, eyes, radius), a.reps, a.warmup)
                case["seen_1"] = stats(lib, lambda: ops.viewshed_seen(dfree, dexp, d1, radius, device=True), a.reps, a.warmup)
                case["seen_64"] = stats(lib, lambda: ops.viewshed_seen(dfree, dexp, d64, radius, device=True), a.reps, a.warmup)
                if radius == 60:
                    cells = np.argwhere(known)
                    start = cells[np.argmin(np.sum((cells - (H // 2, W // 2)) ** 2, axis=1))] + (int(vm.rmin), int(vm.cmin))
                    start = [float(start[0]), float(start[1])]
                    tour = vm.plan_exploration(start, k=5, max_range=radius * CS + CS / 2)
                    case["tour_gains"] = [t[2] for t in tour]
                    case["tour_5"] = stats(lib, lambda: vm.plan_exploration(start, k=5, max_range=radius * CS + CS / 2),
                                           max(3, a.reps // 6), 1)
                pick = np.linspace(0, len(eyes) - 1, a.host_eyes).astype(np.int64)
                t0 = time.perf_counter()
                rows = [numpy_gain(free, explored, eyes[i], radius) for i in pick]
                dt = (time.perf_counter() - t0) * 1e3
                case["numpy"] = {"ms_scaled": dt * len(eyes) / len(pick), "ms_walked": dt, "eyes_walked": int(len(pick)), "numpy_scaled": True}
                case["walked_share"] = sum(r[1] for r in rows) / float(sum(r[2] for r in rows))
                case["same"] = bool(np.array_equal(np.stack([r[0] for r in rows]), got[pick]))
                checks.append((H, W, radius, case["same"]))
            res["cases"][f"{H}x{W}_R{radius}"] = case
            print(f"[probe_viewshed] {H}x{W} R={radius}: gain_resident {case['gain_resident']['median_ms']:.3f} ms", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    assert all(c[3] for c in checks), checks


if __name__ == "__main__":
    main()
