"""GPU box: time the cost-weighted travel field and the layered costmap (csrc/avl_costfield.hip) beside the plain travel field
(csrc/avl_travel.hip) and against scipy.sparse.csgraph.dijkstra on the weighted graph, on the same box in the same process.
Prints one JSON object (and writes it to --out).

    probe_costfield.py [--reps 30] [--host-reps 3] [--warmup 3] [--out profiles/costfield_probe.txt]

The travel probe's three crops, 300 x 400, 600 x 700 and 1000 x 1000 cells of probe_travel.indoor_map(1000), one source each: the
cell nearest to the crop's centre that the default costmap leaves passable (a source inside the robot's radius of an obstacle could
not step off under that costmap).  Everything is device-resident (free map, sources, prices; planes left on the device), both
paths end synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` (host: `host_reps`)
calls after `warmup`, with the minimum and maximum next to it.
  (a) unit_price    travel_a, cost_one, travel_b: ops.travel_field, ops.cost_field with price 1 everywhere, ops.travel_field again,
                    three series one after the other.  The planes are asserted equal.  ratio = cost_one / mean(travel_a, travel_b);
                    travel_spread = |travel_a - travel_b| / their mean, what two series of the SAME call differ by.
  (b) inflated      ops.cost_field under the default inflation costmap (robot radius 3 cells, inflation radius 10 cells, scaling
                    0.25 per cell, peak 100: Map.get_costmap's defaults at 5 cm), with its rounds, launches and tile runs beside
                    the unit-price field's; passable = the free cells the costmap leaves passable.
  (c) costmap       ops.build_costmap(device=True) on resident distance planes with one layer (the inflation) and with three (two
                    avoidance layers of 40 boxes each, radius 6 cells, penalty 200); the EDTs that make the planes are timed apart
                    (edt_clearance).
  (d) host_dijkstra scipy.sparse.csgraph.dijkstra(min_only=True) on the graph of legal steps with float64 weights
                    price[v] and price[v] * sqrt(2) under the inflated costmap; host_graph: building that graph.  `same`: equal
                    reached sets and prices within 1e-9 relative, asserted.
Kernel times and counters are not collected here (that needs a separate rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402
from probe_travel import indoor_map  # noqa: E402


def priced_graph(passable, src, price):
    """the CSR graph of legal steps u -> v on the passable map, weighted with the price of the cell entered"""
    H, W = passable.shape
    idx = np.arange(H * W).reshape(H, W)
    start = passable | src
    rows, cols, wts = [], [], []
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            ur = slice(max(0, -dr), H - max(0, dr))
            uc = slice(max(0, -dc), W - max(0, dc))
            vr = slice(max(0, dr), H - max(0, -dr))
            vc = slice(max(0, dc), W - max(0, -dc))
            ok = start[ur, uc] & passable[vr, vc]
            if dr and dc:
                ok = ok & passable[ur, vc] & passable[vr, uc]
            rows.append(idx[ur, uc][ok])
            cols.append(idx[vr, vc][ok])
            wts.append(price[vr, vc][ok].astype(np.float64) * (np.sqrt(2.0) if dr and dc else 1.0))
    return coo_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W)).tocsr()


def boxes(H, W, seed, n=40):
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.uint8)
    for _ in range(n):
        h, w = int(rng.integers(4, 30)), int(rng.integers(4, 30))
        r, c = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        m[r:r + h, c:c + w] = 1
    return m


def schedule(field, tiles):
    launched = 8 * -(-field.rounds // 8)
    return {"rounds": field.rounds, "launched": launched, "tile_runs": field.tile_runs, "active_share": field.tile_runs / float(tiles * launched)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    gs = 1000
    obstacles = indoor_map(gs)
    inflation = ops.inflation_table(3.0, 10.0, 0.25)
    penalty = ops.penalty_table(6.0, 200)
    res = {"gs": gs, "method": "host clock around synchronised calls, median of reps", "tile": ops.TRAVEL_TILE, "sweep_cap": ops.TRAVEL_SWEEPS,
           "inflation": {"inscribed_cells": 3.0, "inflation_cells": 10.0, "scaling_per_cell": 0.25, "peak": 100},
           "kernel_times": "not collected", "counters": "not collected", "cases": {}}
    for H, W in ((300, 400), (600, 700), (1000, 1000)):
        r0, c0 = (gs - H) // 2, (gs - W) // 2
        tiles = -(-H // ops.TRAVEL_TILE) * -(-W // ops.TRAVEL_TILE)
        free = np.ascontiguousarray(~obstacles[r0:r0 + H, c0:c0 + W]).astype(np.uint8)
        dfree = DeviceArray.from_numpy(free)
        clearance = ops.distance_transform_edt(dfree, device=True)
        dcost = ops.build_costmap(dfree, [(clearance, inflation)], device=True)
        price = dcost.numpy()
        passable = (free != 0) & (price != 0)
        cells = np.argwhere(passable)
        r, c = cells[np.argmin(np.sum((cells - (H // 2, W // 2)) ** 2, axis=1))]
        src = np.zeros((H, W), np.uint8)
        src[r, c] = 1
        dsrc, done = DeviceArray.from_numpy(src), DeviceArray.from_numpy(np.ones((H, W), np.uint8))
        planes = [(clearance, inflation)] + [(ops.distance_to_mask(DeviceArray.from_numpy(boxes(H, W, s))), penalty) for s in (1, 2)]

        def travel():
            return ops.travel_field(dfree, dsrc, device=True)

        def cost_one():
            return ops.cost_field(dfree, done, dsrc, device=True)

        def inflated():
            return ops.cost_field(dfree, dcost, dsrc, device=True)

        t, u, f = travel(), cost_one(), inflated()
        assert np.array_equal(t.planes()[0], u.planes()[0]) and np.array_equal(t.planes()[1], u.planes()[1]), (H, W)
        case = {"tiles": tiles, "free_cells": int(free.sum()), "passable": int(passable.sum()), "source": [int(r), int(c)]}
        ta = stats(lib, travel, a.reps, a.warmup)
        cu = stats(lib, cost_one, a.reps, a.warmup)
        tb = stats(lib, travel, a.reps, a.warmup)
        mean = 0.5 * (ta["median_ms"] + tb["median_ms"])
        case["unit_price"] = {"travel_a": ta, "cost_one": cu, "travel_b": tb, "ratio": cu["median_ms"] / mean,
                              "travel_spread": abs(ta["median_ms"] - tb["median_ms"]) / mean, "planes_equal": True,
                              "reached": u.reached, "travel_schedule": schedule(t, tiles), "cost_schedule": schedule(u, tiles)}
        case["inflated"] = dict(stats(lib, inflated, a.reps, a.warmup), reached=f.reached, ratio_to_travel=None, **schedule(f, tiles))
        case["inflated"]["ratio_to_travel"] = case["inflated"]["median_ms"] / mean
        case["costmap"] = {"one_layer": stats(lib, lambda: ops.build_costmap(dfree, planes[:1], device=True), a.reps, a.warmup),
                           "three_layers": stats(lib, lambda: ops.build_costmap(dfree, planes, device=True), a.reps, a.warmup),
                           "edt_clearance": stats(lib, lambda: ops.distance_transform_edt(dfree, device=True), a.reps, a.warmup)}
        graph = priced_graph(passable, src != 0, price)
        sources = np.flatnonzero(src.ravel())

        def host_dijkstra():
            return dijkstra(graph, directed=True, indices=sources, min_only=True)

        want = host_dijkstra().reshape(H, W)
        got = f.cost()
        reached = np.isfinite(want)
        same = bool(np.array_equal(reached, f.reachable()) and np.all(np.abs(got[reached] - want[reached]) <= 1e-9 * np.maximum(want[reached], 1.0)))
        assert same, (H, W)
        case["host"] = {"same": same, "dearest_walk": float(got[reached].max()), "graph_edges": int(graph.nnz),
                        "host_dijkstra": stats(lib, host_dijkstra, a.host_reps, 0),
                        "host_graph": stats(lib, lambda: priced_graph(passable, src != 0, price), a.host_reps, 0)}
        res["cases"][f"{H}x{W}"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
