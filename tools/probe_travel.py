"""GPU box: time the travel-distance field, its decay map and the travel distribution-map chain (csrc/avl_travel.hip, the float32
gaussian of csrc/avl_morph2d.hip) against scipy.sparse.csgraph.dijkstra on the same box.  Prints one JSON object (and writes it to
--out).

    probe_travel.py [--reps 30] [--host-reps 3] [--warmup 3] [--out profiles/travel_probe.txt]

Crops of 300 x 400, 600 x 700 and 1000 x 1000 cells of a (1000, 1000) indoor-like obstacle map (indoor_map: rooms of 80 .. 180
cells between walls 2-3 cells thick, a 16-cell door in every wall segment, 120 furniture boxes of 8 .. 40 cells and 0.1 % salt
noise; all free cells of every crop are connected), two kinds of sources each:
  cell     one free cell, the free cell nearest to the crop's centre
  sofa     a 20 x 40 block of cells (1 m x 2 m at 5 cm) near the crop's centre, whose cells are obstacles as well as sources
  field_resident   ops.travel_field(device=True) on device-resident free and source images: the field alone, planes left on the device
  field_host       ops.travel_field on host arrays, both int32 planes copied back
  decay_resident   ops.travel_decay_2d(normalize=True, device=True) on the resident planes
  decay_host       the same with the float64 map copied back
  chain            ops.mask_smooth_2d(window=crop, device=True) on the device-resident full-map mask, ops.travel_field on its result
                   and the host's free crop, ops.travel_decay_2d(normalize=True) copied to the host: what
                   VLMap.get_travel_distribution_map does after the pooling (sofa sources only)
  host_dijkstra    scipy.sparse.csgraph.dijkstra(min_only=True) on the graph of legal steps with float64 weights 1 and sqrt(2)
  host_graph       building that graph with NumPy slices (not part of host_dijkstra)
Both paths end synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` (host:
`host_reps`) calls after `warmup`, with the minimum and maximum next to it.  `same` says that the device field has SciPy's reached
set and its distances within 1e-12 relative (SciPy adds float64 weights along the path, the field is exact).  `rounds` is the
number of rounds with an active tile, `launched` the number of round launches (batches of 8), `active_share` = tile runs /
(tiles x launched).  Kernel times and counters are not collected here (that needs a separate rocprofv3 --kernel-trace --stats run)."""
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


def indoor_map(gs, seed=0):
    """(gs, gs) bool, True = obstacle: see the head of the file"""
    rng = np.random.default_rng(seed)
    m = np.zeros((gs, gs), bool)
    m[:3] = m[-3:] = True
    m[:, :3] = m[:, -3:] = True

    def cuts():
        out, x = [0], 0
        while True:
            x += int(rng.integers(80, 180))
            if x > gs - 80:
                return out + [gs - 1]
            out.append(x)
    rows, cols = cuts(), cuts()
    for r in rows[1:-1]:
        t = int(rng.integers(2, 4))
        m[r:r + t] = True
        for ca, cb in zip(cols[:-1], cols[1:]):
            d = int(rng.integers(ca + 8, cb - 24))
            m[r:r + t, d:d + 16] = False
    for c in cols[1:-1]:
        t = int(rng.integers(2, 4))
        m[:, c:c + t] = True
        for ra, rb in zip(rows[:-1], rows[1:]):
            d = int(rng.integers(ra + 8, rb - 24))
            m[d:d + 16, c:c + t] = False
    for _ in range(120):
        h, w = int(rng.integers(8, 40)), int(rng.integers(8, 40))
        r, c = int(rng.integers(3, gs - h - 3)), int(rng.integers(3, gs - w - 3))
        m[r:r + h, c:c + w] = True
    return m | (rng.random((gs, gs)) < 0.001)


def legal_graph(free, src):
    """the CSR graph of legal steps u -> v (v free; u free or a source; a diagonal step with both edge-sharing cells free)"""
    H, W = free.shape
    idx = np.arange(H * W).reshape(H, W)
    start = free | src
    rows, cols, wts = [], [], []
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            ur = slice(max(0, -dr), H - max(0, dr))
            uc = slice(max(0, -dc), W - max(0, dc))
            vr = slice(max(0, dr), H - max(0, -dr))
            vc = slice(max(0, dc), W - max(0, -dc))
            ok = start[ur, uc] & free[vr, vc]
            if dr and dc:
                ok = ok & free[ur, vc] & free[vr, uc]
            rows.append(idx[ur, uc][ok])
            cols.append(idx[vr, vc][ok])
            wts.append(np.full(int(ok.sum()), np.sqrt(2.0) if dr and dc else 1.0))
    return coo_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W)).tocsr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    gs, rate = 1000, 0.1
    obstacles = indoor_map(gs)
    res = {"gs": gs, "method": "host clock around synchronised calls, median of reps", "decay_rate": rate, "tile": ops.TRAVEL_TILE,
           "sweep_cap": ops.TRAVEL_SWEEPS, "kernel_times": "not collected", "cases": {}}
    for H, W in ((300, 400), (600, 700), (1000, 1000)):
        r0, c0 = (gs - H) // 2, (gs - W) // 2
        tiles = -(-H // ops.TRAVEL_TILE) * -(-W // ops.TRAVEL_TILE)
        for kind in ("cell", "sofa"):
            free = ~obstacles[r0:r0 + H, c0:c0 + W]
            src = np.zeros((H, W), bool)
            if kind == "cell":
                cells = np.argwhere(free)
                r, c = cells[np.argmin(np.sum((cells - (H // 2, W // 2)) ** 2, axis=1))]
                src[r, c] = True
            else:
                src[H // 2 - 10:H // 2 + 10, W // 2 - 20:W // 2 + 20] = True
                free = free & ~src
            full = np.zeros((gs, gs), np.uint8)
            full[r0:r0 + H, c0:c0 + W] = src
            free_u8, src_u8 = free.astype(np.uint8), src.astype(np.uint8)
            dfree, dsrc, dfull = DeviceArray.from_numpy(free_u8), DeviceArray.from_numpy(src_u8), DeviceArray.from_numpy(full)
            field = ops.travel_field(dfree, dsrc, device=True)

            def field_resident():
                return ops.travel_field(dfree, dsrc, device=True)

            def field_host():
                return ops.travel_field(free_u8, src_u8)

            def decay_resident():
                return ops.travel_decay_2d(field, rate, normalize=True, device=True)

            def decay_host():
                return ops.travel_decay_2d(field, rate, normalize=True)

            def chain():
                mask = ops.mask_smooth_2d(dfull, 1, window=(r0, r0 + H, c0, c0 + W), device=True)
                return ops.travel_decay_2d(ops.travel_field(free_u8, mask, device=True), rate, normalize=True)

            graph = legal_graph(free, src)
            sources = np.flatnonzero(src.ravel())

            def host_dijkstra():
                return dijkstra(graph, directed=True, indices=sources, min_only=True)

            want = host_dijkstra().reshape(H, W)
            got = field.distance()
            reached = np.isfinite(want)
            same = bool(np.array_equal(reached, field.reachable())
                        and np.all(np.abs(got[reached] - want[reached]) <= 1e-12 * np.maximum(want[reached], 1.0)))
            assert same, (H, W, kind)
            launched = 8 * -(-field.rounds // 8)
            case = {"same": same, "sources": int(src.sum()), "free_cells": int(free.sum()), "reached": field.reached,
                    "longest_walk": float(got[reached].max()), "rounds": field.rounds, "launched": launched, "tiles": tiles,
                    "tile_runs": field.tile_runs, "active_share": field.tile_runs / float(tiles * launched),
                    "graph_edges": int(graph.nnz)}
            case["field_resident"] = stats(lib, field_resident, a.reps, a.warmup)
            case["field_host"] = stats(lib, field_host, a.reps, a.warmup)
            case["decay_resident"] = stats(lib, decay_resident, a.reps, a.warmup)
            case["decay_host"] = stats(lib, decay_host, a.reps, a.warmup)
            if kind == "sofa":
                case["chain"] = stats(lib, chain, a.reps, a.warmup)
            case["host_dijkstra"] = stats(lib, host_dijkstra, a.host_reps, 0)
            case["host_graph"] = stats(lib, lambda: legal_graph(free, src), a.host_reps, 0)
            res["cases"][f"{kind}_{H}x{W}"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
