"""GPU box: time the room segmentation and its parts (csrc/avl_rooms.hip over csrc/avl_edt2d.hip, avl_islands.hip and
avl_travel.hip) against the host chain of SciPy on the same box.  Prints one JSON object (and writes it to --out).

    probe_rooms.py [--reps 30] [--host-reps 3] [--warmup 3] [--radius 9] [--min-seed-cells 100] [--out profiles/rooms_probe.txt]

Crops of 300 x 400, 600 x 700 and 1000 x 1000 cells of probe_travel.indoor_map (rooms of 80 .. 180 cells between walls 2-3 cells
thick, a 16-cell door in every wall segment, 120 furniture boxes, 0.1 % salt noise).  radius = 9 cells is a door width of 0.9 m at
5 cm: it closes the map's 16-cell doors, and the furniture splits rooms as DESIGN.md 4.27 says it does.
  rooms_resident   ops.segment_rooms(device=True) on a device-resident free map: labels left on the device, both tables read back
  rooms_host       ops.segment_rooms on a host array, labels, clearance and seeds copied back
  edt              ops.distance_transform_edt(device=True) on the resident free map
  seeds            ops.room_seeds on the resident clearance
  grow             ops.grow_labels(device=True) on the resident free map and seeds: the distance phase and the label phase
  field            ops.travel_field(device=True) from the same seeds: the distance phase alone, the call the parent commit has
  tables           ops.room_tables on the resident labels, seeds and clearance
label_ms = grow - field is the label phase; label_over_field is its ratio to the field.  rounds / tile_runs are given for both
phases.  The host chain: scipy.ndimage.distance_transform_edt, scipy.ndimage.label with the renumbering loop, and
scipy.sparse.csgraph.dijkstra(min_only=True) on probe_travel.legal_graph, whose returned sources are the host's owners.  Ties
differ (SciPy keeps the first source it met), so times are compared and equality is asserted only on cells with a unique nearest
seed label: cells where the growth gives the same owner when ties go to the largest label instead of the smallest.  Both paths
end synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` (host: `host_reps`) calls after `warmup`.  Kernel times and counters are not
collected here."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
from scipy import ndimage
from scipy.sparse.csgraph import dijkstra

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402
from probe_travel import indoor_map, legal_graph  # noqa: E402


def host_seeds(free, radius, least):
    E = ndimage.distance_transform_edt(free)
    lab, n = ndimage.label(E > radius, structure=np.ones((3, 3)))
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    keep = sizes >= least
    keep[0] = False
    renumber = np.where(keep, np.cumsum(keep), 0).astype(np.int32)
    return renumber[lab], int(keep.sum()), E


def unique_owner(free_dev, seeds, owner, n):
    """bool (H, W): the cells whose nearest seed label is unique -- the growth with the labels' order reversed (k -> n + 1 - k, so
    that ties go to the LARGEST label) gives the same owner as the growth itself"""
    flipped = np.where(seeds > 0, n + 1 - seeds, 0).astype(np.int32)
    other = ops.grow_labels(free_dev, flipped).owner
    return (owner > 0) & (seeds == 0) & (np.where(other > 0, n + 1 - other, 0) == owner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=float, default=9.0)
    ap.add_argument("--min-seed-cells", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    gs = 1000
    obstacles = indoor_map(gs)
    res = {"gs": gs, "method": "host clock around synchronised calls, median of reps", "radius": a.radius, "min_seed_cells": a.min_seed_cells,
           "tile": ops.TRAVEL_TILE, "sweep_cap": ops.TRAVEL_SWEEPS, "kernel_times": "not collected", "cases": {}}
    for H, W in ((300, 400), (600, 700), (1000, 1000)):
        r0, c0 = (gs - H) // 2, (gs - W) // 2
        free = np.ascontiguousarray(~obstacles[r0:r0 + H, c0:c0 + W])
        free_u8 = free.astype(np.uint8)
        dfree = DeviceArray.from_numpy(free_u8)
        seg = ops.segment_rooms(dfree, a.radius, a.min_seed_cells, device=True)
        assert seg.n > 0, "the probe's radius leaves no room"
        dE, dseeds, dlabels = seg.clearance, seg.seeds, seg.labels
        growth = seg.growth
        labels, seeds = dlabels.numpy(), dseeds.numpy()
        A, B = growth.field.planes()

        # the host chain, and where it must agree
        hseeds, hn, hE = host_seeds(free, a.radius, a.min_seed_cells)
        assert hn == seg.n and np.array_equal(hseeds, seeds) and np.array_equal(hE, dE.numpy())
        graph = legal_graph(free, seeds > 0)
        sources = np.flatnonzero(seeds.ravel() > 0)

        def host_dijkstra():
            return dijkstra(graph, directed=True, indices=sources, min_only=True, return_predecessors=True)

        dist, _, nearest = host_dijkstra()
        howner = np.where(nearest >= 0, seeds.ravel()[np.maximum(nearest, 0)], 0).reshape(H, W).astype(np.int32)
        reached = np.isfinite(dist).reshape(H, W)
        unique = unique_owner(dfree, seeds, labels, seg.n)
        same = bool(np.array_equal(reached, A >= 0) and np.array_equal(howner[unique], labels[unique]))
        assert same, (H, W)

        tiles = -(-H // ops.TRAVEL_TILE) * -(-W // ops.TRAVEL_TILE)
        case = {"same_where_unique": same, "unique_share": float(unique.sum()) / max(int((A >= 0).sum() - (seeds > 0).sum()), 1),
                "rooms": seg.n, "doors": int(len(seg.doors)), "free_cells": int(free.sum()), "seed_cells": int((seeds > 0).sum()),
                "unlabelled_free_cells": int(((labels == 0) & free).sum()), "tiles": tiles,
                "field_rounds": growth.field.rounds, "field_tile_runs": growth.field.tile_runs,
                "label_rounds": growth.rounds, "label_tile_runs": growth.tile_runs}
        case["rooms_resident"] = stats(lib, lambda: ops.segment_rooms(dfree, a.radius, a.min_seed_cells, device=True), a.reps, a.warmup)
        case["rooms_host"] = stats(lib, lambda: ops.segment_rooms(free_u8, a.radius, a.min_seed_cells), a.reps, a.warmup)
        case["edt"] = stats(lib, lambda: ops.distance_transform_edt(dfree, device=True), a.reps, a.warmup)
        case["seeds"] = stats(lib, lambda: ops.room_seeds(dE, a.radius, a.min_seed_cells), a.reps, a.warmup)
        case["grow"] = stats(lib, lambda: ops.grow_labels(dfree, dseeds, device=True), a.reps, a.warmup)
        dmask = DeviceArray.from_numpy((seeds > 0).astype(np.uint8))
        case["field"] = stats(lib, lambda: ops.travel_field(dfree, dmask, device=True), a.reps, a.warmup)
        case["tables"] = stats(lib, lambda: ops.room_tables(dlabels, dseeds, dE, seg.n), a.reps, a.warmup)
        case["label_ms"] = case["grow"]["median_ms"] - case["field"]["median_ms"]
        case["label_over_field"] = case["label_ms"] / case["field"]["median_ms"]
        case["host_edt"] = stats(lib, lambda: ndimage.distance_transform_edt(free), a.host_reps, 0)
        case["host_seeds"] = stats(lib, lambda: host_seeds(free, a.radius, a.min_seed_cells), a.host_reps, 0)
        case["host_dijkstra"] = stats(lib, host_dijkstra, a.host_reps, 0)
        case["host_graph"] = stats(lib, lambda: legal_graph(free, seeds > 0), a.host_reps, 0)
        res["cases"][f"{H}x{W}"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
