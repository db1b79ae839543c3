#!/usr/bin/env python3
"""Timing probe of the GPU navigator (csrc/avl_nav.hip) on synthetic indoor maps: rooms with one-pixel walls and doors,
furniture blocks and diagonal walls, scaled to about 1 000, 5 000 and 20 000 path vertices.  Reports V, the visibility edges,
the build time (upload, vertices, visibility bitset) and the plan time (query rows and shortest path), and -- at the smallest
size -- the CPU time of the test oracle (tests/test_navigator_gpu.py), extrapolated from a sample of its rows.

    python tools/probe_navigator.py [--out profiles/navigator_probe.json] [--no-oracle]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def indoor_map(rooms_r, rooms_c, room=40, blocks=6, diagonals=1, seed=0):
    rng = np.random.default_rng(seed)
    H, W = rooms_r * room + 1, rooms_c * room + 1
    free = np.ones((H, W), bool)
    free[::room, :] = False
    free[:, ::room] = False
    for i in range(rooms_r):
        for j in range(rooms_c):
            r0, c0 = i * room, j * room
            if j + 1 < rooms_c:                              # a door in the east wall
                d = r0 + rng.integers(5, room - 8)
                free[d:d + 4, c0 + room] = True
            if i + 1 < rooms_r:                              # a door in the south wall
                d = c0 + rng.integers(5, room - 8)
                free[r0 + room, d:d + 4] = True
            for _ in range(blocks):                          # furniture
                h, w = rng.integers(2, 8, size=2)
                r, c = r0 + rng.integers(3, room - h - 2), c0 + rng.integers(3, room - w - 2)
                free[r:r + h, c:c + w] = False
            for _ in range(diagonals):
                r, c, n = r0 + rng.integers(4, room // 2), c0 + rng.integers(4, room // 2), rng.integers(6, room // 2)
                s = 1 if rng.random() < 0.5 else -1
                for k in range(n):
                    rr, cc = r + k, c + (k if s > 0 else n - k)
                    if r0 < rr < r0 + room and c0 < cc < c0 + room:
                        free[rr, cc] = False
    return free


def free_point(rng, free):
    cells = np.argwhere(free)
    r, c = cells[rng.integers(0, len(cells))]
    return [float(r), float(c)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--plans", type=int, default=10)
    args = ap.parse_args(argv)
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    sizes = [("~1k", 5, 6, 11), ("~5k", 11, 12, 11), ("~20k", 23, 24, 11)]
    ops.nav_graph(indoor_map(2, 2)).close()                  # warm-up: module load, first allocations
    rows = []
    for name, rr, cc, blocks in sizes:
        free = indoor_map(rr, cc, blocks=blocks, seed=1)
        t0 = time.perf_counter()
        g = ops.nav_graph(free)                              # synchronous: returns when the bitset is complete
        t_build = time.perf_counter() - t0
        words = g.visibility_words() if g.V <= 30000 else None
        edges = int(np.unpackbits(words.view(np.uint8)).sum() // 2) if words is not None else None
        rng = np.random.default_rng(2)
        times, reached, hops = [], 0, []
        for _ in range(args.plans):
            s, t = free_point(rng, free), free_point(rng, free)
            t0 = time.perf_counter()
            dist, ids = g.plan(s, t)
            times.append(time.perf_counter() - t0)
            if ids:
                reached += 1
                hops.append(len(ids) - 1)
        row = dict(size=name, H=free.shape[0], W=free.shape[1], V=g.V, edges=edges, build_ms=round(1e3 * t_build, 3),
                   plan_ms_median=round(1e3 * float(np.median(times)), 3), plan_ms_max=round(1e3 * max(times), 3),
                   plans=len(times), reached=reached, median_hops=float(np.median(hops)) if hops else None)
        if name == "~1k" and not args.no_oracle:
            sys.path.insert(0, str(ROOT / "tests"))
            import test_navigator_gpu as T
            verts = g.vertices().astype(np.int64)
            t0 = time.perf_counter()
            prim = T.Primitives(free)
            t_prim = time.perf_counter() - t0
            sample = np.random.default_rng(3).choice(g.V - 1, size=min(40, g.V - 1), replace=False)
            t0 = time.perf_counter()
            for a in sample:
                T.oracle_blocked(prim, verts[a], verts[a + 1:])
            per_pair = (time.perf_counter() - t0) / max(1, sum(g.V - 1 - a for a in sample))
            row["oracle_cpu_s_extrapolated"] = round(t_prim + per_pair * g.V * (g.V - 1) / 2, 1)
            row["oracle_rows_sampled"] = int(len(sample))
        g.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(dict(rows=rows), indent=1) + "\n")


if __name__ == "__main__":
    main()
