#!/usr/bin/env python3
"""Timing probe of the many-goal planner (avl_navmany_* of csrc/avl_nav.hip) on the three indoor maps of tools/probe_navigator.py
(about 1 000, 5 000 and 20 000 path vertices).  For M = 64 / 1 024 / 16 384 goals, drawn once from free cells and once from
obstacle cells (snapped first), it reports medians of 30 runs, host clock around the synchronous calls:

  * plan_many: the start's tree and all M goals;
  * snap: M points;
  * M single plans (G.plan) on the same graph, timed over at most 256 of the goals and SCALED to M;
  * the share of goal-vertex walks that the pruning skipped.

    python tools/probe_plan_many.py [--out profiles/plan_many_<date>.txt] [--repeats 30]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def median_ms(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--single-cap", type=int, default=256, help="single plans timed per row (scaled to M)")
    args = ap.parse_args(argv)
    from avlmaps_amd import _lib, ops
    from probe_navigator import indoor_map
    _lib.load()
    _lib.require_gpu()
    ops.nav_graph(indoor_map(2, 2)).close()                  # warm-up: module load, first allocations
    head = (f"{'V':>6} {'goals':>9} {'M':>6} {'plan_many ms':>13} {'snap ms':>8} {'M x plan ms (scaled)':>21} {'timed':>6} "
            f"{'speed-up':>9} {'walks':>11} {'pruned':>7} {'reached':>8}")
    lines = [f"# tools/probe_plan_many.py: medians of {args.repeats}, host clock around synchronous calls; the single plans are timed over",
             f"# at most {args.single_cap} goals (one pass) and scaled to M", head]
    print("\n".join(lines), flush=True)
    for rr, cc in ((5, 6), (11, 12), (23, 24)):
        free = indoor_map(rr, cc, blocks=11, seed=1)
        g = ops.nav_graph(free)
        rng = np.random.default_rng(4)
        cells = {"free": np.argwhere(free), "obstacle": np.argwhere(~free)}
        start = cells["free"][rng.integers(0, len(cells["free"]))].astype(np.float64)
        for kind in ("free", "obstacle"):
            for M in (64, 1024, 16384):
                pts = cells[kind][rng.integers(0, len(cells[kind]), M)].astype(np.float64)
                t_snap = median_ms(lambda: g.snap(pts), args.repeats)
                goals, _ = g.snap(pts)
                g.plan_many(start, goals)                    # grows the buffers
                t_many = median_ms(lambda: g.plan_many(start, goals), args.repeats)
                g.count_walks(True)                          # one extra batch with counters; the timed ones run without
                pm = g.plan_many(start, goals)
                st = g.many_stats()
                g.count_walks(False)
                n1 = min(M, args.single_cap)
                t0 = time.perf_counter()
                for t in goals[:n1]:
                    g.plan(start, t)
                t_single = 1e3 * (time.perf_counter() - t0) * (M / n1)
                pruned = 1.0 - st["walks"] / max(st["candidates"], 1)
                line = (f"{g.V:6d} {kind:>9} {M:6d} {t_many:13.3f} {t_snap:8.3f} {t_single:21.1f} {n1:6d} {t_single / t_many:8.1f}x "
                        f"{st['walks']:11d} {100 * pruned:6.1f}% {int(np.isfinite(pm.dist).sum()):8d}")
                lines.append(line)
                print(line, flush=True)
        g.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
