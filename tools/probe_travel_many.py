"""GPU box: time K travel fields in one batch (csrc/avl_travel_many.hip through ops.travel_fields) against a loop of K
ops.travel_field calls in the same process, and the sound field around walls (ops.sound_travel_field) against the Euclidean
ops.sound_field.  Prints one JSON object (and writes it to --out).

    probe_travel_many.py [--reps 30] [--warmup 3] [--out profiles/travel_many_probe.txt]

The maps are probe_travel.py's: crops of 300 x 400, 600 x 700 and 1000 x 1000 cells of its (1000, 1000) indoor-like obstacle map,
device-resident.  The K = 1 / 8 / 64 sets are single free cells: the free cell nearest to the crop's centre first (probe_travel's
"cell" case), then free cells drawn with a fixed seed.
  single_a, single_b   two series of ops.travel_field(device=True) on the resident free map and the resident mask of set 0, one
                       before and one after batch_1: `spread` = |a - b| / min(a, b) of their medians is what two series of the
                       same call differ by in this process
  batch_K              ops.travel_fields(device=True) on the resident free map and the host CSR sets (its interface)
  loop_K               K calls of ops.travel_field(device=True), each on the resident mask of its set: the only way to the same
                       planes without the batch
  k1_within_spread     (batch_1 - single) / single <= spread, single = the smaller of the two medians
  sound_travel         ops.sound_travel_field, 300 segments of 1 .. 3 free cells, peaks in (0, 1], decay 0.01, chunk 64
  sound_euclid         ops.sound_field on the same segments over the square grid of side max(H, W): the gap is the price of walls
Every path ends synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it.  `rounds`: rounds with an active (field, tile) pair; `launched`: round launches
(batches of 8); `pair_runs`: pairs that ran; `idle_share` = 1 - pair_runs / (K x tiles x launched), the share of the launched
workgroups that found their mark unset and returned at once.  `same`: the batch's planes equal the loop's, byte for byte."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402
from probe_travel import indoor_map  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    gs, decay, n_seg = 1000, 0.01, 300
    obstacles = indoor_map(gs)
    res = {"gs": gs, "method": "host clock around synchronised calls, median of reps", "tile": ops.TRAVEL_TILE,
           "sweep_cap": ops.TRAVEL_SWEEPS, "kernel_times": "not collected", "cases": {}}
    for H, W in ((300, 400), (600, 700), (1000, 1000)):
        r0, c0 = (gs - H) // 2, (gs - W) // 2
        tiles = -(-H // ops.TRAVEL_TILE) * -(-W // ops.TRAVEL_TILE)
        free = ~obstacles[r0:r0 + H, c0:c0 + W]
        free_cells = np.argwhere(free)
        rng = np.random.default_rng(H + W)
        centre = free_cells[np.argmin(np.sum((free_cells - (H // 2, W // 2)) ** 2, axis=1))]
        cells = np.concatenate([centre[None], free_cells[rng.choice(len(free_cells), 63, replace=False)]]).astype(np.int32)
        dfree = DeviceArray.from_numpy(free.astype(np.uint8))
        masks = []
        for r, c in cells:
            m = np.zeros((H, W), np.uint8)
            m[r, c] = 1
            masks.append(DeviceArray.from_numpy(m))
        case = {"tiles": tiles, "free_cells": int(free.sum())}

        def single():
            return ops.travel_field(dfree, masks[0], device=True)

        def batch(K):
            return ops.travel_fields(dfree, np.arange(K + 1, dtype=np.int64), cells[:K], device=True)

        def loop(K):
            return [ops.travel_field(dfree, masks[k], device=True) for k in range(K)]

        case["single_a"] = stats(lib, single, a.reps, a.warmup)
        case["batch_1"] = stats(lib, lambda: batch(1), a.reps, a.warmup)
        case["single_b"] = stats(lib, single, a.reps, a.warmup)
        sa, sb = case["single_a"]["median_ms"], case["single_b"]["median_ms"]
        case["spread"] = abs(sa - sb) / min(sa, sb)
        case["k1_excess"] = (case["batch_1"]["median_ms"] - min(sa, sb)) / min(sa, sb)
        case["k1_within_spread"] = bool(case["k1_excess"] <= case["spread"])
        for K in (1, 8, 64):
            tf = batch(K)
            launched = 8 * -(-tf.rounds // 8)
            info = {"rounds": tf.rounds, "launched": launched, "pair_runs": tf.tile_runs,
                    "idle_share": 1.0 - tf.tile_runs / float(K * tiles * launched)}
            if K > 1:
                ones = loop(K)
                a_all, b_all = tf.planes()
                info["same"] = bool(all(np.array_equal(a_all[k], ones[k].planes()[0]) and np.array_equal(b_all[k], ones[k].planes()[1])
                                        for k in range(K)))
                assert info["same"], (H, W, K)
                info["loop_rounds_sum"] = int(sum(f.rounds for f in ones))
                info["loop_rounds_max"] = int(max(f.rounds for f in ones))
                del ones, a_all, b_all
                case[f"batch_{K}"] = stats(lib, lambda: batch(K), a.reps, a.warmup)
                case[f"loop_{K}"] = stats(lib, lambda: loop(K), a.reps, a.warmup)
                info["speedup"] = case[f"loop_{K}"]["median_ms"] / case[f"batch_{K}"]["median_ms"]
            del tf
            case[f"schedule_{K}"] = info
            print(f"{H} x {W}: K = {K} done", file=sys.stderr, flush=True)
        case["k64_faster_than_loop"] = bool(case["batch_64"]["median_ms"] < case["loop_64"]["median_ms"])
        counts = rng.integers(1, 4, n_seg)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        locs = free_cells[rng.choice(len(free_cells), int(counts.sum()), replace=False)].astype(np.int32)
        peaks = (1.0 - rng.random(n_seg)).astype(np.float32)
        case["sound_segments"] = n_seg
        case["sound_travel"] = stats(lib, lambda: ops.sound_travel_field(dfree, offsets, locs, peaks, decay, chunk=64), a.reps, a.warmup)
        case["sound_euclid"] = stats(lib, lambda: ops.sound_field(offsets, locs, peaks, max(H, W), decay), a.reps, a.warmup)
        res["cases"][f"{H}x{W}"] = case
        del masks, dfree
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
