"""GPU box: time the island step of VLMap.get_pos and the contour midpoint (csrc/avl_islands.hip) against the host paths they replace.
Prints one JSON object (and writes it to --out).

    probe_islands.py [--reps 30] [--warmup 3] [--out profiles/islands_probe.txt]

Crops of 300 x 400, 600 x 700 and 1000 x 1000 cells of a (1000, 1000) pooled mask (rooms with gapped walls and 1 % salt noise, the
mask of tools/probe_morph2d.py), taken through ops.mask_foreground as get_pos does; the foreground stays on the device.
  islands_device   navigation_utils.get_segment_islands_pos_device on the device foreground: label, table, count pass, write pass, the
                   table and the points copied to the host, the Python lists built -- what get_pos runs without OpenCV
  islands_host     the foreground copied to the host, then navigation_utils.get_segment_islands_pos: scipy.ndimage.label and the
                   Python Moore trace per island -- what get_pos ran before
  label_device     ops.label_islands(device=True) alone (seven launches, the count read back, three launches for the table)
  middle_device    ops.contour_nearest_pair on the two longest contours of the crop (host arrays: the upload is part of it)
  middle_host      map.py:351-358 in NumPy on the same two contours: the |A| x |B| float64 matrix and its argmin
Both paths end synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it.  `same` says that the two paths returned equal results."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from avlmaps_amd.utils.navigation_utils import get_segment_islands_pos, get_segment_islands_pos_device  # noqa: E402
from probe_morph2d import pooled_mask, stats  # noqa: E402


def numpy_middle(a, b):
    d = np.linalg.norm(a.reshape((-1, 1, 2)) - b.reshape((1, -1, 2)), axis=2)
    i, j = np.unravel_index(np.argmin(d), d.shape)
    return int(i), int(j)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    gs = 1000
    dmask = DeviceArray.from_numpy(pooled_mask(gs).astype(np.uint8))
    res = {"gs": gs, "method": "host clock around synchronised calls, median of reps", "cases": {}}
    for H, W in ((300, 400), (600, 700), (1000, 1000)):
        r0, c0 = (gs - H) // 2, (gs - W) // 2
        dfg = ops.mask_foreground(dmask, r0, r0 + H, c0, c0 + W, device=True)

        def dev_islands():
            return get_segment_islands_pos_device(dfg, 1)

        def host_islands():
            return get_segment_islands_pos(dfg.numpy().astype(bool), 1)

        def dev_label():
            ops.label_islands(dfg, device=True).close()
        got, want = dev_islands(), host_islands()
        same = len(got[0]) == len(want[0]) and all(np.array_equal(x, y) for x, y in zip(got[0], want[0])) \
            and got[1] == want[1] and got[2] == want[2]
        order = np.argsort([-len(c) for c in want[0]])
        ca, cb = want[0][order[0]], want[0][order[1]]

        def dev_middle():
            return ops.contour_nearest_pair(ca, cb)[:2]

        def host_middle():
            return numpy_middle(ca, cb)
        case = {"islands": len(want[0]), "longest_contour": int(len(ca)), "contour_points": int(sum(len(c) for c in want[0])),
                "same": bool(same and dev_middle() == host_middle()), "middle_sizes": [int(len(ca)), int(len(cb))]}
        case["islands_device"] = stats(lib, dev_islands, a.reps, a.warmup)
        case["islands_host"] = stats(lib, host_islands, a.reps, a.warmup)
        case["label_device"] = stats(lib, dev_label, a.reps, a.warmup)
        case["middle_device"] = stats(lib, dev_middle, a.reps, a.warmup)
        case["middle_host"] = stats(lib, host_middle, a.reps, a.warmup)
        res["cases"][f"rooms_{H}x{W}"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
