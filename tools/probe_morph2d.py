"""GPU box: time the 2-D morphology composites (csrc/avl_morph2d.hip) against the host chains they replace.  Prints one JSON object
(and writes it to --out).

    probe_morph2d.py [--reps 30] [--warmup 3] [--out profiles/morph2d_probe.txt]

Crops of 300 x 400, 600 x 700 and 1000 x 1000 cells of a (1000, 1000) pooled mask (rooms, gapped walls, 1 % salt noise).
  get_pos mask chain   device path: ops.mask_foreground on the device-resident pooled mask, the foreground copied to the host --
                       what VLMap.get_pos does.  host path: the pooled mask copied to the host, cropped, then SciPy's
                       binary_closing(iterations=3), gaussian_filter(0.8, truncate=3), > 0.5, binary_dilation -- what VLMap.get_pos
                       did before.
  _dilate_map          device path: Map._dilate_map (host bool image in, host float64 image out, the copies included), dilate_iter 3,
                       sigma 1.0.  host path: the same chain in NumPy / SciPy with the half-pixel x2 / x0.5 resizes written out
                       (OpenCV, which upstream calls, is not installed: there is no earlier version of this call to time).
  _dilate_map == 0     the device path as VLMap.customize_obstacle_map calls it: only the byte image `result == 0` is built.
Both paths end synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it.  `same` says that the two paths returned equal arrays.  Run under
rocprofv3 --kernel-trace --stats for the kernels of each composite."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
from scipy.ndimage import binary_closing, binary_dilation, gaussian_filter

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from avlmaps_amd.map.map import Map  # noqa: E402


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


def pooled_mask(gs, seed=0):
    rng = np.random.default_rng(seed)
    m = np.zeros((gs, gs), bool)
    for _ in range(60):
        h, w = int(rng.integers(40, 300)), int(rng.integers(40, 300))
        r, c, t = int(rng.integers(0, gs - h)), int(rng.integers(0, gs - w)), int(rng.integers(1, 4))
        room = np.zeros((gs, gs), bool)
        room[r:r + h, c:c + w] = True
        room[r + t:r + h - t, c + t:c + w - t] = False
        room[int(rng.integers(r, r + h)), c:c + t] = False
        room[r:r + t, int(rng.integers(c, c + w))] = False
        m |= room
    return m | (rng.random((gs, gs)) < 0.01)


def up2(x):
    def taps(n):
        s = (np.arange(2 * n) + 0.5) / 2 - 0.5
        f = np.floor(s)
        return np.clip(f, 0, n - 1).astype(int), np.clip(f + 1, 0, n - 1).astype(int), s - f
    y0, y1, fy = taps(x.shape[0])
    x0, x1, fx = taps(x.shape[1])
    top = x[y0][:, x0] * (1 - fx) + x[y0][:, x1] * fx
    bot = x[y1][:, x0] * (1 - fx) + x[y1][:, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


def host_dilate(binary, dilate_iter, sigma):
    m = up2(binary.astype(float))
    m = gaussian_filter(m, sigma=sigma, truncate=3)
    m = (m > 0.5).astype(np.uint8)
    m = binary_dilation(m, structure=np.ones((3, 3)), iterations=dilate_iter * 2)
    m = m.astype(float)
    return (m[0::2, 0::2] + m[0::2, 1::2] + m[1::2, 0::2] + m[1::2, 1::2]) / 4


def host_foreground(mask):
    f = binary_closing(mask, iterations=3)
    f = gaussian_filter(f.astype(float), sigma=0.8, truncate=3)
    return binary_dilation(f > 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    gs = 1000
    mask = pooled_mask(gs)
    dmask = DeviceArray.from_numpy(mask.astype(np.uint8))
    res = {"gs": gs, "method": "host clock around synchronised calls, median of reps", "dilate_iter": 3, "gaussian_sigma": 1.0, "cases": {}}
    for H, W in ((300, 400), (600, 700), (1000, 1000)):
        r0, c0 = (gs - H) // 2, (gs - W) // 2
        crop = np.ascontiguousarray(mask[r0:r0 + H, c0:c0 + W])

        def dev_fg():
            return ops.mask_foreground(dmask, r0, r0 + H, c0, c0 + W)

        def host_fg():
            return host_foreground(dmask.numpy().astype(bool)[r0:r0 + H, c0:c0 + W])

        def dev_dm():
            return Map._dilate_map(crop, 3, 1.0)

        def dev_dm_zero():
            return ops.dilate_map(crop, 3, 1.0, want_values=False)[1]

        def host_dm():
            return host_dilate(crop, 3, 1.0)
        case = {"same": bool(np.array_equal(dev_fg(), host_fg()) and np.array_equal(dev_dm(), host_dm())
                             and np.array_equal(dev_dm_zero(), host_dm() == 0))}
        case["get_pos_chain_device"] = stats(lib, dev_fg, a.reps, a.warmup)
        case["get_pos_chain_host"] = stats(lib, host_fg, a.reps, a.warmup)
        case["dilate_map_device"] = stats(lib, dev_dm, a.reps, a.warmup)
        case["dilate_map_zero_device"] = stats(lib, dev_dm_zero, a.reps, a.warmup)
        case["dilate_map_host"] = stats(lib, host_dm, a.reps, a.warmup)
        res["cases"][f"{H}x{W}"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
