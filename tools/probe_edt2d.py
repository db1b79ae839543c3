"""GPU box: time the exact 2-D distance transform and the distribution-map chain (csrc/avl_edt2d.hip, the float32 gaussian of
csrc/avl_morph2d.hip) against the SciPy chain they replace.  Prints one JSON object (and writes it to --out).

    probe_edt2d.py [--reps 30] [--warmup 3] [--out profiles/edt2d_probe.txt]

Crops of 300 x 400, 600 x 700 and 1000 x 1000 cells of a (1000, 1000) pooled mask, two scenes each:
  rooms    rectangular rooms with gapped walls and 1 % salt noise (the mask of tools/probe_morph2d.py)
  corner   one 6 x 6 blob in the crop's top-left corner and nothing else: the longest search of the row pass
  edt              device: ops.distance_transform_edt(device=True) on the device-resident byte image `crop == 0` -- the transform
                   alone (two launches and the 4-byte flag).  host: scipy.ndimage.distance_transform_edt on the host crop.
  chain            device: ops.mask_decay_2d(normalize=True, smooth_sigma=1, window=crop) on the device-resident pooled mask, the
                   finished float64 map copied to the host -- what VLMap.get_distribution_map does after the pooling.  host: the
                   pooled mask copied to the host and cropped, then habitat_lang_robot.py:231-236 in NumPy / SciPy -- the route
                   without these kernels.
Both paths end synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it.  `same` says that the two paths returned equal arrays.  Run under
rocprofv3 --kernel-trace --stats for the kernels of the chain."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
from scipy.ndimage import distance_transform_edt, gaussian_filter

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import pooled_mask, stats  # noqa: E402


def host_chain(predict_mask, decay_rate):
    predict_mask = predict_mask.astype(np.float32)
    predict_mask = (gaussian_filter(predict_mask, sigma=1) > 0.5).astype(np.float32)
    dists = distance_transform_edt(predict_mask == 0)
    tmp = np.ones_like(dists) - (dists * decay_rate)
    dist_map = np.where(tmp < 0, np.zeros_like(tmp), tmp)
    return (dist_map - np.min(dist_map)) / (np.max(dist_map) - np.min(dist_map))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    gs, rate = 1000, 0.1
    res = {"gs": gs, "method": "host clock around synchronised calls, median of reps", "decay_rate": rate, "cases": {}}
    for H, W in ((300, 400), (600, 700), (1000, 1000)):
        r0, c0 = (gs - H) // 2, (gs - W) // 2
        corner = np.zeros((gs, gs), bool)
        corner[r0:r0 + 6, c0:c0 + 6] = True
        for scene, mask in (("rooms", pooled_mask(gs)), ("corner", corner)):
            dmask = DeviceArray.from_numpy(mask.astype(np.uint8))
            crop = np.ascontiguousarray(mask[r0:r0 + H, c0:c0 + W])
            dzero = DeviceArray.from_numpy((crop == 0).astype(np.uint8))

            def dev_edt():
                return ops.distance_transform_edt(dzero, device=True)

            def host_edt():
                return distance_transform_edt(crop == 0)

            def dev_chain():
                return ops.mask_decay_2d(dmask, rate, normalize=True, smooth_sigma=1, window=(r0, r0 + H, c0, c0 + W))

            def host_chain_():
                return host_chain(dmask.numpy()[r0:r0 + H, c0:c0 + W], rate)
            case = {"same": bool(np.array_equal(dev_edt().numpy(), host_edt()) and np.array_equal(dev_chain(), host_chain_()))}
            case["edt_device"] = stats(lib, dev_edt, a.reps, a.warmup)
            case["edt_host"] = stats(lib, host_edt, a.reps, a.warmup)
            case["chain_device"] = stats(lib, dev_chain, a.reps, a.warmup)
            case["chain_host"] = stats(lib, host_chain_, a.reps, a.warmup)
            res["cases"][f"{scene}_{H}x{W}"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
