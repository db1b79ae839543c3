"""GPU box: time CLIP's preprocess on the GPU (csrc/avl_resize.hip through ops.clip_preprocess) against the path it replaces on the
same box: Pillow's bicubic resize, the centre crop and the float32 normalisation per frame on one host core.  Prints one JSON
object (and writes it to --out).

    probe_preprocess.py [--reps 30] [--warmup 3] [--host-reps 10] [--scene-frames 64] [--out profiles/preprocess_probe.txt]

720 x 1080 x 3 uint8 frames of random bytes (the arithmetic does not depend on the values) to (B, 3, 224, 224) float32, B = 1, 16, 64:
  resident        ops.clip_preprocess of a DeviceArray: the two launches alone (tables and workspace come from the pools)
  from_host       the same from a host array: the pageable upload of the batch included
  required_bytes  what the kernels must read and write: the input rows and the bytes of their columns that reach the crop (from the
                  bounds tables) plus the float32 output; the workspace's traffic between the two passes is NOT counted, so
                  resident_GBps is the rate on the required bytes, not the traffic the kernels cause
  pillow          Image.fromarray(frame).resize((336, 224), BICUBIC), the crop, (v / 255 - mean) / std in float32, transposed: one
                  frame, --host-reps times (`pillow` is null and `pillow_missing` true where Pillow is not installed)
  same            the device result equals that host path bit for bit
  area_map        AreaMap.create_map on a scene of --scene-frames PNGs of 720 x 1080 (blocky images, so that they compress), with
                  the model-free encoders: per_frame (image_encoder=HashImageEncoder(), the path as it was) and batched
                  (batch_encoder=HashBatchImageEncoder(), batch_size 64), and png_decode, load_rgb_png of all frames alone, which
                  both paths contain
Every device figure is the median of `reps` synchronised calls after `warmup` (host clock), minimum and maximum next to it."""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402

H, W, N_PX = 720, 1080, 224


def required_bytes(B):
    oh, ow, top, left = ops.clip_preprocess_plan(H, W, N_PX)
    _, bh = ops.resize_coeffs(W, ow)
    _, bv = ops.resize_coeffs(H, oh)
    cols = int(bh[left + N_PX - 1].sum() - bh[left, 0])
    rows = int(bv[top + N_PX - 1].sum() - bv[top, 0])
    return B * (rows * cols * 3 + 3 * N_PX * N_PX * 4), rows, cols


def pillow_preprocess(frame):
    from PIL import Image
    oh, ow, top, left = ops.clip_preprocess_plan(H, W, N_PX)
    a = np.asarray(Image.fromarray(frame).resize((ow, oh), Image.BICUBIC))[top:top + N_PX, left:left + N_PX]
    x = (a.astype(np.float32) / np.float32(255) - np.asarray(ops.CLIP_MEAN, np.float32)) / np.asarray(ops.CLIP_STD, np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def host_stats(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--scene-frames", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (64, H, W, 3), dtype=np.uint8)
    res = {"frame": [H, W, 3], "n_px": N_PX, "library": os.environ.get("AVLMAPS_HIP_LIB") or "stock",
           "method": "host clock around synchronised calls, median of reps", "cases": {}}
    try:
        import PIL
        res["pillow_version"], res["pillow_missing"] = PIL.__version__, False
        want = pillow_preprocess(frames[0])
        res["pillow"] = host_stats(lambda: pillow_preprocess(frames[0]), a.host_reps)
        res["same"] = bool(np.array_equal(ops.clip_preprocess(frames[0], device=False)[0], want))
    except ImportError:
        res["pillow_version"], res["pillow_missing"], res["pillow"], res["same"] = None, True, None, None
    for B in (1, 16, 64):
        host = frames[:B]
        dev = DeviceArray.from_numpy(host)
        nbytes, rows, cols = required_bytes(B)
        case = {"required_bytes": nbytes, "input_rows": rows, "input_columns": cols,
                "resident": stats(lib, lambda: ops.clip_preprocess(dev), a.reps, a.warmup),
                "from_host": stats(lib, lambda: ops.clip_preprocess(host), a.reps, a.warmup)}
        case["resident_GBps"] = nbytes / (case["resident"]["median_ms"] * 1e-3) / 1e9
        case["resident_us_per_frame"] = case["resident"]["median_ms"] * 1e3 / B
        case["from_host_ms_per_frame"] = case["from_host"]["median_ms"] / B
        res["cases"][f"B_{B}"] = case
    if a.scene_frames > 0 and not res["pillow_missing"]:
        from PIL import Image
        from avlmaps_amd.apps.common import HashBatchImageEncoder, HashImageEncoder
        from avlmaps_amd.map.area_map import AreaMap
        from avlmaps_amd.utils.mapping_utils import load_rgb_png
        with tempfile.TemporaryDirectory() as tmp:
            root = Path(tmp)
            (root / "rgb").mkdir()
            for i in range(a.scene_frames):
                small = rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8)
                Image.fromarray(np.repeat(np.repeat(small, 8, axis=0), 8, axis=1)).save(root / "rgb" / f"{i:06d}.png")
            poses = np.zeros((a.scene_frames, 7))
            poses[:, 6] = 1.0
            np.savetxt(root / "poses.txt", poses)
            paths = sorted((root / "rgb").glob("*.png"))
            am, per_frame, batched = AreaMap(), HashImageEncoder(), HashBatchImageEncoder()
            am.create_map(root, batch_encoder=batched, batch_size=64)              # warm-up: tables, pools, torch
            res["area_map"] = {
                "frames": a.scene_frames,
                "png_decode": host_stats(lambda: [load_rgb_png(p) for p in paths], 3),
                "per_frame": host_stats(lambda: am.create_map(root, image_encoder=per_frame), 3),
                "batched": host_stats(lambda: am.create_map(root, batch_encoder=batched, batch_size=64), 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
