"""GPU box: time the render kernels (csrc/avl_render.hip) and AVLMap.render_heat against NumPy on the same box.
Prints one JSON object (and writes it to --out).

    probe_render.py [--voxels 2000000] [--reps 30] [--warmup 3] [--out profiles/render_probe.txt]

A map of `voxels` unique voxels on a (1000, 1000, 60) grid (rooms are irrelevant here: the kernels' cost depends on N and on the
footprints), a float32 heat, JET.  Device rows run on arrays that are already resident, as they are after a query; `*_host_arrays`
rows upload grid_pos, heat and grid_rgb on every call, which is what a caller without a map object pays.
  colorize_f64 / colorize_u8     ops.colorize_heat, the (N, 3) float64 form and the uint8 form, results left on the device
  colorize_u8_to_host            the uint8 form copied back (6 MB at 2 M voxels)
  colorize_numpy                 convert_heatmap_to_rgb's NumPy expression with the table lookup, plus .astype(np.uint8)
  topdown / topdown_host_arrays  ops.render_topdown of the whole map, image copied back
  topdown_numpy                  np.lexsort + np.maximum.at + the blend on the occupied cells
  view_640x480 / view_1920x1080  ops.render_view from an outside camera (smax 16), image copied back; colours resident
  view_numpy_640x480             a NumPy painter: project, sort far to near, paint single pixels (no footprints: a lower bound)
  render_heat_topdown / _orbit   AVLMap.render_heat end to end on resident grid_pos / grid_rgb with a host heat (8 MB upload)
Every path ends synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it."""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from avlmaps_amd.map.avlmap import AVLMap  # noqa: E402
from avlmaps_amd.utils.visualize_utils import frame_intrinsics, orbit_camera  # noqa: E402
from probe_morph2d import stats  # noqa: E402


def numpy_colorize(heat, rgb, t, table):
    sim_new = (heat * 255).astype(np.uint8)
    h = table[sim_new].reshape(-1, 3).astype(np.float32)
    return h * t + rgb * (1 - t)


def numpy_topdown(pos, heat, rgb, gs, t, table):
    cell = pos[:, 0].astype(np.int64) * gs + pos[:, 1]
    order = np.lexsort((pos[:, 2], cell))
    sc = cell[order]
    last = np.flatnonzero(np.concatenate([sc[1:] != sc[:-1], [True]]))
    top = order[last]
    hmax = np.zeros(gs * gs, heat.dtype)
    np.maximum.at(hmax, cell, heat)
    cells = sc[last]
    idx = (hmax[cells] * 255).astype(np.uint8)
    out = np.zeros((gs * gs, 3), np.uint8)
    out[cells] = (table[idx].astype(np.float32) * t + rgb[top] * (1 - t)).astype(np.uint8)
    return out.reshape(gs, gs, 3)


def numpy_view(pos, color, T, fx, fy, cx, cy, size, znear):
    W, H = size
    P = pos.astype(np.float64)
    x, y, z = (T[k, 0] * P[:, 0] + T[k, 1] * P[:, 1] + T[k, 2] * P[:, 2] + T[k, 3] for k in range(3))
    keep = z > znear
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = np.floor(fx * x / z + cx), np.floor(fy * y / z + cy)
    keep &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
    ids = np.flatnonzero(keep)
    ids = ids[np.argsort(-z[ids], kind="stable")]
    img = np.zeros((H, W, 3), np.uint8)
    img[v[ids].astype(np.int64), u[ids].astype(np.int64)] = color[ids]          # later (nearer) assignments win
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    gs, vh, N, t = 1000, 60, a.voxels, 0.5
    rng = np.random.default_rng(0)
    flat = rng.choice(gs * gs * vh, N, replace=False)
    pos = np.stack([flat // (gs * vh), (flat // vh) % gs, flat % vh], axis=1).astype(np.int32)
    heat = rng.random(N).astype(np.float32)
    rgb = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    table = ops.jet_table()
    dpos, dheat, drgb, dtable = (DeviceArray.from_numpy(x) for x in (pos, heat, rgb, table))
    dcolor = ops.colorize_heat(dheat, drgb, t, table=dtable, as_uint8=True, device=True)
    color = dcolor.numpy()
    T = orbit_camera(pos)
    res = {"voxels": N, "gs": gs, "vh": vh, "method": "host clock around synchronised calls, median of reps", "cases": {}}
    same = {"colorize": bool(np.array_equal(ops.colorize_heat(dheat, drgb, t, table=dtable), numpy_colorize(heat, rgb, t, table))),
            "topdown": bool(np.array_equal(ops.render_topdown(dpos, dheat, drgb, gs, table=dtable), numpy_topdown(pos, heat, rgb, gs, t, table)))}
    res["same"] = same
    c = res["cases"]
    c["colorize_f64"] = stats(lib, lambda: ops.colorize_heat(dheat, drgb, t, table=dtable, device=True), a.reps, a.warmup)
    c["colorize_u8"] = stats(lib, lambda: ops.colorize_heat(dheat, drgb, t, table=dtable, as_uint8=True, device=True), a.reps, a.warmup)
    c["colorize_u8_to_host"] = stats(lib, lambda: ops.colorize_heat(dheat, drgb, t, table=dtable, as_uint8=True), a.reps, a.warmup)
    c["colorize_numpy"] = stats(lib, lambda: numpy_colorize(heat, rgb, t, table).astype(np.uint8), a.reps, a.warmup)
    c["topdown"] = stats(lib, lambda: ops.render_topdown(dpos, dheat, drgb, gs, table=dtable), a.reps, a.warmup)
    c["topdown_host_arrays"] = stats(lib, lambda: ops.render_topdown(pos, heat, rgb, gs, table=table), a.reps, a.warmup)
    c["topdown_numpy"] = stats(lib, lambda: numpy_topdown(pos, heat, rgb, gs, t, table), max(3, a.reps // 6), 1)
    for size in ((640, 480), (1920, 1080)):
        k = frame_intrinsics(size)
        c[f"view_{size[0]}x{size[1]}"] = stats(lib, lambda: ops.render_view(dpos, dcolor, T, *k, size, znear=1.0, smax=16), a.reps, a.warmup)
    k = frame_intrinsics((640, 480))
    c["view_numpy_640x480"] = stats(lib, lambda: numpy_view(pos, color, T, *k, (640, 480), 1.0), max(3, a.reps // 6), 1)
    # AVLMap.render_heat needs nothing of AVLMap but its vlmap's resident arrays
    vm = SimpleNamespace(grid_pos=pos, grid_rgb=rgb, gs=gs, _device_pos=lambda: dpos, _device_rgb=lambda: drgb)
    av = SimpleNamespace(vlmap=vm)
    c["render_heat_topdown"] = stats(lib, lambda: AVLMap.render_heat(av, heat), a.reps, a.warmup)
    c["render_heat_orbit_640x480"] = stats(lib, lambda: AVLMap.render_heat(av, heat, view=T, size=(640, 480), znear=1.0), a.reps, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
