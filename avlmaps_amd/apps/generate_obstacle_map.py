"""Write a saved VLMap's obstacle map and its customised version as images.  Counterpart of the reference's
application/generate_obstacle_map.py (:19-33), with PNG files where upstream opens cv2 windows.

    python -m avlmaps_amd.apps.generate_obstacle_map --data-dir <scene> [--out-dir DIR] [--text-model clip|hash]
                                                     [--potential-obstacles a,b,c --obstacles a,b] [--dilate-iter N] [--gaussian-sigma S]
                                                     [--known-free] [--rooms [--door-width M] [--min-core-area M2]]

Loads <scene>/vlmap/vlmaps.h5df, builds the obstacle map from the occupancy between --h-min and --h-max
(Map.generate_obstacle_map), then keeps only the obstacles of the classes --obstacles and smooths the map
(VLMap.customize_obstacle_map; the class lists and the smoothing parameters default to the map config's).  Writes obstacles.png
and obstacles_customized.png (white = free, the cropped maps) under --out-dir (default <scene>/vlmap) and prints one JSON line with
the crop and the number of obstacle cells of both maps.  With --known-free it also writes obstacles_known_free.png: the obstacle map
AND-ed with the explored map (Map.get_known_free_cropped; needs <scene>/vlmap/explored.npz, apps.create_map --explored), in which a
cell no camera ever looked at is not free.  With --rooms it also writes rooms.png: the rooms of the customised map (Map.get_rooms with
customized=True), room k of n in the colour (255 k) // n of the heat maps' colour table (ops.jet_table), cells of
no room black; the JSON line then has "rooms", the number of rooms, and "doors", the door table's (i, j, door row, door col)."""
from __future__ import annotations

import argparse
import json
from pathlib import Path


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--config", default=None)
    ap.add_argument("--text-model", choices=["clip", "hash"], default="clip",
                    help="clip = OpenAI CLIP on PyTorch-ROCm (as upstream); hash = model-free stand-in for smoke runs")
    ap.add_argument("--h-min", type=float, default=0.0)
    ap.add_argument("--h-max", type=float, default=1.5)
    ap.add_argument("--potential-obstacles", default=None, help="comma separated class list the voxels are scored against")
    ap.add_argument("--obstacles", default=None, help="comma separated classes (of --potential-obstacles) that stay obstacles")
    ap.add_argument("--dilate-iter", type=int, default=None)
    ap.add_argument("--gaussian-sigma", type=float, default=None)
    ap.add_argument("--known-free", action="store_true", help="also write obstacles_known_free.png (free AND observed)")
    ap.add_argument("--rooms", action="store_true", help="also write rooms.png (Map.get_rooms on the customised map)")
    ap.add_argument("--door-width", type=float, default=None, metavar="M", help="--rooms: openings up to M metres separate rooms (default 0.9)")
    ap.add_argument("--min-core-area", type=float, default=None, metavar="M2", help="--rooms: the smallest room core in square metres (default 0.25)")
    args = ap.parse_args(argv)
    if not args.rooms and (args.door_width is not None or args.min_core_area is not None):
        ap.error("--door-width and --min-core-area belong to --rooms")
    return args


def room_colours(labels, n):
    """(H, W, 3) uint8: room k of n in entry (255 k) // n of ops.jet_table, label 0 black"""
    import numpy as np
    from avlmaps_amd import ops
    table = np.concatenate([np.zeros((1, 3), np.uint8), ops.jet_table()[(255 * np.arange(1, n + 1)) // max(n, 1)]])
    return table[np.asarray(labels)]


def save_mask_png(path, mask) -> None:
    """bool (H, W) -> 8-bit grey PNG, True = 255 (what upstream shows: obs_map.astype(np.uint8) * 255)"""
    import numpy as np
    from PIL import Image
    Image.fromarray(np.asarray(mask).astype(np.uint8) * 255).save(str(path))


def main(argv=None):
    args = parse_args(argv)

    from avlmaps_amd.apps.common import HashClip, load_config
    from avlmaps_amd.apps.plan_path import obstacle_overrides
    from avlmaps_amd.map import VLMap
    cfg = load_config(args.config, overrides={f"map_config.{k}": v for k, v in obstacle_overrides(args).items()})
    vm = VLMap(cfg.map_config, data_dir=args.data_dir)
    if not vm.load_map(args.data_dir):
        raise SystemExit(f"no map under {args.data_dir}: run apps.create_map first")
    if args.text_model == "hash":
        vm.clip_feat_dim = vm.grid_feat.shape[1]
        vm.clip_model = HashClip(vm.clip_feat_dim)
    else:
        vm._init_clip()
    vm.generate_obstacle_map(args.h_min, args.h_max)
    vm.customize_obstacle_map(cfg.map_config.potential_obstacle_names, cfg.map_config.obstacle_names)
    raw, custom = vm.get_obstacle_cropped(), vm.get_customized_obstacle_cropped()
    out_dir = Path(args.out_dir) if args.out_dir else Path(args.data_dir) / "vlmap"
    out_dir.mkdir(parents=True, exist_ok=True)
    save_mask_png(out_dir / "obstacles.png", raw)
    save_mask_png(out_dir / "obstacles_customized.png", custom)
    out = {"crop": [int(vm.rmin), int(vm.rmax), int(vm.cmin), int(vm.cmax)], "shape": [int(raw.shape[0]), int(raw.shape[1])],
           "obstacle_cells": int((raw == 0).sum()), "customized_obstacle_cells": int((custom == 0).sum()),
           "files": [str(out_dir / "obstacles.png"), str(out_dir / "obstacles_customized.png")]}
    if args.known_free:
        if vm.first_seen is None:
            raise SystemExit(f"no explored map under {args.data_dir}: run apps.create_map --explored first")
        known = vm.get_known_free_cropped()
        save_mask_png(out_dir / "obstacles_known_free.png", known)
        out["known_free_blocked_cells"] = int((known == 0).sum())
        out["files"].append(str(out_dir / "obstacles_known_free.png"))
    if args.rooms:
        from PIL import Image
        rooms = vm.get_rooms(0.9 if args.door_width is None else args.door_width, 0.25 if args.min_core_area is None else args.min_core_area,
                            customized=True)
        Image.fromarray(room_colours(rooms.labels, rooms.n)).save(str(out_dir / "rooms.png"))
        out["rooms"] = rooms.n
        out["doors"] = rooms.doors[:, [0, 1, 7, 8]].tolist()
        out["files"].append(str(out_dir / "rooms.png"))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
