"""Find the stale voxels of a saved VLMap: voxels that later frames saw through.  Upstream has no counterpart (its maps are static).

    python -m avlmaps_amd.apps.audit_map --data-dir <scene> [--revisit <dir> ...] [--stride 4] [--end-margin 2] [--min-rays 3]
                                         [--prune --out <dir>] [--render PNG] [--config YAML]

Loads <scene>/vlmap/vlmaps.h5df and walks the depth rays of the scene's frames, then of every --revisit directory (the same
dataset layout, poses.txt in the scene's world frame), through the map's voxels (Map.audit_visibility): per voxel
the last frame that hit it and the rays of later frames that passed through it.  A voxel with at least --min-rays such rays is
stale.  Writes <scene>/vlmap/visibility.npz and prints one JSON line with the voxel counts: hit, seen through, stale.  --prune
removes the stale voxels and saves the pruned map under --out/vlmap (the input map is only overwritten when --out is the scene
itself).  --render writes a top-down PNG of the map's columns: grey = kept voxels, white = a stale voxel in the column."""
from __future__ import annotations

import argparse
import json
from pathlib import Path


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--revisit", action="append", default=[], help="a later recording of the same place (repeatable)")
    ap.add_argument("--config", default=None)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--end-margin", type=int, default=2)
    ap.add_argument("--min-rays", type=int, default=3)
    ap.add_argument("--prune", action="store_true", help="remove the stale voxels and save the map under --out")
    ap.add_argument("--out", default=None, help="scene directory the pruned map is written to (needed with --prune)")
    ap.add_argument("--render", default=None, help="PNG of the stale voxels over the map, top-down")
    args = ap.parse_args(argv)
    if args.prune and not args.out:
        ap.error("--prune needs --out (pass the scene itself to overwrite its map)")
    return args


def main(argv=None):
    args = parse_args(argv)

    import numpy as np
    from avlmaps_amd import ops
    from avlmaps_amd.apps.common import load_config
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.utils.mapping_utils import save_3d_map
    cfg = load_config(args.config)
    vm = VLMap(cfg.map_config, data_dir=args.data_dir)
    vm.prefetch_device = False                          # no query follows: the features stay on the host
    if not vm.load_map(args.data_dir):
        raise SystemExit(f"no map under {args.data_dir}: run apps.create_map first")
    audit = vm.audit_visibility([args.data_dir, *args.revisit], stride=args.stride, end_margin=args.end_margin)
    stale = audit.stale(args.min_rays)
    out = {"voxels": audit.N, "frames": audit.frame_counts, "hit": int((audit.last_hit >= 0).sum()),
           "seen_through": int((audit.through > 0).sum()), "stale": int(stale.sum()),
           "files": [str(Path(args.data_dir) / "vlmap" / vm.VISIBILITY_FILE)]}
    if args.render:
        gs = int(vm.gs)
        image = np.zeros((gs, gs), np.uint8)
        if audit.N:
            image[ops.pool_label_2d(np.ones((audit.N,), np.uint8), vm.grid_pos, gs) != 0] = 128
            image[ops.pool_label_2d(stale.astype(np.uint8), vm.grid_pos, gs) != 0] = 255
        from PIL import Image
        Image.fromarray(image).save(str(args.render))
        out["files"].append(str(args.render))
    if args.prune:
        out["removed"] = vm.prune_voxels(stale)
        save_dir = Path(args.out) / "vlmap"
        save_dir.mkdir(parents=True, exist_ok=True)
        save_3d_map(save_dir / "vlmaps.h5df", vm.grid_feat, vm.grid_pos, vm.weight, vm.occupied_ids, vm.mapped_iter_list, vm.grid_rgb)
        out["files"].append(str(save_dir / "vlmaps.h5df"))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
