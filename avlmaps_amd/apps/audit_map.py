"""Find the stale voxels of a saved VLMap: voxels that later frames saw through.  Upstream has no counterpart (its maps are static).

    python -m avlmaps_amd.apps.audit_map --data-dir <scene> [--revisit <dir> ...] [--stride 4] [--end-margin 2] [--min-rays 3]
                                         [--prune --out <dir>] [--render PNG] [--config YAML]
                                         [--register [--register-angle DEG] [--register-step DEG] [--register-radius M]
                                                     [--register-min-fraction F]]

Loads <scene>/vlmap/vlmaps.h5df and walks the depth rays of the scene's frames, then of every --revisit directory (the same
dataset layout, poses.txt in the scene's world frame), through the map's voxels (Map.audit_visibility): per voxel
the last frame that hit it and the rays of later frames that passed through it.  A voxel with at least --min-rays such rays is
stale.  Writes <scene>/vlmap/visibility.npz and prints one JSON line with the voxel counts: hit, seen through, stale.  --prune
removes the stale voxels and saves the pruned map under --out/vlmap (the input map is only overwritten when --out is the scene
itself).  --render writes a top-down PNG of the map's columns: grey = kept voxels, white = a stale voxel in the column.

--register first registers every --revisit directory to the map (Map.register_frames, DESIGN.md 4.23: a search over planar rotations
of up to --register-angle degrees in steps of --register-step and whole-cell shifts of up to --register-radius metres) and audits
it under the correction found, for a recording whose poses.txt is NOT in the scene's world frame.  The JSON line then carries
"registration": one {dir, angle_deg, shift_cells, score, valid, fraction} per revisit.  A revisit of which fewer than
--register-min-fraction of the points land on occupied cells is not audited under a bad pose: the app stops with a message."""
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
    ap.add_argument("--register", action="store_true", help="register every --revisit directory to the map before the audit")
    ap.add_argument("--register-angle", type=float, default=None, help="largest rotation searched, degrees (default 10)")
    ap.add_argument("--register-step", type=float, default=None, help="angle step, degrees (default 0.5)")
    ap.add_argument("--register-radius", type=float, default=None, help="largest shift searched, metres (default 0.5)")
    ap.add_argument("--register-min-fraction", type=float, default=None,
                    help="stop when fewer than this share of a revisit's points land on occupied cells (default 0.5)")
    args = ap.parse_args(argv)
    if args.prune and not args.out:
        ap.error("--prune needs --out (pass the scene itself to overwrite its map)")
    tuning = ("register_angle", "register_step", "register_radius", "register_min_fraction")
    if not args.register and any(getattr(args, k) is not None for k in tuning):
        ap.error("--register-angle, --register-step, --register-radius and --register-min-fraction need --register")
    for k, default in zip(tuning, (10.0, 0.5, 0.5, 0.5)):
        if getattr(args, k) is None:
            setattr(args, k, default)
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
    corrections, registration = None, []
    if args.register:
        corrections = [None]
        for d in args.revisit:
            reg = vm.register_frames(d, max_angle_deg=args.register_angle, angle_step_deg=args.register_step, radius_m=args.register_radius,
                                     stride=args.stride)
            registration.append({"dir": str(d), "angle_deg": float(reg.angle_deg[0]), "shift_cells": [int(x) for x in reg.shift_cells[0]],
                                 "score": int(reg.score[0]), "valid": int(reg.valid[0]), "fraction": float(reg.fraction[0])})
            if reg.fraction[0] < args.register_min_fraction:
                raise SystemExit(f"{d}: only {reg.fraction[0]:.2f} of {int(reg.valid[0])} depth points land on the map at the best pose found "
                                 f"(--register-min-fraction {args.register_min_fraction}): not auditing under a pose this poor")
            corrections.append(reg.correction)
    audit = vm.audit_visibility([args.data_dir, *args.revisit], stride=args.stride, end_margin=args.end_margin, corrections=corrections)
    stale = audit.stale(args.min_rays)
    out = {"voxels": audit.N, "frames": audit.frame_counts, "hit": int((audit.last_hit >= 0).sum()),
           "seen_through": int((audit.through > 0).sum()), "stale": int(stale.sum()),
           "files": [str(Path(args.data_dir) / "vlmap" / vm.VISIBILITY_FILE)]}
    if args.register:
        out["registration"] = registration
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
