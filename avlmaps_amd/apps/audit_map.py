"""Find the stale voxels of a saved VLMap: voxels that later frames saw through.  Upstream has no counterpart (its maps are static).

    python -m avlmaps_amd.apps.audit_map --data-dir <scene> [--revisit <dir> ...] [--stride 4] [--end-margin 2] [--min-rays 3]
                                         [--prune --out <dir>] [--render PNG] [--config YAML]
                                         [--register [--register-angle DEG] [--register-step DEG] [--register-radius M]
                                                     [--register-min-fraction F]]
                                         [--compare OTHER_SCENE_DIR [--compare-radius R] [--compare-threshold T]
                                                    [--compare-shift DR DC DH] [--compare-json PATH]]
                                         [--fuse OTHER_SCENE_DIR --fuse-out DIR [--fuse-keep-vanished] [--fuse-keep-changed]
                                                 [--fuse-gain G] [--fuse-json PATH]
                                                 [--fuse-resample forward|nearest|linear] [--fuse-min-support S]]

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
--register-min-fraction of the points land on occupied cells is not audited under a bad pose: the app stops with a message.

--compare loads the map under OTHER_SCENE_DIR -- a later map of the same place on the same grid -- and says what changed between
the two (VLMap.compare): the JSON line then carries "compare": the summary (voxels that vanished, appeared, changed,
the changed volume in m^3) and the object-sized changes, which are also printed one per line.  A voxel's partner is the nearest
occupied cell of the other map within --compare-radius cells (0 .. 2, default 1); a pair whose feature rows have a cosine below
--compare-threshold (default 0.8) counts as changed; --compare-shift moves this map's cells by whole cells first.  The audit of
this map under the --revisit frames tells vanished from never looked at.  --compare-json also writes the summary and the list to
PATH.  Whole-cell shifts only: for a revisit from another odometry origin use --fuse, which resamples it onto this grid first.

--fuse loads the map under OTHER_SCENE_DIR -- a later map of the same place, built on its own -- and folds it into this one
(VLMap.fuse): the transform between the two recordings' frames (Map.transform_from; with --register corrected by
the registration of OTHER_SCENE_DIR's frames to this map), the other map resampled onto this grid (VLMap.resample), the comparison
of the two (VLMap.compare with the --compare-* settings), then the fusion: vanished voxels of this map leave (unless
--fuse-keep-vanished), replaced ones give way to the other map's (unless --fuse-keep-changed), shared cells get the weighted mean,
with the other map's weights times --fuse-gain (default 1).  The fused map is saved under --fuse-out/vlmap, which may be neither
input scene: no input map is written over.  The JSON line then carries "fuse": the transform, the comparison's summary and the
counts; --fuse-json also writes that to PATH.  --fuse-resample chooses how the other map is resampled (VLMap.resample's method,
DESIGN.md 4.34): forward (the default) moves every voxel to its nearest cell and leaves pinholes under a rotation, which the
comparison reads as vanished voxels; linear and nearest ask backward from every cell of this grid and leave none -- use linear for
a turned revisit, nearest where features must not be blended across object borders.  --fuse-min-support (0 < S <= 1, default 0.5)
is linear's threshold on a cell's support.  The "fuse" JSON echoes both."""
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
    ap.add_argument("--compare", default=None, metavar="OTHER_SCENE_DIR", help="a later map of the same place: list what changed")
    ap.add_argument("--compare-radius", type=int, default=None, help="cells within which a voxel finds its partner, 0 .. 2 (default 1)")
    ap.add_argument("--compare-threshold", type=float, default=None, help="cosine below which a matched pair has changed (default 0.8)")
    ap.add_argument("--compare-shift", type=int, nargs=3, default=None, metavar=("DR", "DC", "DH"),
                    help="this map's cell c is the other map's cell c + shift (default 0 0 0)")
    ap.add_argument("--compare-json", default=None, metavar="PATH", help="also write the summary and the change list to PATH")
    ap.add_argument("--compare-min-voxels", type=int, default=None, help="smallest component listed as a change (default 20)")
    ap.add_argument("--fuse", default=None, metavar="OTHER_SCENE_DIR", help="a later map of the same place, built on its own: fold it into this one")
    ap.add_argument("--fuse-out", default=None, metavar="DIR", help="scene directory the fused map is written to (needed with --fuse)")
    ap.add_argument("--fuse-keep-vanished", action="store_true", help="keep this map's voxels that the other map no longer holds")
    ap.add_argument("--fuse-keep-changed", action="store_true", help="average replaced voxels with the other map's instead of giving way")
    ap.add_argument("--fuse-gain", type=float, default=None, help="factor on the other map's weights, > 0 (default 1)")
    ap.add_argument("--fuse-json", default=None, metavar="PATH", help="also write the transform, the summary and the counts to PATH")
    ap.add_argument("--fuse-resample", default=None, choices=("forward", "nearest", "linear"),
                    help="how the other map is resampled onto this grid (default forward; linear for a turned revisit)")
    ap.add_argument("--fuse-min-support", type=float, default=None, metavar="S",
                    help="the support a cell needs under --fuse-resample linear, 0 < S <= 1 (default 0.5)")
    args = ap.parse_args(argv)
    if args.fuse is None and (args.fuse_out or args.fuse_keep_vanished or args.fuse_keep_changed or args.fuse_gain is not None or args.fuse_json):
        ap.error("--fuse-out, --fuse-keep-vanished, --fuse-keep-changed, --fuse-gain and --fuse-json need --fuse")
    if args.fuse is None and (args.fuse_resample is not None or args.fuse_min_support is not None):
        ap.error("--fuse-resample and --fuse-min-support need --fuse")
    if args.fuse_min_support is not None and args.fuse_resample != "linear":
        ap.error("--fuse-min-support needs --fuse-resample linear")
    if args.fuse_resample is None:
        args.fuse_resample = "forward"
    if args.fuse_min_support is None:
        args.fuse_min_support = 0.5
    if not 0.0 < args.fuse_min_support <= 1.0:
        ap.error("--fuse-min-support is greater than 0 and at most 1")
    if args.fuse is not None:
        if not args.fuse_out:
            ap.error("--fuse needs --fuse-out")
        if Path(args.fuse_out).resolve() in (Path(args.data_dir).resolve(), Path(args.fuse).resolve()):
            ap.error("--fuse-out may be neither input scene: no input map is written over")
    if args.fuse_gain is None:
        args.fuse_gain = 1.0
    if not (args.fuse_gain > 0.0 and args.fuse_gain < float("inf")):
        ap.error("--fuse-gain is a finite factor greater than 0")
    compare = ("compare_radius", "compare_threshold", "compare_shift", "compare_json", "compare_min_voxels")
    if args.compare is None and args.fuse is None and any(getattr(args, k) is not None for k in compare):
        ap.error("--compare-radius, --compare-threshold, --compare-shift, --compare-json and --compare-min-voxels need --compare")
    for k, default in zip(compare, (1, 0.8, [0, 0, 0], None, 20)):
        if getattr(args, k) is None:
            setattr(args, k, default)
    if not 0 <= args.compare_radius <= 2:
        ap.error("--compare-radius is 0, 1 or 2 cells")
    if not 0.0 < args.compare_threshold <= 1.0:
        ap.error("--compare-threshold is a cosine, 0 < T <= 1")
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
    if args.compare:
        other = VLMap(cfg.map_config, data_dir=args.compare)
        other.prefetch_device = False
        if not other.load_map(args.compare):
            raise SystemExit(f"no map under {args.compare}: run apps.create_map first")
        # the audit above saw this map through the --revisit frames: with a revisit, an unmatched voxel they never looked at is unseen
        changes = vm.compare(other, radius=args.compare_radius, threshold=args.compare_threshold, shift=tuple(args.compare_shift),
                             audit=audit if args.revisit else None, min_rays=args.min_rays)
        found = [c.to_json() for c in changes.objects(min_voxels=args.compare_min_voxels)]
        out["compare"] = {"other": str(args.compare), "summary": changes.summary(), "changes": found}
        for c in found:
            print(f"{c['kind']:9s} {c['count']:7d} voxels  box {c['bbox']}  {c.get('name', '')}")
        if args.compare_json:
            Path(args.compare_json).write_text(json.dumps(out["compare"]))
            out["files"].append(str(args.compare_json))
    if args.prune:
        out["removed"] = vm.prune_voxels(stale)
        save_dir = Path(args.out) / "vlmap"
        save_dir.mkdir(parents=True, exist_ok=True)
        save_3d_map(save_dir / "vlmaps.h5df", vm.grid_feat, vm.grid_pos, vm.weight, vm.occupied_ids, vm.mapped_iter_list, vm.grid_rgb)
        out["files"].append(str(save_dir / "vlmaps.h5df"))
    if args.fuse:
        other = VLMap(cfg.map_config, data_dir=args.fuse)
        other.prefetch_device = False
        if not other.load_map(args.fuse):
            raise SystemExit(f"no map under {args.fuse}: run apps.create_map first")
        reg = None
        if args.register:
            reg = vm.register_frames(args.fuse, max_angle_deg=args.register_angle, angle_step_deg=args.register_step,
                                     radius_m=args.register_radius, stride=args.stride)
            if reg.fraction[0] < args.register_min_fraction:
                raise SystemExit(f"{args.fuse}: only {reg.fraction[0]:.2f} of {int(reg.valid[0])} depth points land on the map at the best pose "
                                 f"found (--register-min-fraction {args.register_min_fraction}): not fusing under a pose this poor")
        T = vm.transform_from(args.fuse, registration=reg)
        moved = other.resample(T, method=args.fuse_resample, min_support=args.fuse_min_support)
        changes = vm.compare(moved, radius=args.compare_radius, threshold=args.compare_threshold)
        counts = vm.fuse(moved, changes=changes, drop_vanished=not args.fuse_keep_vanished, replace_changed=not args.fuse_keep_changed,
                         gain=args.fuse_gain)
        save_dir = Path(args.fuse_out) / "vlmap"
        save_dir.mkdir(parents=True, exist_ok=True)
        save_3d_map(save_dir / "vlmaps.h5df", vm.grid_feat, vm.grid_pos, vm.weight, vm.occupied_ids, vm.mapped_iter_list, vm.grid_rgb)
        out["files"].append(str(save_dir / "vlmaps.h5df"))
        out["fuse"] = {"other": str(args.fuse), "transform": [[float(v) for v in row] for row in T], "resampled": moved.resample_counts,
                       "resample": args.fuse_resample, "min_support": args.fuse_min_support,
                       "summary": changes.summary(), "counts": counts}
        if args.fuse_json:
            Path(args.fuse_json).write_text(json.dumps(out["fuse"]))
            out["files"].append(str(args.fuse_json))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
