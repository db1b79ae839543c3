"""Plan a path to a named object on a saved VLMap: name -> goal cell -> path.  Counterpart of the reference's HabitatLanguageRobot
setup_scene + move_to (robot/habitat_lang_robot.py:88-104, 432-461) without the simulator.

    python -m avlmaps_amd.apps.plan_path --data-dir <scene> --query sofa --start ROW COL [--text-model clip|hash]

Loads <scene>/vlmap/vlmaps.h5df (with --text-model hash a missing map is first created with the model-free feature stand-in, as
apps.create_map --features hash does), builds the obstacle map (Map.generate_obstacle_map), takes the goal from
Map.get_nearest_pos, plans with Navigator on the GPU and prints one JSON line: the query, the start, the goal and the path, all
in full-map (row, col) cells."""
from __future__ import annotations

import argparse
import json


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--query", required=True)
    ap.add_argument("--start", type=float, nargs=2, required=True, metavar=("ROW", "COL"), help="full-map cell of the robot")
    ap.add_argument("--config", default=None)
    ap.add_argument("--text-model", choices=["clip", "hash"], default="clip",
                    help="clip = OpenAI CLIP on PyTorch-ROCm (as upstream); hash = model-free stand-ins for smoke runs")
    ap.add_argument("--categories", default=None, help="comma separated category list of get_pos (default: the query and 'other')")
    ap.add_argument("--h-min", type=float, default=0.0)
    ap.add_argument("--h-max", type=float, default=1.5)
    args = ap.parse_args(argv)

    from avlmaps_amd.apps.common import HashClip, load_config
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.navigator import Navigator
    cfg = load_config(args.config)
    hashed = args.text_model == "hash"
    vm = VLMap(cfg.map_config, data_dir=args.data_dir)
    if not vm.load_map(args.data_dir):
        if not hashed:
            raise SystemExit(f"no map under {args.data_dir}: run apps.create_map first")
        from avlmaps_amd.apps import create_map
        create_map.main(["--data-dir", args.data_dir, "--features", "hash", "--feat-dim", "64"]
                        + (["--config", args.config] if args.config else []))
        if not vm.load_map(args.data_dir):
            raise SystemExit(1)
    if hashed:
        vm.clip_feat_dim = vm.grid_feat.shape[1]
        vm.clip_model = HashClip(vm.clip_feat_dim)
    else:
        vm._init_clip()
    cats = [c.strip() for c in args.categories.split(",")] if args.categories else [args.query, "other"]
    vm.init_categories(cats)
    vm.generate_obstacle_map(args.h_min, args.h_max)
    start = [float(args.start[0]), float(args.start[1])]
    goal = vm.get_nearest_pos(start, args.query)
    nav = Navigator()
    try:
        nav.build_visgraph(vm.obstacles_cropped, vm.rmin, vm.cmin)
        path = nav.plan_to(start, goal)
    finally:
        nav.close()
    out = {"query": args.query, "start": start, "goal": [float(goal[0]), float(goal[1])],
           "path": [[float(p[0]), float(p[1])] for p in path]}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
