"""Score a saved VLMap against the scene's ground-truth label map.  Upstream has no counterpart: its GT pieces stop at loading
(avlmaps/map/gtmap.py:18-30, habitat_dataloader.py:85).

    python -m avlmaps_amd.apps.evaluate_map --data-dir <scene> --categories-file FILE [--text-model clip|hash] [--dim 3d|2d]
                                            [--config cfg.yaml] [--json OUT]

<scene>/vlmap holds vlmaps.h5df and gt_labels.npz (apps.create_map --gt).  --categories-file lists the class names, one per line,
the line number being the class id of the GT map; the map's prediction for a voxel is the best of these names and "other"
(VLMap.init_categories).  --dim 3d compares voxel by voxel, 2d the top-down label maps over the obstacle crop.  Prints pixel
accuracy, mean accuracy, mIoU and frequency-weighted IoU and the per-class table; --json writes them to a file."""
from __future__ import annotations

import argparse


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--categories-file", required=True, metavar="FILE", help="class names, one per line; the line number is the class id")
    ap.add_argument("--config", default=None)
    ap.add_argument("--text-model", choices=["clip", "hash"], default="clip",
                    help="clip = OpenAI CLIP on PyTorch-ROCm (as upstream); hash = model-free stand-in for smoke runs")
    ap.add_argument("--dim", choices=["3d", "2d"], default="3d", help="3d = per voxel; 2d = per cell of the top-down maps")
    ap.add_argument("--json", default=None, metavar="OUT", help="write the scores as JSON")
    return ap.parse_args(argv)


def format_scores(scores) -> str:
    d = scores.as_dict()
    f = lambda x: "   nan" if x is None else f"{x:6.4f}"       # noqa: E731
    lines = [f"pixel_acc {f(d['pixel_acc'])}  mean_acc {f(d['mean_acc'])}  mIoU {f(d['miou'])}  fwIoU {f(d['fwiou'])}  "
             f"({d['total']} compared, skipped {d['skipped']})",
             f"{'id':>4} {'class':<24} {'support':>10} {'acc':>7} {'iou':>7}"]
    for c in d["classes"]:
        lines.append(f"{c['id']:>4} {c['name'][:24]:<24} {c['support']:>10} {f(c['acc']):>7} {f(c['iou']):>7}")
    return "\n".join(lines)


def main(argv=None):
    args = parse_args(argv)
    from avlmaps_amd.apps.common import HashClip, load_config, read_categories_file
    from avlmaps_amd.map import GTMap, VLMap
    cfg = load_config(args.config)
    categories = read_categories_file(args.categories_file)
    vm = VLMap(cfg.map_config)
    if not vm.load_map(args.data_dir):
        raise SystemExit(1)
    gt = GTMap(cfg.map_config)
    if not gt.load_map(args.data_dir, vlmap=vm):
        raise SystemExit(1)
    if len(categories) != len(gt.categories):
        raise SystemExit(f"{args.categories_file} lists {len(categories)} classes, the GT map has {len(gt.categories)}")
    gt.load_categories(categories)
    if args.text_model == "hash":
        vm.clip_feat_dim = vm.grid_feat.shape[1]
        vm.clip_model = HashClip(vm.clip_feat_dim)
    else:
        vm._init_clip()
    scores = gt.evaluate(vm, dim=args.dim)
    print(format_scores(scores))
    if args.json:
        import json
        from pathlib import Path
        Path(args.json).write_text(json.dumps(dict(scores.as_dict(), dim=args.dim), indent=1))
    return scores


if __name__ == "__main__":
    main()
