"""Index a saved AVLMap with a goal query.  Counterpart of the reference's application/index_map.py (the object, area, sound
and image branches, :23-142; the Open3D viewer and the habitat branches are not part of the hot path).

    python -m avlmaps_amd.apps.index_map --data-dir <scene> --query sofa [--modality object|area|sound|image]
                                         [--decay-rate R] [--text-model clip|hash]
    python -m avlmaps_amd.apps.index_map --data-dir <scene> --modality fused [--object NAME]... [--area NAME]... [--sound NAME]...
                                         [--image PNG] [--object-decay R] [--area-decay R] [--sound-decay R] [--image-decay R]
    ... --modality object --categories A,B,...   [--instances] [--instance K] [--min-voxels M] [--connectivity 6|18|26]
    ... --modality object --categories A,B,...   --quantile P [--instances]
    ... --modality object --categories A,B,...   [--inventory] [--inventory-json PATH] [--min-voxels M] [--connectivity 6|18|26]
    ... --modality object --categories A,B,...   --inventory --relations [--relation-radius M] [--relations-json PATH]
    ... --modality object --categories A,B,...   --inventory --rooms [--door-width M]
    ... --modality object --categories A,B,...   --related "SUBJECT near|on|under|touching ANCHOR" [--relation-radius M]
    ... any modality ...                 [--render PNG [--view topdown|frame:<i>|orbit] [--render-size W H]] [--save-ply PLY]

object (default): the VLMap text query; area: the area map's frame embeddings (area_map/clip_sparse_map.h5df); sound: the sound
map (audio_video/audio_data_<difficulty>.pkl); image: --image (a PNG) localised at row --image-pose of poses.txt (the model-free
localiser; upstream uses HLoc); fused: the cross-modal goal, the product of every --object, --area, --sound and --image heat
(AVLMap.index_goal; at least one of them, decay rates default to the stand-alone queries' 0.1, 0.1, 0.01, 0.01).  Prints the heat statistics and the voxel the navigator would go to (argmax of the heat,
habitat_lang_robot.py:427-430); --save writes the (N,) heat vector as .npy (float64 for fused).

--instances lists the objects of the queried category in 3-D (VLMap.get_instances_3d: the connected components of its voxels), one
line each: label, voxels, box, centre, best score.  --instance K makes --save, --render and --save-ply use the heat of that object
alone (AVLMap.index_object_instance).  Both need --categories; --min-voxels and --connectivity are their two parameters.

--quantile P makes the object query open-set: the voxels of --query's category are those whose score lies above the P-th percentile
of the category's own score column (VLMap.index_map_quantile; upstream's map/clip_map.py:45-75 uses 95), not those whose row
maximum it is, so the answer does not depend on the other names in --categories.  The heat, --save, --render and --save-ply follow
that mask, and --instances lists its connected components.  Needs --categories.

--inventory lists what is in the scene (VLMap.get_objects: the objects of ALL of --categories in one labelling), one line each:
label, category, the category with the largest mean score over the object's voxels when it differs, voxels, box, centre, best
score and the margin between the two largest mean scores.  --inventory-json writes the same objects as JSON
(SceneObjects.to_json).  Both need --categories and reuse --min-voxels and --connectivity.

--relations, after --inventory, lists how the listed objects stand to one another (VLMap.get_scene_graph: every pair within
--relation-radius metres, at most 15 cells), one line each: the nearest gap and its two voxels, the touching voxel pairs, the voxels
of each lying directly on the other and who rests on whom.  --relations-json writes the same edges as JSON (SceneGraph.to_json).
--related "mug on table" makes --save, --render and --save-ply use the heat of the first such object alone
(AVLMap.index_related_object).  They need --categories and reuse --min-voxels and --connectivity.

--render writes the picture the reference shows in a window (visualize_heatmap_3d, application/index_map.py): the heat in JET
colours over the map's own, rendered on the GPU (AVLMap.render_heat).  --view topdown (default) is the map from above, frame:<i>
what the robot's camera saw at frame i, orbit an outside view of the whole map.  --save-ply writes the coloured voxels as a binary
PLY point cloud (visualize_heatmap_3d with save_path) for any viewer."""
from __future__ import annotations

import argparse

import numpy as np

DEFAULT_DECAY = {"object": 0.01, "area": 0.1, "sound": 0.01, "image": 0.01}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--query", default=None, help="object, area or sound name (not used by --modality image and fused)")
    ap.add_argument("--modality", choices=["object", "area", "sound", "image", "fused"], default="object")
    ap.add_argument("--config", default=None)
    ap.add_argument("--decay-rate", type=float, default=None, help="default: 0.01 (object, sound, image), 0.1 (area)")
    ap.add_argument("--text-model", choices=["clip", "hash"], default="clip",
                    help="clip = OpenAI CLIP on PyTorch-ROCm (as upstream); hash = model-free stand-ins for smoke runs (text towers "
                         "and the audio-text model)")
    ap.add_argument("--categories", default=None, help="comma separated list: preload scores_mat (VLMap.init_categories)")
    ap.add_argument("--instances", action="store_true", help="object: list the category's objects in 3-D (needs --categories)")
    ap.add_argument("--instance", type=int, default=None, metavar="K",
                    help="object: --save / --render / --save-ply use the heat of instance K alone (needs --categories)")
    ap.add_argument("--min-voxels", type=int, default=50, help="--instances / --instance: drop objects with fewer voxels (default 50)")
    ap.add_argument("--connectivity", type=int, choices=[6, 18, 26], default=26, help="--instances / --instance: voxel adjacency (default 26)")
    ap.add_argument("--quantile", type=float, default=None, metavar="P",
                    help="object: the voxels above the P-th percentile of the category's own scores instead of the row maximum "
                         "(needs --categories)")
    ap.add_argument("--inventory", action="store_true", help="object: list the objects of all categories in 3-D (needs --categories)")
    ap.add_argument("--inventory-json", default=None, metavar="PATH", help="object: write the inventory as JSON (needs --categories)")
    ap.add_argument("--relations", action="store_true", help="object: after --inventory, list how the listed objects stand to one another")
    ap.add_argument("--rooms", action="store_true", help="object: print the --inventory grouped by room (Map.get_rooms, SceneObjects.assign_rooms)")
    ap.add_argument("--door-width", type=float, default=None, metavar="M", help="--rooms: openings up to M metres separate rooms (default 0.9)")
    ap.add_argument("--relation-radius", type=float, default=0.25, metavar="M",
                    help="--relations / --relations-json / --related: objects within M metres are related (default 0.25; at most 15 cells)")
    ap.add_argument("--relations-json", default=None, metavar="PATH", help="object: write the relations as JSON (needs --categories)")
    ap.add_argument("--related", default=None, metavar="\"SUBJECT REL ANCHOR\"",
                    help="object: --save / --render / --save-ply use the heat of the first SUBJECT that is REL (near, on, under, "
                         "touching) an ANCHOR, e.g. \"mug on table\" (needs --categories)")
    ap.add_argument("--image", default=None, help="query image (PNG) of --modality image and fused")
    ap.add_argument("--image-pose", type=int, default=0, help="row of poses.txt the model-free localiser places the image at")
    ap.add_argument("--object", action="append", default=[], help="fused: an object name (repeatable)")
    ap.add_argument("--area", action="append", default=[], help="fused: an area name (repeatable)")
    ap.add_argument("--sound", action="append", default=[], help="fused: a sound name (repeatable)")
    ap.add_argument("--object-decay", type=float, default=None, help="fused: decay rate of the object heats (default 0.1)")
    ap.add_argument("--area-decay", type=float, default=None, help="fused: decay rate of the area heats (default 0.1)")
    ap.add_argument("--sound-decay", type=float, default=None, help="fused: decay rate of the sound heats (default 0.01)")
    ap.add_argument("--image-decay", type=float, default=None, help="fused: decay rate of the image heat (default 0.01)")
    ap.add_argument("--save", default=None)
    ap.add_argument("--render", default=None, metavar="PNG", help="write the heat over the map's colours as a PNG")
    ap.add_argument("--view", default="topdown", help="topdown (default), frame:<i> (the camera of frame i) or orbit")
    ap.add_argument("--render-size", type=int, nargs=2, default=[640, 480], metavar=("W", "H"), help="image size of a camera view")
    ap.add_argument("--save-ply", default=None, metavar="PLY", help="write the coloured voxels as a binary PLY point cloud")
    args = ap.parse_args(argv)
    if not valid_view(args.view):
        ap.error(f"--view {args.view}: expected topdown, orbit or frame:<i> with a frame number")
    if args.modality == "fused":
        if not (args.object or args.area or args.sound or args.image):
            ap.error("--modality fused needs at least one of --object, --area, --sound, --image")
    elif args.object or args.area or args.sound:
        ap.error("--object, --area and --sound belong to --modality fused")
    elif args.modality != "image" and not args.query:
        ap.error(f"--modality {args.modality} needs --query")
    elif args.modality == "image" and not args.image:
        ap.error("--modality image needs --image")
    if args.instances or args.instance is not None:
        if args.modality != "object" or not args.categories:
            ap.error("--instances and --instance need --modality object and --categories")
    if args.quantile is not None:
        if args.modality != "object" or not args.categories:
            ap.error("--quantile needs --modality object and --categories")
        if not 0.0 <= args.quantile <= 100.0:
            ap.error(f"--quantile {args.quantile}: a percentile lies in 0 .. 100")
        if args.instance is not None:
            ap.error("--instance picks an object of the row-maximum mask; with --quantile use --instances")
    if args.inventory or args.inventory_json:
        if args.modality != "object" or not args.categories:
            ap.error("--inventory and --inventory-json need --modality object and --categories")
    if args.relations and not args.inventory:
        ap.error("--relations lists the edges of the inventory: it needs --inventory")
    if args.rooms and not args.inventory:
        ap.error("--rooms groups the inventory by room: it needs --inventory")
    if args.door_width is not None and not args.rooms:
        ap.error("--door-width belongs to --rooms")
    if args.relations_json or args.related is not None:
        if args.modality != "object" or not args.categories:
            ap.error("--relations-json and --related need --modality object and --categories")
    if not (np.isfinite(args.relation_radius) and args.relation_radius > 0.0):
        ap.error(f"--relation-radius {args.relation_radius}: metres, finite and > 0")
    if args.related is not None:
        parts = args.related.split()
        if len(parts) != 3 or parts[1] not in ("near", "on", "under", "touching"):
            ap.error(f"--related {args.related!r}: expected \"SUBJECT REL ANCHOR\" with REL one of near, on, under, touching")
        if args.instance is not None:
            ap.error("--related and --instance both choose the heat: give one of them")
        args.related = tuple(parts)
    return args


def valid_view(view: str) -> bool:
    if view in ("topdown", "orbit"):
        return True
    return view.startswith("frame:") and view[len("frame:"):].isdigit()


def write_pictures(avlmap, heat, args) -> None:
    """--render and --save-ply of a finished query"""
    if args.render:
        from PIL import Image
        img = avlmap.render_heat(heat, view=args.view, size=tuple(args.render_size))
        Image.fromarray(img).save(args.render)
        print(f"wrote {args.render}: {args.view} view, {img.shape[1]} x {img.shape[0]}")
    if args.save_ply:
        from avlmaps_amd.utils.visualize_utils import visualize_heatmap_3d
        vm = avlmap.vlmap
        visualize_heatmap_3d(vm.grid_pos, heat, vm.grid_rgb, save_path=args.save_ply)
        print(f"wrote {args.save_ply}: {len(heat)} points")


def print_instances(instances, name: str) -> None:
    """--instances: one line per object of VLMap.get_instances_3d"""
    print(f"{len(instances)} instances of {name!r}")
    for it in instances:
        r0, r1, c0, c1, h0, h1 = it.bbox
        print(f"  instance {it.label}: {it.count} voxels, rows {r0}..{r1}, cols {c0}..{c1}, heights {h0}..{h1}, "
              f"centre ({it.center[0]:.2f}, {it.center[1]:.2f}, {it.center[2]:.2f}), best score {it.best_score:.4f} at voxel {it.best_voxel}")


def print_inventory(scene) -> None:
    """--inventory: one line per object of VLMap.get_objects"""
    print(f"{len(scene.objects)} objects of at least {scene.min_voxels} voxels ({scene.n} in all)")
    for it in scene.objects:
        r0, r1, c0, c1, h0, h1 = it.bbox
        voted = "" if it.voted == it.category else f" (voted {it.voted_name!r})"
        print(f"  object {it.label}: {it.name!r}{voted}, {it.count} voxels, rows {r0}..{r1}, cols {c0}..{c1}, heights {h0}..{h1}, "
              f"centre ({it.center[0]:.2f}, {it.center[1]:.2f}, {it.center[2]:.2f}), best score {it.best_score:.4f}, margin {it.margin:.4f}")


def print_rooms(scene, rooms) -> None:
    """--inventory --rooms: the listed objects under the room that holds most of their voxels, room 0 = in no room"""
    scene.assign_rooms(rooms)
    print(f"{rooms.n} rooms, {len(rooms.door_table)} doors")
    for k in list(range(1, rooms.n + 1)) + [0]:
        inside = scene.in_room(k)
        if k == 0 and not inside:
            continue
        head = f"room {k}: {rooms.area_m2(k):.2f} m^2, centre {rooms.centre(k)}, next to {rooms.neighbours(k)}" if k else "in no room"
        print(f"  {head}: {len(inside)} objects")
        for it in inside:
            print(f"    object {it.label}: {it.voted_name!r}, {it.count} voxels")


def print_relations(graph) -> None:
    """--relations: one line per pair of listed objects of VLMap.get_scene_graph"""
    print(f"{len(graph.edges)} relations among the listed objects within {graph.R} cells ({graph.relations.P} pairs in all)")
    names = {it.label: it.voted_name for it in graph.objects.objects}
    for e in graph.edges:
        how = f"{e.a} on {e.b}" if e.rests() else (f"{e.b} on {e.a}" if e.mirrored().rests() else "side by side")
        print(f"  relation {e.a} {names[e.a]!r} - {e.b} {names[e.b]!r}: gap {e.distance:.3f} m (d2 {e.d2}) between voxels {e.voxel_a} and "
              f"{e.voxel_b}, {e.contacts} contacts, {e.a_on_b} / {e.b_on_a} voxels on top, {how}")


def quantile_query(avlmap, args, cats, decay):
    """--quantile: (heat, instances or None) of the voxels above the category's own percentile"""
    from avlmaps_amd import ops
    from avlmaps_amd.map.map import cfg_get
    vm = avlmap.vlmap
    vm.init_categories(cats[1:-1])
    cat_id, mask, counts = vm._quantile_mask_device(args.query, args.quantile)
    print(f"{int(counts[cat_id])} of {len(vm.grid_pos)} voxels lie above the {args.quantile:g}th percentile "
          f"({vm.quantile_thresholds(args.quantile)[cat_id]:.6f}) of {vm.categories[cat_id]!r}; ", end="")
    if not counts[cat_id]:
        raise SystemExit(f"--quantile {args.quantile:g}: no voxel lies above it")
    instances = None
    if args.instances:
        scores = np.ascontiguousarray(vm.scores_mat[:, cat_id], dtype=np.float32)
        with ops.label_voxels(vm._device_pos(), mask, connectivity=args.connectivity, scores=scores, device=True) as inst:
            table, best = inst.table, inst.best_score
            instances = [ops.Instance3D.from_row(k + 1, table[k], best[k]) for k in range(inst.n) if table[k, 0] >= args.min_voxels]
    cs = cfg_get(cfg_get(avlmap.config, "params"), "cs")
    return vm.heatmap_from_mask(mask, cs, decay).numpy(), instances


def fused_decay_rates(args) -> dict:
    """the decay_rates argument of AVLMap.index_goal from the per-flag overrides"""
    given = {"obj": args.object_decay, "area": args.area_decay, "sound": args.sound_decay, "img": args.image_decay}
    return {k: v for k, v in given.items() if v is not None}


def main(argv=None):
    args = parse_args(argv)
    decay = DEFAULT_DECAY.get(args.modality) if args.decay_rate is None else args.decay_rate

    from avlmaps_amd import ops
    from avlmaps_amd.apps.common import FixedPoseLocalizer, HashAudioText, HashClip, load_config
    from avlmaps_amd.map import AVLMap
    cfg = load_config(args.config)
    hashed = args.text_model == "hash"
    avlmap = AVLMap(cfg, data_dir=args.data_dir, area_text_model=HashClip(768) if hashed else None,
                    audio_text_model=HashAudioText() if hashed else None)
    if not avlmap.load_map(args.data_dir):
        raise SystemExit(1)
    vm = avlmap.vlmap
    if args.modality == "object" or args.object:
        if hashed:
            vm.clip_feat_dim = vm.grid_feat.shape[1]
            vm.clip_model = HashClip(vm.clip_feat_dim)
        else:
            vm._init_clip()
    if args.modality == "fused":
        img = None
        if args.image:
            from avlmaps_amd.utils.mapping_utils import load_rgb_png
            poses = np.loadtxt(vm.pose_path).reshape(-1, 7)
            avlmap.visual_map.localizer = FixedPoseLocalizer(poses[args.image_pose], vm.base2cam_tf)
            img = load_rgb_png(args.image)
        goal = avlmap.index_goal(obj=args.object or None, area=args.area or None, sound=args.sound or None, img=img,
                                 decay_rates=fused_decay_rates(args))
        heat = goal.heat
        what = " * ".join(args.object + args.area + args.sound + ([args.image] if args.image else []))
        print(f"fused {what!r}: heat>0 on {int((heat > 0).sum())} of {len(heat)} voxels; "
              f"goal voxel id {goal.voxel} at grid_pos {goal.pos.tolist()} (heat {goal.value:.3f})")
        if args.save:
            np.save(args.save, heat)
        write_pictures(avlmap, heat, args)
        return heat
    if args.modality == "object":
        cats = None
        if args.categories:
            cats = ["void"] + [c.strip() for c in args.categories.split(",")] + ["void"]   # upstream passes categories[1:-1]
        if args.quantile is not None:
            heat, instances = quantile_query(avlmap, args, cats, decay)
            if instances is not None:
                print()
                print_instances(instances, args.query)
        else:
            heat = avlmap.index_object(args.query, init_categories=cats, decay_rate=decay)
            print(f"{int((heat == 1.0).sum())} of {len(heat)} voxels match {args.query!r}; ", end="")
        if args.instances and args.quantile is None:
            print()
            print_instances(vm.get_instances_3d(args.query, args.min_voxels, args.connectivity), args.query)
        if args.inventory or args.inventory_json:
            scene = vm.get_objects(args.min_voxels, args.connectivity)      # the query above has run init_categories
            if args.inventory:
                print()
                print_inventory(scene)
            if args.inventory_json:
                scene.save(args.inventory_json)
                print(f"\nwrote {args.inventory_json}: {len(scene.objects)} objects")
            if args.rooms:
                print()
                print_rooms(scene, vm.get_rooms(0.9 if args.door_width is None else args.door_width))
        if args.relations or args.relations_json:
            graph = vm.get_scene_graph(args.relation_radius, args.min_voxels, args.connectivity)
            if args.relations:
                print()
                print_relations(graph)
            if args.relations_json:
                graph.save(args.relations_json)
                print(f"\nwrote {args.relations_json}: {len(graph.edges)} relations")
        if args.related is not None:
            try:
                heat = avlmap.index_related_object(*args.related, decay_rate=decay, radius=args.relation_radius, min_voxels=args.min_voxels,
                                                   connectivity=args.connectivity)
            except LookupError as e:
                raise SystemExit(f"--related: {e}")
            print(f"related {' '.join(args.related)!r}: ", end="")
        if args.instance is not None:
            try:
                heat = avlmap.index_object_instance(args.query, args.instance, decay_rate=decay, min_voxels=args.min_voxels,
                                                    connectivity=args.connectivity)
            except IndexError as e:
                raise SystemExit(f"--instance {args.instance}: {e}")
            print(f"instance {args.instance}: ", end="")
    elif args.modality == "area":
        heat = avlmap.index_area(args.query, decay_rate=decay)
    elif args.modality == "sound":
        heat = avlmap.index_sound(args.query, decay_rate=decay)
    else:
        from avlmaps_amd.utils.mapping_utils import load_rgb_png
        poses = np.loadtxt(vm.pose_path).reshape(-1, 7)
        avlmap.visual_map.localizer = FixedPoseLocalizer(poses[args.image_pose], vm.base2cam_tf)
        heat = avlmap.index_image(load_rgb_png(args.image), decay_rate=decay)
    idx, val = ops.argmax_f32(heat.astype(np.float32, copy=False))
    what = args.query if args.modality != "image" else args.image
    print(f"{args.modality} {what!r}: heat>0 on {int((heat > 0).sum())} of {len(heat)} voxels; "
          f"goal voxel id {idx} at grid_pos {vm.grid_pos[idx].tolist()} (heat {val:.3f})")
    if args.save:
        np.save(args.save, heat)
    write_pictures(avlmap, heat, args)
    return heat


if __name__ == "__main__":
    main()
