"""Build a VLMap for one scene directory.  Counterpart of the reference's application/create_map.py:7-17.

    python -m avlmaps_amd.apps.create_map --data-dir <scene> [--config cfg.yaml] [--features lseg|hash] [--seed N]
                                          [--sound [--audio-model hash]] [--explored [--ray-stride N]]
                                          [--gt [--obj2cls FILE] [--categories-file FILE]]
                                          [--area [--area-model clip|hash] [--area-batch N]]

<scene>/ holds rgb/*.png, depth/*.npy (float32 metres) and poses.txt (x y z qx qy qz qw per line), the layout of the
reference's dataset/README.md:76-93; the map goes to <scene>/vlmap/vlmaps.h5df (a real HDF5 file: through h5py, or through
the HDF5 C library where h5py is missing).
--sound also builds the sound map (<scene>/audio_video/audio_data_<level>.pkl) from <scene>/audio_video/<seq>/ (a .wav next to
output_with_audio_<level>.mp4 at any sample rate, as 16-, 24- or 32-bit PCM or 32-bit float: it is resampled on the GPU to the
configured rate; or the video itself when ffmpeg is installed; poses.txt; the meta file); --audio-model hash is the
model-free audio encoder, the only one built in (AudioCLIP is attached through AVLMap(audio_encoder=...) from Python).
--explored also carves the sight rays of every depth frame into the explored map (<scene>/vlmap/explored.npz: per cell the first
frame that saw it, Map.create_explored_map), one ray per --ray-stride pixels in both image directions; VLMap.load_map picks the
file up, and the known-free map and the frontier goals need it.
--gt also builds the ground-truth label map (<scene>/vlmap/gt_labels.npz, GTMap.create_map) from <scene>/semantic/*.npy, the object
id of every pixel: --obj2cls is the object id -> class id table (.json dict or list, or .npy; default <scene>/semantic/obj2cls.json
when it exists, else the frames are taken as class ids), --categories-file a text file with one class name per line, the line
number being the class id.  apps.evaluate_map scores a map against it.
--area also builds the area map (<scene>/area_map/clip_sparse_map.h5df, AreaMap.create_map: one image embedding per frame, what
apps.index_map --modality area reads): the frames are preprocessed for CLIP on the GPU --area-batch at a time and encoded as
batches; --area-model clip is OpenAI CLIP ViT-L/14 (it must be installed), hash the model-free stand-in.
Multi-GPU: launch with torchrun; frames are sharded over ranks and merged with one row-sharded RCCL exchange (every --save-every
frames per rank as a checkpoint, and at the end); an interrupted run is continued with --resume; with --seed the N-rank map
equals the single-process map (every rank replays the RNG draws of the frames before its shard)."""
from __future__ import annotations

import argparse
import time

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--config", default=None, help="YAML with params / map_config overrides")
    ap.add_argument("--features", choices=["lseg", "hash"], default="lseg",
                    help="lseg = upstream LSegEncNet + demo_e200.ckpt on PyTorch-ROCm; hash = model-free stand-in for smoke runs")
    ap.add_argument("--feat-dim", type=int, default=512)
    ap.add_argument("--seed", type=int, default=None, help="seed of the global NumPy RNG that orders the pixel sampling")
    ap.add_argument("--capacity", type=int, default=None, help="voxel capacity (default gs*gs)")
    ap.add_argument("--prefetch", type=int, default=None, help="frames decoded ahead on host threads (default 4, 0 = inline)")
    ap.add_argument("--batch-frames", type=int, default=None, help="frames fused per launch pair (default 1)")
    ap.add_argument("--deferred-fuse", action="store_true",
                    help="frame-by-frame fusion in one launch per frame (the extractor must return a new tensor per frame)")
    ap.add_argument("--pixel-sampling", choices=["reference", "uniform"], default=None,
                    help="reference = np.random.shuffle on the global RNG like upstream (6 ms per 720x1080 frame, serial); uniform = "
                         "the same distribution from per-frame generators (0.25 ms, other pixels than a seeded upstream run)")
    ap.add_argument("--shard-sampling", choices=["replay", "independent"], default=None,
                    help="several ranks: replay = sample the pixels of the single-process run (default); independent = do not "
                         "fast-forward the RNG past the other ranks' frames (unseeded runs)")
    ap.add_argument("--merge-mode", choices=["sharded", "reduce"], default=None,
                    help="several ranks: sharded = all_to_all of every rank's own voxel rows (default); reduce = one dense sum-reduce")
    ap.add_argument("--save-every", type=int, default=None, help="checkpoint every N frames (per rank); default 100 like upstream")
    ap.add_argument("--resume", action="store_true",
                    help="continue from an existing vlmaps.h5df and skip the frames it lists (upstream re-fuses every frame)")
    ap.add_argument("--sound", action="store_true", help="also build the sound map from <scene>/audio_video (a .wav next to the video may have any sample rate and PCM "
                                                         "width: it is resampled on the GPU to sound_data_collect_params.sample_rate)")
    ap.add_argument("--audio-model", choices=["hash"], default="hash",
                    help="--sound: the audio encoder; hash = model-free stand-in (apps/common.HashAudioEncoder)")
    ap.add_argument("--explored", action="store_true", help="also build the explored map (<scene>/vlmap/explored.npz) from the depth frames")
    ap.add_argument("--ray-stride", type=int, default=4, metavar="N", help="--explored: one sight ray per N pixels in both image directions")
    ap.add_argument("--gt", action="store_true", help="also build the ground-truth label map (<scene>/vlmap/gt_labels.npz) from <scene>/semantic")
    ap.add_argument("--obj2cls", default=None, metavar="FILE", help="--gt: object id -> class id table (.json or .npy)")
    ap.add_argument("--categories-file", default=None, metavar="FILE", help="--gt: class names, one per line; the line number is the class id")
    ap.add_argument("--area", action="store_true", help="also build the area map (<scene>/area_map/clip_sparse_map.h5df) from the rgb frames")
    ap.add_argument("--area-model", choices=["clip", "hash"], default="clip",
                    help="--area: the image encoder; clip = OpenAI CLIP ViT-L/14, hash = model-free stand-in (apps/common.HashBatchImageEncoder)")
    ap.add_argument("--area-batch", type=int, default=64, metavar="N", help="--area: frames preprocessed and encoded per batch")
    args = ap.parse_args(argv)
    if args.area_batch < 1:
        ap.error("--area-batch must be at least 1")
    if args.ray_stride < 1:
        ap.error("--ray-stride must be at least 1")
    if (args.obj2cls or args.categories_file) and not args.gt:
        ap.error("--obj2cls and --categories-file belong to --gt")

    from avlmaps_amd import parallel
    from avlmaps_amd.apps.common import HashAudioEncoder, HashFeatureExtractor, load_config
    from avlmaps_amd.map import AVLMap
    rank, ws, _ = parallel.init_distributed()
    cfg = load_config(args.config)
    if args.seed is not None:
        np.random.seed(args.seed)
    extractor = HashFeatureExtractor(args.feat_dim) if args.features == "hash" else None
    avlmap = AVLMap(cfg, data_dir=args.data_dir)
    if (args.capacity or args.prefetch is not None or args.batch_frames or args.shard_sampling or args.deferred_fuse or args.pixel_sampling
            or args.merge_mode or args.save_every is not None or args.resume):
        import avlmaps_amd.map.vlmap_builder as vb
        orig = vb.VLMapBuilder.__init__

        def patched(self, *a, **k):
            orig(self, *a, **k)
            if args.capacity:
                self.capacity = args.capacity
            if args.prefetch is not None:
                self.prefetch_frames = args.prefetch
            if args.batch_frames:
                self.batch_frames = args.batch_frames
            if args.shard_sampling:
                self.shard_sampling = args.shard_sampling
            if args.deferred_fuse:
                self.deferred_fuse = True
            if args.pixel_sampling:
                self.pixel_sampling = args.pixel_sampling
            if args.merge_mode:
                self.merge_mode = args.merge_mode
            if args.save_every is not None:
                self.save_every = args.save_every
            if args.resume:
                self.skip_mapped_frames = True
        vb.VLMapBuilder.__init__ = patched
    t0 = time.perf_counter()
    avlmap.create_map(args.data_dir, feat_extractor=extractor)
    if args.sound and rank == 0:
        path = avlmap.sound_map.create_sound_map(args.data_dir, audio_encoder=HashAudioEncoder())
        print(f"sound map with {len(avlmap.sound_map.load_sound_map(args.data_dir))} segments written to {path}")
    if args.area and rank == 0:
        from avlmaps_amd.apps.common import HashBatchImageEncoder
        avlmap.area_map.create_map(args.data_dir, batch_encoder=HashBatchImageEncoder() if args.area_model == "hash" else None,
                                   batch_size=args.area_batch)
        print(f"area map with {len(avlmap.area_map.clip_sparse_map)} frame embeddings written to {avlmap.area_map.data_dir / 'area_map'}")
    if args.explored and rank == 0:
        first_seen = avlmap.vlmap.create_explored_map(args.data_dir, stride=args.ray_stride)
        print(f"explored map: {int((first_seen >= 0).sum())} cells seen in {avlmap.vlmap.explored_params['n_frames']} frames, written to "
              f"{avlmap.vlmap.data_dir / 'vlmap' / avlmap.vlmap.EXPLORED_FILE}")
    if args.gt and rank == 0:
        from avlmaps_amd.apps.common import read_categories_file
        from avlmaps_amd.map import GTMap
        gt = GTMap(cfg.map_config)
        vm = avlmap.vlmap
        if vm.occupied_ids is None and not vm.load_map(args.data_dir):
            raise SystemExit(1)
        gt.create_map(args.data_dir, vlmap=vm, obj2cls=args.obj2cls,
                      categories=read_categories_file(args.categories_file) if args.categories_file else None)
        print(f"GT map: {int((gt.labels >= 0).sum())} of {len(gt.labels)} voxels labelled by {int(gt.stats[3])} votes of "
              f"{gt.gt_params['n_frames']} frames, written to {gt.data_dir / 'vlmap' / gt.GT_FILE}")
    if rank == 0:
        n = len(avlmap.vlmap.map_builder.last_map["grid_pos"]) if hasattr(avlmap.vlmap.map_builder, "last_map") else -1
        print(f"map with {n} voxels written to {avlmap.vlmap.map_builder.map_save_path} in {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()
