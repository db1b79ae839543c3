"""VLMap with the reference's interface (avlmaps/map/vlmap.py:27-187), indexing on the MI355X.

grid_feat stays a host NumPy attribute (the navigator reads it) and is mirrored ONCE into HBM; every
index_map / init_categories call then streams the device copy through the similarity kernel."""
from __future__ import annotations

from pathlib import Path
from typing import List, Union

import numpy as np

from ..utils.clip_utils import get_lseg_score, landmark_text_feats
from ..utils.mapping_utils import load_3d_map, map_file_exists
from .map import Map, cfg_get

CLIP_FEAT_DIM = {"RN50": 1024, "RN101": 512, "RN50x4": 640, "RN50x16": 768, "RN50x64": 1024, "ViT-B/32": 512,
                 "ViT-B/16": 512, "ViT-L/14": 768}


_UPLOADS = []       # map-upload threads still running: joined at interpreter exit so that the process never tears HIP down mid-copy


def _join_uploads():
    for th in list(_UPLOADS):
        th.join(timeout=30)


import atexit  # noqa: E402
atexit.register(_join_uploads)


class VLMap(Map):
    def __init__(self, map_config, data_dir: str = ""):
        super().__init__(map_config, data_dir=data_dir)
        self.scores_mat = None
        self.categories = None
        self._dev_feat = None
        self._dev_feat_src = None
        import threading
        self._dev_lock = threading.RLock()
        self.prefetch_device = True       # load_map starts the one-off upload + conversion of grid_feat (1.1 s at 2 M voxels: 4 GB over
                                          # PCIe from pageable memory) on a host thread, so that it overlaps with whatever the
                                          # caller does next (upstream: loading CLIP, seconds) instead of sitting in the first query
        self.compact_map = True           # the resident copy is the 3-byte form (ops.prepare_map(compact=True): fp16 hi + one
                                          # byte of residual in units of ulp(hi)/256, per-row scale): a query pass reads a quarter less
                                          # HBM (0.70 -> 0.61 ms at 2 M voxels x 64 queries), the copy is a quarter smaller, and the
                                          # scores stay float32-class (max error 2.3e-6 against 1.4e-6 for the 4-byte form; the path's
                                          # contract is 1e-4).  False: the 4-byte split-fp16 form
        self.shard_index_rows = True      # with torch.distributed initialised (one process per GPU) every rank keeps and scores
                                          # only its block of voxel rows; the per-voxel results are all-gathered (parallel.gather_rows)

    # ------------------------------------------------------------------ build / load
    def create_map(self, data_dir: Union[Path, str], feat_extractor=None) -> None:
        """Reference: vlmap.py:33-48."""
        from .vlmap_builder import VLMapBuilder
        print("Creating map for scene at: ", data_dir)
        self._setup_paths(data_dir)
        self.map_builder = VLMapBuilder(self.data_dir, self.map_config, self.pose_path, self.rgb_paths, self.depth_paths,
                                        self.base2cam_tf, self.base_transform, feat_extractor=feat_extractor)
        pose_type = cfg_get(cfg_get(self.map_config, "pose_info"), "pose_type")
        if pose_type == "mobile_base":
            self.map_builder.create_mobile_base_map()
        elif pose_type == "camera":
            self.map_builder.create_camera_map()

    def load_map(self, data_dir: str) -> bool:
        """Reference: vlmap.py:50-65 (prints and returns False when the file is missing)."""
        self._setup_paths(data_dir)
        self.map_save_path = Path(data_dir) / "vlmap" / "vlmaps.h5df"
        if not map_file_exists(self.map_save_path):
            print("Loading VLMap failed because the file doesn't exist.")
            return False
        (self.mapped_iter_list, self.grid_feat, self.grid_pos, self.weight, self.occupied_ids,
         self.grid_rgb) = load_3d_map(self.map_save_path)[:6]
        self._dev_feat = None
        self.load_explored_map(data_dir)                 # vlmap/explored.npz when it exists; a map without it behaves as ever
        self.load_visibility(data_dir)                   # vlmap/visibility.npz when it exists and is this map's (same voxel count)
        # straight after a multi-GPU build in this process the merged map already lies row-sharded in the ranks' HBM
        # (VLMapBuilder.map_shard): take this rank's block as the resident copy instead of uploading it again from the file
        shard = getattr(getattr(self, "map_builder", None), "map_shard", None)
        if shard is not None and self.adopt_device_shard(shard):
            self.map_builder.map_shard = None            # the compact copy replaces the float32 block
            return True
        self._start_device_prefetch()
        return True

    def _start_device_prefetch(self) -> None:
        if not self.prefetch_device or self.grid_feat is None or len(self.grid_feat) == 0:
            return
        import threading
        from .. import _lib
        # the device the CALLING thread works on (HIP keeps the current device per thread): what it selected through
        # _lib.set_device or torch; asking HIP itself would start the runtime right here (~0.8 s), so if nothing is known yet the
        # upload goes to device 0 and _device_feat() checks at query time that the resident copy lives on the querying
        # thread's device (re-uploading once if the caller picked another GPU in between)
        dev = _lib.current_device(query_runtime=False)
        dev = 0 if dev is None else dev

        def work():
            try:
                _lib.load()
                _lib.require_gpu()                                         # first HIP call of the process: runtime start-up
                _lib.set_device(dev)
                self._device_feat()
            except Exception:             # no GPU / no library / upload failed: the query path repeats it on the calling thread
                pass                      # and reports the error there
        th = threading.Thread(target=work, name="avl-map-upload", daemon=True)
        th.start()
        _UPLOADS.append(th)
        del _UPLOADS[:-8]

    def prune_voxels(self, mask) -> int:
        """Remove the voxels of `mask` (N,) bool -- VisibilityAudit.stale(), say -- from the map; returns how many went.  Host NumPy:
        the rows leave grid_feat, grid_pos, weight, grid_rgb and scores_mat (when set), occupied_ids is renumbered (-1 where a cell
        was emptied), and every device copy derived from the old arrays is dropped (the resident features, positions, colours, the
        heat plan, the scores, the instances, the audit itself), so that queries afterwards equal those of a freshly loaded pruned
        map.  Saving goes through utils.mapping_utils.save_3d_map as ever.  Upstream has no counterpart (its maps are static)."""
        if self.grid_pos is None or self.grid_feat is None:
            raise ValueError("prune_voxels: no map loaded")
        n = len(self.grid_pos)
        mask = np.asarray(mask)
        if mask.dtype != np.dtype(bool) or mask.shape != (n,):
            raise ValueError(f"prune_voxels: expected a bool mask of shape ({n},), got {mask.dtype} {mask.shape}")
        removed = int(np.count_nonzero(mask))
        if removed == 0:
            return 0
        keep = ~mask
        new_id = np.full((n,), -1, dtype=np.int64)
        new_id[keep] = np.arange(n - removed)
        with self._dev_lock:
            self.grid_feat = np.ascontiguousarray(np.asarray(self.grid_feat)[keep])
            self.grid_pos = np.ascontiguousarray(np.asarray(self.grid_pos)[keep])
            self.weight = np.ascontiguousarray(np.asarray(self.weight)[keep])
            if self.grid_rgb is not None:
                self.grid_rgb = np.ascontiguousarray(np.asarray(self.grid_rgb)[keep])
            if self.occupied_ids is not None:
                occ = np.asarray(self.occupied_ids)
                out = np.full(occ.shape, -1, dtype=occ.dtype)
                held = (occ >= 0) & (occ < n)
                out[held] = new_id[occ[held]].astype(occ.dtype)
                self.occupied_ids = out
            if self.scores_mat is not None:
                self.scores_mat = np.ascontiguousarray(np.asarray(self.scores_mat)[keep])
            self._drop_derived()
        return removed

    def _drop_derived(self) -> None:
        """Forget everything that mirrors the voxel arrays on the device, or was computed from them: prune_voxels and fuse call it
        under _dev_lock after they replaced the arrays."""
        self._dev_feat = self._dev_feat_src = None
        self._dev_pos = self._dev_pos_src = None
        self._dev_rgb = self._dev_rgb_src = None
        plan = getattr(self, "_heat_plan_obj", None)
        if plan is not None:
            plan.close()
        self._heat_plan_obj = self._heat_plan_src = None
        self._dev_scores = self._dev_scores_src = None
        self._quantile_cache = {}
        self._argmax = self._argmax_src = None
        self._dev_argmax = self._dev_argmax_src = None
        cached = getattr(self, "_instances_cache", None)
        if cached is not None:
            cached[1].close()
        self._instances_cache = None
        cached = getattr(self, "_objects_cache", None)
        if cached is not None:
            cached[1].close()
        self._objects_cache = None
        self.visibility = None

    def resample(self, transform=None, shift=(0, 0, 0), method: str = "forward", min_support: float = 0.5) -> "VLMap":
        """A new VLMap on this map's grid and config whose voxels are this map's moved by the (4, 4) float64 `transform` of base
        coordinates (None = identity; Map.transform_from gives the one between two recordings' frames) and then by `shift` whole
        cells (row, col, h), which is ADDED to the moved cells (map/fuse.py).  scores_mat is not carried over (index the new map);
        categories and mapped_iter_list are.  With no arguments the result equals this map.
        method="forward" (the default; ops.fuse_maps with an empty first map): a voxel's cell centre is moved and
        lands in one cell; rows that land in one cell are averaged by weight, rows that leave the grid or the height band are
        dropped.  Under a rotation some cells receive two or three voxels and neighbouring cells none, so surfaces come out with
        pinholes, which compare() reads as vanished voxels; features are not interpolated.  The voxels keep this map's row order.
        method="linear" or "nearest" (ops.pull_map) work backward: every cell of the grid asks where its centre came
        from under the inverse transform, so a turned surface comes out without pinholes.  For a revisit turned against this map use
        b.resample(T, method="linear"): a voxel is the mean of up to eight neighbouring voxels, by trilinear weight times the
        voxels' weights, and exists when the weights of the neighbours that hold a voxel add up to `min_support` (0 < .. <= 1) or
        more, which keeps a wall one cell thick and shaves the rim of a surface.  "linear" blends rows across the border of two
        objects; choose "nearest", which copies the one voxel that the centre falls into, bit for bit, where features must stay
        what the builder wrote (category maps, compare() with a high threshold).  The backward methods order the voxels by linear
        cell ((row * gs + col) * vh + h), not by this map's rows, and need one voxel per cell.  resample_counts holds the
        method's counts.  The raw float32 rows are resampled, not the compact resident copies; not for rows sharded over ranks."""
        from .fuse import resample_map
        return resample_map(self, transform, shift, method, min_support)

    def fuse(self, other, transform=None, shift=(0, 0, 0), changes=None, drop_vanished: bool = True, replace_changed: bool = True,
             gain: float = 1.0) -> dict:
        """Fold `other` (B, a later map of the same place) into this map (A) in place, like prune_voxels: a cell that both maps hold
        gets the mean of its rows weighted by the maps' weights -- the builder's running mean in closed form --, a cell that only B
        holds is appended (map/fuse.py, ops.fuse_maps).  transform: B's base frame -> A's (None = identity); shift
        has VLMap.compare's meaning: A's cell c corresponds to B's cell c + shift.  gain (> 0) scales B's weights: above 1 the
        revisit counts for more.  changes: the MapChanges of self.compare(other, shift=shift); with it the vanished voxels of A are
        dropped (drop_vanished) and the voxels of A whose content was replaced give way to B's (replace_changed), while B's voxels
        that this session never looked at (unseen_b) stay out.  It is accepted only with transform=None and its own shift: resample
        `other` first otherwise -- for a turned revisit other.resample(T, method="linear"), which leaves no pinholes for compare()
        to read as vanished ("nearest" where features must not be blended across object borders).  Returns the counts (ops.FUSE_COUNTS, voxels_a, voxels_b, voxels).  ValueError unless gs, cs, the
        height cells and the feature width agree.  Afterwards scores_mat is None (the rows changed: index again), every derived
        device copy is dropped, and mapped_iter_list stays this map's: the frames of B's recording are not recorded in it.  The
        raw float32 rows are fused, not the compact resident copies; not for rows sharded over ranks.  The result is not what a
        joint build of both recordings gives: the builder's float32 running mean rounds differently."""
        from .fuse import fuse_into
        return fuse_into(self, other, transform, shift, changes, drop_vanished, replace_changed, gain)

    def compare(self, other, radius: int = 1, threshold: float = 0.8, shift=(0, 0, 0), audit=None, other_audit=None, min_rays: int = 3):
        """What changed between this map (A, the earlier one) and `other` (B, a later map of the same place): a MapChanges
        (map/changes.py) with the voxels of A that vanished, the voxels of B that appeared and the voxels whose feature row was
        replaced by something else (ops.map_diff).  A's cell c corresponds to B's cell c + shift; a voxel's partner is
        the nearest occupied cell of the other map within `radius` cells (0 .. 2), each direction with its own; a pair whose
        rows have a cosine below `threshold` (0 < threshold <= 1) is changed.  The rows are the raw float32 grid_feat of both maps,
        not the compact resident copies.  audit: a VisibilityAudit of THIS map made from the other session's frames
        (self.audit_visibility([other's data_dir])), other_audit: one of `other` made from this session's frames; with one, an
        unmatched voxel that fewer than min_rays of the other session's sight rays passed through is unseen, not vanished /
        appeared.  ValueError unless gs, cs, the number of height cells and the feature width agree.  Whole-cell shifts only: a
        revisit recorded from another odometry origin -- a rotation or a sub-cell shift away -- is resampled onto this map's grid
        first, with T from Map.transform_from (Map.register_frames gives the correction): a.compare(b.resample(T, method="linear")) for a
        turned revisit -- the default forward resampling leaves pinholes that read as vanished voxels here; method="nearest" where
        features must not be blended across object borders.  Upstream has
        no counterpart: its maps are static."""
        from .changes import compare_maps
        return compare_maps(self, other, radius=radius, threshold=threshold, shift=shift, audit=audit, other_audit=other_audit,
                            min_rays=min_rays)

    def _init_clip(self, clip_version="ViT-B/32"):
        """Reference: vlmap.py:67-90."""
        if hasattr(self, "clip_model"):
            print("clip model is already initialized")
            return
        import torch
        import clip
        self.device = "cuda" if torch.cuda.is_available() else "cpu"
        self.clip_version = clip_version
        self.clip_feat_dim = CLIP_FEAT_DIM[self.clip_version]
        print("Loading CLIP model...")
        self.clip_model, self.preprocess = clip.load(self.clip_version)
        self.clip_model.to(self.device).eval()

    # ------------------------------------------------------------------ index
    def _device_feat(self):
        """grid_feat mirrored into HBM once (re-uploaded only if the host array object changes).  The private device copy
        is converted to the split-fp16 layout the matrix-core kernel consumes directly, every row with its own power-of-two
        scale (avl_sim_prepare_map: same bytes, no per-query conversion work, and voxels observed once from far away --
        rows of magnitude 1e-6 ... 1e-15, vlmap_builder.py:166-168 -- score as accurately as any other row);
        self._sim_precision tells the kernels which form it has."""
        from .. import ops, parallel
        from ..device import DeviceArray
        with self._dev_lock:
            return self._device_feat_locked(ops, parallel, DeviceArray)

    def _device_feat_locked(self, ops, parallel, DeviceArray):
        from .. import _lib
        cur = _lib.current_device()
        if self._dev_feat is not None and getattr(self, "_dev_feat_device", cur) != cur:
            # the resident copy was uploaded before the caller selected this GPU (load_map's upload thread had nothing to go
            # by): pointers of another device would fault or crawl through peer access -- upload again, here
            self._dev_feat = None
        if self._dev_feat is None or self._dev_feat_src is not self.grid_feat:
            self._dev_feat_device = cur
            rank, ws = parallel.rank_world()
            self._rows = (0, len(self.grid_feat))
            if ws > 1 and self.shard_index_rows:
                self._rows = parallel.shard_rows(len(self.grid_feat), rank, ws)
            dev = DeviceArray.from_numpy(np.ascontiguousarray(self.grid_feat[self._rows[0]:self._rows[1]], dtype=np.float32))
            self._dev_feat_src = self.grid_feat
            self._sim_precision = "auto"
            if dev.shape[1] % 64 == 0 and dev.shape[0] > 0:
                # the compact form is read by every matrix-core kernel (resident, K-swap, streamed, column-block); its residual plane
                # is laid out in lines of 128 columns, other widths keep the 4-byte copy
                if self.compact_map and dev.shape[1] % 128 == 0:
                    raw = dev
                    dev = ops.prepare_map(raw, compact=True)
                    raw.free()                                        # the float32 device copy is not needed any more
                else:
                    dev = ops.prepare_map(dev, scaled=True)
                self._sim_precision = "prepared"
            self._dev_feat = dev
        return self._dev_feat

    def _device_pos(self):
        """grid_pos mirrored into HBM once (int32, re-uploaded only if the host array object changes)"""
        from ..device import DeviceArray
        if getattr(self, "_dev_pos", None) is None or self._dev_pos_src is not self.grid_pos:
            self._dev_pos = DeviceArray.from_numpy(np.ascontiguousarray(self.grid_pos, dtype=np.int32))
            self._dev_pos_src = self.grid_pos
        return self._dev_pos

    def _device_rgb(self):
        """grid_rgb mirrored into HBM once as (N, 3) uint8 (re-uploaded only if the host array object changes): the renderer's colours"""
        from ..device import DeviceArray
        if getattr(self, "_dev_rgb", None) is None or self._dev_rgb_src is not self.grid_rgb:
            self._dev_rgb = DeviceArray.from_numpy(np.ascontiguousarray(self.grid_rgb).astype(np.uint8, copy=False).reshape(-1, 3))
            self._dev_rgb_src = self.grid_rgb
        return self._dev_rgb

    def _heat_plan(self):
        """ops.HeatPlan of this map's voxel positions (cell order + grid buffers), rebuilt only when the positions change; None
        for a map whose bounding box is too large for one (callers then use the stateless ops.heatmap_from_mask)."""
        from .. import ops
        pos = self._device_pos()
        if getattr(self, "_heat_plan_src", None) is not pos:
            old = getattr(self, "_heat_plan_obj", None)
            if old is not None:
                old.close()
            self._heat_plan_obj = ops.HeatPlan.for_positions(pos) if len(self.grid_pos) else None
            self._heat_plan_src = pos
        return self._heat_plan_obj

    def heatmap_from_mask(self, mask, cell_size, decay_rate):
        """visualize_utils.py:29-49 for this map's voxels: mask (N,) host/device -> device heat (planned when possible)"""
        from .. import ops
        plan = self._heat_plan()
        if plan is not None:
            return plan(mask, cell_size, decay_rate)
        return ops.heatmap_from_mask(self._device_pos(), mask, cell_size, decay_rate)

    def adopt_device_shard(self, shard) -> bool:
        """Take this rank's block of a freshly merged map (VLMapBuilder.map_shard: device tensors of
        parallel.merge_accumulator_sharded) as the resident copy the index kernels read -- no 4 GB host round trip after a
        multi-GPU build.  The host attributes (load_map) must describe the same map; returns False (and changes nothing) if the
        block is not the one shard_index_rows would upload."""
        from .. import _lib, ops, parallel
        if shard is None or self.grid_feat is None or int(shard["M"]) != len(self.grid_feat) or not self.shard_index_rows:
            return False
        rank, ws = parallel.rank_world()
        if tuple(shard["rows"]) != parallel.shard_rows(len(self.grid_feat), rank, ws):
            return False
        feat = shard["grid_feat"]
        D = int(feat.shape[1])
        with self._dev_lock:
            self._rows = tuple(shard["rows"])
            self._sim_precision = "auto"
            dev = feat
            if D % 64 == 0 and feat.shape[0] > 0:
                if self.compact_map and D % 128 == 0:
                    dev = ops.prepare_map(feat, compact=True)
                else:
                    dev = ops.prepare_map(feat.clone(), scaled=True)
                self._sim_precision = "prepared"
            self._dev_feat, self._dev_feat_src, self._dev_feat_device = dev, self.grid_feat, _lib.current_device()
        return True

    def _text_feats(self, names, use_multiple_templates=True, add_other=True):
        """landmark_text_feats with a per-instance cache keyed by the strings: the CLIP text tower costs ~1.6 ms per call, twice
        the similarity kernel, and a navigator asks for the same landmarks again and again"""
        key = (tuple(names), bool(use_multiple_templates), bool(add_other), id(self.clip_model), int(self.clip_feat_dim))
        cache = self.__dict__.setdefault("_text_cache", {})
        q = cache.get(key)
        if q is None:
            q, _ = landmark_text_feats(self.clip_model, list(names), self.clip_feat_dim, use_multiple_templates=use_multiple_templates,
                                       add_other=add_other)
            if len(cache) >= 256:
                cache.clear()
            cache[key] = q
        return q

    def _score_device(self, q):
        """row argmax of this rank's block as a DEVICE array (nothing crosses PCIe)"""
        from .. import ops
        feat = self._device_feat()
        _, am, _ = ops.sim_scores(feat, q, want_scores=False, want_argmax=True, precision=self._sim_precision)
        return am

    def _score(self, q, want_scores: bool):
        """(scores (N, Q) | None, argmax (N,)) as host arrays for ALL voxels: this rank's row block through the similarity
        kernel, the other ranks' blocks through one all_gather of results when the rows are sharded"""
        from .. import ops, parallel
        feat = self._device_feat()
        sc, am, _ = ops.sim_scores(feat, q, want_scores=want_scores, want_argmax=True, precision=self._sim_precision)
        from ..utils.clip_utils import _to_numpy
        to_np = lambda x: None if x is None else _to_numpy(x)        # DeviceArray or (adopted shard) torch tensor
        sc, am = to_np(sc), to_np(am)
        n = len(self.grid_feat)
        if self._rows != (0, n):
            am = parallel.gather_rows(am, n)
            sc = parallel.gather_rows(sc, n) if sc is not None else None
        return sc, am

    def index_queries(self, queries, want_scores: bool = False):
        """Row argmax (N,) int32 -- and, on request, scores (N, Q) float32 -- of the map against an explicit query matrix (Q, D):
        the entry for query sets that do not come from the CLIP text tower.  On a fused visual | audio map (BASELINE config 5:
        D = 512 + 1024, every query non-zero in one modality block) the non-zero column window of every query is detected and
        each group of queries is scored against its own columns of the compact resident copy (ops.sim_scores ->
        avl_sim_scores_blocks); same semantics as scores = grid_feat @ queries.T; np.argmax(scores, axis=1)
        (clip_utils.py:227-229, vlmap.py:123)."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2 or self.grid_feat is None or q.shape[1] != self.grid_feat.shape[1]:
            raise ValueError(f"queries must be (Q, {None if self.grid_feat is None else self.grid_feat.shape[1]}), got {q.shape}")
        sc, am = self._score(q, want_scores=want_scores)
        return (am, sc) if want_scores else am

    def init_categories(self, categories: List[str]) -> np.ndarray:
        """scores_mat (N, Q) float32 cached on the instance.  Reference: vlmap.py:92-102."""
        self.categories = categories
        q = self._text_feats(self.categories)
        # one launch gives scores_mat AND its row argmax (same values, first maximum wins like np.argmax), so index_map
        # does not have to rescan the (N, Q) host matrix per query as upstream does (vlmap.py:123)
        self.scores_mat, self._argmax = self._score(q, want_scores=True)
        self._argmax_src = self.scores_mat
        return self.scores_mat

    def index_map(self, language_desc: str, with_init_cat: bool = True):
        """bool mask (N,): argmax over the query columns == category.  Reference: vlmap.py:104-125."""
        from .. import ops
        if with_init_cat and self.scores_mat is not None and self.categories is not None:
            from ..utils.index_utils import find_similar_category_id
            cat_id = find_similar_category_id(language_desc, self.categories)
            if getattr(self, "_argmax_src", None) is self.scores_mat:
                return self._argmax == cat_id
            return np.argmax(self.scores_mat, axis=1) == cat_id      # scores_mat was replaced from outside
        if with_init_cat:
            raise Exception(
                "Categories are not preloaded. Call init_categories(categories: List[str]) to initialize categories.")
        # fused path: scores and argmax never leave the GPU; the mask is compared and bit-packed there, 1 bit per voxel comes back
        q = self._text_feats([language_desc])
        self._device_feat()
        if self._rows == (0, len(self.grid_feat)):
            am = self._score_device(q)
            if isinstance(am, np.ndarray):
                return am == 0
            return ops.mask_bool_from_argmax(am, 0)
        _, am = self._score(q, want_scores=False)          # rows sharded over ranks: the argmax blocks are all-gathered
        return am == 0

    # ------------------------------------------------------------------ 2-D goal maps
    def _crop_window(self):
        """(r0, r1, c0, c1) of the obstacle crop on the full map; the obstacle map is generated on first use"""
        if self.obstacles_cropped is None:
            self.generate_obstacle_map()
        return int(self.rmin), int(self.rmax) + 1, int(self.cmin), int(self.cmax) + 1

    def _argmax_device(self):
        """the (N,) int32 argmax over scores_mat's columns -- the predicted category of every voxel -- on the device"""
        from ..device import DeviceArray
        if self.scores_mat is None or self.categories is None:
            raise Exception("Categories are not preloaded. Call init_categories(categories: List[str]) to initialize categories.")
        if getattr(self, "_argmax_src", None) is not self.scores_mat:       # scores_mat was replaced from outside
            self._argmax, self._argmax_src = np.argmax(self.scores_mat, axis=1), self.scores_mat
        if getattr(self, "_dev_argmax_src", None) is not self._argmax:      # the argmax goes up once per init_categories
            self._dev_argmax = DeviceArray.from_numpy(np.ascontiguousarray(self._argmax, dtype=np.int32))
            self._dev_argmax_src = self._argmax
        return self._dev_argmax

    def evaluate(self, gt, dim: str = "3d"):
        """ops.MapScores of this map against a GTMap (GTMap.evaluate from the other side): pixel accuracy, mean accuracy, mIoU and
        frequency-weighted IoU over its voxels (dim="3d") or over the cells of the top-down maps (dim="2d")"""
        return gt.evaluate(self, dim)

    def _predict_mask_device(self, name: str):
        """the (gs, gs) uint8 top-down mask of the voxels whose argmax is `name`'s category, on the device"""
        from .. import ops
        from ..device import DeviceArray
        from ..utils.index_utils import find_similar_category_id
        if self.scores_mat is None or self.categories is None:
            raise Exception("Categories are not preloaded. Call init_categories(categories: List[str]) to initialize categories.")
        cat_id = find_similar_category_id(name, self.categories)
        mask = ops.mask_from_argmax(self._argmax_device(), cat_id)
        return ops.pool_label_2d(mask, self._device_pos(), int(self.gs), device=True)

    def _avoid_distance(self, what):
        """Map._avoid_distance that also takes a category name: the predicted mask (_predict_mask_device) is measured to inside the
        crop window in place, so it never leaves the device"""
        from .. import ops
        if isinstance(what, str):
            return ops.distance_to_mask(self._predict_mask_device(what), window=self._crop_window())
        return super()._avoid_distance(what)

    def get_predict_mask(self, name: str) -> np.ndarray:
        """The top-down mask of a category over the obstacle crop: 1 where a voxel whose argmax over scores_mat is the category
        lies in the column, in obstacles_cropped's shape and dtype.  Reference: vlmap_3d.py:75-81.  The comparison and the pooling
        run on the GPU (avl_mask_from_argmax, avl_pool_label_2d) and the pooled mask is cut to [rmin:rmax + 1, cmin:cmax + 1]:
        voxels outside the crop are dropped, where upstream's fancy index would wrap around (negative offsets) or raise IndexError."""
        r0, r1, c0, c1 = self._crop_window()
        pooled = self._predict_mask_device(name).numpy()
        return pooled[r0:r1, c0:c1].astype(np.asarray(self.obstacles_cropped).dtype)

    # ------------------------------------------------------------------ open-set queries: a category's own score quantile
    # closed-set above (a voxel belongs to the ONE category that is its row maximum); below, a category's voxels are those above its own
    # score column's percentile: masks may overlap or leave voxels unclaimed.  index_map_quantile's docstring has the rule.
    def _scores_device(self):
        """scores_mat (N, Q) float32 resident on the device, uploaded once per init_categories (like _argmax_device)"""
        from .. import parallel
        from ..device import DeviceArray
        if self.scores_mat is None or self.categories is None:
            raise Exception("Categories are not preloaded. Call init_categories(categories: List[str]) to initialize categories.")
        if parallel.rank_world()[1] > 1 and self.shard_index_rows:
            raise NotImplementedError("quantile queries on rows sharded over ranks: a global quantile needs a merged histogram")
        if getattr(self, "_dev_scores_src", None) is not self.scores_mat:
            self._dev_scores = DeviceArray.from_numpy(np.ascontiguousarray(self.scores_mat, dtype=np.float32))
            self._dev_scores_src = self.scores_mat
            self._quantile_cache = {}
        return self._dev_scores

    def quantile_thresholds(self, percentile: float = 95.0) -> np.ndarray:
        """(Q,) float64: the percentile of every column of scores_mat, np.percentile(scores_mat[:, c].astype(np.float64), percentile)
        bit for bit (ops.column_quantiles: a radix select on the device, the interpolation in float64 on the host).  Kept per
        percentile until init_categories runs again."""
        from .. import ops
        scores = self._scores_device()
        key = float(percentile)
        if key not in self._quantile_cache:
            self._quantile_cache[key] = ops.column_quantiles(scores, key)
        return self._quantile_cache[key]

    def _quantile_mask_device(self, name: str, percentile: float = 95.0):
        """(category id, (N,) uint8 device mask of the voxels above the category's own percentile, the per-category counts)"""
        from .. import ops
        from ..utils.index_utils import find_similar_category_id
        scores = self._scores_device()
        cat_id = find_similar_category_id(name, self.categories)
        _, counts, mask = ops.cols_above(scores, self.quantile_thresholds(percentile), column=cat_id, device=True)
        return cat_id, mask, counts

    def index_map_quantile(self, name: str, percentile: float = 95.0) -> np.ndarray:
        """bool mask (N,): float64(scores_mat[:, c]) > quantile_thresholds(percentile)[c] for `name`'s category c -- the voxels that
        look most like the category on its own score column (95: the top twentieth), whatever the other categories score.  Needs
        init_categories; NotImplementedError when the rows are sharded over ranks (a global quantile needs a merged histogram).
        The rule is upstream's map/clip_map.py:45-75 (CLIPMap.load_categories), with these differences: upstream divides each column
        by its maximum in float32 first, compares in float32 and works on a dense 2-D CLIP grid; here the threshold is the float64
        quantile of the RAW column (np.percentile(column.astype(np.float64), percentile) bit for bit) over the map's voxel list and
        the comparison is float64(score) > threshold.  Scaling by a positive maximum does not change the order, so the two rules
        select the same ranks up to float32 rounding.  Nothing was compared with CLIPMap, which cannot be imported (its imports name
        a utils package that does not exist)."""
        return self._quantile_mask_device(name, percentile)[1].numpy().astype(bool)

    def quantile_labels(self, percentile: float = 95.0):
        """(words, counts): words (N, ceil(Q / 64)) uint64, bit c % 64 of word c / 64 of row r set iff voxel r lies above category c's
        percentile (a voxel may carry several categories or none); counts (Q,) int64, the voxels of every category.  One pass over
        the resident scores (ops.cols_above)."""
        from .. import ops
        return ops.cols_above(self._scores_device(), self.quantile_thresholds(percentile))

    def get_quantile_predict_mask(self, name: str, percentile: float = 95.0) -> np.ndarray:
        """get_predict_mask for the quantile rule: the top-down mask over the obstacle crop, 1 where a voxel of index_map_quantile's
        mask lies in the column, in obstacles_cropped's shape and dtype (ops.pool_label_2d, cut to the crop like get_predict_mask)."""
        from .. import ops
        self._scores_device()                            # raises when init_categories has not run
        r0, r1, c0, c1 = self._crop_window()
        mask = self._quantile_mask_device(name, percentile)[1]
        pooled = ops.pool_label_2d(mask, self._device_pos(), int(self.gs), device=True).numpy()
        return pooled[r0:r1, c0:c1].astype(np.asarray(self.obstacles_cropped).dtype)

    def _instances_3d(self, name: str, connectivity: int = 26):
        """(category id, ops.VoxelInstances) of the voxels whose argmax is `name`'s category, labels on the device.  The last result
        stays on the map until the categories, the category or the connectivity change."""
        from .. import ops
        from ..device import DeviceArray
        from ..utils.index_utils import find_similar_category_id
        am = self._argmax_device()                       # raises when init_categories has not run
        cat_id = find_similar_category_id(name, self.categories)
        key = (self.scores_mat, self.grid_pos, cat_id, int(connectivity))
        cached = getattr(self, "_instances_cache", None)
        if cached is not None:
            (scores_mat, grid_pos, *rest), inst = cached
            if scores_mat is self.scores_mat and grid_pos is self.grid_pos and tuple(rest) == key[2:]:
                return cat_id, inst
            inst.close()
            self._instances_cache = None
        mask = ops.mask_from_argmax(am, cat_id)
        scores = DeviceArray.from_numpy(np.ascontiguousarray(self.scores_mat[:, cat_id], dtype=np.float32))
        inst = ops.label_voxels(self._device_pos(), mask, connectivity=connectivity, scores=scores, device=True)
        self._instances_cache = (key, inst)
        return cat_id, inst

    def get_instances_3d(self, name: str, min_voxels: int = 50, connectivity: int = 26):
        """The objects of a category in 3-D: a list of ops.Instance3D, one per connected component (connectivity 6 / 18 / 26) of the
        voxels whose argmax over scores_mat is the category, in label order.  Upstream has no counterpart: vlmap_3d.py:75-100 and
        habitat_lang_robot.py:242-265 stop at the category mask.  Needs init_categories.  Components of fewer than min_voxels voxels
        are dropped here on the host; the others keep their labels, which are what AVLMap.index_object_instance takes.  best_voxel
        is the voxel with the category's largest score in scores_mat."""
        from .. import ops
        _, inst = self._instances_3d(name, connectivity)
        table, best = inst.table, inst.best_score
        return [ops.Instance3D.from_row(k + 1, table[k], best[k]) for k in range(inst.n) if table[k, 0] >= int(min_voxels)]

    def get_objects(self, min_voxels: int = 50, connectivity: int = 26, exclude=("other",)):
        """What is in this scene: a SceneObjects (map/scene_objects.py) of ALL objects of ALL categories.  A voxel's class is its row
        argmax over scores_mat; the categories named in `exclude` get class -1 and take part in nothing (scores_mat's columns are
        the init_categories names plus the "other" that init_categories appends).  One labelling by class (ops.label_voxel_classes:
        get_instances_3d's components of every category at once, numbered 1 .. n by (first cell, category)), one table, with every
        voxel's score of its own class (ops.pick_columns), and one pooling of the resident scores_mat (ops.pool_rows) give
        mean_scores, voted and margin per object.  `objects` lists those of at least min_voxels voxels; they keep their scene-wide
        labels, which are what AVLMap.index_scene_object takes.  Needs init_categories.  The labelling stays on the map until the
        categories, the connectivity or `exclude` change.  NotImplementedError when the rows are sharded over ranks, like the
        quantile queries.  Upstream has no counterpart: vlmap_3d.py:75-100 stops at one category's mask."""
        from .. import ops, parallel
        from ..device import DeviceArray
        from .scene_objects import SceneObjects
        if self.scores_mat is not None and self.categories is not None and parallel.rank_world()[1] > 1 and self.shard_index_rows:
            raise NotImplementedError("get_objects on rows sharded over ranks: an object's voxels lie in several ranks' blocks")
        scores = self._scores_device()                   # raises when init_categories has not run
        am = self._argmax_device()
        Q = int(self.scores_mat.shape[1])
        names = list(self.categories)[:Q] + ["other"] * (Q - len(self.categories))
        exclude = tuple(exclude or ())
        key = (self.scores_mat, self.grid_pos, int(connectivity), exclude)
        cached = getattr(self, "_objects_cache", None)
        if cached is not None:
            (scores_mat, grid_pos, *rest), scene = cached
            if scores_mat is self.scores_mat and grid_pos is self.grid_pos and tuple(rest) == key[2:]:
                if scene.min_voxels != int(min_voxels):  # the same labelling, listed again
                    positions = scene.positions
                    scene = SceneObjects(scene.voxel_objects, scene.mean_scores, self._argmax, names, min_voxels, connectivity, exclude)
                    scene.positions = positions
                    self._objects_cache = (key, scene)
                return scene
            scene.close()
            self._objects_cache = None
        classes = am
        out = [c for c, name in enumerate(names) if name in exclude]
        if out:                                          # the excluded columns' voxels leave on the host's copy of the argmax
            host = np.array(self._argmax, dtype=np.int32, copy=True)
            host[np.isin(host, out)] = -1
            classes = DeviceArray.from_numpy(host)
        own = ops.pick_columns(scores, am, device=True)
        vo = ops.label_voxel_classes(self._device_pos(), classes, connectivity=connectivity, scores=own, device=True)
        vo.classes = self._argmax                        # classes_of from the host's copy: an object's first voxel is not excluded
        sums = ops.pool_rows(scores, vo.labels_dev, vo.n)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = sums / vo.table[:, 0:1].astype(np.float64)
        scene = SceneObjects(vo, mean, self._argmax, names, min_voxels, connectivity, exclude)
        scene.positions = self._device_pos()             # assign_rooms lifts the rooms onto these
        self._objects_cache = (key, scene)
        return scene

    def get_scene_graph(self, radius: float = 0.25, min_voxels: int = 50, connectivity: int = 26, exclude=("other",)):
        """How the objects of this scene stand to one another: a SceneGraph (map/scene_graph.py) of get_objects(min_voxels,
        connectivity, exclude) -- its cache, its errors -- and of every pair of objects that come within `radius` metres of each
        other: the nearest gap and its two voxels, how many voxels of one lie directly on the other, and how many touch.  The
        radius in cells is R = min(max(round(radius / cs), 1), 15).  One ops.cell_index over the resident cells and one
        ops.object_relations on the resident labels; the grid is gs x gs x vh with vh the height of occupied_ids, or the largest
        height of grid_pos plus one on a map without it.  Upstream has no counterpart: map.py:183-240 relates one category's 2-D
        islands."""
        from .. import ops
        from .scene_graph import SceneGraph
        scene = self.get_objects(min_voxels=min_voxels, connectivity=connectivity, exclude=exclude)
        cs = float(self.cs)
        radius = float(radius)
        if not (np.isfinite(radius) and radius > 0.0 and np.isfinite(cs) and cs > 0.0):
            raise ValueError(f"get_scene_graph: radius {radius} m at a cell size of {cs} m (both finite and > 0)")
        R = min(max(int(round(radius / cs)), 1), ops.RELATIONS_MAX_RADIUS)
        if getattr(self, "occupied_ids", None) is not None:
            vh = int(np.asarray(self.occupied_ids).shape[2])
        else:
            vh = max(int(np.asarray(self.grid_pos)[:, 2].max()) + 1, 1) if len(self.grid_pos) else 1
        vo = scene.voxel_objects
        pos = self._device_pos()
        with ops.cell_index(pos, int(self.gs), vh) as index:
            relations = ops.object_relations(index, pos, vo.labels_dev, vo.n, R)
        return SceneGraph(scene, relations, cs, R)

    def _distribution_map_device(self, name: str, decay_rate: float = 0.1):
        from .. import ops
        window = self._crop_window()
        return ops.mask_decay_2d(self._predict_mask_device(name), decay_rate, normalize=True, smooth_sigma=1, device=True, window=window)

    def get_distribution_map(self, name: str, decay_rate: float = 0.1) -> np.ndarray:
        """The 2-D distribution map of a category over the obstacle crop, (h, w) float64.  Reference:
        habitat_lang_robot.py:229-240 get_vl_distribution_map: predicted mask -> gaussian_filter(float32, sigma=1) > 0.5 ->
        distance_transform_edt(mask == 0) -> 1 - d * decay_rate, negative values 0 -> min-max normalisation.  The whole chain runs on
        the GPU (avl_gauss2d_f32, avl_mask_decay_2d) with SciPy's and NumPy's bits; between the voxel argmax and the finished map
        only status flags come back to the host.  ValueError when no cell survives the smoothing (a category without a voxel) or the
        map is constant."""
        return self._distribution_map_device(name, decay_rate).numpy()

    def _travel_distribution_map_device(self, name: str, decay_rate: float = 0.1, customized: bool = False):
        from .. import ops
        window = self._crop_window()
        mask = ops.mask_smooth_2d(self._predict_mask_device(name), 1, window=window, device=True)
        try:
            field = ops.travel_field(self._travel_free(customized), mask, device=True)
        except ValueError as e:
            if "no source" not in str(e):
                raise
            raise ValueError("get_travel_distribution_map: the mask has no target cell after the smoothing") from None
        return ops.travel_decay_2d(field, decay_rate, cell_size=1.0, normalize=True, device=True)

    def get_travel_distribution_map(self, name: str, decay_rate: float = 0.1, customized: bool = False) -> np.ndarray:
        """get_distribution_map with the travel distance in place of the straight line: (h, w) float64 over the obstacle crop.  The
        mask chain is get_distribution_map's (predicted mask -> gaussian_filter(float32, sigma=1) > 0.5); its cells are the sources
        of ops.travel_field on the obstacle crop (customized: the customised crop), then 1 - d * decay_rate, negative and unreached
        cells 0, min-max normalisation (ops.travel_decay_2d) -- all on the device.  The heat no longer passes through walls: a cell
        behind one is as cold as the walk around it is long, and a cell no walk reaches is 0.  ValueError when no cell survives the
        smoothing or the map is constant, as get_distribution_map."""
        return self._travel_distribution_map_device(name, decay_rate, customized).numpy()

    def plan_object_tour(self, start, names, closed: bool = False, customized: bool = False):
        """Map.plan_tour over categories: "go to the sofa, the table and the lamp, in the best order".  The goal of a name is the
        set of crop cells of its pooled 2-D mask after get_travel_distribution_map's smoothing (predicted mask ->
        gaussian_filter(float32, sigma=1) > 0.5, on the device; only the (h, w) byte mask comes to the host, where the sets are
        listed).  start: a full-map (row, col).  -> tour.Tour; Tour.names / Tour.skipped_names are the names in visiting order and
        the ones no walk from the start reaches.  ValueError for a name without a target cell after the smoothing."""
        from .. import ops
        names = list(names)
        window = self._crop_window()
        goals = []
        for name in names:
            mask = ops.mask_smooth_2d(self._predict_mask_device(name), 1, window=window)
            if not mask.any():
                raise ValueError(f"plan_object_tour: the mask of {name!r} has no target cell after the smoothing")
            goals.append(mask)
        tour = self.plan_tour(start, goals, closed=closed, customized=customized)
        tour.names = [names[k] for k in tour.order]
        tour.skipped_names = [names[k] for k in tour.skipped]
        return tour

    def get_voxel_rooms(self, rooms, device: bool = False):
        """(N,) int32: the room of every voxel, rooms.labels[row - rmin, col - cmin] of its cell and 0 outside the crop
        (ops.lift_labels_2d on the resident positions).  rooms: Map.get_rooms' result.  A voxel above an obstacle cell -- the top
        of a table -- is in no room unless the rooms were made on a walls-only customised map.  NotImplementedError when the rows
        are sharded over ranks, like get_objects."""
        from .. import ops, parallel
        if parallel.rank_world()[1] > 1 and self.shard_index_rows:
            raise NotImplementedError("get_voxel_rooms on rows sharded over ranks")
        if self.grid_pos is None or len(self.grid_pos) == 0:
            return np.zeros((0,), np.int32)
        return ops.lift_labels_2d(rooms.labels, self._device_pos(), rooms.window, device=device)

    def customize_obstacle_map(self, potential_obstacle_names: List[str], obstacle_names: List[str], vis: bool = False):
        """Reference: vlmap.py:127-156 (like upstream the class lists and the smoothing parameters come from map_config, not from
        the arguments).  The class scoring and the scatter run on the GPU (avl_obstacle_scatter), and so does the 2-D smoothing
        (Map._dilate_map's chain, avl_dilate_map); the (H, W) byte map takes one host hop in between, where upstream negates it."""
        from .. import ops
        from ..utils.index_utils import get_dynamic_obstacles_map_3d
        if self.obstacles_cropped is None and self.obstacles_map is None:
            self.generate_obstacle_map()
        if not hasattr(self, "clip_model"):
            print("init_clip in customize obstacle map")
            self._init_clip()
        potential = list(cfg_get(self.map_config, "potential_obstacle_names"))
        feat, predict = self._device_feat(), None
        if self._rows != (0, len(self.grid_feat)):      # rows sharded over ranks: score here, hand the full argmax down
            q, _ = landmark_text_feats(self.clip_model, potential, self.clip_feat_dim, use_multiple_templates=True, add_other=True)
            predict = self._score(q, want_scores=False)[1]
        self.obstacles_new_cropped = get_dynamic_obstacles_map_3d(
            self.clip_model, self.obstacles_cropped, potential, list(cfg_get(self.map_config, "obstacle_names")), feat,
            self.grid_pos, self.rmin, self.cmin, self.clip_feat_dim, vis=vis, precision=self._sim_precision, predict=predict)
        # Map._dilate_map(...) == 0 (vlmap.py:151-156): the comparison is the composite's second output, the float64 image stays unbuilt
        self.obstacles_new_cropped = ops.dilate_map(self.obstacles_new_cropped == 0, cfg_get(self.map_config, "dilate_iter"),
                                                    cfg_get(self.map_config, "gaussian_sigma"), want_values=False)[1]

    island_path = None          # "host" / "device" forces get_pos's island step; None: host with OpenCV installed, else device

    def _island_path(self) -> str:
        if self.island_path is not None:
            return self.island_path
        try:
            import cv2  # noqa: F401
            return "host"
        except Exception:
            return "device"

    @property
    def _last_foreground(self):
        """the (h, w) bool foreground mask of the last get_pos call (None before the first)"""
        fg = self.__dict__.get("_foreground")
        if fg is not None and not isinstance(fg, np.ndarray):
            fg = self.__dict__["_foreground"] = fg.numpy().astype(bool)
        return fg

    @_last_foreground.setter
    def _last_foreground(self, value):
        self.__dict__["_foreground"] = value

    def get_pos(self, name: str):
        """Contours, centres and bounding boxes of a category on the full map.  Reference: vlmap.py:158-187.  The per-voxel
        work (argmax mask, top-down pooling) and the 2-D morphology (closing, gaussian, threshold, dilation: avl_mask_foreground,
        SciPy's results bit for bit) run on the GPU.  With OpenCV installed the finished foreground mask is copied back and
        utils/navigation_utils.get_segment_islands_pos calls cv2.findContours as upstream does; without it the islands are
        labelled and traced on the GPU too (get_segment_islands_pos_device: the same result as the host function's SciPy path)
        and only the island table and the contour points are copied back."""
        from .. import ops
        from ..utils.navigation_utils import get_segment_islands_pos, get_segment_islands_pos_device
        assert self.categories
        pc_mask = self.index_map(name, with_init_cat=True)
        mask_2d = ops.pool_label_2d(pc_mask, self._device_pos(), int(self.gs), device=True)
        if self._island_path() == "host":
            foreground = ops.mask_foreground(mask_2d, self.rmin, self.rmax + 1, self.cmin, self.cmax + 1)
            self._last_foreground = foreground
            contours, centers, bbox_list, _ = get_segment_islands_pos(foreground, 1)
        else:
            foreground = ops.mask_foreground(mask_2d, self.rmin, self.rmax + 1, self.cmin, self.cmax + 1, device=True)
            self._last_foreground = foreground                  # stays on the device; reading the attribute copies it back
            contours, centers, bbox_list, _ = get_segment_islands_pos_device(foreground, 1)
        for i in range(len(contours)):          # whole-map positions (upstream adds rmin to both row bounds: kept)
            centers[i][0] += self.rmin
            centers[i][1] += self.cmin
            bbox_list[i][0] += self.rmin
            bbox_list[i][1] += self.rmin
            bbox_list[i][2] += self.cmin
            bbox_list[i][3] += self.cmin
            contours[i][:, 0] += self.rmin
            contours[i][:, 1] += self.cmin
        return contours, centers, bbox_list
