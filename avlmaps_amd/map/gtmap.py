"""Ground-truth label map of a scene, and the scores of a VLMap against it (csrc/avl_gtmap.hip).

Upstream has the pieces of a GT map but not the map: Map._setup_paths collects semantic/*.npy and nothing reads them, the
dataloader's get_gt_semantic_cropped / get_obstacles_cropped_no_floor read a gt_cropped nothing sets
(habitat_dataloader.py:85-107), and avlmaps/map/gtmap.py:18-30 loads a grid_gt_1.npy no program of the tree writes (and imports
from a utils.* package that does not exist, so it cannot be imported).  GTMap here MAKES the map: every labelled pixel of every
semantic frame votes for its class in the voxel the builder fuses that pixel into (ops.gt_vote), a voxel takes its majority class
(ops.gt_labels), the top-down grid_gt is the label of each column's highest labelled voxel (ops.pool_labels_2d), and a VLMap is
scored against it with a confusion matrix (ops.label_confusion, ops.map_scores).  get_predict_mask / get_pos and the floor rule
follow gtmap.py:22-30,41-71."""
from __future__ import annotations

from pathlib import Path
from typing import List

import numpy as np

from .map import Map, cfg_get


def load_semantic_npy(path) -> np.ndarray:
    """semantic/*.npy: the object id of every pixel, (H, W) (or (H, W, 1)) of any integer dtype.  Reference: dataset/README.md:78."""
    a = np.load(path, allow_pickle=False)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim != 2 or a.dtype.kind not in "iu":
        raise ValueError(f"{path}: expected an (H, W) integer image of object ids, got {a.dtype}{a.shape}")
    return a


class GTMap(Map):
    GT_FILE = "gt_labels.npz"

    def __init__(self, map_config, data_dir: str = "", floor_id: int = 2):
        super().__init__(map_config, data_dir=data_dir)
        self.floor_id = int(floor_id)             # gtmap.py:22: cells whose GT label is the floor are free
        self.vlmap = None
        self.labels = None                        # (N,) int32 majority class of every voxel of the VLMap, -1 = no vote
        self.support = None                       # (N,) uint32 votes the voxel received
        self.grid_gt = None                       # (gs, gs) int32 top-down label map, -1 = no labelled voxel in the column
        self.stats = None                         # (4,) uint64: pixels dropped by depth or grid, by class, for want of a voxel; votes cast
        self.categories = None
        self.gt_params = None
        self.obstacles_new_cropped = None
        self._dev = {}

    # ------------------------------------------------------------------ the VLMap this GT map labels
    def _attach(self, vlmap) -> None:
        self.vlmap = vlmap
        self.grid_pos, self.occupied_ids = vlmap.grid_pos, vlmap.occupied_ids
        self.obstacles_map = self.obstacles_cropped = self.obstacles_new_cropped = None
        self._dev = {}

    def _load_vlmap(self, data_dir, vlmap):
        if vlmap is None:
            from .vlmap import VLMap
            vlmap = VLMap(self.map_config)
            vlmap.prefetch_device = False         # the votes need the voxel index, not the features
            if not vlmap.load_map(str(data_dir)):
                return None
        if vlmap.occupied_ids is None or vlmap.grid_pos is None:
            raise ValueError("GTMap: the VLMap is not loaded (a GT map labels the voxels of a map: build one first, --features hash will do)")
        return vlmap

    def _device_occupied(self):
        from ..device import DeviceArray
        if self._dev.get("occ_src") is not self.occupied_ids:
            self._dev["occ"] = DeviceArray.from_numpy(np.ascontiguousarray(self.occupied_ids, dtype=np.int32))
            self._dev["occ_src"] = self.occupied_ids
        return self._dev["occ"]

    def _device_labels(self):
        from ..device import DeviceArray
        if self._dev.get("labels_src") is not self.labels:
            self._dev["labels"] = DeviceArray.from_numpy(np.ascontiguousarray(self.labels, dtype=np.int32))
            self._dev["labels_src"] = self.labels
        return self._dev["labels"]

    # ------------------------------------------------------------------ build / load
    def create_map(self, data_dir, vlmap=None, obj2cls=None, categories: List[str] = None, stride: int = 1, batch: int = 16) -> np.ndarray:
        """Vote the semantic frames of the scene into the voxels of its VLMap and write <data_dir>/vlmap/gt_labels.npz; returns
        grid_gt.  vlmap: the scene's loaded VLMap (None: it is loaded from data_dir).  obj2cls: an int array, a dict {object id:
        class id | (class id, name)}, or a path to .npy / .json (ops.obj2cls_table); None: <data_dir>/semantic/obj2cls.json when it
        exists, else the frames hold class ids.  categories: names whose index is the class id; their number is the number of
        classes (without them: the table's largest class + 1).  One vote per stride-th pixel in both directions;
        frames go up in batches of `batch`, one loader thread ahead of the GPU."""
        from .. import ops
        from ..device import DeviceArray
        from ._frames import batch_ranges, depth_batch, prefetch
        from .vlmap_builder import VLMapBuilder
        self._setup_paths(data_dir)
        if not self.semantic_paths:
            raise FileNotFoundError(f"{self.semantic_dir} holds no semantic frames (*.npy with the object id of every pixel): a GT map "
                                    "needs them; the scene's VLMap does not")
        if int(batch) < 1:
            raise ValueError(f"create_map: batch {batch} < 1")
        if int(stride) < 1:
            raise ValueError(f"create_map: stride {stride} < 1")
        vlmap = self._load_vlmap(data_dir, vlmap)
        if vlmap is None:
            raise FileNotFoundError(f"{Path(data_dir) / 'vlmap' / 'vlmaps.h5df'}: a GT map labels the voxels of the scene's VLMap; build it first")
        self._attach(vlmap)
        if obj2cls is None and (self.semantic_dir / "obj2cls.json").exists():
            obj2cls = self.semantic_dir / "obj2cls.json"
        table = ops.obj2cls_table(obj2cls)
        if categories is not None:
            categories = [str(c) for c in categories]
            C = len(categories)
        elif table is not None and table.size and int(table.max()) >= 0:
            C = int(table.max()) + 1
        else:
            raise ValueError("create_map: the number of classes is unknown: pass categories")
        if categories is None:
            categories = [str(k) for k in range(C)]
        builder = VLMapBuilder(self.data_dir, self.map_config, self.pose_path, self.rgb_paths, self.depth_paths, self.base2cam_tf,
                               self.base_transform)
        calib = np.array(list(cfg_get(self.map_config, "cam_calib_mat")), dtype=np.float64).reshape((3, 3))
        poses = np.loadtxt(self.pose_path).reshape((-1, 7))
        transforms = np.stack(builder.frame_transforms(poses)) if len(poses) else np.zeros((0, 4, 4))
        n = min(len(self.depth_paths), len(self.semantic_paths), len(poses))
        N = int(len(self.grid_pos))
        params = dict(cs=float(self.cs), stride=int(stride), min_depth=float(builder.min_depth), max_depth=float(builder.max_depth))

        def load(lo, hi):
            depth = depth_batch(self.depth_paths, lo, hi)
            sem = ops._ids_i32(np.stack([load_semantic_npy(self.semantic_paths[i]) for i in range(lo, hi)]), "semantic")
            return lo, hi, depth.reshape(sem.shape), sem
        frames = prefetch(load, batch_ranges(n, batch), "avl-gtmap-load")
        occ = self._device_occupied()
        votes = DeviceArray((N, C), np.uint32).zero_()
        stats = DeviceArray((4,), np.uint64).zero_()
        flag = DeviceArray((1,), np.int32).zero_()
        table_dev = None if table is None else DeviceArray.from_numpy(table)
        try:
            for lo, hi, depth, sem in frames:
                ops.gt_vote(votes, DeviceArray.from_numpy(depth), DeviceArray.from_numpy(sem), calib, transforms[lo:hi], occ, N, C,
                            obj2cls=table_dev, stats=stats, err_flag=flag, device=True, **params)
            labels, support = ops.gt_labels(votes, device=True)
            grid_gt = ops.pool_labels_2d(labels, occ, err_flag=flag, device=True)
            ops.check_label_flag(flag, "GTMap.create_map")
            self.labels, self.support, self.grid_gt, self.stats = labels.numpy(), support.numpy(), grid_gt.numpy(), stats.numpy()
        finally:
            votes.free()
        self.categories = categories
        self.gt_params = dict(params, gs=int(self.gs), n_classes=C, n_voxels=N, n_frames=n)
        out_dir = self.data_dir / "vlmap"
        out_dir.mkdir(parents=True, exist_ok=True)
        self.save_map(out_dir / self.GT_FILE)
        return self.grid_gt

    def save_map(self, path) -> None:
        np.savez_compressed(path, labels=self.labels, support=self.support, grid_gt=self.grid_gt, stats=self.stats,
                            categories=np.array(self.categories, dtype=np.str_), **self.gt_params)

    def load_map(self, data_dir, vlmap=None) -> bool:
        """Read <data_dir>/vlmap/gt_labels.npz (and the scene's VLMap unless one is given); False when either file is missing.  A
        file made for a map with another number of voxels or another grid is refused: ValueError."""
        self._setup_paths(data_dir)
        path = Path(data_dir) / "vlmap" / self.GT_FILE
        if not path.exists():
            print("Loading GTMap failed because the file doesn't exist.")
            return False
        vlmap = self._load_vlmap(data_dir, vlmap)
        if vlmap is None:
            return False
        with np.load(path, allow_pickle=False) as z:
            arrays = {k: z[k] for k in ("labels", "support", "grid_gt", "stats")}
            categories = [str(c) for c in z["categories"]]
            params = {k: z[k].item() for k in z.files if k not in arrays and k != "categories"}
        N = int(len(vlmap.grid_pos))
        if arrays["labels"].shape != (N,) or int(params.get("n_voxels", N)) != N:
            raise ValueError(f"{path}: GT labels of {arrays['labels'].shape[0]} voxels do not belong to this map of {N} voxels")
        if arrays["grid_gt"].shape != (self.gs, self.gs):
            raise ValueError(f"{path}: GT map of grid {arrays['grid_gt'].shape} does not belong to this map ({self.gs})")
        self._attach(vlmap)
        self.labels = np.ascontiguousarray(arrays["labels"], dtype=np.int32)
        self.support = np.ascontiguousarray(arrays["support"], dtype=np.uint32)
        self.grid_gt = np.ascontiguousarray(arrays["grid_gt"], dtype=np.int32)
        self.stats = np.ascontiguousarray(arrays["stats"], dtype=np.uint64)
        self.categories, self.gt_params = categories, params
        return True

    def _require(self) -> np.ndarray:
        if self.grid_gt is None:
            raise RuntimeError("no GT map loaded: run GTMap.create_map (apps.create_map --gt) or load a scene that has vlmap/gt_labels.npz")
        return self.grid_gt

    def load_categories(self, categories: List[str] = None) -> None:
        """Reference: gtmap.py:32-39, without upstream's built-in lists: the names come with the map or from the caller."""
        if categories is not None:
            self.categories = [str(c) for c in categories]

    # ------------------------------------------------------------------ 2-D products (gtmap.py:18-30,41-71)
    def _crop(self):
        if self.obstacles_cropped is None:
            self.generate_obstacle_map()
        return int(self.rmin), int(self.rmax), int(self.cmin), int(self.cmax)

    def get_gt_cropped(self) -> np.ndarray:
        """grid_gt over the obstacle crop (upstream's map_cropped, gtmap.py:20)"""
        grid_gt = self._require()
        r0, r1, c0, c1 = self._crop()
        return grid_gt[r0:r1 + 1, c0:c1 + 1]

    def get_customized_obstacle_cropped(self) -> np.ndarray:
        """Reference: gtmap.py:22-30: obstacle cells whose GT label is the floor become free, then Map._dilate_map's chain; True = free."""
        from .. import ops
        if self.obstacles_new_cropped is None:
            gt = self.get_gt_cropped()
            free = np.array(self.obstacles_cropped, copy=True)
            free[gt == self.floor_id] = 1
            self.obstacles_new_cropped = ops.dilate_map(free == 0, cfg_get(self.map_config, "dilate_iter"),
                                                        cfg_get(self.map_config, "gaussian_sigma"), want_values=False)[1]
        return self.obstacles_new_cropped

    def get_predict_mask(self, name: str) -> np.ndarray:
        """The foreground of a category over the obstacle crop, bool.  Reference: gtmap.py:46-49: the cells labelled with the
        category, scipy.ndimage.binary_closing(iterations=3) -- three dilations, then three erosions, border value 0, on the GPU
        (ops.binary_morph) -- AND the obstacle cells."""
        from .. import ops
        from ..utils.index_utils import find_similar_category_id
        cat_id = find_similar_category_id(name, self.categories)
        segment = self.get_gt_cropped() == cat_id
        grown = ops.binary_morph(segment, "dilate", iterations=3, device=True)
        closed = ops.binary_morph(grown, "erode", iterations=3)
        return np.logical_and(closed, np.asarray(self.obstacles_cropped) == 0)

    def get_pos(self, name: str):
        """Contours, centres and bounding boxes of a category on the full map.  Reference: gtmap.py:41-71; the islands are labelled
        and traced on the GPU (get_segment_islands_pos_device), the offsets are VLMap.get_pos's (upstream adds rmin to both row
        bounds: kept)."""
        from ..utils.navigation_utils import get_segment_islands_pos_device
        foreground = self.get_predict_mask(name)
        self._last_foreground = foreground
        contours, centers, bbox_list, _ = get_segment_islands_pos_device(foreground.astype(np.uint8), 1)
        for i in range(len(contours)):
            centers[i][0] += self.rmin
            centers[i][1] += self.cmin
            bbox_list[i][0] += self.rmin
            bbox_list[i][1] += self.rmin
            bbox_list[i][2] += self.cmin
            bbox_list[i][3] += self.cmin
            contours[i][:, 0] += self.rmin
            contours[i][:, 1] += self.cmin
        return contours, centers, bbox_list

    # ------------------------------------------------------------------ scores
    def evaluate(self, vlmap=None, dim: str = "3d"):
        """-> ops.MapScores of `vlmap` (default: the map this GT map labels) against the ground truth.  The predicted label of a
        voxel is the argmax of vlmap.init_categories(self.categories) -- len(categories) + 1 columns, the last one "other" -- and goes
        up to the device once.  dim="3d": one pair per voxel; a voxel no labelled pixel reached is skipped.  dim="2d": predictions and
        ground truth each go through ops.pool_labels_2d over the obstacle crop first; one pair per cell.  Only the matrix and the two
        skip counts come back to the host."""
        from .. import ops
        self._require()
        vlmap = self.vlmap if vlmap is None else vlmap
        if dim not in ("3d", "2d"):
            raise ValueError(f"evaluate: dim {dim!r} (3d or 2d)")
        if vlmap.grid_pos is None or len(vlmap.grid_pos) != len(self.labels):
            raise ValueError(f"evaluate: the map has {None if vlmap.grid_pos is None else len(vlmap.grid_pos)} voxels, the GT map {len(self.labels)}")
        vlmap.init_categories(list(self.categories))
        pred = vlmap._argmax_device()
        Cg, Cp = len(self.categories), int(vlmap.scores_mat.shape[1])
        gt = self._device_labels()
        if dim == "2d":
            r0, r1, c0, c1 = self._crop()
            occ = self._device_occupied()
            gt = ops.pool_labels_2d(gt, occ, (r0, r1, c0, c1), device=True)
            pred = ops.pool_labels_2d(pred, occ, (r0, r1, c0, c1), device=True)
        conf, skipped = ops.label_confusion(gt, pred, Cg, Cp)
        return ops.map_scores(conf, skipped=skipped, categories=self.categories)
