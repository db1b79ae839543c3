"""Map base class with the reference's attribute surface (avlmaps/map/map.py:18-129).

Consumers upstream (AVLMap, the Habitat dataloader and robot) read these attributes directly, so they keep
the reference's names, dtypes and host-NumPy type: grid_feat, grid_pos, weight, occupied_ids, grid_rgb,
mapped_iter_list, gs, cs, base2cam_tf, base_transform, obstacles_map, obstacles_cropped, rmin/rmax/cmin/cmax.
"""
from __future__ import annotations

from pathlib import Path
from typing import List, Union

import numpy as np


def cfg_get(cfg, key):
    """attribute-or-item access: works for omegaconf.DictConfig, dicts and plain namespaces"""
    if isinstance(cfg, dict):
        return cfg[key]
    try:
        return getattr(cfg, key)
    except AttributeError:
        return cfg[key]


class VisibilityAudit:
    """Map.audit_visibility's result.  last_hit (N,) int32: the last frame whose depth ray ended in the voxel, -1 = none;
    through (N,) uint32: the rays of frames after that which passed through its cell; params: gs, cs, vh, stride, end_margin,
    n_frames; frame_counts: the frames of every audited directory, in order."""

    def __init__(self, last_hit, through, params, frame_counts):
        self.last_hit = np.ascontiguousarray(last_hit, dtype=np.int32)
        self.through = np.ascontiguousarray(through, dtype=np.uint32)
        if self.last_hit.ndim != 1 or self.through.shape != self.last_hit.shape:
            raise ValueError(f"VisibilityAudit: last_hit {self.last_hit.shape} and through {self.through.shape} must be (N,) both")
        self.params = dict(params)
        self.frame_counts = [int(c) for c in frame_counts]

    @property
    def N(self) -> int:
        return int(self.last_hit.shape[0])

    def stale(self, min_rays: int = 3) -> np.ndarray:
        """(N,) bool: through >= min_rays.  min_rays = 3 (and the audit's end_margin = 2) are defaults chosen by argument -- a
        sparse ray lattice, grazing rays -- not by measurement."""
        if int(min_rays) < 1:
            raise ValueError(f"stale: min_rays {min_rays} < 1")
        return self.through >= np.uint32(min(int(min_rays), 2 ** 32 - 1))

    def save(self, path) -> None:
        np.savez_compressed(path, last_hit=self.last_hit, through=self.through, frame_counts=np.asarray(self.frame_counts, np.int64),
                            **self.params)

    @classmethod
    def load(cls, path) -> "VisibilityAudit":
        with np.load(path, allow_pickle=False) as z:
            params = {k: z[k].item() for k in z.files if k not in ("last_hit", "through", "frame_counts")}
            return cls(z["last_hit"], z["through"], params, z["frame_counts"].tolist())


class Viewpoints:
    """Map.get_viewpoints' result: the candidate eye cells of one target and what each of them sees.  cells (E, 2) int64 full-map
    (row, col) in raster order; visible (E,) uint32, the target voxels with a free sight line from the cell; first (E,) int32, the
    first of them (an index into the target rows that were used), -1 = none; n_targets, how many target voxels were tested;
    eye_h, the height cell of every eye; window = (rmin, cmin, H, W), the obstacle crop the cells were taken from."""

    def __init__(self, cells, visible, first, n_targets, eye_h, window):
        self.cells = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1, 2)
        self.visible = np.ascontiguousarray(visible, dtype=np.uint32).reshape(-1)
        self.first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        if not len(self.cells) == len(self.visible) == len(self.first):
            raise ValueError(f"Viewpoints: {len(self.cells)} cells, {len(self.visible)} counts, {len(self.first)} first targets")
        self.n_targets, self.eye_h = int(n_targets), int(eye_h)
        self.window = tuple(int(v) for v in window)

    def __len__(self) -> int:
        return len(self.cells)

    def best(self, k: int = 1) -> np.ndarray:
        """(<= k,) indices into cells of the cells that see the most, most first, equal counts in raster order; only cells that see
        something"""
        if int(k) < 0:
            raise ValueError(f"best: k {k} < 0")
        order = np.argsort(-self.visible.astype(np.int64), kind="stable")
        return order[:min(int(k), int(np.count_nonzero(self.visible)))]

    def select(self, min_fraction: float = 0.5) -> np.ndarray:
        """indices (in raster order) of the cells with visible >= max(1, ceil(min_fraction * max(visible))); none when nothing is
        visible from anywhere"""
        f = float(min_fraction)
        if not 0.0 <= f <= 1.0:
            raise ValueError(f"select: min_fraction {min_fraction} outside [0, 1]")
        if len(self.visible) == 0 or int(self.visible.max()) == 0:
            return np.zeros((0,), np.int64)
        need = max(1, int(np.ceil(f * int(self.visible.max()))))
        return np.flatnonzero(self.visible >= need)

    def mask(self) -> np.ndarray:
        """(H, W) bool over the obstacle crop: True where visible > 0"""
        r0, c0, H, W = self.window
        out = np.zeros((H, W), dtype=bool)
        seen = self.cells[self.visible > 0]
        out[seen[:, 0] - r0, seen[:, 1] - c0] = True
        return out


class ExplorationViews:
    """Map.get_exploration_views' result: the candidate cells of the next look and what each of them would add.  cells (n, 2) int64
    full-map (row, col) in raster order; gain (n, 8) int32, the unknown cells that become visible from the cell per 45-degree
    sector (ops.viewshed_gain); total (n,) int64 = gain.sum(1); heading (n,) int64, the first sector of the pair of neighbouring
    sectors with the largest sum (ops.best_heading); distance (n, 2) int32, the travel field's pair (straight, diagonal steps)
    from the robot, (-1, -1) when no position was given; window = (rmin, cmin, H, W), the obstacle crop; radius, the sensor
    range in cells; field, the ops.TravelField the distances were read from, or None."""

    def __init__(self, cells, gain, distance, window, radius, field=None):
        from ..ops.viewshed import best_heading
        self.cells = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1, 2)
        self.gain = np.ascontiguousarray(gain, dtype=np.int32).reshape(-1, 8)
        self.distance = np.ascontiguousarray(distance, dtype=np.int32).reshape(-1, 2)
        if not len(self.cells) == len(self.gain) == len(self.distance):
            raise ValueError(f"ExplorationViews: {len(self.cells)} cells, {len(self.gain)} gains, {len(self.distance)} distances")
        self.total = self.gain.astype(np.int64).sum(axis=1)
        self.heading = best_heading(self.gain, 2)[0]
        self.window, self.radius, self.field = tuple(int(v) for v in window), int(radius), field

    def __len__(self) -> int:
        return len(self.cells)

    def select(self, min_fraction: float = 0.5) -> np.ndarray:
        """indices (in raster order) of the cells with total >= max(1, ceil(min_fraction * max(total))), Viewpoints.select's rule;
        none when no cell gains anything"""
        f = float(min_fraction)
        if not 0.0 <= f <= 1.0:
            raise ValueError(f"select: min_fraction {min_fraction} outside [0, 1]")
        if len(self.total) == 0 or int(self.total.max()) <= 0:
            return np.zeros((0,), np.int64)
        need = max(1, int(np.ceil(f * int(self.total.max()))))
        return np.flatnonzero(self.total >= need)

    def best(self):
        """the index of the cell with the largest total, the first in raster order among equals; None when no cell gains anything"""
        if len(self.total) == 0 or int(self.total.max()) <= 0:
            return None
        return int(np.argmax(self.total))

    def nearest(self, min_fraction: float = 0.5):
        """the index of the selected cell (select) with the shortest travel distance -- a1 + b1 sqrt(2) < a2 + b2 sqrt(2) decided in
        integers, as the field does -- the first in raster order among equals; None when no cell gains anything.  Without
        distances it is the first selected cell."""
        best = None
        for i in self.select(min_fraction):
            pair = (int(self.distance[i, 0]), int(self.distance[i, 1]))
            if best is None or _pair_less(pair, best[1]):
                best = (int(i), pair)
        return None if best is None else best[0]


def _pair_less(p, q) -> bool:
    """a1 + b1 sqrt(2) < a2 + b2 sqrt(2) for integer pairs, without rounding (Python's integers are unbounded)"""
    da, db = p[0] - q[0], p[1] - q[1]
    if da <= 0 and db <= 0:
        return (da, db) != (0, 0)
    if da >= 0 and db >= 0:
        return False
    return da * da > 2 * db * db if da < 0 else da * da < 2 * db * db


class Registration:
    """Map.register_frames' result.  corrections (V, 4, 4) float64, V = 1 (joint) or one per frame: to be left-multiplied onto the
    recording's transforms (audit_visibility(corrections=[..., reg.correction])).  transforms (n, 4, 4): the corrected camera -> map
    transforms of every frame of the directory.  best (V, 4) int32 = (angle index, di, dj, score) of each winner; valid (V,) uint32,
    the points that took part; fraction = score / valid (0 without a point); angle_deg and shift_cells (V, 2) spell the winners
    out.  frames: the indices of the frames that were matched; pivots (V, 2); params: the grid and the search window.  The shift
    is a whole number of cells: the translation is accurate to one cell, and pitch, roll and height are not searched."""

    def __init__(self, corrections, transforms, best, valid, angles, frames, pivots, joint, params):
        self.corrections, self.transforms = np.asarray(corrections, dtype=np.float64), np.asarray(transforms, dtype=np.float64)
        self.best, self.valid = np.asarray(best, dtype=np.int32).reshape(-1, 4), np.asarray(valid, dtype=np.uint32).reshape(-1)
        self.angles, self.frames, self.pivots = np.asarray(angles, dtype=np.float64), np.asarray(frames, dtype=np.int64), np.asarray(pivots)
        self.joint, self.params = bool(joint), dict(params)
        self.score = self.best[:, 3].copy()
        v = self.valid.astype(np.float64)
        self.fraction = np.divide(self.score.astype(np.float64), v, out=np.zeros(len(v)), where=v > 0)
        a = self.angles[self.best[:, 0]]
        self.angle_deg = np.degrees(np.arctan2(a[:, 1], a[:, 0]))
        self.shift_cells = self.best[:, 1:3].copy()

    @property
    def correction(self) -> np.ndarray:
        """the one 4 x 4 correction of a joint registration"""
        if not self.joint:
            raise ValueError("Registration.correction: a per-frame registration has one correction per frame (corrections)")
        return self.corrections[0]


class Map:
    def __init__(self, map_config, data_dir: str = ""):
        self.map_config = map_config
        self.gs = cfg_get(map_config, "grid_size")
        self.cs = cfg_get(map_config, "cell_size")
        self.mapped_iter_list = None
        self.grid_feat = None
        self.grid_pos = None
        self.weight = None
        self.occupied_ids = None
        self.grid_rgb = None
        self.obstacles_map = None
        self.obstacles_cropped = None
        self.first_seen = None            # (gs, gs) int32, the first frame that saw a cell, -1 = never (create_explored_map / load_explored_map)
        self.explored_params = None
        self.visibility = None            # VisibilityAudit of the voxels (audit_visibility / load_visibility)
        self._setup_transforms()
        if data_dir:
            self._setup_paths(data_dir)

    def _setup_paths(self, data_dir: Union[Path, str]) -> None:
        """Dataset layout of dataset/README.md:76-93.  Reference: map.py:41-52."""
        self.data_dir = Path(data_dir)
        self.rgb_dir = self.data_dir / "rgb"
        self.depth_dir = self.data_dir / "depth"
        self.semantic_dir = self.data_dir / "semantic"
        self.pose_path = self.data_dir / "poses.txt"
        self.rgb_paths = sorted(self.rgb_dir.glob("*.png"))
        self.depth_paths = sorted(self.depth_dir.glob("*.npy"))
        self.semantic_paths = sorted(self.semantic_dir.glob("*.npy"))

    def _setup_transforms(self):
        """base->camera transform and the (forward, left, up) re-basing matrix.  Reference: map.py:54-68."""
        pose_info = cfg_get(self.map_config, "pose_info")
        self.base2cam_tf = np.eye(4)
        self.base2cam_tf[:3, :3] = np.array([list(cfg_get(pose_info, "base2cam_rot"))]).reshape((3, 3))
        self.base2cam_tf[1, 3] = cfg_get(pose_info, "camera_height")
        self.base_transform = np.eye(4)
        self.base_transform[0, :3] = list(cfg_get(pose_info, "base_forward_axis"))
        self.base_transform[1, :3] = list(cfg_get(pose_info, "base_left_axis"))
        self.base_transform[2, :3] = list(cfg_get(pose_info, "base_up_axis"))
        return self.base2cam_tf, self.base_transform

    def create_map(self, data_dir):
        return NotImplementedError

    def load_map(self, map_dir: str):
        return NotImplementedError

    def index_map(self, language_desc: str, with_init_cat: bool = True):
        return NotImplementedError

    def generate_obstacle_map(self, h_min: float = 0, h_max: float = 1.5) -> np.ndarray:
        """(gs, gs) bool, True = free.  Reference: map.py:79-95 (note `> 0`: voxel id 0 does not count upstream)."""
        assert self.occupied_ids is not None, "map not loaded"
        from .. import ops
        self.obstacles_map = ops.obstacle_map(self.occupied_ids, self.cs, h_min, h_max)      # avl_obstacle_map
        self.generate_cropped_obstacle_map(self.obstacles_map)
        return self.obstacles_map

    def generate_cropped_obstacle_map(self, obstacle_map: np.ndarray) -> np.ndarray:
        """Reference: map.py:97-104."""
        x_indices, y_indices = np.where(obstacle_map == 0)
        self.rmin, self.rmax = np.min(x_indices), np.max(x_indices)
        self.cmin, self.cmax = np.min(y_indices), np.max(y_indices)
        self.obstacles_cropped = obstacle_map[self.rmin:self.rmax + 1, self.cmin:self.cmax + 1]
        return self.obstacles_cropped

    def generate_rgb_topdown_map(self) -> np.ndarray:
        """Last voxel written per (row, col) wins, like the reference's sequential loop (map.py:106-113)."""
        assert self.grid_rgb is not None, "map not loaded"
        assert self.grid_pos is not None
        from .. import ops
        return ops.rgb_topdown(self.grid_pos, self.grid_rgb, self.gs)                         # avl_rgb_topdown

    def init_categories(self, categories: List[str]) -> np.ndarray:
        return NotImplementedError

    def get_distribution_map(self, name: str, decay_rate: float = 0.1) -> np.ndarray:
        """Abstract upstream (map.py:153-154); VLMap implements it."""
        raise NotImplementedError(f"{type(self).__name__} has no 2-D distribution map")

    def get_predict_mask(self, name: str) -> np.ndarray:
        """Abstract upstream (map.py:156-157); VLMap implements it."""
        raise NotImplementedError(f"{type(self).__name__} has no predicted mask")

    def get_max_pos(self, map_2d: np.ndarray):
        """(row + rmin, col + cmin) of the first maximum of a map over the obstacle crop: np.argmax + np.unravel_index plus the crop
        offset, found on the GPU (ops.product_argmax_2d).  Reference: habitat_lang_robot.py:419-425."""
        from .. import ops
        m = np.asarray(map_2d)
        if m.ndim != 2 or m.size == 0:
            raise ValueError(f"expected a non-empty 2-D map, got shape {m.shape}")
        if m.dtype not in (np.float32, np.float64):
            m = m.astype(np.float64)
        row, col = ops.product_argmax_2d([m], want_heat=False).cell
        return row + self.rmin, col + self.cmin

    def get_obstacle_cropped(self) -> np.ndarray:
        """Reference: map.py:159-160."""
        return self.obstacles_cropped

    def get_customized_obstacle_cropped(self) -> np.ndarray:
        """the map VLMap.customize_obstacle_map left behind.  Reference: map.py:162-163."""
        return self.obstacles_new_cropped

    # ------------------------------------------------------------------------ observed free space (csrc/avl_explore.hip)
    # generate_obstacle_map calls a cell free when no voxel was fused in its height band, which is also true of every cell no camera
    # ever looked at.  The explored map says which cells a sight ray crossed; upstream only has the unused seed of it
    # (mapping_utils.py:403-454 generate_mask).  DESIGN.md 4.14.
    EXPLORED_FILE = "explored.npz"

    def create_explored_map(self, data_dir=None, stride: int = 4, h_min: float = 0, h_max: float = 1.5, batch: int = 16) -> np.ndarray:
        """Carve the sight rays of every depth frame of the scene into self.first_seen (gs, gs) int32 -- the first frame that saw a
        cell inside the height band, -1 = never -- and write <data_dir>/vlmap/explored.npz.  Reads poses.txt and depth/*.npy as the
        builder does: its frame_transforms, cam_calib_mat, min_depth and max_depth.  Frames go up in batches of `batch`, one
        loader thread ahead of the GPU; one ray per stride-th pixel in both directions."""
        from .. import ops
        from ..device import DeviceArray
        from ._frames import batch_ranges, depth_batch, prefetch
        from .vlmap_builder import VLMapBuilder
        if data_dir is not None:
            self._setup_paths(data_dir)
        if not hasattr(self, "data_dir"):
            raise ValueError("create_explored_map: no scene directory (pass data_dir)")
        if int(batch) < 1:
            raise ValueError(f"create_explored_map: batch {batch} < 1")
        builder = VLMapBuilder(self.data_dir, self.map_config, self.pose_path, self.rgb_paths, self.depth_paths, self.base2cam_tf,
                               self.base_transform)
        calib = np.array(list(cfg_get(self.map_config, "cam_calib_mat")), dtype=np.float64).reshape((3, 3))
        poses = np.loadtxt(self.pose_path).reshape((-1, 7))
        transforms = np.stack(builder.frame_transforms(poses)) if len(poses) else np.zeros((0, 4, 4))
        n = min(len(self.depth_paths), len(poses))
        gs, cs = int(self.gs), float(self.cs)
        params = dict(gs=gs, cs=cs, stride=int(stride), h_min=float(h_min), h_max=float(h_max), min_depth=float(builder.min_depth),
                      max_depth=float(builder.max_depth))
        frames = prefetch(lambda lo, hi: (lo, hi, depth_batch(self.depth_paths, lo, hi)), batch_ranges(n, batch), "avl-explore-load")
        first_seen = DeviceArray.from_numpy(np.full((gs, gs), ops.NEVER_SEEN, np.int32))
        try:
            for lo, hi, depth in frames:
                ops.carve_free_space(first_seen, DeviceArray.from_numpy(depth), calib, transforms[lo:hi], np.arange(lo, hi), device=True,
                                     **params)
            self.first_seen = first_seen.numpy()
        finally:
            first_seen.free()
        self.explored_params = dict(params, n_frames=n)
        out_dir = self.data_dir / "vlmap"
        out_dir.mkdir(parents=True, exist_ok=True)
        np.savez_compressed(out_dir / self.EXPLORED_FILE, first_seen=self.first_seen, **self.explored_params)
        return self.first_seen

    def load_explored_map(self, data_dir=None) -> bool:
        """Read <data_dir>/vlmap/explored.npz into self.first_seen / self.explored_params; False (and no explored map) when the file
        does not exist.  A file made for another grid is an error, not a silent crop."""
        path = Path(data_dir if data_dir is not None else self.data_dir) / "vlmap" / self.EXPLORED_FILE
        self.first_seen, self.explored_params = None, None
        if not path.exists():
            return False
        with np.load(path, allow_pickle=False) as z:
            first_seen = np.ascontiguousarray(z["first_seen"], dtype=np.int32)
            params = {k: z[k].item() for k in z.files if k != "first_seen"}
        if first_seen.shape != (self.gs, self.gs) or float(params.get("cs", self.cs)) != float(self.cs):
            raise ValueError(f"{path}: explored map of grid {first_seen.shape}, cell {params.get('cs')} does not belong to this "
                             f"map ({self.gs}, cell {self.cs})")
        self.first_seen, self.explored_params = first_seen, params
        return True

    def _require_explored(self) -> np.ndarray:
        if getattr(self, "first_seen", None) is None:
            raise RuntimeError("no explored map loaded: run create_explored_map (apps.create_map --explored) or load a scene that has "
                               "vlmap/explored.npz")
        return self.first_seen

    def generate_explored_map(self) -> np.ndarray:
        """(gs, gs) bool, True = a sight ray crossed the cell inside the height band"""
        self.explored_map = self._require_explored() >= 0
        return self.explored_map

    def _explored_crop(self) -> np.ndarray:
        explored = self.generate_explored_map()
        if self.obstacles_cropped is None:
            self.generate_obstacle_map()
        return explored[self.rmin:self.rmax + 1, self.cmin:self.cmax + 1]

    def get_explored_cropped(self) -> np.ndarray:
        """the explored map over the obstacle crop (generated on first use)"""
        return self._explored_crop()

    def generate_known_free_map(self, h_min: float = 0, h_max: float = 1.5) -> np.ndarray:
        """(gs, gs) bool, True = free AND observed: generate_obstacle_map(h_min, h_max) & generate_explored_map()"""
        self._require_explored()
        return self.generate_obstacle_map(h_min, h_max) & self.generate_explored_map()

    def get_known_free_cropped(self, customized: bool = False) -> np.ndarray:
        """The obstacle crop (customized: obstacles_new_cropped) AND-ed with the explored crop: the same window, so a Navigator takes
        it as it takes any obstacle map -- and no longer plans through space nobody observed."""
        explored = self._explored_crop()
        base = self.get_customized_obstacle_cropped() if customized else self.get_obstacle_cropped()
        return (np.asarray(base) != 0) & explored

    def get_frontiers(self, min_cells: int = 5):
        """-> (centres (n, 2) int, sizes (n,) int): the frontier of the explored area over the obstacle crop -- explored free cells with an
        unknown 4-neighbour (ops.frontier_mask) -- grouped into 8-connected islands (ops.label_islands) of at least min_cells cells,
        largest first (equal sizes in raster order of their first cell).  A centre is the island's own cell nearest to its centroid
        (the first in raster order among equals), in full-map (row, col): a frontier cell, so a planner can end on it."""
        explored = self._explored_crop()
        free = np.asarray(self.get_obstacle_cropped()) != 0
        return self._frontiers_of(free, explored, min_cells)

    def _frontiers_of(self, free, explored, min_cells: int = 5):
        """get_frontiers on a free map and an explored map of the obstacle crop's shape (host or device masks)"""
        from .. import ops
        mask = ops.frontier_mask(free, explored, device=True)
        with ops.label_islands(mask) as isl:
            labels, areas = np.asarray(isl.labels), isl.table[:, 0].astype(np.int64)
        keep = [k for k in np.argsort(-areas, kind="stable") if areas[k] >= int(min_cells)]
        centres = np.zeros((len(keep), 2), dtype=np.int64)
        for i, k in enumerate(keep):
            cells = np.argwhere(labels == k + 1)
            d2 = np.sum((cells - cells.mean(axis=0)) ** 2, axis=1)
            centres[i] = cells[int(np.argmin(d2))] + (int(self.rmin), int(self.cmin))
        return centres, (areas[keep] if keep else np.zeros((0,), np.int64))

    # ------------------------------------------------------------------------ next-best-view goals (csrc/avl_viewshed.hip)
    # get_frontiers ranks the edge of the explored area by size and plan_to_nearest_frontier walks to its closest cell; neither
    # knows how much unknown space the robot would SEE from a cell.  The viewshed does: per candidate cell the unknown cells of
    # the obstacle crop with a free 2-D sight line within sensor range.  One height band (the explored map's own), cell centres,
    # no field of view other than sums of 45-degree sectors; optimistic by default (unknown cells do not block).  Upstream has
    # no counterpart.  DESIGN.md 4.28.
    def _view_radius(self, max_range: float) -> int:
        from .. import ops
        max_range = float(max_range)
        if not (np.isfinite(max_range) and max_range > 0.0):
            raise ValueError(f"max_range {max_range} (metres; finite and > 0)")
        radius = int(max_range / float(self.cs))
        if radius < 1:
            raise ValueError(f"max_range {max_range} m is less than one cell of {self.cs} m")
        if radius > ops.VIEWSHED_MAX_RADIUS:
            raise ValueError(f"max_range {max_range} m is {radius} cells: the viewshed reaches {ops.VIEWSHED_MAX_RADIUS} cells, "
                             f"{ops.VIEWSHED_MAX_RADIUS * float(self.cs):g} m on this map")
        return radius

    def _view_free(self, customized: bool = False) -> np.ndarray:
        if self.obstacles_cropped is None:
            self.generate_obstacle_map()
        base = self.get_customized_obstacle_cropped() if customized else self.get_obstacle_cropped()
        if base is None:
            raise ValueError("get_exploration_views: no customised obstacle map (call customize_obstacle_map first)")
        return np.asarray(base) != 0

    def _exploration_views(self, free, explored, curr_pos, radius: int, stride: int, opaque_unknown: bool) -> "ExplorationViews":
        """get_exploration_views on a free map and an explored map (host bool arrays over the obstacle crop)"""
        from .. import ops
        stride = int(stride)
        if stride < 1:
            raise ValueError(f"get_exploration_views: stride {stride} < 1")
        rmin, cmin = int(self.rmin), int(self.cmin)
        window = (rmin, cmin, free.shape[0], free.shape[1])
        known = free & explored
        cand = np.zeros(free.shape, dtype=bool)
        cand[::stride, ::stride] = known[::stride, ::stride]
        centres = self._frontiers_of(free, explored)[0]
        cand[centres[:, 0] - rmin, centres[:, 1] - cmin] = True
        field, planes = None, None
        if curr_pos is not None:
            cell = np.asarray(curr_pos, dtype=np.float64).reshape(2).astype(np.int64) - (rmin, cmin)
            if not (0 <= cell[0] < free.shape[0] and 0 <= cell[1] < free.shape[1]):
                raise ValueError(f"get_exploration_views: {list(curr_pos)} lies outside the obstacle crop [{self.rmin}:{self.rmax + 1}, "
                                 f"{self.cmin}:{self.cmax + 1}]")
            field = ops.travel_field(known, cell.reshape(1, 2))
            planes = field.planes()
            cand &= planes[0] >= 0
        local = np.argwhere(cand)                                           # raster order
        if planes is None:
            distance = np.full((len(local), 2), -1, np.int32)
        else:
            distance = np.stack([planes[0][local[:, 0], local[:, 1]], planes[1][local[:, 0], local[:, 1]]], axis=1)
        gain = ops.viewshed_gain(free, explored, local.astype(np.int32), radius, opaque_unknown)
        return ExplorationViews(local + (rmin, cmin), gain, distance, window, radius, field)

    def get_exploration_views(self, curr_pos=None, max_range: float = 3.0, stride: int = 4, customized: bool = False,
                              opaque_unknown: bool = False) -> "ExplorationViews":
        """Which cells are worth going to?  The candidates are the known-free cells of the obstacle crop (get_known_free_cropped;
        customized: of the customised crop) whose crop row and column are multiples of `stride`, plus the centres of
        get_frontiers(), in raster order; with curr_pos (full-map (row, col), inside the crop) only those the robot can reach --
        one travel field from its cell over the known-free map (get_travel_field([curr_pos], known_free=True)), whose pairs are
        kept as the travel distance.  One ops.viewshed_gain call over the crop tells for each how many unknown cells within
        radius = int(max_range / cs) cells it would see; a max_range of less than one cell or of more than
        ops.VIEWSHED_MAX_RADIUS cells raises ValueError.  opaque_unknown: unknown cells block the view (the conservative
        variant).  -> ExplorationViews."""
        radius = self._view_radius(max_range)
        free = self._view_free(customized)
        return self._exploration_views(free, self._explored_crop(), curr_pos, radius, stride, bool(opaque_unknown))

    def _view_path(self, views: "ExplorationViews", k: int, curr_pos, navigator):
        """the path from curr_pos to candidate k: the navigator's, or the travel field's own walk in full-map cells"""
        pos = [int(views.cells[k, 0]), int(views.cells[k, 1])]
        if navigator is not None:
            return pos, navigator.plan_to_next_best_view(curr_pos, views, among=[k])[1]
        if views.field is None:
            return pos, [curr_pos, pos]
        r0, c0 = views.window[:2]
        walk = views.field.descend((pos[0] - r0, pos[1] - c0))
        return pos, [[r + r0, c + c0] for r, c in reversed(walk)]

    def get_next_best_view(self, curr_pos: List[float], navigator=None, min_fraction: float = 0.5, **kw):
        """-> (pos, heading_octant, gain, path): among the candidates of get_exploration_views(curr_pos, **kw) that gain at least
        max(1, ceil(min_fraction * the best cell's gain)) unknown cells (ExplorationViews.select) the one with the shortest travel
        distance from curr_pos (the field's exact comparison of pairs, the first in raster order among equals), the first of its
        best two neighbouring sectors, its gain, and the path to it: Navigator.plan_to_next_best_view's with a navigator, else the
        cells of the travel field's shortest walk.  (curr_pos, None, 0, [curr_pos]) when no reachable candidate gains anything:
        the map is fully explored."""
        views = self.get_exploration_views(curr_pos, **kw)
        k = views.nearest(min_fraction)
        if k is None:
            return curr_pos, None, 0, [curr_pos]
        pos, path = self._view_path(views, k, curr_pos, navigator)
        return pos, int(views.heading[k]), int(views.total[k]), path

    def plan_exploration(self, curr_pos: List[float], k: int = 5, navigator=None, min_fraction: float = 0.5, max_range: float = 3.0,
                         stride: int = 4, customized: bool = False, opaque_unknown: bool = False):
        """A greedy tour of at most k views -> [(pos, heading_octant, gain, path), ...]: take the next best view
        (get_next_best_view's choice), OR what it sees (ops.viewshed_seen) into a device copy of the explored crop, and choose
        again from there -- candidates, frontier centres, travel field and gains all on the map as it would then be known -- until
        k views are chosen or no candidate gains anything.  Every gain is the one at the time of choice.  A navigator plans the
        first leg only (its graph is of the map as it is known now); the later legs are the travel field's walks over the map as it
        would be known by then.  self.first_seen and the file on disk are not modified."""
        from .. import ops
        from ..device import DeviceArray
        if int(k) < 0:
            raise ValueError(f"plan_exploration: k {k} < 0")
        radius = self._view_radius(max_range)
        free = self._view_free(customized)
        explored = DeviceArray.from_numpy(np.ascontiguousarray(self._explored_crop()).view(np.uint8))
        rmin, cmin = int(self.rmin), int(self.cmin)
        tour, pos = [], curr_pos
        try:
            for _ in range(int(k)):
                views = self._exploration_views(free, explored.numpy() != 0, pos, radius, stride, bool(opaque_unknown))
                i = views.nearest(min_fraction)
                if i is None:
                    break
                cell, path = self._view_path(views, i, pos, navigator if not tour else None)
                tour.append((cell, int(views.heading[i]), int(views.total[i]), path))
                eye = np.array([[cell[0] - rmin, cell[1] - cmin]], np.int32)
                ops.viewshed_seen(free, explored, eye, radius, bool(opaque_unknown), out=explored, device=True)
                pos = cell
        finally:
            explored.free()
        return tour

    # ------------------------------------------------------------------------ stale voxels (csrc/avl_audit.hip)
    # The builder only adds voxels: what a later visit saw through stays in the map.  The audit walks the sight rays of the frames
    # through the voxel list in 3-D and records, per voxel, the last frame that hit it and the rays of later frames that passed
    # through it.  Upstream has no counterpart (its maps are static).  DESIGN.md 4.21.
    VISIBILITY_FILE = "visibility.npz"

    def _own_first_pose(self):
        """the first pose of the scene the map was built from, which defines the map's frame; None for a map without a scene"""
        own = getattr(self, "pose_path", None)
        if own is None or not Path(own).exists():
            return None
        poses = np.loadtxt(own).reshape((-1, 7))
        return poses[0] if len(poses) else None

    def _audit_frames(self, data_dir, first_pose=None):
        """(depth paths, (n, 4, 4) transforms, min_depth, max_depth, the directory's first pose) of one scene directory, read as
        create_explored_map reads its own.  The map's frame is the first pose of the scene it was built from: first_pose, when
        given, takes the place of this directory's own first pose in the builder's frame_transforms, so that a revisit (whose
        poses.txt is in the same world frame) lands in the map's frame."""
        from .vlmap_builder import VLMapBuilder
        data_dir = Path(data_dir)
        depth_paths = sorted((data_dir / "depth").glob("*.npy"))
        pose_path = data_dir / "poses.txt"
        builder = VLMapBuilder(data_dir, self.map_config, pose_path, sorted((data_dir / "rgb").glob("*.png")), depth_paths,
                               self.base2cam_tf, self.base_transform)
        poses = np.loadtxt(pose_path).reshape((-1, 7))
        own_first = poses[0].copy() if len(poses) else None
        if len(poses) and first_pose is not None:
            transforms = np.stack(builder.frame_transforms(np.concatenate([np.reshape(first_pose, (1, 7)), poses])))[1:]
        else:
            transforms = np.stack(builder.frame_transforms(poses)) if len(poses) else np.zeros((0, 4, 4))
        n = min(len(depth_paths), len(poses))
        return depth_paths[:n], transforms[:n], float(builder.min_depth), float(builder.max_depth), own_first

    def transform_from(self, other_data_dir, registration=None) -> np.ndarray:
        """(4, 4) float64: the transform from the base frame of a map built from `other_data_dir` on its own into this map's base
        frame, for VLMap.resample and VLMap.fuse.  Host only.  Both frames are defined by _audit_frames: with own = the directory's
        camera -> map transforms in its own frame (its first pose) and here = the same frames in this map's frame (this map's
        first pose), S = here[0] @ inv(own[0]) satisfies S @ own[i] == here[i] for every frame.  registration: a joint
        Registration of that directory against this map (register_frames); its correction is left-multiplied.  A map without a
        scene of its own shares the directory's frame: the identity."""
        own = self._audit_frames(other_data_dir)[1]
        here = self._audit_frames(other_data_dir, self._own_first_pose())[1]
        if len(own) == 0:
            raise ValueError(f"transform_from: {other_data_dir} holds no posed frame")
        S = np.asarray(here[0], dtype=np.float64) @ np.linalg.inv(np.asarray(own[0], dtype=np.float64))
        if registration is not None:
            S = np.asarray(registration.correction, dtype=np.float64) @ S
        S[3] = (0.0, 0.0, 0.0, 1.0)
        return S

    def audit_visibility(self, data_dirs=None, stride: int = 4, end_margin: int = 2, batch: int = 16, corrections=None) -> "VisibilityAudit":
        """Audit the map's voxels against the depth frames of `data_dirs` (default: the map's own scene; a revisit is a second
        directory; frame ids run on consecutively across directories).  Pass A folds every frame's hits into last_hit (N,) int32,
        pass B counts in through (N,) uint32 the rays of frames AFTER a voxel's last hit that passed through its cell
        (ops.audit_rays with after = last_hit).  Reads poses.txt and depth/*.npy as create_explored_map does, in batches of
        `batch` frames, one loader thread ahead of the GPU.  corrections: None, or a sequence with one entry per directory, each
        None or a 4 x 4 matrix that is left-multiplied onto that directory's transforms (register_frames's correction of a
        recording that was not made in the map's frame).  The result is kept as self.visibility and written to
        <data_dir>/vlmap/visibility.npz."""
        from .. import ops
        from ..device import DeviceArray
        from ._frames import batch_ranges, depth_batch, prefetch
        if self.grid_pos is None or self.occupied_ids is None:
            raise ValueError("audit_visibility: no map loaded")
        if int(batch) < 1:
            raise ValueError(f"audit_visibility: batch {batch} < 1")
        if int(stride) < 1 or int(end_margin) < 0:
            raise ValueError(f"audit_visibility: stride {stride} (>= 1), end_margin {end_margin} (>= 0)")
        if data_dirs is None:
            if not hasattr(self, "data_dir"):
                raise ValueError("audit_visibility: no scene directory (pass data_dirs)")
            data_dirs = [self.data_dir]
        elif isinstance(data_dirs, (str, Path)):
            data_dirs = [data_dirs]
        calib = np.array(list(cfg_get(self.map_config, "cam_calib_mat")), dtype=np.float64).reshape((3, 3))
        first_pose = self._own_first_pose()             # the map's frame: its own scene's when it has one, else the first directory's
        if corrections is not None:
            corrections = [None if c is None else np.asarray(c, dtype=np.float64) for c in corrections]
            if len(corrections) != len(data_dirs) or any(c is not None and c.shape != (4, 4) for c in corrections):
                raise ValueError(f"audit_visibility: corrections must hold one 4 x 4 matrix or None for each of the {len(data_dirs)} directories")
        scenes = []
        for i, d in enumerate(data_dirs):
            scene = self._audit_frames(d, first_pose)
            first_pose = scene[4] if first_pose is None else first_pose
            if corrections is not None and corrections[i] is not None and len(scene[1]):
                scene = (scene[0], corrections[i] @ scene[1]) + scene[2:]
            scenes.append(scene[:4])
        counts = [len(s[0]) for s in scenes]
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        gs, cs, vh = int(self.gs), float(self.cs), int(np.asarray(self.occupied_ids).shape[2])
        N = len(self.grid_pos)

        ranges = [(s, lo, hi) for s, count in enumerate(counts) for lo, hi in batch_ranges(count, batch)]      # (no batch spans two directories)

        def load(s, lo, hi):
            paths, transforms, mn, mx = scenes[s]
            return depth_batch(paths, lo, hi), transforms[lo:hi], np.arange(starts[s] + lo, starts[s] + hi), mn, mx

        def run_pass(index, **outputs):
            for depth, transforms, ids, mn, mx in prefetch(load, ranges, "avl-audit-load"):
                ops.audit_rays(index, DeviceArray.from_numpy(depth), calib, transforms, ids, cs, stride=int(stride), min_depth=mn,
                               max_depth=mx, end_margin=int(end_margin), **outputs)

        last_hit = DeviceArray.from_numpy(np.full((N,), ops.NEVER_HIT, np.int32))
        through = DeviceArray((N,), np.uint32).zero_()
        try:
            with ops.cell_index(np.ascontiguousarray(self.grid_pos, dtype=np.int32), gs, vh) as index:
                run_pass(index, last_hit=last_hit)                                  # pass A
                run_pass(index, through=through, after=last_hit)                    # pass B
            params = dict(gs=gs, cs=cs, vh=vh, stride=int(stride), end_margin=int(end_margin), n_frames=int(starts[-1]))
            audit = VisibilityAudit(last_hit.numpy(), through.numpy(), params, counts)
        finally:
            last_hit.free()
            through.free()
        self.visibility = audit
        out_dir = Path(getattr(self, "data_dir", data_dirs[0])) / "vlmap"
        out_dir.mkdir(parents=True, exist_ok=True)
        audit.save(out_dir / self.VISIBILITY_FILE)
        return audit

    def load_visibility(self, data_dir=None) -> bool:
        """Read <data_dir>/vlmap/visibility.npz into self.visibility; False (and no audit) when the file does not exist or was made
        for a map of another voxel count -- a pruned or rebuilt map simply has no audit yet."""
        self.visibility = None
        path = Path(data_dir if data_dir is not None else self.data_dir) / "vlmap" / self.VISIBILITY_FILE
        if not path.exists() or self.grid_pos is None:
            return False
        audit = VisibilityAudit.load(path)
        if audit.N != len(self.grid_pos):
            return False
        self.visibility = audit
        return True

    # ------------------------------------------------------------------------ registration (csrc/avl_match.hip)
    # The audit, the explored map and the GT vote take a recording's poses as they come.  A second recording of the same rooms starts
    # from another odometry origin and drifts: a few centimetres or one degree move every sight ray by a cell or more at range.
    # register_frames slides the recording's depth points over the map's own voxels, every planar rotation of a table and every
    # whole-cell shift of a window, and returns the correction under which most points land on occupied cells.  Upstream has no
    # counterpart.  DESIGN.md 4.23.
    def register_frames(self, data_dir, max_angle_deg: float = 10.0, angle_step_deg: float = 0.5, radius_m: float = 0.5, joint: bool = True,
                        max_frames: int = 32, stride: int = 4, h_band_m=(0.1, None), batch: int = 16) -> "Registration":
        """Register the depth frames of `data_dir` to the map (ops.match_frames): read the directory as audit_visibility reads a
        revisit -- its poses.txt taken relative to the map's first pose -- and search rotations of -max_angle_deg .. max_angle_deg
        in steps of angle_step_deg about z and shifts of up to radius_m in whole cells.  joint=True: one correction for the
        recording, from up to max_frames evenly spaced frames in one call, rotated about the first frame's origin.  joint=False: a
        correction per frame, about the frame's own origin, every frame of the directory in batches of `batch`.  Only points whose
        height lies in h_band_m (metres, inclusive in cells; None = the top of the grid) take part: the default leaves the floor
        out.  The search is planar (no pitch, roll or height), a shift is a whole number of cells -- the translation is accurate to
        one cell -- and only occupied cells count.  Writes nothing."""
        from .. import ops
        from ._frames import batch_ranges, depth_batch
        if self.grid_pos is None or self.occupied_ids is None:
            raise ValueError("register_frames: no map loaded")
        if int(batch) < 1 or int(max_frames) < 1 or int(stride) < 1:
            raise ValueError(f"register_frames: batch {batch}, max_frames {max_frames}, stride {stride} (all >= 1)")
        gs, cs, vh = int(self.gs), float(self.cs), int(np.asarray(self.occupied_ids).shape[2])
        radius = int(round(float(radius_m) / cs))
        if not 0 <= radius <= ops.MATCH_MAX_RADIUS:
            raise ValueError(f"register_frames: radius_m {radius_m} is {radius} cells (0 .. {ops.MATCH_MAX_RADIUS})")
        angles = ops.match_angles(max_angle_deg, angle_step_deg)
        k0 = len(angles) // 2
        h_lo = 0 if h_band_m[0] is None else min(max(int(float(h_band_m[0]) / cs), 0), vh - 1)
        h_hi = vh - 1 if h_band_m[1] is None else min(max(int(float(h_band_m[1]) / cs), 0), vh - 1)
        if h_lo > h_hi:
            raise ValueError(f"register_frames: height band {tuple(h_band_m)} m is empty")
        calib = np.array(list(cfg_get(self.map_config, "cam_calib_mat")), dtype=np.float64).reshape((3, 3))
        paths, transforms, mn, mx, _ = self._audit_frames(data_dir, self._own_first_pose())
        n = len(paths)
        if n == 0:
            raise ValueError(f"register_frames: no frames under {data_dir}")
        kw = dict(stride=int(stride), min_depth=mn, max_depth=mx, h_band=(h_lo, h_hi), k0=k0)
        with ops.cell_index(np.ascontiguousarray(self.grid_pos, dtype=np.int32), gs, vh) as index:
            if joint:
                frames = np.unique(np.round(np.linspace(0, n - 1, min(n, int(max_frames)))).astype(np.int64))
                pivots = transforms[frames[0], :2, 3][None].copy()
                depth = np.stack([depth_batch(paths, int(i), int(i) + 1)[0] for i in frames])
                res = ops.match_frames(index, depth, calib, transforms[frames], cs, angles, radius, joint=True, pivot=pivots[0], **kw)
                best, valid = np.asarray(res.best), np.asarray(res.valid)
            else:
                frames = np.arange(n, dtype=np.int64)
                pivots = transforms[:, :2, 3].copy()
                parts = [ops.match_frames(index, depth_batch(paths, lo, hi), calib, transforms[lo:hi], cs, angles, radius, joint=False, **kw)
                         for lo, hi in batch_ranges(n, batch)]
                best = np.concatenate([np.asarray(r.best) for r in parts])
                valid = np.concatenate([np.asarray(r.valid) for r in parts])
        corrections = ops.MatchResult(None, best, valid, radius).corrections(cs, angles, pivots)
        return Registration(corrections, (corrections if not joint else corrections[:1]) @ transforms, best, valid, angles, frames, pivots,
                            bool(joint), dict(gs=gs, cs=cs, vh=vh, radius=radius, stride=int(stride), h_band=(h_lo, h_hi),
                                              max_angle_deg=float(max_angle_deg), angle_step_deg=float(angle_step_deg)))

    # ------------------------------------------------------------------------ viewpoints (csrc/avl_sight.hip)
    # get_nearest_reachable_pos ends on a contour point, which may lie under the table or behind a half-height partition: whether an
    # object can be SEEN from a cell is a 3-D property of the voxels.  A sight line runs from the eye's cell to a target voxel's cell
    # (that direction: the walk is not symmetric) between cell centres; the robot's field of view and heading are not modelled.
    # Upstream has no counterpart.  DESIGN.md 4.22.
    def get_viewpoints(self, target, eye_height: float = None, max_range: float = 3.0, max_targets: int = 1024, free=None,
                       customized: bool = False, end_margin: int = 0) -> "Viewpoints":
        """From which free cells can `target` be seen?  target: a category name (self.index_map(name)) or an (N,) bool / uint8 voxel
        mask (index_map's, get_quantile_predict_mask's, an Instance3D's).  The targets are the mask's rows in row order, every
        ceil(n / max_targets)-th of them when there are more than max_targets; the mask itself is `transparent`, so an object does not
        hide itself.  The candidate eyes are the True cells of `free` -- a bool array over the obstacle crop, default
        get_obstacle_cropped() != 0 (customized: the customized crop), e.g. get_known_free_cropped() -- inside the 2-D bounding box
        of the target cells grown by ceil(max_range / cs) cells, at height cell min(max(int(eye_height / cs), 0), vh - 1)
        (eye_height in metres, default the map config's pose_info.camera_height).  The exact 3-D range, max_range / cs cells,
        is applied on the device.  One ops.cell_index and one ops.visible_counts call."""
        from .. import ops
        if self.grid_pos is None or self.occupied_ids is None:
            raise ValueError("get_viewpoints: no map loaded")
        max_range = float(max_range)
        if not (np.isfinite(max_range) and max_range > 0.0):
            raise ValueError(f"get_viewpoints: max_range {max_range} (metres; finite and > 0)")
        max_targets = int(max_targets)
        if not 1 <= max_targets <= ops.LOS_MAX_TARGETS:
            raise ValueError(f"get_viewpoints: max_targets {max_targets} (1 .. {ops.LOS_MAX_TARGETS})")
        if int(end_margin) < 0:
            raise ValueError(f"get_viewpoints: end_margin {end_margin} < 0")
        gs, cs, vh = int(self.gs), float(self.cs), int(np.asarray(self.occupied_ids).shape[2])
        N = len(self.grid_pos)
        mask = self.index_map(target) if isinstance(target, str) else target
        mask = np.asarray(mask)
        if mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)) or mask.shape != (N,):
            raise ValueError(f"get_viewpoints: the target mask must be ({N},) bool or uint8, got {mask.dtype} {mask.shape}")
        mask = mask != 0
        if eye_height is None:
            eye_height = cfg_get(cfg_get(self.map_config, "pose_info"), "camera_height")
        eye_h = min(max(int(float(eye_height) / cs), 0), vh - 1)
        if self.obstacles_cropped is None:
            self.generate_obstacle_map()
        base = self.get_customized_obstacle_cropped() if customized else self.get_obstacle_cropped()
        free = np.asarray(base) != 0 if free is None else np.asarray(free)
        if free.dtype != np.dtype(bool) or free.shape != np.asarray(base).shape:
            raise ValueError(f"get_viewpoints: free must be a bool array over the obstacle crop {np.asarray(base).shape}, got "
                             f"{free.dtype} {free.shape}")
        rmin, cmin = int(self.rmin), int(self.cmin)
        window = (rmin, cmin, free.shape[0], free.shape[1])
        rows = np.flatnonzero(mask)
        if len(rows) > max_targets:
            rows = rows[::-(-len(rows) // max_targets)]
        targets = np.ascontiguousarray(np.asarray(self.grid_pos)[rows], dtype=np.int32).reshape(-1, 3)
        empty = Viewpoints(np.zeros((0, 2)), np.zeros(0), np.zeros(0), len(rows), eye_h, window)
        if len(rows) == 0:
            return empty
        grow = int(np.ceil(max_range / cs))
        r0 = max(int(targets[:, 0].min()) - grow, rmin)
        r1 = min(int(targets[:, 0].max()) + grow, rmin + free.shape[0] - 1)
        c0 = max(int(targets[:, 1].min()) - grow, cmin)
        c1 = min(int(targets[:, 1].max()) + grow, cmin + free.shape[1] - 1)
        if r0 > r1 or c0 > c1:
            return empty
        cells = np.argwhere(free[r0 - rmin:r1 - rmin + 1, c0 - cmin:c1 - cmin + 1]) + (r0, c0)      # raster order
        if len(cells) == 0:
            return empty
        eyes = np.concatenate([cells, np.full((len(cells), 1), eye_h)], axis=1).astype(np.int32)
        with ops.cell_index(np.ascontiguousarray(self.grid_pos, dtype=np.int32), gs, vh) as index:
            visible, first = ops.visible_counts(index, eyes, targets, transparent=mask.astype(np.uint8), end_margin=int(end_margin),
                                                max_range=max_range / cs)
        return Viewpoints(cells, visible, first, len(rows), eye_h, window)

    def get_viewpoint_pos(self, curr_pos: List[float], target, navigator=None, min_fraction: float = 0.5, **kw):
        """-> (pos, path): a cell `target` can be seen from (get_viewpoints(target, **kw)), among the cells that see at least
        max(1, ceil(min_fraction * the best cell's count)) of its voxels (Viewpoints.select): with a navigator the one with the
        shortest TRAVEL distance from curr_pos and the path to it (Navigator.plan_to_viewpoint; NoPathError when none can be
        reached), without one the nearest in the plane (the first in raster order among equals) and the path [curr_pos, pos].
        (curr_pos, [curr_pos]) when nothing is visible from anywhere, as get_nearest_reachable_pos without islands.  A Viewpoints
        that get_viewpoints has already returned may be passed as `target`."""
        vp = target if isinstance(target, Viewpoints) else self.get_viewpoints(target, **kw)
        keep = vp.select(min_fraction)
        if len(keep) == 0:
            return curr_pos, [curr_pos]
        if navigator is not None:
            k, path = navigator.plan_to_viewpoint(curr_pos, vp, min_fraction)
            return [int(vp.cells[k, 0]), int(vp.cells[k, 1])], path
        cand = vp.cells[keep]
        d2 = np.sum((cand.astype(np.float64) - np.asarray(curr_pos, dtype=np.float64).reshape(1, 2)) ** 2, axis=1)
        pos = [int(v) for v in cand[int(np.argmin(d2))]]
        return pos, [curr_pos, pos]

    # ------------------------------------------------------------------------ travel-distance fields (csrc/avl_travel.hip)
    # "near" that goes around walls: per free cell of a crop the length of the shortest 8-connected walk from the nearest source
    # that stays on free cells and cuts no corner (the 8-neighbour chamfer metric, not the Navigator's visibility-graph length).
    # Upstream has no counterpart.  DESIGN.md 4.26.
    def _travel_free(self, customized: bool = False, known_free: bool = False) -> np.ndarray:
        """the (h, w) bool free map a travel field runs on: the obstacle crop, the customised one, or either AND-ed with the
        explored crop"""
        if self.obstacles_cropped is None:
            self.generate_obstacle_map()
        if known_free:
            return self.get_known_free_cropped(customized)
        base = self.get_customized_obstacle_cropped() if customized else self.get_obstacle_cropped()
        if base is None:
            raise ValueError("get_travel_field: no customised obstacle map (call customize_obstacle_map first)")
        return np.asarray(base) != 0

    def get_travel_field(self, sources, customized: bool = False, known_free: bool = False, device: bool = False):
        """ops.travel_field over the obstacle crop (customized: the customised crop; known_free: get_known_free_cropped).
        sources: (M, 2) full-map (row, col) points -- their int() cells, which must lie inside the crop -- or a mask of the crop's
        shape (nonzero = source; a source may lie on an obstacle cell, as the cells of a sofa do).  -> ops.TravelField over the
        crop: cell (r, c) of its planes is full-map cell (r + rmin, c + cmin)."""
        from .. import ops
        free = self._travel_free(customized, known_free)
        src = sources if ops._is_dev(sources) else np.asarray(sources)
        if not ops._is_dev(src) and src.shape != free.shape:
            pts = np.asarray(src, dtype=np.float64).reshape(-1, 2)
            cells = pts.astype(np.int64) - np.array([int(self.rmin), int(self.cmin)])
            if len(cells) and (cells.min() < 0 or cells[:, 0].max() >= free.shape[0] or cells[:, 1].max() >= free.shape[1]):
                raise ValueError(f"get_travel_field: a source lies outside the obstacle crop [{self.rmin}:{self.rmax + 1}, "
                                 f"{self.cmin}:{self.cmax + 1}]")
            src = cells
        return ops.travel_field(free, src, device=device)

    def get_reachable_cropped(self, curr_pos: List[float], customized: bool = False, known_free: bool = False) -> np.ndarray:
        """(h, w) bool over the obstacle crop: the cells the robot can walk to from curr_pos (full-map (row, col)), its own cell
        included -- even when that cell is an obstacle, from which it may step onto a free neighbour"""
        return self.get_travel_field([curr_pos], customized, known_free).reachable()

    # ------------------------------------------------------------------------ many travel fields in one batch (csrc/avl_travel_many.hip)
    # K fields on one free map in one call, the distances between sets of cells read from them, and the order in which to visit a
    # handful of goals.  Upstream has no counterpart.  DESIGN.md 4.30.
    def _travel_sets(self, sets, shape, what: str):
        """[set, ...] -> [[(row, col), ...], ...] in crop cells: a set is a list of full-map (row, col) points -- their int() cells,
        which must lie inside the crop -- or a mask of the crop's shape (its nonzero cells in raster order)"""
        out = []
        for k, s in enumerate(sets):
            s = np.asarray(s)
            if s.shape == tuple(shape):
                cells = np.argwhere(s != 0)
            else:
                cells = np.asarray(s, dtype=np.float64).reshape(-1, 2).astype(np.int64) - np.array([int(self.rmin), int(self.cmin)])
                if len(cells) and (cells.min() < 0 or cells[:, 0].max() >= shape[0] or cells[:, 1].max() >= shape[1]):
                    raise ValueError(f"{what}: a cell of set {k} lies outside the obstacle crop [{self.rmin}:{self.rmax + 1}, "
                                     f"{self.cmin}:{self.cmax + 1}]")
            if len(cells) == 0:
                raise ValueError(f"{what}: set {k} is empty")
            out.append([(int(r), int(c)) for r, c in cells])
        if not out:
            raise ValueError(f"{what}: no set")
        return out

    @staticmethod
    def _sets_csr(sets):
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
        return offsets, np.array([c for s in sets for c in s], dtype=np.int32).reshape(-1, 2)

    def get_travel_fields(self, sets, customized: bool = False, known_free: bool = False, device: bool = False):
        """ops.travel_fields over the obstacle crop, one field per set, in one batch (customized / known_free / device as
        get_travel_field).  A set is a list of full-map (row, col) points -- their int() cells, which must lie inside the crop -- or
        a mask of the crop's shape; its cells may be obstacle cells.  -> ops.TravelFields over the crop: field k's planes are
        get_travel_field(sets[k])'s, byte for byte."""
        from .. import ops
        free = self._travel_free(customized, known_free)
        offsets, cells = self._sets_csr(self._travel_sets(sets, free.shape, "get_travel_fields"))
        return ops.travel_fields(free, offsets, cells, device=device)

    def get_travel_matrix(self, sets, customized: bool = False, known_free: bool = False):
        """-> ops.TravelArrivals, (K, K): how far it is to walk from every set to every other one (get_travel_fields over the sets,
        then ops.travel_arrivals at the same sets).  Entry [k, j] is the pair (a, b) of the shortest walk that leaves set k and
        arrives at set j, a + b sqrt(2) cells; sets on obstacle cells are left and arrived at by one step off / onto them, so the
        matrix is symmetric; (0, 0) where two sets share a cell, -1 where no walk connects them.  cell[k, j] indexes the
        concatenated cells of the sets."""
        from .. import ops
        free = self._travel_free(customized, known_free)
        offsets, cells = self._sets_csr(self._travel_sets(sets, free.shape, "get_travel_matrix"))
        return ops.travel_arrivals(ops.travel_fields(free, offsets, cells, device=True), offsets, cells)

    def plan_tour(self, start, goals, closed: bool = False, customized: bool = False, known_free: bool = False):
        """The order in which to visit `goals` from `start`, and the walks.  start: a full-map (row, col); goals: 1 to
        tour.TOUR_MAX_GOALS sets as get_travel_fields takes them.  One ops.travel_fields call over [start] + goals and one
        ops.travel_arrivals give the matrix of set-to-set distances; the order is an exact Held-Karp on its integer pairs
        (tour.held_karp: sums compared like the kernel compares pairs, ties to the lexicographically smallest order); closed=True
        also returns to the start.  Goals no walk from the start reaches are left out and listed in Tour.skipped.

        The order is optimal for the set-to-set matrix.  The legs are then driven: leg i is fields.field(goal).descend(cell) from
        the cell the last leg ended on, trimmed to its last free cell.  The driven length can exceed the matrix length, because a
        set is entered at one cell and left from there, while the matrix lets every leg leave from the set's best cell.
        -> tour.Tour with full-map cells."""
        from .. import ops
        from . import tour as T
        goals = list(goals)
        if not 1 <= len(goals) <= T.TOUR_MAX_GOALS:
            raise ValueError(f"plan_tour: 1 to {T.TOUR_MAX_GOALS} goals, got {len(goals)}")
        free = self._travel_free(customized, known_free)
        sets = self._travel_sets([[start]] + goals, free.shape, "plan_tour")
        offsets, cells = self._sets_csr(sets)
        fields = ops.travel_fields(free, offsets, cells, device=True)
        arr = ops.travel_arrivals(fields, offsets, cells)
        order, pair, skipped = T.held_karp(arr.a, arr.b, closed)
        fields.planes()                                  # one copy for all legs
        at, legs, driven = sets[0][0], [], []
        for g in order + ([0] if closed and order else []):
            walk = T.drive_leg(fields.field(g), free, at, ops.TRAVEL_NEIGHBOURS)
            at = walk[-1]
            driven.append(T.step_counts(walk))
            legs.append([(r + int(self.rmin), c + int(self.cmin)) for r, c in walk])
        return T.Tour([g - 1 for g in order], [g - 1 for g in skipped], pair, legs, driven, closed)

    # ------------------------------------------------------------------------ costmaps and cost-aware paths (csrc/avl_costfield.hip)
    # A price per cell of the obstacle crop -- lethal within the robot's radius of an obstacle, decaying with the clearance out to
    # the inflation radius, plus a penalty around anything to keep off -- and the cheapest 8-connected walk under those prices.
    # Narrow doors get expensive instead of closed (upstream's Map._dilate_map closes them).  DESIGN.md 4.29.
    def _avoid_distance(self, what):
        """the distance plane of one `avoid` entry: per cell of the crop the distance to the nearest cell of the mask, on the
        device; None for an empty mask.  A plain Map knows no names (VLMap resolves them)."""
        from .. import ops
        if isinstance(what, str):
            raise ValueError(f"get_costmap: avoiding {what!r} by name needs a VLMap with categories; pass a mask of the crop's shape")
        shape = tuple(np.asarray(self.obstacles_cropped).shape)
        if ops._image_shape(what) != shape:
            raise ValueError(f"get_costmap: an avoid mask is {ops._image_shape(what)}, the obstacle crop {shape}")
        return ops.distance_to_mask(what)

    def get_costmap(self, robot_radius: float = 0.15, inflation_radius: float = 0.5, cost_scaling: float = 5.0, avoid=(),
                    customized: bool = False, known_free: bool = False, device: bool = False, peak: int = 100):
        """The (h, w) uint8 costmap of the obstacle crop (customized / known_free as get_travel_field), the price of entering each
        cell (ops.build_costmap): 0 = impassable, else 1 .. 254.  The inflation layer prices the clearance d, the distance to the
        nearest obstacle cell of the crop (ops.distance_transform_edt of the free map): lethal where d < robot_radius, else
        floor(peak * exp(-cost_scaling * (d - robot_radius))) out to inflation_radius, 0 beyond; radii in metres, cost_scaling
        per metre, all converted with cs.  avoid: a list of (mask_or_name, radius_m, penalty[, lethal]) -- a crop-shaped mask
        (host or device) or, on a VLMap, a category name; each adds floor(penalty * (1 - distance / radius_m)) within radius_m of
        the mask's cells, the penalty itself on them, and lethal=True makes those cells impassable.  An empty mask adds nothing.
        A map without any obstacle cell has no inflation layer."""
        from .. import ops
        free = self._travel_free(customized, known_free)
        cs = float(self.cs)
        layers = []
        try:
            clearance = ops.distance_transform_edt(free, device=True)
        except ValueError:                              # no obstacle cell to measure to: nothing to inflate
            clearance = None
        if clearance is not None:
            layers.append((clearance, ops.inflation_table(robot_radius / cs, inflation_radius / cs, cost_scaling * cs, peak)))
        for entry in avoid:
            if not 3 <= len(entry) <= 4:
                raise ValueError(f"get_costmap: an avoid entry is (mask_or_name, radius_m, penalty[, lethal]), got {entry!r}")
            table = ops.penalty_table(float(entry[1]) / cs, entry[2], bool(entry[3]) if len(entry) == 4 else False)
            plane = self._avoid_distance(entry[0])
            if plane is not None:
                layers.append((plane, table))
        return ops.build_costmap(free, layers, device=device)

    def _cost_inputs(self, costmap, costmap_kw, device):
        """(the free map, the costmap) of get_cost_field and plan_cost_path: a costmap that is passed in is taken as it is, and then
        only customized / known_free, which choose the free map, may accompany it"""
        free = self._travel_free(bool(costmap_kw.get("customized", False)), bool(costmap_kw.get("known_free", False)))
        if costmap is None:
            return free, self.get_costmap(**dict(costmap_kw, device=device))
        extra = sorted(set(costmap_kw) - {"customized", "known_free"})
        if extra:
            raise ValueError(f"a costmap was passed: {', '.join(extra)} would be ignored")
        return free, costmap

    def get_cost_field(self, sources, costmap=None, **costmap_kw):
        """ops.cost_field over the obstacle crop under `costmap` (default: get_costmap(**costmap_kw)): the cheapest walk from the
        nearest source to every cell.  sources as get_travel_field: (M, 2) full-map (row, col) points or a crop-shaped mask.
        customized / known_free in costmap_kw choose the free map also when a costmap is passed.  -> ops.CostField over the crop."""
        from .. import ops
        free, costmap = self._cost_inputs(costmap, costmap_kw, device=True)
        src = sources if ops._is_dev(sources) else np.asarray(sources)
        if not ops._is_dev(src) and src.shape != free.shape:
            pts = np.asarray(src, dtype=np.float64).reshape(-1, 2)
            cells = pts.astype(np.int64) - np.array([int(self.rmin), int(self.cmin)])
            if len(cells) and (cells.min() < 0 or cells[:, 0].max() >= free.shape[0] or cells[:, 1].max() >= free.shape[1]):
                raise ValueError(f"get_cost_field: a source lies outside the obstacle crop [{self.rmin}:{self.rmax + 1}, "
                                 f"{self.cmin}:{self.cmax + 1}]")
            src = cells
        return ops.cost_field(free, costmap, src)

    def plan_cost_path(self, start, goal, costmap=None, waypoints: bool = True, with_cost: bool = False, **costmap_kw):
        """The cheapest 8-connected path from start to goal under `costmap` (default: get_costmap(**costmap_kw)), full-map
        (row, col) in and out like Navigator.plan_to: [[row, col], ...] cell centres from the start's cell to the goal's.  The
        field is grown from the GOAL and descended from the start (CostField.descend), so one field serves many starts; the path
        driven forwards enters the same cells but for the two ends, so its price differs from the field's by
        cost[start] - cost[goal], the same for every path between the two.  waypoints=True keeps the ends and the cells where the
        direction changes.  A start or goal on an impassable cell snaps to the nearest passable one, by the rule the Navigator snaps
        to the nearest free cell.  with_cost=True: -> (path, the field's price A + B sqrt(2) at the start).  NoPathError when the
        start is not reached; ValueError for a point outside the crop."""
        from .. import ops
        from ..utils.navigation_utils import NoPathError, _inside, _nearest_free
        free, costmap = self._cost_inputs(costmap, costmap_kw, device=False)
        cost = costmap if isinstance(costmap, np.ndarray) else costmap.numpy()
        passable = free & (cost != 0)
        r0, c0 = int(self.rmin), int(self.cmin)
        cells = []
        for point in (start, goal):
            r, c = _inside(passable, (float(point[0]) - r0, float(point[1]) - c0))
            if not passable[int(r), int(c)]:
                r, c = _nearest_free(passable, (r, c))
            cells.append((int(r), int(c)))
        field = ops.cost_field(free, cost, np.array([cells[1]], dtype=np.int64))
        a, b = field.planes()
        if a[cells[0]] < 0:
            raise NoPathError(f"no passable way from cell {cells[0]} to cell {cells[1]} of the obstacle crop")
        walk = field.descend(cells[0], waypoints=waypoints)
        path = [[float(r + r0), float(c + c0)] for r, c in walk]
        if with_cost:
            return path, float(a[cells[0]]) + float(b[cells[0]]) * float(np.sqrt(2.0))
        return path

    def get_rooms(self, door_width: float = 0.9, min_core_area: float = 0.25, customized: bool = False, known_free: bool = False):
        """The rooms of this map: a Rooms (map/rooms.py) of ops.segment_rooms over the obstacle crop (customized: the customised
        crop; known_free: get_known_free_cropped), DESIGN.md 4.27.  The free space is eroded by half a door width -- radius =
        door_width / (2 cs) cells -- so that rooms fall apart at their doors; the pieces of at least min_core_area square metres
        (min_seed_cells = ceil(min_core_area / cs^2)) are the seeds, and they grow back along the travel field until they meet in
        the doorways.  Openings wider than door_width do not separate rooms, and furniture does: call customize_obstacle_map with
        the walls only and pass customized=True, or a sofa across a room splits it.  Upstream has no counterpart."""
        from .. import ops
        from .rooms import Rooms, room_parameters
        free = self._travel_free(customized, known_free)
        radius, least = room_parameters(door_width, min_core_area, self.cs)
        seg = ops.segment_rooms(free, radius, least)
        params = dict(door_width=float(door_width), min_core_area=float(min_core_area), radius=radius, min_seed_cells=least)
        return Rooms(seg.labels, seg.rooms, seg.doors, seg.clearance, (int(self.rmin), int(self.cmin)), self.cs, params, seg.field)

    @staticmethod
    def _dilate_map(binary_map: np.ndarray, dilate_iter: int = 0, gaussian_sigma: float = 1.0):
        """2x bilinear upsample -> gaussian -> threshold -> dilation -> downsample, (h, w) float64.  Reference: map.py:169-181
        (cv2.resize, scipy.ndimage); here one composite of csrc/avl_morph2d.hip (avl_dilate_map)."""
        from .. import ops
        return ops.dilate_map(np.asarray(binary_map) != 0, dilate_iter, gaussian_sigma, want_zero=False)[0]

    # ------------------------------------------------------------------------ goal helpers of the planner (map.py:183-240)
    def get_nearest_pos(self, curr_pos: List[float], name: str) -> List[float]:
        """the point of the nearest sizeable `name` object's contour closest to curr_pos (full-map (row, col)); curr_pos itself
        when there is none"""
        contours, centers, bbox_list = self.get_pos(name)
        keep = self.filter_small_objects(bbox_list, area_thres=10)
        contours = [contours[i] for i in keep]
        centers = [centers[i] for i in keep]
        bbox_list = [bbox_list[i] for i in keep]
        if not centers:
            return curr_pos
        k = self.select_nearest_obj(centers, bbox_list, curr_pos)
        return self.nearest_point_on_polygon(curr_pos, contours[k])

    def get_nearest_reachable_pos(self, curr_pos: List[float], name: str, navigator):
        """-> (pos, path): the contour point of a sizeable `name` object with the shortest TRAVEL distance from curr_pos on the
        navigator's obstacle map, and the path to it (Navigator.plan_to_nearest; full-map (row, col)).  The candidates are the
        contour points of every island that survives filter_small_objects(area_thres=10), island by island in get_pos order; ties
        go to the first candidate.  (curr_pos, [curr_pos]) when there is no island; NoPathError when no candidate can be reached.
        get_nearest_pos picks as the crow flies, which may be the object behind the wall."""
        contours, centers, bbox_list = self.get_pos(name)
        keep = self.filter_small_objects(bbox_list, area_thres=10)
        if not keep:
            return curr_pos, [curr_pos]
        cand = np.concatenate([np.asarray(contours[i]).reshape(-1, 2) for i in keep], axis=0)
        k, path = navigator.plan_to_nearest(curr_pos, cand)
        return [int(cand[k, 0]), int(cand[k, 1])], path

    @staticmethod
    def nearest_point_on_polygon(coord: List[float], polygon) -> List[int]:
        """The exact nearest point to `coord` on the closed ring through `polygon`'s points (no shapely): among equally near points
        the one with the smallest arc length from the first point, then int() truncation of both coordinates as upstream."""
        pts = np.asarray(polygon, dtype=np.float64).reshape(-1, 2)
        x = np.asarray(coord, dtype=np.float64)
        if len(pts) == 0:
            raise ValueError("empty polygon")
        best, best_d2 = pts[0], float(np.sum((x - pts[0]) ** 2))
        for k in range(len(pts)):
            a, b = pts[k], pts[(k + 1) % len(pts)]
            ab = b - a
            L2 = float(ab @ ab)
            if L2 == 0.0:
                continue
            t = min(1.0, max(0.0, float((x - a) @ ab) / L2))
            q = a + t * ab
            d2 = float(np.sum((x - q) ** 2))
            if d2 < best_d2:
                best, best_d2 = q, d2
        return [int(best[0]), int(best[1])]

    def get_forward_pos(self, curr_pos: List[float], curr_angle_deg: float, meters: float) -> List[float]:
        """the cell `meters` ahead of curr_pos (row, col) at heading curr_angle_deg (0 = towards smaller rows)"""
        rad = np.deg2rad(curr_angle_deg)
        pix = meters / self.cs
        return [curr_pos[0] - pix * np.cos(rad), curr_pos[1] + pix * np.sin(rad)]

    def filter_small_objects(self, bbox_list: List[List[int]], area_thres: int = 50) -> List[int]:
        """indices of the boxes [rmin, rmax, cmin, cmax] whose (rmax - rmin) * (cmax - cmin) exceeds area_thres"""
        return [i for i, b in enumerate(bbox_list) if (b[1] - b[0]) * (b[3] - b[2]) > area_thres]

    def select_nearest_obj(self, centers: List[List[float]], bbox_list: List[List[float]], curr_pos) -> int:
        """index of the box nearest to curr_pos (utils.navigation_utils.get_dist_to_bbox_2d), the first on ties"""
        from ..utils.navigation_utils import get_dist_to_bbox_2d
        d = [get_dist_to_bbox_2d(np.array(c), np.array([b[1] - b[0], b[3] - b[2]]), np.array(curr_pos))
             for c, b in zip(centers, bbox_list)]
        return int(np.argmin(d))

    # ------------------------------------------------------------------- spatial-relation goals of the robot (map.py:243-485)
    # Angles: 0 = towards smaller rows ("up"), clockwise positive, like get_forward_pos.  Positions are full-map (row, col).
    # Upstream's conventions are kept as they are, the odd ones included; each is named where it happens.
    @staticmethod
    def _side_pos(curr_pos, tar_pos, tar_bbox, sign: float, margin: float) -> List[float]:
        """the point beside the target as seen from curr_pos: half the box diagonal (+ margin) away from its centre, at a right angle
        to the line of sight; sign +1 = left, -1 = right"""
        angle = np.arctan2(-(tar_pos[1] - curr_pos[1]), -(tar_pos[0] - curr_pos[0]))
        h = tar_bbox[1] - tar_bbox[0]
        w = tar_bbox[3] - tar_bbox[2]
        d = 0.5 * np.sqrt(h * h + w * w) + margin
        return [tar_pos[0] + sign * (np.sin(angle) * d), tar_pos[1] - sign * (np.cos(angle) * d)]

    def _get_left_pos(self, curr_pos: List[float], tar_pos: List[float], tar_bbox: List[float]) -> List[float]:
        """Reference: map.py:243-260.  Upstream first derives a distance from the box's extent along the line of sight and then
        overwrites it with half the diagonal + 2; only the latter reaches the result, so only it is computed."""
        return self._side_pos(curr_pos, tar_pos, tar_bbox, 1.0, 2)

    def _get_right_pos(self, curr_pos: List[float], tar_pos: List[float], tar_bbox: List[float]) -> List[float]:
        """Reference: map.py:262-276: half the diagonal, without the left side's + 2."""
        return self._side_pos(curr_pos, tar_pos, tar_bbox, -1.0, 0)

    def select_front_objs(self, centers: List[List[float]], curr_pos: List[float], curr_angle_deg: float, fov_deg: float = 90) -> List[int]:
        """indices of the centres inside the field of view of a robot at curr_pos heading curr_angle_deg.  Reference: map.py:308-349,
        with its two wrap-around branches for headings beyond +-90 degrees."""
        theta = curr_angle_deg * np.pi / 180
        half_fov = fov_deg * np.pi / 360
        quarter = np.pi / 2
        row0, col0 = curr_pos
        keep = []
        for k, (row, col) in enumerate(centers):
            a = np.arctan2(-col + col0, -row + row0)
            if (np.abs(a - theta) < half_fov
                    or (theta > quarter and a < -quarter and np.abs(2 * np.pi - theta + a) < half_fov)
                    or (theta < -quarter and a > quarter and np.abs(2 * np.pi - a + theta) < half_fov)):
                keep.append(k)
        return keep

    def get_front_nearest_obj_pos(self, curr_pos: List[float], curr_angle_deg: float, name: str):
        """centre of the nearest `name` object in front, None when there is none.  Reference: map.py:278-287 -- the front centres
        are paired with the UNFILTERED box list there (box k of all objects goes with front centre k); kept."""
        _, centers, bbox_list = self.get_pos(name)
        front = self.select_front_objs(centers, curr_pos, curr_angle_deg)
        if not front:
            return None
        front_centers = [centers[i] for i in front]
        return front_centers[self.select_nearest_obj(front_centers, bbox_list, curr_pos)]

    def get_front_nearest_obj_pos_box(self, curr_pos: List[float], curr_angle_deg: float, name: str):
        """(centre, box) of the nearest `name` object in front, (None, None) when there is none.  Reference: map.py:289-306."""
        _, centers, bbox_list = self.get_pos(name)
        front = self.select_front_objs(centers, curr_pos, curr_angle_deg)
        if not front:
            return None, None
        front_centers = [centers[i] for i in front]
        front_boxes = [bbox_list[i] for i in front]
        k = self.select_nearest_obj(front_centers, front_boxes, curr_pos)
        return front_centers[k], front_boxes[k]

    def find_middle_bewteen_contours(self, cona, conb):
        """midpoint of the nearest pair of points of two contours (upstream's spelling).  Reference: map.py:351-364 builds the
        |A| x |B| float64 distance matrix for its argmin; here the pair comes from the GPU (ops.contour_nearest_pair: the same first
        minimum, the matrix never built)."""
        from .. import ops
        i, j, _ = ops.contour_nearest_pair(cona, conb)
        return (cona[i] + conb[j]) / 2

    def get_pos_in_between(self, curr_pos: List[float], curr_angle_deg: float, obj_a_name: str, obj_b_name: str):
        """the point between the pair of sizeable front objects a, b whose centre midpoint is nearest to curr_pos; None when either
        has nothing in front.  Reference: map.py:366-413.  Upstream filters the FRONT boxes by size and then uses the surviving
        indices on the front contours but on the FULL centre lists; kept, so the chosen pair of centres need not belong to the
        contours the midpoint is taken between."""
        contours_a, centers_a, bbox_a = self.get_pos(obj_a_name)
        contours_b, centers_b, bbox_b = self.get_pos(obj_b_name)
        front_a = self.select_front_objs(centers_a, curr_pos, curr_angle_deg)
        front_b = self.select_front_objs(centers_b, curr_pos, curr_angle_deg)
        if not front_a or not front_b:
            return None
        contours_a = [contours_a[i] for i in front_a]
        contours_b = [contours_b[i] for i in front_b]
        big_a = self.filter_small_objects([bbox_a[i] for i in front_a])
        big_b = self.filter_small_objects([bbox_b[i] for i in front_b])
        if not big_a or not big_b:
            return None
        ca = np.array([centers_a[i] for i in big_a]).reshape((-1, 1, 2))
        cb = np.array([centers_b[i] for i in big_b]).reshape((1, -1, 2))
        cona = [contours_a[i] for i in big_a]
        conb = [contours_b[i] for i in big_b]
        to_curr = np.linalg.norm((ca + cb) / 2 - np.array(curr_pos).reshape((1, 1, 2)), axis=-1)
        row, col = np.unravel_index(np.argmin(to_curr), to_curr.shape)
        return self.find_middle_bewteen_contours(cona[row], conb[col])

    def get_left_pos(self, curr_pos: List[float], curr_angle_deg: float, name: str) -> List[float]:
        """Reference: map.py:415-422; [None, None] with nothing in front."""
        center, box = self.get_front_nearest_obj_pos_box(curr_pos, curr_angle_deg, name)
        if center is None:
            return [None, None]
        return self._get_left_pos(curr_pos, center, box)

    def get_right_pos(self, curr_pos: List[float], curr_angle_deg: float, name: str) -> List[float]:
        """Reference: map.py:424-430; [None, None] with nothing in front."""
        center, box = self.get_front_nearest_obj_pos_box(curr_pos, curr_angle_deg, name)
        if center is None:
            return [None, None]
        return self._get_right_pos(curr_pos, center, box)

    def get_delta_angle_to(self, curr_pos: List[float], curr_angle_deg: float, name: str):
        """degrees to turn right to face the nearest `name` object (front or not).  Reference: map.py:432-449: np.mod brings the
        turn into [0, 360) and values above 180 come back as negative turns."""
        _, centers, bbox_list = self.get_pos(name)
        center = centers[self.select_nearest_obj(centers, bbox_list, curr_pos)]
        down = center[0] - curr_pos[0]
        right = center[1] - curr_pos[1]
        turn = np.mod(np.arctan2(right, -down) * 180.0 / np.pi - curr_angle_deg, 360)
        if turn < -180:
            turn += 360
        elif turn > 180:
            turn -= 360
        return turn

    def _compass_pos(self, curr_pos, curr_angle_deg, name, side: int, sign: int):
        """10 cells beyond side `side` of the nearest front object's box, level with its centre; ["stop"] with nothing in front"""
        center, box = self.get_front_nearest_obj_pos_box(curr_pos, curr_angle_deg, name)
        if center is None:
            return ["stop"]
        edge = box[side] + sign * 10
        return [edge, center[1]] if side < 2 else [center[0], edge]

    def get_north_pos(self, curr_pos: List[float], curr_angle_deg: float, name: str):
        """Reference: map.py:451-458."""
        return self._compass_pos(curr_pos, curr_angle_deg, name, 0, -1)

    def get_south_pos(self, curr_pos: List[float], curr_angle_deg: float, name: str):
        """Reference: map.py:460-467."""
        return self._compass_pos(curr_pos, curr_angle_deg, name, 1, 1)

    def get_west_pos(self, curr_pos: List[float], curr_angle_deg: float, name: str):
        """Reference: map.py:469-476."""
        return self._compass_pos(curr_pos, curr_angle_deg, name, 2, -1)

    def get_east_pos(self, curr_pos: List[float], curr_angle_deg: float, name: str):
        """Reference: map.py:478-485."""
        return self._compass_pos(curr_pos, curr_angle_deg, name, 3, 1)

    @staticmethod
    def create(map_config) -> "Map":
        """Reference: map.py:120-129."""
        from .vlmap import VLMap
        if cfg_get(map_config, "map_type") == "vlmap":
            return VLMap(map_config)
        if cfg_get(map_config, "map_type") == "vlmap_openmap":
            from .vlmap_multi_floor import VLMapMultiFloor
            return VLMapMultiFloor(map_config)
        raise NotImplementedError(f"map_type {cfg_get(map_config, 'map_type')!r}: only 'vlmap' and 'vlmap_openmap' are on the accelerated path")
