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
