"""Reference interface of avlmaps/utils/visualize_utils.py: the heat and pooling functions of the hot path, and its pictures without a
window (PLY / PNG writers on the render kernels, cameras, a small host drawer)."""
from __future__ import annotations

import numpy as np


def get_heatmap_from_mask_3d(pc: np.ndarray, mask: np.ndarray, cell_size: float = 0.05, decay_rate: float = 0.01) -> np.ndarray:
    """Nearest-target distance-decay heat per voxel, (N,) float32.  Reference: visualize_utils.py:29-49
    (an O(N_other * N_target) Python loop upstream; here the windowed / brute-force HIP kernels)."""
    from .. import ops
    mask = np.asarray(mask)
    if mask.sum() == 0:
        raise ValueError("attempt to get argmin of an empty sequence")   # what np.argmin raises upstream
    # the same grid_pos array comes back on every query of a map: its device copy and cell order are kept between calls --
    # only when the array reaches the library as it is (a converted temporary is a new object every time: stateless path)
    pos = np.ascontiguousarray(pc, dtype=np.int32)
    return ops.heatmap_from_mask(pos, mask.astype(np.uint8), cell_size, decay_rate, reuse_plan=pos is pc)


def pool_3d_label_to_2d(mask_3d: np.ndarray, grid_pos: np.ndarray, gs: int) -> np.ndarray:
    """Top-down OR-pooling of a per-voxel mask, (gs, gs) bool.  Reference: visualize_utils.py:77-83 (a Python loop over all
    voxels upstream; here one scatter kernel, avl_pool_label_2d).  grid_pos / mask_3d may be device-resident."""
    from .. import ops
    return ops.pool_label_2d(mask_3d, grid_pos, int(gs))


def get_heatmap_from_mask_2d(mask: np.ndarray, cell_size: float = 0.05, decay_rate: float = 0.01) -> np.ndarray:
    """Distance-decay heat of a 2-D mask, (H, W) float64: 1 - distance_transform_edt(mask == 0) / cell_size * decay_rate, negative
    values 0.  Reference: visualize_utils.py:97-102 (scipy's EDT upstream; here the exact transform of csrc/avl_edt2d.hip and the
    decay in one chain on the GPU, NumPy's bits).  A mask without a set cell raises ValueError (upstream: distances to an imaginary
    cell outside the image)."""
    from .. import ops
    return ops.mask_decay_2d(np.asarray(mask) != 0, decay_rate, cell_size=cell_size)


# ---------------------------------------------------------------------------------------- headless rendering (csrc/avl_render.hip)
# Upstream shows these in Open3D / OpenCV windows.  A GPU box has no display and neither library is a dependency here: every
# function below writes a file (save_path) and raises without one.

def _need_save_path(name: str, save_path):
    if save_path is None:
        raise ValueError(f"{name}: save_path is required -- this build is headless and opens no window (upstream does when "
                         "save_path is None)")


def convert_heatmap_to_rgb(heatmap: np.ndarray, rgb: np.ndarray, transparency: float = 0.5, table=None) -> np.ndarray:
    """(N, 3) float64: table[(heatmap * 255).astype(uint8)] as float32 * transparency + rgb * (1 - transparency), NumPy 2's bits.
    Reference: visualize_utils.py:59-64 (cv2.applyColorMap + NumPy upstream; here avl_render_colorize).  heatmap float32 or
    float64; table: (256, 3) uint8 RGB, default ops.jet_table() (built from COLORMAP_JET's published definition, never compared
    with OpenCV).  A heat outside [0, 1] raises (upstream: an undefined uint8 cast)."""
    from .. import ops
    return ops.colorize_heat(np.asarray(heatmap).reshape(-1), rgb, transparency, table=table)


def pool_3d_rgb_to_2d(rgb: np.ndarray, grid_pos: np.ndarray, gs: int) -> np.ndarray:
    """(gs, gs, 3) uint8 top-down colour map.  Reference: visualize_utils.py:86-94.  Upstream compares h with `height` but never
    updates `height` (it stays -100), so every voxel overwrites its cell and the LAST voxel of a column wins: exactly
    ops.rgb_topdown (avl_rgb_topdown), which is reused here."""
    from .. import ops
    return ops.rgb_topdown(grid_pos, rgb, int(gs))


def ply_colors(rgb: np.ndarray) -> np.ndarray:
    """(N, 3) uint8 as a PLY file stores the colours of visualize_rgb_map_3d: rgb / 255.0 (what upstream hands to Open3D) scaled
    back by 255, clipped and truncated to a byte.  The layout follows Open3D's documented writer; it was not compared with it."""
    c = (np.asarray(rgb) / 255.0) * 255.0
    return np.clip(c, 0.0, 255.0).astype(np.uint8)


_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def write_ply(save_path, points: np.ndarray, colors_u8: np.ndarray) -> None:
    """binary little-endian PLY point cloud: float x, y, z and uchar red, green, blue per vertex"""
    pts = np.asarray(points).reshape(-1, 3)
    col = np.asarray(colors_u8, dtype=np.uint8).reshape(-1, 3)
    if len(pts) != len(col):
        raise ValueError(f"{len(pts)} points but {len(col)} colours")
    v = np.empty(len(pts), dtype=_PLY_VERTEX)
    v["x"], v["y"], v["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    v["red"], v["green"], v["blue"] = col[:, 0], col[:, 1], col[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\ncomment avlmaps_amd\n"
              f"element vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(str(save_path), "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())


def read_ply(path):
    """-> (points (N, 3) float32, colors (N, 3) uint8) of a file write_ply wrote (that vertex layout only)"""
    with open(str(path), "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        n, props, fmt = None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: the PLY header does not end")
            words = line.decode("ascii", errors="replace").split()
            if not words or words[0] == "comment":
                continue
            if words[0] == "format":
                fmt = words[1]
            elif words[0] == "element":
                if words[1] != "vertex" or n is not None:
                    raise ValueError(f"{path}: only a single vertex element is supported")
                n = int(words[2])
            elif words[0] == "property":
                props.append((words[1], words[2]))
            elif words[0] == "end_header":
                break
        want = [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
        if fmt != "binary_little_endian" or n is None or props != want:
            raise ValueError(f"{path}: expected binary_little_endian vertices of float x, y, z and uchar red, green, blue")
        data = f.read(n * _PLY_VERTEX.itemsize)
    if len(data) != n * _PLY_VERTEX.itemsize:
        raise ValueError(f"{path}: truncated vertex data")
    v = np.frombuffer(data, dtype=_PLY_VERTEX, count=n)
    return np.stack([v["x"], v["y"], v["z"]], axis=1), np.stack([v["red"], v["green"], v["blue"]], axis=1)


def visualize_rgb_map_3d(pc: np.ndarray, rgb: np.ndarray, save_path=None):
    """Writes the coloured point cloud to save_path as PLY.  Reference: visualize_utils.py:10-26 (Open3D's writer, or a window
    when save_path is None; here the file only)."""
    _need_save_path("visualize_rgb_map_3d", save_path)
    write_ply(save_path, pc, ply_colors(rgb))


def visualize_heatmap_3d(pc: np.ndarray, heatmap: np.ndarray, rgb: np.ndarray, transparency: float = 0.5, save_path=None):
    """The heat blended over the voxel colours, as a PLY point cloud.  Reference: visualize_utils.py:67-74 (without its three
    prints: np.unique of 2 M floats is not a statistic anybody reads)."""
    _need_save_path("visualize_heatmap_3d", save_path)
    visualize_rgb_map_3d(pc, convert_heatmap_to_rgb(heatmap, rgb, transparency), save_path)


def visualize_masked_map_3d(pc: np.ndarray, mask: np.ndarray, rgb: np.ndarray, transparency: float = 0.5, save_path=None):
    """Reference: visualize_utils.py:52-56.  Upstream casts the mask to float16; 0 and 1 give table entries 0 and 255 in every
    float format, so float32 is used here (the kernels take float32 and float64)."""
    _need_save_path("visualize_masked_map_3d", save_path)
    visualize_heatmap_3d(pc, (np.asarray(mask) != 0).astype(np.float32), rgb, transparency, save_path)


def _save_png(save_path, image_u8: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(image_u8, dtype=np.uint8)).save(str(save_path))


def visualize_rgb_map_2d(rgb: np.ndarray, save_path=None) -> np.ndarray:
    """Writes rgb.astype(np.uint8) (H, W, 3) as a PNG and returns it.  Reference: visualize_utils.py:105-114 (cv2.imshow)."""
    _need_save_path("visualize_rgb_map_2d", save_path)
    img = np.asarray(rgb).astype(np.uint8)
    _save_png(save_path, img)
    return img


def visualize_heatmap_2d(rgb: np.ndarray, heatmap: np.ndarray, transparency: float = 0.5, save_path=None, table=None) -> np.ndarray:
    """The 2-D heat (H, W) blended over the colour map (H, W, 3) uint8, written as a PNG.  Reference: visualize_utils.py:117-128:
    the same expression as convert_heatmap_to_rgb per pixel and visualize_rgb_map_2d's truncation (avl_render_colorize's uint8
    form)."""
    _need_save_path("visualize_heatmap_2d", save_path)
    from .. import ops
    heat = np.asarray(heatmap)
    if heat.ndim != 2 or np.asarray(rgb).shape != heat.shape + (3,):
        raise ValueError(f"expected a (H, W) heat and a (H, W, 3) colour map, got {heat.shape} and {np.asarray(rgb).shape}")
    img = ops.colorize_heat(heat.reshape(-1), np.asarray(rgb).reshape(-1, 3), transparency, table=table, as_uint8=True)
    img = img.reshape(heat.shape + (3,))
    _save_png(save_path, img)
    return img


def visualize_masked_map_2d(rgb: np.ndarray, mask: np.ndarray, save_path=None) -> np.ndarray:
    """Reference: visualize_utils.py:131-138."""
    _need_save_path("visualize_masked_map_2d", save_path)
    return visualize_heatmap_2d(rgb, np.asarray(mask).astype(np.float32), save_path=save_path)


# ---------------------------------------------------------------------------------------- cameras (cell coordinates)
def look_at(eye, target, up=(0.0, 0.0, 1.0)) -> np.ndarray:
    """(3, 4) float64 T of ops.render_view: from cell coordinates (row, col, h) to the frame of a camera at `eye` looking at
    `target` (x right, y down, z forward, in cells).  (row, col, h) is right-handed, so right = forward x up, down = forward x right."""
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    f = target - eye
    nf = np.linalg.norm(f)
    if not nf > 0:
        raise ValueError("look_at: eye and target coincide")
    f = f / nf
    r = np.cross(f, up)
    nr = np.linalg.norm(r)
    if not nr > 0:
        raise ValueError("look_at: up is parallel to the viewing direction")
    r = r / nr
    d = np.cross(f, r)
    rot = np.stack([r, d, f])
    return np.concatenate([rot, (-rot @ eye)[:, None]], axis=1)


def cell_to_base(gs: int, cs: float) -> np.ndarray:
    """(4, 4): (row, col, h, 1) -> metres in the map's base frame, the inverse of the affine part of base_pos2grid_id_3d
    (row = gs / 2 - x / cs, col = gs / 2 - y / cs, h = z / cs; mapping_utils.py:345-349 without its int())"""
    a = np.zeros((4, 4))
    a[0, 0], a[0, 3] = -cs, gs / 2 * cs
    a[1, 1], a[1, 3] = -cs, gs / 2 * cs
    a[2, 2] = cs
    a[3, 3] = 1.0
    return a


def camera_of_frame(vlmap, frame_i: int, base_poses=None) -> np.ndarray:
    """(3, 4) float64 T of ops.render_view for the camera that took frame `frame_i` of a mobile-base map: the inverse of that
    frame's pc_transform (VLMapBuilder.frame_transforms: camera frame -> the map's base frame, metres) composed with cell_to_base,
    divided by the cell size so that depths are in cells.  base_poses: (F, 7) rows of poses.txt, read from vlmap.pose_path when
    None."""
    from types import SimpleNamespace
    from ..map.vlmap_builder import VLMapBuilder
    poses = np.loadtxt(vlmap.pose_path) if base_poses is None else np.asarray(base_poses, dtype=np.float64)
    poses = poses.reshape(-1, 7)
    if not 0 <= int(frame_i) < len(poses):
        raise IndexError(f"frame {frame_i} of {len(poses)}")
    chain = SimpleNamespace(base_transform=np.asarray(vlmap.base_transform), base2cam_tf=np.asarray(vlmap.base2cam_tf))
    pc_transform = VLMapBuilder.frame_transforms(chain, poses[: int(frame_i) + 1])[int(frame_i)]
    m = np.linalg.inv(pc_transform) @ cell_to_base(int(vlmap.gs), float(vlmap.cs))
    return np.ascontiguousarray(m[:3] / float(vlmap.cs))


def orbit_camera(grid_pos: np.ndarray, azimuth_deg: float = 45.0, elevation_deg: float = 35.0, distance: float = 1.2) -> np.ndarray:
    """(3, 4) T of an outside view of the whole map: the camera looks at the centre of the voxels' bounding box from `distance`
    times its diagonal away, `azimuth_deg` around the height axis and `elevation_deg` above the floor"""
    pos = np.asarray(grid_pos, dtype=np.float64).reshape(-1, 3)
    if len(pos) == 0:
        return look_at((0.0, -1.0, 1.0), (0.0, 0.0, 0.0))
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    centre = (lo + hi) / 2.0
    diag = max(float(np.linalg.norm(hi - lo)), 1.0)
    az, el = np.deg2rad(azimuth_deg), np.deg2rad(elevation_deg)
    eye = centre + distance * diag * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    return look_at(eye, centre)


def frame_intrinsics(size):
    """(fx, fy, cx, cy) of the 90-degree pinhole the simulator's frames were taken with (mapping_utils.get_sim_cam_mat) for an
    image of size = (W, H)"""
    from .mapping_utils import get_sim_cam_mat
    k = get_sim_cam_mat(int(size[1]), int(size[0]))
    return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])


# ---------------------------------------------------------------------------------------- drawing on a small host image
def bresenham(r0: int, c0: int, r1: int, c1: int):
    """the cells of the integer Bresenham line from (r0, c0) to (r1, c1), both ends included, in order: list of (row, col)"""
    r0, c0, r1, c1 = int(r0), int(c0), int(r1), int(c1)
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sr, sc = (1 if r1 >= r0 else -1), (1 if c1 >= c0 else -1)
    err = dr - dc
    out = [(r0, c0)]
    while (r0, c0) != (r1, c1):
        e2 = 2 * err
        if e2 > -dc:
            err -= dc
            r0 += sr
        if e2 < dr:
            err += dr
            c0 += sc
        out.append((r0, c0))
    return out


def draw_polyline(image: np.ndarray, points, color) -> np.ndarray:
    """draws the polyline through `points` ((row, col) pairs, rounded to cells) into image (H, W, 3) uint8 in place; cells outside
    the image are skipped"""
    H, W = image.shape[:2]
    pts = [(int(round(float(p[0]))), int(round(float(p[1])))) for p in points]
    segs = zip(pts[:-1], pts[1:]) if len(pts) > 1 else [(pts[0], pts[0])] if pts else []
    for (a, b) in segs:
        for r, c in bresenham(a[0], a[1], b[0], b[1]):
            if 0 <= r < H and 0 <= c < W:
                image[r, c] = color
    return image


def draw_marker(image: np.ndarray, point, color, radius: int = 2) -> np.ndarray:
    """a filled (2 * radius + 1) square around point = (row, col), clipped to the image, in place"""
    H, W = image.shape[:2]
    r, c = int(round(float(point[0]))), int(round(float(point[1])))
    image[max(r - radius, 0):max(min(r + radius + 1, H), 0), max(c - radius, 0):max(min(c + radius + 1, W), 0)] = color
    return image
