"""CPU-side checks of the headless renderer: the avl_render_* ABI, the PLY writer and reader, the cameras, the default colour table,
the Bresenham drawer, the save_path contract of the visualize_* functions and the applications' new flags."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
RENDER_SYMBOLS = {"avl_render_colorize", "avl_render_topdown_work_bytes", "avl_render_topdown", "avl_render_view_work_bytes",
                  "avl_render_view"}


def test_header_and_ctypes_table_declare_the_render_set():
    from avlmaps_amd import _lib
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    declared = set(re.findall(r"AVL_API\s+[\w\s\*]+?\b(avl_render_\w+)\s*\(", text))
    assert declared == RENDER_SYMBOLS
    assert {n for n in _lib.EXPORTED_SYMBOLS if n.startswith("avl_render_")} == RENDER_SYMBOLS


def test_render_source_is_built_unfused():
    from avlmaps_amd import build
    assert build.SOURCES["avl_render.hip"] == ["-ffp-contract=off"]


def test_argument_checks_need_no_device():
    import ctypes as C
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    build()
    lib = _lib.load()
    n = C.c_size_t(0)
    assert lib.avl_render_view_work_bytes(64, 48, C.byref(n)) == 0 and n.value == 64 * 48 * 8
    assert lib.avl_render_view_work_bytes(8192, 8192, C.byref(n)) == 0
    assert lib.avl_render_view_work_bytes(8193, 48, C.byref(n)) != 0 and lib.avl_render_view_work_bytes(64, 0, C.byref(n)) != 0
    assert lib.avl_render_view_work_bytes(64, 48, None) != 0 and b"null" in lib.avl_last_error()
    assert lib.avl_render_topdown_work_bytes(10, 7, C.byref(n)) == 0 and n.value == 10 * 7 * 16
    assert lib.avl_render_topdown_work_bytes(0, 7, C.byref(n)) != 0
    assert lib.avl_render_colorize(None, 0, None, None, 4, 1.5, None, None, None) != 0 and b"transparency" in lib.avl_last_error()
    assert lib.avl_render_colorize(None, 0, None, None, 4, 0.5, None, None, None) != 0 and b"null" in lib.avl_last_error()


def test_ply_round_trip(tmp_path):
    from avlmaps_amd.utils.visualize_utils import read_ply, write_ply
    rng = np.random.default_rng(0)
    for n in (0, 1, 1000):
        pts = rng.integers(-500, 500, (n, 3)).astype(np.int32)
        col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
        path = tmp_path / f"cloud{n}.ply"
        write_ply(path, pts, col)
        raw = path.read_bytes()
        assert raw.startswith(b"ply\nformat binary_little_endian 1.0\n") and len(raw.split(b"end_header\n", 1)[1]) == 15 * n
        p2, c2 = read_ply(path)
        assert p2.dtype == np.float32 and c2.dtype == np.uint8 and p2.shape == (n, 3) and c2.shape == (n, 3)
        assert np.array_equal(p2, pts.astype(np.float32)) and np.array_equal(c2, col)
    with pytest.raises(ValueError):
        write_ply(tmp_path / "bad.ply", np.zeros((3, 3)), np.zeros((2, 3), np.uint8))
    (tmp_path / "not.ply").write_bytes(b"hello\n")
    with pytest.raises(ValueError):
        read_ply(tmp_path / "not.ply")


def test_ply_colors_are_the_truncated_expression():
    from avlmaps_amd.utils.visualize_utils import ply_colors
    rgb = np.array([[0.0, 127.5, 255.0], [254.999, 300.0, -3.0], [1.0, 2.0, 3.0]])
    want = np.clip((rgb / 255.0) * 255.0, 0, 255).astype(np.uint8)
    assert np.array_equal(ply_colors(rgb), want)


def test_look_at_principal_point_and_axes():
    from avlmaps_amd.utils.visualize_utils import look_at
    T = look_at((0, 0, 0), (1, 0, 0), (0, 0, 1))                      # looking down +row from the origin
    assert T.shape == (3, 4) and T.dtype == np.float64
    p = T @ np.array([10.0, 0.0, 0.0, 1.0])
    assert np.allclose(p, [0.0, 0.0, 10.0], atol=1e-15)              # on the optical axis: u = cx, v = cy
    fx = fy = 32.0
    cx, cy = 32.0, 24.0
    assert fx * p[0] / p[2] + cx == cx and fy * p[1] / p[2] + cy == cy
    up = T @ np.array([10.0, 0.0, 2.0, 1.0])                          # higher cells appear higher in the image: y is down
    assert up[1] < 0 and abs(up[0]) < 1e-15
    # (row, col, h) is right-handed; looking down +row with h up, +col lies to the LEFT
    left = T @ np.array([10.0, 3.0, 0.0, 1.0])
    assert left[0] < 0
    T2 = look_at((5, 6, 7), (5, 6, 0), (1, 0, 0))                     # straight down, +row up in the image
    assert np.allclose(T2 @ np.array([5.0, 6.0, 0.0, 1.0]), [0, 0, 7])
    with pytest.raises(ValueError):
        look_at((1, 1, 1), (1, 1, 1))
    with pytest.raises(ValueError):
        look_at((0, 0, 0), (0, 0, 1), (0, 0, 1))


def _stub_map(gs=400, cs=0.05):
    """the transforms of the default config (camera 1.5 m above the base, x right / y down / z forward)"""
    from avlmaps_amd.apps.common import load_config
    from avlmaps_amd.map.map import Map
    m = Map(load_config(None).map_config)
    return SimpleNamespace(base_transform=m.base_transform, base2cam_tf=m.base2cam_tf, gs=gs, cs=cs, pose_path=None), m


def test_camera_of_frame_projects_a_hand_computed_cell():
    """identity base pose, default base2cam: pc_transform = base_transform @ base2cam_tf.  A camera-frame point (x, y, z) metres is
    sent to the map's base frame by pc_transform and from there to cells by row = gs / 2 - X / cs, col = gs / 2 - Y / cs,
    h = Z / cs; camera_of_frame must undo exactly that."""
    from avlmaps_amd.utils.visualize_utils import camera_of_frame
    stub, m = _stub_map()
    poses = np.array([[0, 0, 0, 0, 0, 0, 1.0]])
    T = camera_of_frame(stub, 0, base_poses=poses)
    assert T.shape == (3, 4)
    pc_transform = m.base_transform @ m.base2cam_tf
    cam = np.array([0.5, -0.25, 2.0, 1.0])                            # metres, camera frame
    X, Y, Z, _ = pc_transform @ cam
    cell = np.array([400 / 2 - X / 0.05, 400 / 2 - Y / 0.05, Z / 0.05, 1.0])
    p = T @ cell                                                       # camera frame again, in cells
    assert np.allclose(p, cam[:3] / 0.05, atol=1e-9)
    fx = fy = 64.0
    cx, cy = 64.0, 48.0
    u, v = fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy               # by hand: 64 * 0.25 + 64 = 80, 64 * -0.125 + 48 = 40
    assert abs(u - 80.0) < 1e-9 and abs(v - 40.0) < 1e-9
    with pytest.raises(IndexError):
        camera_of_frame(stub, 1, base_poses=poses)


def test_jet_table():
    from avlmaps_amd import ops
    t = ops.jet_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert tuple(t[0]) == (0, 0, 128) and tuple(t[255]) == (128, 0, 0)
    r, g, b = (t[:, k].astype(int) for k in range(3))
    # the definition: each channel is a trapezoid 1.5 - |4 x - c| clipped to [0, 1]: it rises up to its plateau and falls after it
    for ch, c in ((r, 3.0), (g, 2.0), (b, 1.0)):
        peak = int(round(c / 4.0 * 255))
        assert np.all(np.diff(ch[: peak + 1]) >= 0) and np.all(np.diff(ch[peak:]) <= 0) and ch[peak] == 255
    assert np.all(r[:96] == 0) and np.all(b[160:] == 0) and g[0] == 0 and g[255] == 0
    assert tuple(t[128]) == (130, 255, 126)                           # 1.5 - |4 * 128 / 255 - c| by hand: 0.5078, 1, 0.4922
    assert "compared" in ops.jet_table.__doc__


@pytest.mark.parametrize("a,b", [((0, 0), (5, 2)), ((0, 0), (2, 5)), ((0, 0), (-5, 2)), ((0, 0), (-2, 5)),
                                 ((0, 0), (5, -2)), ((0, 0), (2, -5)), ((0, 0), (-5, -2)), ((0, 0), (-2, -5)),
                                 ((3, 4), (3, 9)), ((3, 4), (8, 4)), ((1, 1), (6, 6)), ((2, 7), (2, 7))])
def test_bresenham(a, b):
    from avlmaps_amd.utils.visualize_utils import bresenham
    cells = bresenham(a[0], a[1], b[0], b[1])
    n = max(abs(b[0] - a[0]), abs(b[1] - a[1]))
    assert cells[0] == a and cells[-1] == b and len(cells) == n + 1          # one cell per step of the major axis
    assert len(set(cells)) == len(cells)
    for (r0, c0), (r1, c1) in zip(cells[:-1], cells[1:]):
        assert max(abs(r1 - r0), abs(c1 - c0)) == 1                              # 8-connected
    # never further than half a cell from the true line, measured along the minor axis
    dr, dc = b[0] - a[0], b[1] - a[1]
    for r, c in cells:
        assert 2 * abs((r - a[0]) * dc - (c - a[1]) * dr) <= n


def test_draw_polyline_and_marker_clip():
    from avlmaps_amd.utils.visualize_utils import draw_marker, draw_polyline
    img = np.zeros((6, 8, 3), np.uint8)
    draw_polyline(img, [(0, 0), (0, 7), (5, 7), (9, 12)], (1, 2, 3))           # the last leg leaves the image
    assert np.all(img[0, :] == (1, 2, 3)) and np.all(img[:, 7] == (1, 2, 3)) and img[3, 3].sum() == 0
    draw_polyline(img, [(2, 2)], (9, 9, 9))
    assert tuple(img[2, 2]) == (9, 9, 9)
    draw_marker(img, (0, 0), (5, 5, 5), radius=1)
    assert np.all(img[:2, :2] == 5) and tuple(img[2, 2]) == (9, 9, 9)
    draw_marker(img, (20, 20), (7, 7, 7))                                        # entirely outside: nothing changes
    assert not np.any(img == 7)


def test_visualize_functions_raise_without_save_path():
    from avlmaps_amd.utils import visualize_utils as vu
    pc = np.zeros((2, 3), np.int32)
    rgb = np.zeros((2, 3), np.uint8)
    heat = np.zeros(2, np.float32)
    img = np.zeros((4, 4, 3), np.uint8)
    calls = [lambda: vu.visualize_rgb_map_3d(pc, rgb), lambda: vu.visualize_heatmap_3d(pc, heat, rgb),
             lambda: vu.visualize_masked_map_3d(pc, heat > 0, rgb), lambda: vu.visualize_rgb_map_2d(img),
             lambda: vu.visualize_heatmap_2d(img, np.zeros((4, 4), np.float32)),
             lambda: vu.visualize_masked_map_2d(img, np.zeros((4, 4), np.uint8))]
    for call in calls:
        with pytest.raises(ValueError, match="save_path"):
            call()


def test_visualize_rgb_outputs_need_no_gpu(tmp_path):
    from PIL import Image
    from avlmaps_amd.utils import visualize_utils as vu
    rgb = np.arange(4 * 5 * 3).reshape(4, 5, 3).astype(np.float64) + 0.75
    out = vu.visualize_rgb_map_2d(rgb, save_path=tmp_path / "a.png")
    assert np.array_equal(out, rgb.astype(np.uint8)) and np.array_equal(np.asarray(Image.open(tmp_path / "a.png")), out)
    pc = np.arange(12).reshape(4, 3)
    col = np.array([[0, 128, 255]] * 4, np.uint8)
    vu.visualize_rgb_map_3d(pc, col, save_path=tmp_path / "a.ply")
    p2, c2 = vu.read_ply(tmp_path / "a.ply")
    assert np.array_equal(p2, pc) and np.array_equal(c2, np.clip((col / 255.0) * 255.0, 0, 255).astype(np.uint8))


def test_compat_maps_the_new_functions():
    import inspect
    from avlmaps_amd import compat
    src = inspect.getsource(compat.install)
    for fn in ("convert_heatmap_to_rgb", "pool_3d_rgb_to_2d", "visualize_rgb_map_3d", "visualize_heatmap_3d", "visualize_masked_map_3d",
               "visualize_rgb_map_2d", "visualize_heatmap_2d", "visualize_masked_map_2d"):
        assert f'"{fn}"' in src


def test_index_map_flags():
    from avlmaps_amd.apps import index_map
    base = ["--data-dir", "x", "--query", "sofa"]
    a = index_map.parse_args(base)
    assert a.render is None and a.view == "topdown" and a.save_ply is None
    a = index_map.parse_args(base + ["--render", "o.png", "--view", "frame:12", "--save-ply", "o.ply"])
    assert a.render == "o.png" and a.view == "frame:12" and a.save_ply == "o.ply"
    assert index_map.parse_args(base + ["--view", "orbit"]).view == "orbit"
    a = index_map.parse_args(["--data-dir", "x", "--modality", "fused", "--object", "sofa", "--render", "o.png"])
    assert a.render == "o.png"
    for bad in ("frame:x", "frame:", "side", "frame:-1"):
        with pytest.raises(SystemExit):
            index_map.parse_args(base + ["--view", bad])


def test_plan_path_flags():
    from avlmaps_amd.apps import plan_path
    base = ["--data-dir", "x", "--query", "sofa", "--start", "1", "2"]
    assert plan_path.parse_args(base).render is None
    assert plan_path.parse_args(base + ["--render", "p.png"]).render == "p.png"
    with pytest.raises(SystemExit):
        plan_path.parse_args(base + ["--render", "p.png", "--relation", "face", "--heading", "0"])
    with pytest.raises(SystemExit):
        plan_path.parse_args(base + ["--view", "frame:x"])
