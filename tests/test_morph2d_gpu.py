"""2-D image morphology on the GPU (csrc/avl_morph2d.hip through ops.binary_morph, gaussian_filter2d, resize2x_up / resize2x_down,
dilate_map, mask_foreground, and their users Map._dilate_map, VLMap.customize_obstacle_map and VLMap.get_pos) against SciPy, called
the way upstream calls it.  The two cv2.resize calls of Map._dilate_map have no library to compare with here; their reference is
the NumPy restatement below of OpenCV's documented half-pixel rule.

Every comparison is np.array_equal.  The thresholded composites carry one condition, asserted on the reference side: no reference
gaussian value lies within 1e-12 of 0.5, so that no threshold is decided by the last bit of a weight."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy.ndimage import binary_closing, binary_dilation, binary_erosion, gaussian_filter

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(ROOT / "tools"))

BOX = np.ones((3, 3))


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


# ------------------------------------------------------------------ inputs
def scene(seed, H, W):
    """rectangular rooms with axis-aligned walls 1-3 cells thick, one-cell gaps in them, blobs touching all four image edges and
    1 % salt noise -> (H, W) bool"""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), bool)
    for _ in range(max(1, (H * W) // 20000 + 2)):
        h, w = int(rng.integers(max(2, H // 6), max(3, H // 2 + 1))), int(rng.integers(max(2, W // 6), max(3, W // 2 + 1)))
        r, c = int(rng.integers(0, max(1, H - h))), int(rng.integers(0, max(1, W - w)))
        t = int(rng.integers(1, 4))
        room = np.zeros((H, W), bool)
        room[r:r + h, c:c + w] = True
        room[r + t:max(r + t, r + h - t), c + t:max(c + t, c + w - t)] = False
        for _gap in range(3):                                  # one-cell gaps through the wall's whole thickness
            if rng.random() < 0.5:
                rr = min(int(rng.integers(r, r + h)), H - 1)
                room[rr, c:c + t] = False
            else:
                cc = min(int(rng.integers(c, c + w)), W - 1)
                room[r:r + t, cc] = False
        m |= room
    bh, bw = max(1, H // 10), max(1, W // 10)
    m[:bh, W // 3:W // 3 + bw] = True                          # blobs on the four edges
    m[H - bh:, W // 2:W // 2 + bw] = True
    m[H // 3:H // 3 + bh, :bw] = True
    m[H // 2:H // 2 + bh, W - bw:] = True
    m |= rng.random((H, W)) < 0.01
    return m


def images():
    out = [("zeros", np.zeros((37, 52), bool)), ("ones", np.ones((40, 33), bool)), ("ones9", np.ones((9, 9), bool)),
           ("1x1_set", np.ones((1, 1), bool)), ("1x1_clear", np.zeros((1, 1), bool)), ("1xN", scene(1, 1, 77)), ("Nx1", scene(2, 64, 1)),
           ("odd", scene(3, 61, 95)), ("even", scene(4, 128, 200)), ("odd_even", scene(5, 97, 130)), ("tiny", scene(6, 5, 4))]
    return out


@pytest.fixture(scope="module")
def big():
    return scene(11, 1000, 1000)


# ------------------------------------------------------------------ references
def ref_up2(x):
    """destination index i samples the source at (i + 0.5) / 2 - 0.5, source indices clamped at both ends, bilinear"""
    x = np.asarray(x, dtype=np.float64)

    def taps(n):
        s = (np.arange(2 * n) + 0.5) / 2 - 0.5
        f = np.floor(s)
        return np.clip(f, 0, n - 1).astype(int), np.clip(f + 1, 0, n - 1).astype(int), s - f
    y0, y1, fy = taps(x.shape[0])
    x0, x1, fx = taps(x.shape[1])
    top = x[y0][:, x0] * (1 - fx) + x[y0][:, x1] * fx
    bot = x[y1][:, x0] * (1 - fx) + x[y1][:, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


def ref_down2(x):
    x = np.asarray(x, dtype=np.float64)
    return (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2]) / 4


def _clear_of_half(g):
    assert not (np.abs(g - 0.5) <= 1e-12).any(), "a reference gaussian value lies within 1e-12 of the threshold"


def reference_dilate(binary, dilate_iter, sigma):
    """Map._dilate_map (upstream map.py:169-181) with the NumPy resizes"""
    m = ref_up2(np.asarray(binary).astype(float))
    g = gaussian_filter(m.astype(float), sigma=sigma, truncate=3)
    _clear_of_half(g)
    m = (g > 0.5).astype(np.uint8)
    m = binary_dilation(m, structure=BOX, iterations=dilate_iter * 2)
    return ref_down2(m.astype(float))


def reference_foreground(mask_2d):
    """the mask chain of VLMap.get_pos (upstream vlmap.py:168-171)"""
    f = binary_closing(mask_2d, iterations=3)
    g = gaussian_filter(f.astype(float), sigma=0.8, truncate=3)
    _clear_of_half(g)
    return binary_dilation(g > 0.5)


# ------------------------------------------------------------------ primitives
@pytest.mark.parametrize("iterations", [1, 2, 3, 6, 10])
@pytest.mark.parametrize("structure", ["cross", "box"])
@pytest.mark.parametrize("op", ["dilate", "erode"])
def test_binary_morph_equals_scipy(ops, big, op, structure, iterations):
    fn = binary_dilation if op == "dilate" else binary_erosion
    st = None if structure == "cross" else BOX
    for name, img in images() + [("big", big)]:
        want = fn(img, structure=st, iterations=iterations)
        got = ops.binary_morph(img, op, structure, iterations)
        assert got.dtype == bool and got.shape == img.shape
        assert np.array_equal(got, want), (name, op, structure, iterations, int((got != want).sum()))


def test_closing_of_ones_keeps_the_centre(ops):
    """erosion eats k cells inwards from every image edge: binary_closing(np.ones((9, 9)), iterations=3) keeps the centre 3 x 3"""
    x = np.ones((9, 9), bool)
    got = ops.binary_morph(ops.binary_morph(x, "dilate", "cross", 3), "erode", "cross", 3)
    want = np.zeros((9, 9), bool)
    want[3:6, 3:6] = True
    assert np.array_equal(binary_closing(x, iterations=3), want) and np.array_equal(got, want)


def test_binary_morph_radius_limit_and_device_results(ops):
    from avlmaps_amd import _lib
    from avlmaps_amd.device import DeviceArray
    img = scene(8, 80, 90)
    want = binary_dilation(img, structure=BOX, iterations=32)
    assert np.array_equal(ops.binary_morph(img, "dilate", "box", 32), want)          # the supported radius is at least 32
    with pytest.raises(_lib.AvlError):
        ops.binary_morph(img, "dilate", "box", 128)
    dev = ops.binary_morph(DeviceArray.from_numpy(img.astype(np.uint8)), "erode", "cross", 2, device=True)
    assert isinstance(dev, DeviceArray) and dev.dtype == np.uint8
    assert np.array_equal(dev.numpy().astype(bool), binary_erosion(img, iterations=2))


@pytest.mark.parametrize("sigma", [0.8, 1.0, 2.3])
def test_gaussian_filter2d_has_scipys_bits(ops, big, sigma):
    rng = np.random.default_rng(int(sigma * 10))
    for name, img in images() + [("big", big)]:
        want = gaussian_filter(img.astype(float), sigma, truncate=3)
        got = ops.gaussian_filter2d(img, sigma, truncate=3)
        assert got.dtype == np.float64 and np.array_equal(got, want), (name, sigma, float(np.abs(got - want).max()))
        x = rng.random(img.shape)
        want = gaussian_filter(x, sigma, truncate=3)
        got, gt = ops.gaussian_filter2d(x, sigma, truncate=3, threshold=0.5)
        assert np.array_equal(got, want), (name, sigma, "float64 input", float(np.abs(got - want).max()))
        assert gt.dtype == bool and np.array_equal(gt, want > 0.5)


def test_resizes_equal_the_half_pixel_rule(ops, big):
    rng = np.random.default_rng(5)
    for name, img in images() + [("big", big)]:
        up = ops.resize2x_up(img)
        assert up.dtype == np.float64 and up.shape == (2 * img.shape[0], 2 * img.shape[1])
        want = ref_up2(img)
        assert np.array_equal(want * 16, np.round(want * 16))                        # multiples of 1/16: exact in any order
        assert np.array_equal(up, want), name
        assert np.array_equal(ops.resize2x_down(up), ref_down2(want)), name
        if name != "big":
            x = rng.integers(0, 257, img.shape) / 256.0                              # dyadic values: every product and sum is exact
            assert np.array_equal(ops.resize2x_up(x), ref_up2(x)), name
            y = np.kron(img, np.ones((2, 2), bool)) ^ (rng.random((2 * img.shape[0], 2 * img.shape[1])) < 0.3)
            got = ops.resize2x_down(y)
            assert np.array_equal(got, ref_down2(y)) and set(np.unique(got)) <= {0.0, 0.25, 0.5, 0.75, 1.0}, name


# ------------------------------------------------------------------ composites
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("dilate_iter", [0, 1, 3, 5])
def test_dilate_map_equals_the_chained_reference(ops, dilate_iter, sigma):
    from avlmaps_amd.map.map import Map
    for name, img in images() + [("room", scene(21, 300, 400))]:
        want = reference_dilate(img, dilate_iter, sigma)
        vals, zero = ops.dilate_map(img, dilate_iter, sigma)
        assert vals.dtype == np.float64 and zero.dtype == bool and vals.shape == zero.shape == img.shape
        assert np.array_equal(vals, want), (name, dilate_iter, sigma, int((vals != want).sum()))
        assert np.array_equal(zero, want == 0), (name, dilate_iter, sigma)
    got = Map._dilate_map(img, dilate_iter, sigma)                                   # the public spelling, on the last image
    assert got.dtype == np.float64 and np.array_equal(got, want)


def test_dilate_map_at_full_size(ops, big):
    want = reference_dilate(big, 3, 1.0)
    vals, zero = ops.dilate_map(big, 3, 1.0)
    assert np.array_equal(vals, want) and np.array_equal(zero, want == 0)
    only_zero = ops.dilate_map(big, 3, 1.0, want_values=False)
    assert only_zero[0] is None and np.array_equal(only_zero[1], want == 0)


def test_mask_foreground_equals_the_chained_reference(ops, big):
    from avlmaps_amd.device import DeviceArray
    for name, img in images() + [("big", big)]:
        assert np.array_equal(ops.mask_foreground(img), reference_foreground(img)), name
    # crops of a pooled (gs, gs) mask, device-resident as VLMap.get_pos hands it over: the image corners and the interior; all
    # borders are the crop's
    dev = DeviceArray.from_numpy(big.astype(np.uint8))
    for r0, r1, c0, c1 in [(0, 300, 0, 400), (700, 1000, 600, 1000), (0, 1, 0, 1000), (999, 1000, 999, 1000), (123, 724, 250, 951),
                           (400, 401, 100, 164), (0, 1000, 0, 1000)]:
        got = ops.mask_foreground(dev, r0, r1, c0, c1)
        assert got.dtype == bool and np.array_equal(got, reference_foreground(big[r0:r1, c0:c1])), (r0, r1, c0, c1)
    with pytest.raises(ValueError):
        ops.mask_foreground(dev, 10, 10, 0, 5)


# ------------------------------------------------------------------ product
@pytest.fixture(scope="module")
def synth_map(tmp_path_factory):
    """a VLMap built from a synthetic scene with the model-free text model (the recipe of test_navigator_gpu)"""
    import yaml
    from make_synth_dataset import make
    tmp = tmp_path_factory.mktemp("morph2d")
    scene_dir = make(tmp / "scene", frames=6, H=96, W=128)
    cfg = tmp / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                  "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    from avlmaps_amd.apps import create_map
    create_map.main(["--data-dir", str(scene_dir), "--config", str(cfg), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    from avlmaps_amd.apps.common import HashClip, load_config
    from avlmaps_amd.map import VLMap
    conf = load_config(str(cfg))
    vm = VLMap(conf.map_config, data_dir=str(scene_dir))
    assert vm.load_map(str(scene_dir))
    vm.clip_feat_dim = vm.grid_feat.shape[1]
    vm.clip_model = HashClip(vm.clip_feat_dim)
    vm.init_categories(["sofa", "other"])
    vm.generate_obstacle_map()
    return vm, conf, scene_dir, cfg


def test_customize_obstacle_map_equals_the_reference(ops, synth_map):
    from avlmaps_amd.utils.index_utils import get_dynamic_obstacles_map_3d
    vm, conf, _, _ = synth_map
    mc = conf.map_config
    vm.customize_obstacle_map(mc.potential_obstacle_names, mc.obstacle_names)
    got = vm.get_customized_obstacle_cropped()
    assert got is vm.obstacles_new_cropped and vm.get_obstacle_cropped() is vm.obstacles_cropped
    assert got.dtype == bool and got.shape == vm.obstacles_cropped.shape
    dyn = get_dynamic_obstacles_map_3d(vm.clip_model, vm.obstacles_cropped, list(mc.potential_obstacle_names), list(mc.obstacle_names),
                                       vm._device_feat(), vm.grid_pos, vm.rmin, vm.cmin, vm.clip_feat_dim, precision=vm._sim_precision)
    want = reference_dilate(dyn == 0, mc.dilate_iter, mc.gaussian_sigma) == 0
    assert np.array_equal(got, want)
    assert (got == 0).any() and got.any()                      # the scene has obstacles, and free cells survive the dilation


def test_get_pos_equals_the_host_chain(ops, synth_map):
    from avlmaps_amd.utils.navigation_utils import get_segment_islands_pos
    from avlmaps_amd.utils.visualize_utils import pool_3d_label_to_2d
    vm, _, _, _ = synth_map
    islands = 0
    for name in ("sofa", "other"):
        contours, centers, bboxes = vm.get_pos(name)
        # the chain VLMap.get_pos ran on the host before the morphology moved to the GPU
        mask_2d = pool_3d_label_to_2d(vm.index_map(name, with_init_cat=True), vm.grid_pos, vm.gs)
        mask_2d = mask_2d[vm.rmin:vm.rmax + 1, vm.cmin:vm.cmax + 1]
        fg = reference_foreground(mask_2d)
        assert vm._last_foreground.dtype == bool and np.array_equal(vm._last_foreground, fg)
        wc, wcen, wbox, _ = get_segment_islands_pos(fg, 1)
        assert len(contours) == len(centers) == len(bboxes) == len(wc)
        islands += len(wc)
        for k in range(len(wc)):
            assert np.array_equal(contours[k], np.asarray(wc[k]) + [vm.rmin, vm.cmin])
            assert list(centers[k]) == [wcen[k][0] + vm.rmin, wcen[k][1] + vm.cmin]
            assert list(bboxes[k]) == [wbox[k][0] + vm.rmin, wbox[k][1] + vm.rmin, wbox[k][2] + vm.cmin, wbox[k][3] + vm.cmin]
    assert islands > 0                                         # the two categories split the voxels: at least one has an island


def test_plan_on_the_customized_map_and_the_app(ops, synth_map):
    from scipy import ndimage
    from avlmaps_amd.navigator import Navigator, NoPathError
    vm, conf, scene_dir, cfg = synth_map
    mc = conf.map_config
    vm.customize_obstacle_map(mc.potential_obstacle_names, mc.obstacle_names)
    free = vm.get_customized_obstacle_cropped()
    lab, n = ndimage.label(free)                               # 4-connected free regions: 8-connected walls separate them
    assert n >= 1
    sizes = ndimage.sum(free, lab, index=np.arange(1, n + 1))
    cells = np.argwhere(lab == 1 + int(np.argmax(sizes)))
    assert len(cells) >= 2
    a, b = cells[0], cells[-1]
    nav = Navigator()
    nav.build_visgraph(free, vm.rmin, vm.cmin)
    s, g = [float(a[0] + vm.rmin), float(a[1] + vm.cmin)], [float(b[0] + vm.rmin), float(b[1] + vm.cmin)]
    path = nav.plan_to(s, g)
    assert path[0] == s and path[-1] == g
    # name -> goal -> path on the customised map, in process and through the app; the start is the first free cell (in region order,
    # largest region first) from which the planner reaches the goal
    found = None
    for region in np.argsort(-sizes)[:4]:
        c = np.argwhere(lab == 1 + int(region))[0]
        start = [float(c[0] + vm.rmin), float(c[1] + vm.cmin)]
        goal = vm.get_nearest_pos(start, "sofa")
        try:
            found = (start, goal, nav.plan_to(start, goal))
            break
        except NoPathError:
            continue
    nav.close()
    assert found is not None, "no free region of the customised map reaches the goal"
    start, goal, path = found
    r = subprocess.run([sys.executable, "-m", "avlmaps_amd.apps.plan_path", "--data-dir", str(scene_dir), "--config", str(cfg),
                        "--query", "sofa", "--start", str(start[0]), str(start[1]), "--text-model", "hash", "--customize-obstacles",
                        "--potential-obstacles", ",".join(mc.potential_obstacle_names), "--obstacles", ",".join(mc.obstacle_names),
                        "--dilate-iter", str(mc.dilate_iter), "--gaussian-sigma", str(mc.gaussian_sigma)],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["path"] == [[float(p[0]), float(p[1])] for p in path] and out["goal"] == [float(goal[0]), float(goal[1])]


def test_generate_obstacle_map_app_writes_both_maps(ops, synth_map, tmp_path):
    from PIL import Image
    from avlmaps_amd.apps import generate_obstacle_map
    vm, conf, scene_dir, cfg = synth_map
    out = generate_obstacle_map.main(["--data-dir", str(scene_dir), "--config", str(cfg), "--text-model", "hash", "--out-dir", str(tmp_path)])
    raw = np.asarray(Image.open(tmp_path / "obstacles.png")) > 0
    custom = np.asarray(Image.open(tmp_path / "obstacles_customized.png")) > 0
    assert np.array_equal(raw, vm.obstacles_cropped)
    vm.customize_obstacle_map(conf.map_config.potential_obstacle_names, conf.map_config.obstacle_names)
    assert np.array_equal(custom, vm.get_customized_obstacle_cropped())
    assert out["obstacle_cells"] == int((raw == 0).sum()) and out["customized_obstacle_cells"] == int((custom == 0).sum())
