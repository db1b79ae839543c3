"""The render kernels (csrc/avl_render.hip) through ops, AVLMap.render_heat and the headless visualize_* functions, bit for bit
against NumPy restatements: the verbatim expression of upstream's convert_heatmap_to_rgb (visualize_utils.py:59-64, the colour
table looked up where upstream calls cv2.applyColorMap), an np.lexsort + loop over cells for the top-down overlay, and a painter
that draws the voxels far to near for the camera view."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(ROOT / "tools"))


def random_table(seed=7):
    return np.random.default_rng(seed).integers(0, 256, (256, 3)).astype(np.uint8)


# ------------------------------------------------------------------ colorize
def upstream_convert_heatmap_to_rgb(heatmap, rgb, transparency, table):
    """visualize_utils.py:59-64 verbatim, with cv2.applyColorMap(sim_new, cv2.COLORMAP_JET) ... [:, ::-1] (BGR -> RGB) written as the
    lookup in the (256, 3) RGB table it is"""
    sim_new = (heatmap * 255).astype(np.uint8)
    heat = table[sim_new]
    heat = heat.reshape(-1, 3).astype(np.float32)
    heat_rgb = heat * transparency + rgb * (1 - transparency)
    return heat_rgb


def edge_heats(dtype):
    """0, 1, every k / 255 and its two floating neighbours in `dtype`, inside [0, 1]: where heat * 255 falls on either side of an
    integer"""
    k = np.arange(256, dtype=dtype) / dtype(255)
    pool = np.concatenate([np.array([0.0, 1.0], dtype=dtype), k, np.nextafter(k, dtype(-1)), np.nextafter(k, dtype(2))])
    pool = pool[(pool >= 0) & (pool <= 1)]
    assert pool.dtype == dtype and len(pool) >= 3 * 256 - 2
    return pool


def colorize_case(N, dtype, seed):
    rng = np.random.default_rng(seed)
    pool = edge_heats(dtype)
    if N >= len(pool):
        heat = np.concatenate([pool, rng.random(N - len(pool)).astype(dtype)])
        rng.shuffle(heat)
    else:
        heat = rng.choice(pool, N, replace=False) if N else np.zeros(0, dtype)
    return heat.astype(dtype), rng.integers(0, 256, (N, 3)).astype(np.uint8)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [0, 1, 255, 256, 257, 70001])
def test_colorize_equals_the_upstream_expression(N, dtype):
    from avlmaps_amd import ops
    heat, rgb = colorize_case(N, dtype, N + (dtype == np.float64))
    for table in (ops.jet_table(), random_table()):
        for t in (0.0, 0.3, 0.5, 1.0):
            want = upstream_convert_heatmap_to_rgb(heat, rgb, t, table)
            assert want.dtype == np.float64 and want.shape == (N, 3)
            got = ops.colorize_heat(heat, rgb, t, table=table)
            assert got.dtype == np.float64 and np.array_equal(got, want), (t, np.abs(got - want).max())
            got8 = ops.colorize_heat(heat, rgb, t, table=table, as_uint8=True)
            assert got8.dtype == np.uint8 and np.array_equal(got8, want.astype(np.uint8))
    if N == 257:
        from avlmaps_amd.device import DeviceArray
        dev = ops.colorize_heat(DeviceArray.from_numpy(heat), DeviceArray.from_numpy(rgb), 0.5, device=True)
        assert isinstance(dev, DeviceArray)
        assert np.array_equal(dev.numpy(), upstream_convert_heatmap_to_rgb(heat, rgb, 0.5, ops.jet_table()))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("bad", [1.0000001, -1e-9, float("nan")])
def test_colorize_rejects_a_heat_without_a_uint8_cast(bad, dtype):
    from avlmaps_amd import ops
    from avlmaps_amd._lib import AvlError
    heat = np.full(300, 0.25, dtype=dtype)
    heat[173] = bad
    assert not (0 <= heat[173] <= 1)
    rgb = np.zeros((300, 3), np.uint8)
    with pytest.raises(AvlError, match="heat"):
        ops.colorize_heat(heat, rgb)
    with pytest.raises(AvlError, match="heat"):
        ops.colorize_heat(heat, rgb, as_uint8=True)
    with pytest.raises(TypeError):
        ops.colorize_heat(heat.astype(np.float16), rgb)


# ------------------------------------------------------------------ top-down
def ref_topdown(pos, heat, rgb, gs, window, t, table, background):
    """np.lexsort by (row, col, h) and a loop over the occupied cells: the highest voxel's colour, the column's largest heat"""
    rmin, rmax, cmin, cmax = window
    H, W = rmax - rmin + 1, cmax - cmin + 1
    out = np.empty((H, W, 3), np.uint8)
    out[:] = np.asarray(background, np.uint8)
    if len(pos) == 0:
        return out
    r, c, h = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64), pos[:, 2].astype(np.int64)
    r = np.where(r < 0, r + gs, r)
    c = np.where(c < 0, c + gs, c)
    assert r.min() >= 0 and r.max() < gs and c.min() >= 0 and c.max() < gs
    order = np.lexsort((h, c, r))
    cell = (r * gs + c)[order]
    starts = np.flatnonzero(np.concatenate([[True], cell[1:] != cell[:-1]]))
    ends = np.concatenate([starts[1:], [len(order)]])
    for s, e in zip(starts, ends):
        ids = order[s:e]
        rr, cc = int(r[ids[0]]), int(c[ids[0]])
        if not (rmin <= rr <= rmax and cmin <= cc <= cmax):
            continue
        top = ids[-1]                                                 # (row, col, h) is unique: the last of the group is the highest
        assert e - s == 1 or h[ids[-1]] > h[ids[-2]]
        hmax = heat[ids].max(keepdims=True)                           # stays an array of the heat's dtype
        idx = (hmax * 255).astype(np.uint8)
        val = table[idx].reshape(-1, 3).astype(np.float32) * t + rgb[top] * (1 - t)
        assert val.dtype == np.float64
        out[rr - rmin, cc - cmin] = val.astype(np.uint8)[0]
    return out


def topdown_case(gs, vh, seed, dtype, n_neg=1):
    """columns holding 1, 2 and vh voxels in shuffled id order, equal maximal heats inside a column, one wrapped negative position"""
    rng = np.random.default_rng(seed)
    cols = rng.permutation(gs * gs)[: max(6, gs * gs // 3)]
    pos = []
    for k, cell in enumerate(cols):
        n = (1, 2, vh)[k % 3]
        hs = rng.permutation(vh)[:n]
        pos += [(cell // gs, cell % gs, int(h)) for h in hs]
    pos = np.array(pos, dtype=np.int32)
    perm = rng.permutation(len(pos))
    pos = pos[perm]
    heat = rng.random(len(pos)).astype(dtype)
    # equal maximal heats inside the columns that hold several voxels
    key = pos[:, 0].astype(np.int64) * gs + pos[:, 1]
    for cell in np.unique(key)[::2]:
        ids = np.flatnonzero(key == cell)
        if len(ids) >= 2:
            heat[ids[:2]] = heat[ids].max()
    heat[0], heat[-1] = 0.0, 1.0
    for j in range(n_neg):                                            # row r is written as r - gs: NumPy's wrap
        pos[j, 0] -= gs
    rgb = rng.integers(0, 256, (len(pos), 3)).astype(np.uint8)
    return pos, heat, rgb


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("gs,vh", [(8, 5), (37, 9)])
def test_topdown_equals_the_sorted_oracle(gs, vh, dtype):
    from avlmaps_amd import ops
    pos, heat, rgb = topdown_case(gs, vh, gs + vh, dtype)
    assert (pos[:, 0] < 0).sum() == 1
    counts = np.unique(np.where(pos[:, 0] < 0, pos[:, 0] + gs, pos[:, 0]).astype(np.int64) * gs + pos[:, 1], return_counts=True)[1]
    assert {1, 2, vh} <= set(counts.tolist())
    for table, t, bg in ((ops.jet_table(), 0.5, (0, 0, 0)), (random_table(), 0.3, (9, 200, 31))):
        full = (0, gs - 1, 0, gs - 1)
        want = ref_topdown(pos, heat, rgb, gs, full, t, table, bg)
        got = ops.render_topdown(pos, heat, rgb, gs, transparency=t, table=table, background=bg)
        assert got.dtype == np.uint8 and got.shape == (gs, gs, 3) and np.array_equal(got, want)
        assert np.any(np.all(want == np.asarray(bg, np.uint8), axis=2)) and np.any(np.any(want != np.asarray(bg, np.uint8), axis=2))
        win = (1, gs - 3, 2, gs - 2)                                  # cuts the occupied area on all four sides
        got = ops.render_topdown(pos, heat, rgb, gs, window=win, transparency=t, table=table, background=bg)
        assert got.shape == (gs - 3, gs - 3, 3) and np.array_equal(got, want[1:gs - 2, 2:gs - 1])
        assert np.array_equal(got, ref_topdown(pos, heat, rgb, gs, win, t, table, bg))
        one = ops.render_topdown(pos, heat, rgb, gs, window=(3, 3, 4, 4), transparency=t, table=table, background=bg)
        assert one.shape == (1, 1, 3) and np.array_equal(one, want[3:4, 4:5])


def test_topdown_empty_map_and_bad_input():
    from avlmaps_amd import ops
    from avlmaps_amd._lib import AvlError
    img = ops.render_topdown(np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros((0, 3), np.uint8), 8, background=(1, 2, 3))
    assert img.shape == (8, 8, 3) and np.all(img == np.array([1, 2, 3], np.uint8))
    pos, heat, rgb = topdown_case(8, 5, 1, np.float32, n_neg=0)
    bad = pos.copy()
    bad[3, 1] = 8                                                     # a position equal to gs: IndexError upstream
    with pytest.raises(AvlError, match="outside"):
        ops.render_topdown(bad, heat, rgb, 8)
    bad = pos.copy()
    bad[3, 0] = -9                                                    # wraps once only
    with pytest.raises(AvlError, match="outside"):
        ops.render_topdown(bad, heat, rgb, 8)
    h2 = heat.copy()
    h2[5] = np.nan
    with pytest.raises(AvlError, match="heat"):
        ops.render_topdown(pos, h2, rgb, 8)
    with pytest.raises(AvlError):
        ops.render_topdown(pos, heat, rgb, 8, window=(0, 8, 0, 7))
    with pytest.raises(ValueError):
        ops.render_topdown(pos, heat[:-1], rgb, 8)


def test_topdown_200k_voxels_is_reproducible():
    from avlmaps_amd import ops
    rng = np.random.default_rng(64)
    gs, vh, N = 64, 64, 200_000
    flat = rng.permutation(gs * gs * vh)[:N]
    pos = np.stack([flat // (gs * vh), (flat // vh) % gs, flat % vh], axis=1).astype(np.int32)
    heat = rng.random(N).astype(np.float32)
    rgb = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    table = ops.jet_table()
    a = ops.render_topdown(pos, heat, rgb, gs, table=table)
    b = ops.render_topdown(pos, heat, rgb, gs, table=table)
    assert np.array_equal(a, b)
    assert np.array_equal(a, ref_topdown(pos, heat, rgb, gs, (0, gs - 1, 0, gs - 1), 0.5, table, (0, 0, 0)))


# ------------------------------------------------------------------ camera view
def view_footprints(pos, T, fx, fy, cx, cy, znear, smax):
    """the float64 expressions of the splat, in its operation order: (visible, float32 depth, unclipped pixel ranges)"""
    P = pos.astype(np.float64)
    row, col, h = P[:, 0], P[:, 1], P[:, 2]
    x = T[0, 0] * row + T[0, 1] * col + T[0, 2] * h + T[0, 3] * 1.0
    y = T[1, 0] * row + T[1, 1] * col + T[1, 2] * h + T[1, 3] * 1.0
    z = T[2, 0] * row + T[2, 1] * col + T[2, 2] * h + T[2, 3] * 1.0
    vis = z > znear
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * x / z + cx
        v = fy * y / z + cy
        half = np.minimum(0.5 * fx / z, 0.5 * smax)
        ulo, uhi, vlo, vhi = np.floor(u - half), np.floor(u + half), np.floor(v - half), np.floor(v + half)
    return vis, z.astype(np.float32), ulo, uhi, vlo, vhi


def ref_view(pos, color, T, fx, fy, cx, cy, size, znear, smax, background):
    """paints the voxels in descending (float32 z, id) order: the nearest is drawn last, an equal depth ends with the smaller id"""
    W, H = size
    img = np.empty((H, W, 3), np.uint8)
    img[:] = np.asarray(background, np.uint8)
    if len(pos) == 0:
        return img
    vis, z32, ulo, uhi, vlo, vhi = view_footprints(pos, np.asarray(T, np.float64), fx, fy, cx, cy, znear, smax)
    ids = np.arange(len(pos))
    for i in np.lexsort((ids, z32))[::-1]:
        if not vis[i] or not (uhi[i] >= 0 and ulo[i] <= W - 1 and vhi[i] >= 0 and vlo[i] <= H - 1):
            continue
        x0, x1 = int(max(ulo[i], 0)), int(min(uhi[i], W - 1))
        y0, y1 = int(max(vlo[i], 0)), int(min(vhi[i], H - 1))
        img[y0:y1 + 1, x0:x1 + 1] = color[i]
    return img


def view_scene(size, seed, n_random=1500):
    """a camera at the origin looking down +row (fx = fy = W / 2): random voxels in front, behind and beside it, plus by hand one
    behind the camera, one at z == znear exactly, one footprint cut by each image border, one entirely outside"""
    from avlmaps_amd.utils.visualize_utils import look_at
    W, H = size
    rng = np.random.default_rng(seed)
    T = look_at((0, 0, 0), (1, 0, 0), (0, 0, 1))
    special = np.array([(-5, 0, 0), (2, 0, 0), (4, 4, 0), (4, -4, 0), (4, 0, 3), (4, 0, -3), (10, 100, 0), (3, 0, 0)], np.int32)
    rnd = np.stack([rng.integers(-10, 60, n_random), rng.integers(-40, 41, n_random), rng.integers(-30, 31, n_random)], axis=1)
    pos = np.concatenate([special, rnd.astype(np.int32)])
    color = rng.integers(0, 256, (len(pos), 3)).astype(np.uint8)
    return pos, color, T, (W / 2.0, W / 2.0, W / 2.0, H / 2.0)


@pytest.mark.parametrize("smax", [1, 4, 64])
@pytest.mark.parametrize("size", [(16, 12), (64, 48)])
def test_view_equals_the_painter(size, smax):
    from avlmaps_amd import ops
    W, H = size
    pos, color, T, (fx, fy, cx, cy) = view_scene(size, W + smax)
    assert len(pos) <= 2000
    znear = 2.0
    vis, z32, ulo, uhi, vlo, vhi = view_footprints(pos, T, fx, fy, cx, cy, znear, smax)
    assert not vis[0] and not vis[1] and pos[1, 0] == znear            # behind the camera; z == znear exactly: both culled
    # voxels 2 .. 5 sit at z = 4 on the four image borders (u = 0, u = W, v = 0, v = H, exact in binary): each footprint is cut
    assert ulo[2] < 0 <= uhi[2] and ulo[3] <= W - 1 < uhi[3] and vlo[4] < 0 <= vhi[4] and vlo[5] <= H - 1 < vhi[5]
    assert vis[6] and uhi[6] < 0                                       # entirely left of the image
    if smax < fx / 3.0:                                                # voxel 7 at z = 3 would span fx / 3 pixels: capped
        assert uhi[7] - ulo[7] <= smax
    bg = (17, 0, 99)
    want = ref_view(pos, color, T, fx, fy, cx, cy, size, znear, smax, bg)
    got = ops.render_view(pos, color, T, fx, fy, cx, cy, size, znear=znear, smax=smax, background=bg)
    assert got.dtype == np.uint8 and got.shape == (H, W, 3) and np.array_equal(got, want)
    assert np.any(np.any(want != np.asarray(bg, np.uint8), axis=2))


def test_view_equal_float32_depth_goes_to_the_smaller_id():
    from avlmaps_amd import ops
    T = np.array([[0.0, 0.001, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 1e-9, 0.0, 0.0]])
    pos = np.array([(10, 1, 0), (10, 0, 0)], np.int32)                # z = 10 + 1e-9 and 10: id 1 is nearer in float64 ...
    color = np.array([(255, 0, 0), (0, 255, 0)], np.uint8)
    fx, fy, cx, cy = 8.0, 8.0, 8.0, 6.0
    vis, z32, ulo, uhi, vlo, vhi = view_footprints(pos, T, fx, fy, cx, cy, 0.5, 16)
    z64 = T[2, 0] * pos[:, 0] + T[2, 1] * pos[:, 1]
    assert z64[1] < z64[0] and z32[0] == z32[1]                        # ... and equal in float32
    assert (ulo[0], uhi[0], vlo[0], vhi[0]) == (ulo[1], uhi[1], vlo[1], vhi[1])
    got = ops.render_view(pos, color, T, fx, fy, cx, cy, (16, 12), znear=0.5, smax=16)
    assert np.array_equal(got, ref_view(pos, color, T, fx, fy, cx, cy, (16, 12), 0.5, 16, (0, 0, 0)))
    assert tuple(got[6, 8]) == (255, 0, 0) and not np.any(np.all(got == (0, 255, 0), axis=2))
    # the other way round: id 0 is the farther one in float32 too and loses
    pos2 = np.array([(11, 0, 0), (10, 0, 0)], np.int32)
    got = ops.render_view(pos2, color, T, fx, fy, cx, cy, (16, 12), znear=0.5, smax=16)
    assert tuple(got[6, 8]) == (0, 255, 0)
    assert np.array_equal(got, ref_view(pos2, color, T, fx, fy, cx, cy, (16, 12), 0.5, 16, (0, 0, 0)))


def test_view_empty_map_and_bad_input():
    from avlmaps_amd import ops
    from avlmaps_amd._lib import AvlError
    T = np.eye(4)[:3]
    img = ops.render_view(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8), T, 8, 8, 8, 6, (16, 12), background=(4, 5, 6))
    assert img.shape == (12, 16, 3) and np.all(img == np.array([4, 5, 6], np.uint8))
    pos, col = np.zeros((1, 3), np.int32), np.zeros((1, 3), np.uint8)
    for kw in (dict(size=(8193, 12)), dict(size=(16, 0)), dict(size=(16, 12), smax=0.5), dict(size=(16, 12), znear=-1.0)):
        with pytest.raises(AvlError):
            ops.render_view(pos, col, T, 8, 8, 8, 6, **kw)
    with pytest.raises(ValueError):
        ops.render_view(pos, col, np.eye(4), 8, 8, 8, 6, (16, 12))
    # a non-finite camera paints nothing and touches nothing outside the image
    Tn = T.copy()
    Tn[0, 3] = np.nan
    img = ops.render_view(np.array([(0, 0, 5)], np.int32), col + 200, Tn, 8, 8, 8, 6, (16, 12))
    assert not img.any()
    img = ops.render_view(np.array([(0, 0, 5)], np.int32), col + 200, T, 8, 8, 8, 6, (16, 12))
    assert img.any()


def test_view_50k_voxels_is_reproducible():
    from avlmaps_amd import ops
    from avlmaps_amd.utils.visualize_utils import look_at
    rng = np.random.default_rng(50)
    N, size = 50_000, (128, 96)
    pos = np.stack([rng.integers(0, 200, N), rng.integers(0, 200, N), rng.integers(0, 40, N)], axis=1).astype(np.int32)
    color = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    T = look_at((-30.0, 100.5, 60.25), (100.0, 100.0, 10.0))
    a = ops.render_view(pos, color, T, 64.0, 64.0, 64.0, 48.0, size, znear=1.0, smax=8)
    b = ops.render_view(pos, color, T, 64.0, 64.0, 64.0, 48.0, size, znear=1.0, smax=8)
    assert np.array_equal(a, b)
    assert np.array_equal(a, ref_view(pos, color, T, 64.0, 64.0, 64.0, 48.0, size, 1.0, 8, (0, 0, 0)))
    assert np.any(a)


# ------------------------------------------------------------------ API
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the small synthetic map of the multimodal GPU tests (their construction, copied)"""
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map
    from avlmaps_amd.apps.common import HashImageEncoder, load_config
    from avlmaps_amd.map.area_map import AreaMap
    tmp = tmp_path_factory.mktemp("render")
    sc = make(tmp / "scene", frames=8, H=96, W=128)
    cfg_path = tmp / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                       "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(sc), "--config", str(cfg_path), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    AreaMap().create_map(sc, image_encoder=HashImageEncoder())
    return sc, cfg_path, load_config(str(cfg_path))


def _avlmap(scene):
    from avlmaps_amd.apps.common import HashAudioText, HashClip
    from avlmaps_amd.map import AVLMap
    sc, _, cfg = scene
    av = AVLMap(cfg, data_dir=str(sc), area_text_model=HashClip(768), audio_text_model=HashAudioText())
    assert av.load_map(str(sc))
    return av


def test_render_heat_equals_the_ops_on_host_arrays(scene):
    from avlmaps_amd import ops
    from avlmaps_amd.utils.visualize_utils import camera_of_frame, frame_intrinsics
    av = _avlmap(scene)
    vm = av.vlmap
    N = len(vm.grid_pos)
    heat = np.random.default_rng(2).random(N).astype(np.float32)
    top = av.render_heat(heat)
    assert top.dtype == np.uint8 and top.shape == (400, 400, 3)
    assert np.array_equal(top, ops.render_topdown(vm.grid_pos, heat, vm.grid_rgb, vm.gs))
    assert np.array_equal(top, ref_topdown(np.asarray(vm.grid_pos, np.int32), heat, np.asarray(vm.grid_rgb).astype(np.uint8), vm.gs,
                                           (0, 399, 0, 399), 0.5, ops.jet_table(), (0, 0, 0)))
    size = (128, 96)
    view = av.render_heat(heat.astype(np.float64), view="frame:0", size=size, transparency=0.3)
    color = ops.colorize_heat(heat.astype(np.float64), vm.grid_rgb, 0.3, as_uint8=True)
    want = ops.render_view(vm.grid_pos, color, camera_of_frame(vm, 0), *frame_intrinsics(size), size)
    assert view.shape == (96, 128, 3) and np.array_equal(view, want)
    # the camera that took frame 0 sees the voxels it made: a wrong pose shows nothing or a sliver
    assert np.mean(np.any(view != 0, axis=2)) > 0.05
    orbit = av.render_heat(heat, view="orbit", size=size)
    assert orbit.shape == (96, 128, 3) and np.any(orbit)
    with pytest.raises(ValueError):
        av.render_heat(heat, view="sideways")


def test_visualize_heatmap_3d_writes_the_truncated_colours(tmp_path):
    from avlmaps_amd import ops
    from avlmaps_amd.utils import visualize_utils as vu
    rng = np.random.default_rng(3)
    N = 1000
    pc = rng.integers(0, 400, (N, 3)).astype(np.int32)
    heat = rng.random(N).astype(np.float32)
    rgb = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    vu.visualize_heatmap_3d(pc, heat, rgb, 0.4, save_path=tmp_path / "heat.ply")
    pts, col = vu.read_ply(tmp_path / "heat.ply")
    heat_rgb = upstream_convert_heatmap_to_rgb(heat, rgb, 0.4, ops.jet_table())
    assert np.array_equal(pts, pc) and np.array_equal(col, np.clip((heat_rgb / 255.0) * 255.0, 0, 255).astype(np.uint8))
    assert np.array_equal(vu.convert_heatmap_to_rgb(heat, rgb, 0.4), heat_rgb)
    mask = heat > 0.5
    vu.visualize_masked_map_3d(pc, mask, rgb, save_path=tmp_path / "mask.ply")
    want = upstream_convert_heatmap_to_rgb(mask.astype(np.float16), rgb, 0.5, ops.jet_table())      # upstream's float16 heat
    assert np.array_equal(vu.read_ply(tmp_path / "mask.ply")[1], np.clip((want / 255.0) * 255.0, 0, 255).astype(np.uint8))


def test_visualize_heatmap_2d_writes_the_blend(tmp_path):
    from PIL import Image
    from avlmaps_amd import ops
    from avlmaps_amd.utils import visualize_utils as vu
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, (13, 17, 3)).astype(np.uint8)
    heat = rng.random((13, 17)).astype(np.float32)
    table = ops.jet_table()
    # visualize_utils.py:124-128 and :111, with the table lookup for cv2.applyColorMap
    sim_new = (heat * 255).astype(np.uint8)
    h = table[sim_new].astype(np.float32)
    want = (h * 0.5 + rgb * (1 - 0.5)).astype(np.uint8)
    got = vu.visualize_heatmap_2d(rgb, heat, save_path=tmp_path / "h.png")
    assert np.array_equal(got, want) and np.array_equal(np.asarray(Image.open(tmp_path / "h.png")), want)
    mask = (heat > 0.5).astype(np.uint8)
    got = vu.visualize_masked_map_2d(rgb, mask, save_path=tmp_path / "m.png")
    want = (table[(mask.astype(np.float32) * 255).astype(np.uint8)].astype(np.float32) * 0.5 + rgb * (1 - 0.5)).astype(np.uint8)
    assert np.array_equal(got, want)


def test_pool_3d_rgb_to_2d_equals_upstreams_loop():
    from avlmaps_amd.utils.visualize_utils import pool_3d_rgb_to_2d
    rng = np.random.default_rng(5)
    gs, N = 20, 500
    grid_pos = np.stack([rng.integers(0, gs, N), rng.integers(0, gs, N), rng.integers(0, 30, N)], axis=1).astype(np.int32)
    rgb = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    # visualize_utils.py:86-94: `height` is never updated
    rgb_2d = np.zeros((gs, gs, 3), dtype=np.uint8)
    height = -100 * np.ones((gs, gs), dtype=np.int32)
    for i, pos in enumerate(grid_pos):
        row, col, h = pos
        if h > height[row, col]:
            rgb_2d[row, col] = rgb[i]
    assert np.array_equal(pool_3d_rgb_to_2d(rgb, grid_pos, gs), rgb_2d)


def test_index_map_writes_the_picture_and_the_cloud(scene, tmp_path):
    from PIL import Image
    from avlmaps_amd.apps import index_map
    from avlmaps_amd.utils.visualize_utils import read_ply
    sc, cfg_path, _ = scene
    av = _avlmap(scene)
    base = ["--data-dir", str(sc), "--config", str(cfg_path), "--text-model", "hash", "--modality", "area", "--query", "kitchen"]
    heat = index_map.main(base + ["--render", str(tmp_path / "top.png"), "--save-ply", str(tmp_path / "k.ply")])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "top.png")), av.render_heat(heat))
    pts, col = read_ply(tmp_path / "k.ply")
    assert np.array_equal(pts, av.vlmap.grid_pos) and col.shape == (len(heat), 3)
    index_map.main(base + ["--render", str(tmp_path / "f.png"), "--view", "frame:2", "--render-size", "64", "48"])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "f.png")), av.render_heat(heat, view="frame:2", size=(64, 48)))


def test_plan_path_draws_the_plan(scene, tmp_path):
    from PIL import Image
    from avlmaps_amd.apps import plan_path
    from avlmaps_amd.navigator import NoPathError
    sc, cfg_path, cfg = scene
    from avlmaps_amd.map import VLMap
    vm = VLMap(cfg.map_config, data_dir=str(sc))
    assert vm.load_map(str(sc))
    vm.generate_obstacle_map()
    obstacles = vm.get_obstacle_cropped()
    H, W = obstacles.shape
    # the drawing itself, on a hand-made plan
    start, goal = (vm.rmin + 1.0, vm.cmin + 1.0), (vm.rmin + H - 2.0, vm.cmin + W - 2.0)
    path = [start, (vm.rmin + 1.0, vm.cmin + W - 2.0), goal]
    img = plan_path.render_plan(vm, obstacles, start, goal, path)
    base_img = vm.generate_rgb_topdown_map()[vm.rmin:vm.rmin + H, vm.cmin:vm.cmin + W]
    want = base_img.copy()
    want[obstacles == 0] = want[obstacles == 0] // 3
    drawn = np.any(img != want, axis=2)
    assert img.shape == (H, W, 3) and tuple(img[1, 1]) == (0, 255, 0) and tuple(img[H - 2, W - 2]) == (255, 0, 0)
    assert tuple(img[1, W // 2]) == (255, 255, 0) and tuple(img[H // 2, W - 2]) == (255, 255, 0)
    assert drawn.sum() <= (W + H) + 50 and np.array_equal(img[~drawn], want[~drawn])
    # end to end: the first free start cell the planner finds a path from
    free = np.argwhere(obstacles)
    base = ["--data-dir", str(sc), "--config", str(cfg_path), "--text-model", "hash", "--query", "sofa", "--render", str(tmp_path / "p.png")]
    out = None
    for r, c in free[:: max(1, len(free) // 8)]:
        try:
            out = plan_path.main(base + ["--start", str(float(r + vm.rmin)), str(float(c + vm.cmin))])
            break
        except NoPathError:
            continue
    assert out is not None and out["render"] == str(tmp_path / "p.png")
    png = np.asarray(Image.open(tmp_path / "p.png"))
    assert png.shape == (H, W, 3) and np.any(np.all(png == (255, 0, 0), axis=2)) and np.any(np.all(png == (0, 255, 0), axis=2))
