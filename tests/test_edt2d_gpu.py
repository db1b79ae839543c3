"""The exact 2-D distance transform and the 2-D goal maps on the GPU (csrc/avl_edt2d.hip, the float32 gaussian of
csrc/avl_morph2d.hip and the window product of csrc/avl_goal.hip, through ops.distance_transform_edt, mask_decay_2d,
gaussian_filter2d_f32, product_argmax_2d, and their users get_heatmap_from_mask_2d, VLMap.get_predict_mask / get_distribution_map,
Map.get_max_pos, AVLMap.index_goal_2d and apps.plan_path --goal-2d) against SciPy and NumPy, called the way upstream calls them
(robot/habitat_lang_robot.py:229-240, 357-375, 419-425; utils/visualize_utils.py:97-102; map/vlmap_3d.py:75-81).

Every comparison is np.array_equal: the squared distance between integer cells is an exact integer, sqrt and the divisions are
correctly rounded, and the float32 gaussian rounds where SciPy rounds."""
import json
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy.ndimage import distance_transform_edt, gaussian_filter

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tools"))


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


# ------------------------------------------------------------------ inputs
def scene(seed, H, W):
    """rectangular rooms with axis-aligned walls 1-3 cells thick, one-cell gaps in them, blobs touching all four image edges and
    1 % salt noise -> (H, W) bool (the recipe of the morphology tests, restated)"""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), bool)
    for _ in range(max(1, (H * W) // 20000 + 2)):
        h, w = int(rng.integers(max(2, H // 6), max(3, H // 2 + 1))), int(rng.integers(max(2, W // 6), max(3, W // 2 + 1)))
        r, c = int(rng.integers(0, max(1, H - h))), int(rng.integers(0, max(1, W - w)))
        t = int(rng.integers(1, 4))
        room = np.zeros((H, W), bool)
        room[r:r + h, c:c + w] = True
        room[r + t:max(r + t, r + h - t), c + t:max(c + t, c + w - t)] = False
        for _gap in range(3):
            if rng.random() < 0.5:
                rr = min(int(rng.integers(r, r + h)), H - 1)
                room[rr, c:c + t] = False
            else:
                cc = min(int(rng.integers(c, c + w)), W - 1)
                room[r:r + t, cc] = False
        m |= room
    bh, bw = max(1, H // 10), max(1, W // 10)
    m[:bh, W // 3:W // 3 + bw] = True
    m[H - bh:, W // 2:W // 2 + bw] = True
    m[H // 3:H // 3 + bh, :bw] = True
    m[H // 2:H // 2 + bh, W - bw:] = True
    m |= rng.random((H, W)) < 0.01
    return m


def one(H, W, r, c):
    m = np.zeros((H, W), bool)
    m[r, c] = True
    return m


def masks():
    """(name, m): m marks the features, the transform is called on m == 0 as upstream calls it"""
    rng = np.random.default_rng(7)
    S = 1000
    out = [("all_features", np.ones((37, 52), bool)),
           ("corner_00", one(S, S, 0, 0)), ("corner_0W", one(S, S, 0, S - 1)), ("corner_H0", one(S, S, S - 1, 0)),
           ("corner_HW", one(S, S, S - 1, S - 1)), ("centre", one(S, S, S // 2, S // 2)),
           ("1x1", np.ones((1, 1), bool)), ("1x77", scene(1, 1, 77)), ("64x1", scene(2, 64, 1)), ("61x95", scene(3, 61, 95)),
           ("128x200", scene(4, 128, 200)), ("300x1700", scene(5, 300, 1700)), ("rooms_1000", scene(11, S, S)),
           ("sparse_0.1%", rng.random((S, S)) < 0.001), ("dense_50%", rng.random((700, 900)) < 0.5)]
    for name, m in out:
        assert m.any(), name                                   # m == 0 has a zero cell
    return out


@pytest.fixture(scope="module")
def cases():
    return masks()


# ------------------------------------------------------------------ the transform
def test_edt_equals_scipy(ops, cases):
    for name, m in cases:
        want = distance_transform_edt(m == 0)
        got = ops.distance_transform_edt(m == 0)
        bad = int((got != want).sum())
        print(f"{name}: {m.shape}, differing cells {bad}, max |diff| {float(np.abs(got - want).max()):.3e}")
        assert got.dtype == np.float64 and got.shape == m.shape and np.array_equal(got, want), (name, bad)


def test_edt_device_in_and_out(ops, cases):
    from avlmaps_amd.device import DeviceArray
    for name, m in cases:
        dev = ops.distance_transform_edt(DeviceArray.from_numpy((m == 0).astype(np.uint8)), device=True)
        assert isinstance(dev, DeviceArray) and dev.dtype == np.float64 and dev.shape == m.shape
        assert np.array_equal(dev.numpy(), distance_transform_edt(m == 0)), name


def test_edt_takes_numeric_images_like_scipy(ops):
    rng = np.random.default_rng(3)
    x = rng.integers(0, 3, (90, 70)) * 0.5                     # float64 with zeros: nonzero = true
    assert np.array_equal(ops.distance_transform_edt(x), distance_transform_edt(x))
    assert np.array_equal(ops.distance_transform_edt(x.astype(np.int32)), distance_transform_edt(x.astype(np.int32)))


def test_edt_without_a_zero_cell_is_a_value_error(ops):
    from avlmaps_amd.device import DeviceArray
    for shape in ((1, 1), (40, 33), (300, 1000)):
        with pytest.raises(ValueError, match="no zero cell"):
            ops.distance_transform_edt(np.ones(shape, bool))
    with pytest.raises(ValueError, match="no zero cell"):
        ops.distance_transform_edt(DeviceArray.from_numpy(np.full((20, 20), 7, np.uint8)), device=True)


def test_edt_side_limit_is_an_argument_error(ops):
    from avlmaps_amd import _lib
    for shape in ((16385, 1), (1, 16385)):
        with pytest.raises(_lib.AvlError, match="bad shape"):
            ops.distance_transform_edt(np.zeros(shape, bool))
    m = np.ones((1, 16384), bool)                              # the largest side: distances up to 16383
    m[0, 0] = False
    assert np.array_equal(ops.distance_transform_edt(m), distance_transform_edt(m))
    assert np.array_equal(ops.distance_transform_edt(m.T), distance_transform_edt(m.T))


# ------------------------------------------------------------------ the float32 gaussian
def test_gaussian_f32_has_scipys_float32_bits(ops, cases):
    rng = np.random.default_rng(9)
    imgs = [(n, m) for n, m in cases if n in ("1x1", "1x77", "64x1", "61x95", "128x200", "300x1700", "rooms_1000", "dense_50%")]
    imgs.append(("random_200x300", rng.random((200, 300)) < 0.4))
    for name, m in imgs:
        want = gaussian_filter(m.astype(np.float32), sigma=1)
        got, gt = ops.gaussian_filter2d_f32(m, 1, threshold=0.5)
        assert want.dtype == np.float32 and got.dtype == np.float32
        assert np.array_equal(got, want), (name, float(np.abs(got.astype(np.float64) - want).max()))
        assert gt.dtype == bool and np.array_equal(gt, want > 0.5), name
    for sigma in (0.8, 2.3):
        x = rng.random((97, 130)).astype(np.float32)           # a float32 image, not a mask
        assert np.array_equal(ops.gaussian_filter2d_f32(x, sigma), gaussian_filter(x, sigma=sigma)), sigma
    m = imgs[-1][1]
    assert not np.array_equal(gaussian_filter(m.astype(np.float32), sigma=1).astype(np.float64), gaussian_filter(m.astype(float), sigma=1))


# ------------------------------------------------------------------ the decay maps
def ref_heatmap_2d(mask, cell_size, decay_rate):
    """visualize_utils.py:98-100"""
    dists = distance_transform_edt(mask == 0) / cell_size
    tmp = np.ones_like(dists) - (dists * decay_rate)
    return np.where(tmp < 0, np.zeros_like(tmp), tmp)


def ref_distribution(predict_mask, decay_rate):
    """habitat_lang_robot.py:231-236"""
    predict_mask = predict_mask.astype(np.float32)
    predict_mask = (gaussian_filter(predict_mask, sigma=1) > 0.5).astype(np.float32)
    dists = distance_transform_edt(predict_mask == 0)
    tmp = np.ones_like(dists) - (dists * decay_rate)
    dist_map = np.where(tmp < 0, np.zeros_like(tmp), tmp)
    return (dist_map - np.min(dist_map)) / (np.max(dist_map) - np.min(dist_map))


def test_get_heatmap_from_mask_2d_equals_numpy(ops, cases):
    from avlmaps_amd.utils.visualize_utils import get_heatmap_from_mask_2d
    for name, m in cases:
        for cs, rate in ((0.05, 0.01), (0.05, 0.1), (0.03, 0.0007)):
            got = get_heatmap_from_mask_2d(m, cell_size=cs, decay_rate=rate)
            assert got.dtype == np.float64 and np.array_equal(got, ref_heatmap_2d(m, cs, rate)), (name, cs, rate)
    m = cases[9][1]
    assert np.array_equal(get_heatmap_from_mask_2d(m.astype(np.uint8)), ref_heatmap_2d(m, 0.05, 0.01))      # the defaults
    with pytest.raises(ValueError, match="no target"):
        get_heatmap_from_mask_2d(np.zeros((30, 40), bool))


def test_mask_decay_normalised_equals_the_robots_lines(ops, cases):
    from avlmaps_amd.device import DeviceArray
    for name, m in cases:
        if m.all():
            continue                                           # constant map: below
        for rate in (0.1, 0.01):
            dists = distance_transform_edt(m == 0)
            tmp = np.ones_like(dists) - (dists * rate)
            want = np.where(tmp < 0, np.zeros_like(tmp), tmp)
            want = (want - np.min(want)) / (np.max(want) - np.min(want))
            got = ops.mask_decay_2d(m, rate, normalize=True)
            assert np.array_equal(got, want), (name, rate, int((got != want).sum()))
    for name, m in cases[9:13]:                                # with the float32 smoothing in front, host and device input
        if min(m.shape) < 2:
            continue
        want = ref_distribution(m, 0.1)
        assert np.array_equal(ops.mask_decay_2d(m, 0.1, normalize=True, smooth_sigma=1), want), name
        dev = ops.mask_decay_2d(DeviceArray.from_numpy(m.astype(np.uint8)), 0.1, normalize=True, smooth_sigma=1, device=True)
        assert isinstance(dev, DeviceArray) and np.array_equal(dev.numpy(), want), name
    big = cases[12][1]                                         # a window of a larger mask, read in place
    r0, r1, c0, c1 = 123, 724, 250, 951
    assert np.array_equal(ops.mask_decay_2d(big, 0.03, normalize=True, smooth_sigma=1, window=(r0, r1, c0, c1)),
                          ref_distribution(big[r0:r1, c0:c1], 0.03))
    with pytest.raises(ValueError, match="constant"):
        ops.mask_decay_2d(np.ones((20, 30), bool), 0.1, normalize=True)
    with pytest.raises(ValueError, match="no target"):
        ops.mask_decay_2d(np.zeros((20, 30), bool), 0.1, normalize=True)
    with pytest.raises(ValueError, match="after the smoothing"):
        ops.mask_decay_2d(one(20, 30, 5, 5), 0.1, normalize=True, smooth_sigma=1)      # a lone cell peaks at 0.16 < 0.5


# ------------------------------------------------------------------ the product and its first maximum
def test_product_argmax_2d_equals_numpy(ops):
    from avlmaps_amd.device import DeviceArray
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (7, 300), (301, 257), (600, 700)):
        parts = [rng.random((h, w)) * 1.5, rng.random((h, w)).astype(np.float32), rng.random((h, w)), rng.random((h, w)).astype(np.float32)]
        for K in (1, 2, 4):
            want = parts[0].astype(np.float64)
            for p in parts[1:K]:
                want = want * p.astype(np.float64)
            res = ops.product_argmax_2d(parts[:K])
            assert np.array_equal(res.heat.numpy(), want) and res.heat.dtype == np.float64
            assert res.cell == tuple(int(v) for v in np.unravel_index(np.argmax(want), want.shape)) and res.value == want.max()
            lean = ops.product_argmax_2d(parts[:K], want_heat=False)
            assert lean.heat is None and (lean.cell, lean.value) == (res.cell, res.value)
    # eight terms; windows of larger device images, float32 and float64, read in place
    full64, full32 = rng.random((400, 500)), rng.random((400, 500)).astype(np.float32)
    r0, r1, c0, c1 = 17, 318, 40, 497
    terms = [ops.Window(DeviceArray.from_numpy(full64), r0, r1, c0, c1), ops.Window(full32, r0, r1, c0, c1)] + \
            [rng.random((r1 - r0, c1 - c0)) for _ in range(6)]
    want = full64[r0:r1, c0:c1] * full32[r0:r1, c0:c1].astype(np.float64)
    for t in terms[2:]:
        want = want * t
    res = ops.product_argmax_2d(terms)
    assert np.array_equal(res.heat.numpy(), want) and res.cell == tuple(int(v) for v in np.unravel_index(np.argmax(want), want.shape))
    # ties: the first maximum in raster order, wherever the workgroups split the image
    x = (rng.random((513, 777)) * 0.5).astype(np.float32)
    for r, c in ((512, 776), (300, 5), (299, 776), (300, 4), (77, 700)):
        x[r, c] = 1.0
    res = ops.product_argmax_2d([x], want_heat=False)
    assert res.cell == (77, 700) == tuple(int(v) for v in np.unravel_index(np.argmax(x), x.shape)) and res.value == 1.0
    z = ops.product_argmax_2d([np.zeros((40, 50)), x[:40, :50]])
    assert z.cell == (0, 0) and z.value == 0.0


# ------------------------------------------------------------------ VLMap / AVLMap on a synthetic map
CATS = ["sofa", "table", "lamp", "other"]              # "lamp" wins on no voxel


@pytest.fixture(scope="module")
def avmap(tmp_path_factory):
    """An AVLMap over a synthetic scene with its area and sound maps (the recipe of the cross-modal goal tests), whose voxels and
    scores_mat are then preset: dense blobs for "sofa" and "table" inside the obstacle crop, "table" voxels outside the crop as well
    (they are dropped), lone "table" columns (the smoothing removes them), several voxels per column."""
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map
    from avlmaps_amd.apps.common import HashAudioText, HashClip, HashImageEncoder, load_config
    from avlmaps_amd.map import AVLMap
    from avlmaps_amd.map.area_map import AreaMap
    tmp = tmp_path_factory.mktemp("edt2d")
    sc = make(tmp / "scene", frames=8, H=96, W=128)
    cfg_path = tmp / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                       "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(sc), "--config", str(cfg_path), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    AreaMap().create_map(sc, image_encoder=HashImageEncoder())
    rng = np.random.default_rng(11)
    db = {i: {"audio_features": rng.standard_normal(1024).astype(np.float32),
              "locations": [np.array([rng.uniform(-1.5, 1.5), 0.0, rng.uniform(-1.5, 1.5)]) for _ in range(1 + i % 5)]}
          for i in range(14)}
    (sc / "audio_video").mkdir()
    (sc / "audio_video" / "audio_data_level_3.pkl").write_bytes(pickle.dumps(db))
    av = AVLMap(load_config(str(cfg_path)), data_dir=str(sc), area_text_model=HashClip(768), audio_text_model=HashAudioText())
    assert av.load_map(str(sc))
    vm = av.vlmap
    vm.clip_feat_dim = vm.grid_feat.shape[1]
    vm.clip_model = HashClip(vm.clip_feat_dim)
    vm.generate_obstacle_map()
    h, w = vm.obstacles_cropped.shape
    assert h >= 24 and w >= 24, (h, w)
    r0, c0 = int(vm.rmin), int(vm.cmin)

    def block(ra, rb, ca, cb, heights):
        rr, cc, hh = np.meshgrid(np.arange(ra, rb), np.arange(ca, cb), np.asarray(heights), indexing="ij")
        return np.stack([rr.ravel(), cc.ravel(), hh.ravel()], 1)
    sofa = [block(r0 + h // 8, r0 + h // 8 + max(5, h // 6), c0 + w // 8, c0 + w // 8 + max(6, w // 5), [3, 9])]
    table = [block(r0 + h // 2, r0 + h // 2 + max(5, h // 5), c0 + w // 2, c0 + w // 2 + max(5, w // 6), [5]),
             block(max(r0 - 6, 0), r0 + 3, c0 + 2, c0 + 9, [4]),                     # straddles the crop's top edge
             np.array([[r0 + 2, c0 + w - 3, 6], [r0 + h - 2, c0 + 1, 2]])]           # lone columns
    other = [block(r0, r0 + h, c0, c0 + w, [0])[::7]]
    pos = np.concatenate(sofa + table + other).astype(np.int32)
    label = np.concatenate([np.full(sum(len(b) for b in sofa), 0), np.full(sum(len(b) for b in table), 1),
                            np.full(sum(len(b) for b in other), 3)])
    order = rng.permutation(len(pos))
    pos, label = pos[order], label[order]
    scores = rng.random((len(pos), len(CATS))).astype(np.float32) * 0.5
    scores[np.arange(len(pos)), label] = 1.0
    scores[:, 2] = -1.0
    vm.grid_pos, vm.categories, vm.scores_mat = pos, list(CATS), scores
    return av, sc, cfg_path


def scatter_mask(vm, cat_id):
    """vlmap_3d.py:75-81 as a Python loop; voxels outside the crop are dropped"""
    mask = np.zeros_like(vm.obstacles_cropped)
    ids = np.argmax(vm.scores_mat, axis=1) == cat_id
    for (row, col, _), hit in zip(vm.grid_pos, ids):
        r, c = int(row) - int(vm.rmin), int(col) - int(vm.cmin)
        if hit and 0 <= r < mask.shape[0] and 0 <= c < mask.shape[1]:
            mask[r, c] = 1
    return mask


def test_get_predict_mask_equals_a_python_scatter(ops, avmap):
    vm = avmap[0].vlmap
    for cat_id, name in enumerate(CATS):
        got = vm.get_predict_mask(name)
        want = scatter_mask(vm, cat_id)
        assert got.dtype == vm.obstacles_cropped.dtype and got.shape == vm.obstacles_cropped.shape
        assert np.array_equal(got, want), name
        assert want.any() == (name != "lamp")
    outside = vm.grid_pos[:, 0] < vm.rmin
    assert (outside & (np.argmax(vm.scores_mat, axis=1) == 1)).any()         # the fixture has "table" voxels outside the crop


def test_get_distribution_map_equals_the_chain(ops, avmap):
    vm = avmap[0].vlmap
    for name in ("sofa", "table"):
        for rate in (0.1, 0.01):
            got = vm.get_distribution_map(name, decay_rate=rate)
            want = ref_distribution(vm.get_predict_mask(name), rate)
            assert got.dtype == np.float64 and got.shape == vm.obstacles_cropped.shape
            assert np.array_equal(got, want), (name, rate, int((got != want).sum()))
            assert got.max() == 1.0 and got.min() == 0.0
    assert np.array_equal(vm.get_distribution_map("sofa"), ref_distribution(vm.get_predict_mask("sofa"), 0.1))   # the default rate
    # the lone "table" columns are in the predicted mask and gone after the smoothing
    pm = vm.get_predict_mask("table")
    sm = gaussian_filter(pm.astype(np.float32), sigma=1) > 0.5
    assert pm[2, pm.shape[1] - 3] and not sm[2, pm.shape[1] - 3]


def test_a_category_without_a_voxel_is_a_value_error(ops, avmap):
    av = avmap[0]
    with pytest.raises(ValueError, match="no target"):
        av.vlmap.get_distribution_map("lamp")
    with pytest.raises(ValueError, match="no target"):
        av.index_goal_2d(obj="lamp", sound="dog")
    saved = av.vlmap.scores_mat
    av.vlmap.scores_mat = None
    try:
        with pytest.raises(Exception, match="not preloaded"):
            av.vlmap.get_predict_mask("sofa")
    finally:
        av.vlmap.scores_mat = saved


def test_get_max_pos_is_argmax_plus_the_crop_offset(ops, avmap):
    vm = avmap[0].vlmap
    rng = np.random.default_rng(2)
    h, w = vm.obstacles_cropped.shape
    for m in (rng.random((h, w)), rng.random((h, w)).astype(np.float32), vm.get_distribution_map("sofa")):
        r, c = np.unravel_index(np.argmax(m), m.shape)
        assert tuple(vm.get_max_pos(m)) == (r + vm.rmin, c + vm.cmin)
    tied = (rng.random((h, w)) * 0.5)
    for r, c in ((h - 1, w - 1), (h // 2, 3), (h // 2, 2), (h // 3, w - 2)):
        tied[r, c] = 2.0
    assert tuple(vm.get_max_pos(tied)) == (h // 3 + vm.rmin, w - 2 + vm.cmin)
    sofa = vm.get_distribution_map("sofa")                     # a plateau of ones: the first cell of the smoothed mask
    r, c = np.unravel_index(np.argmax(sofa), sofa.shape)
    assert (sofa == 1.0).sum() > 1 and tuple(vm.get_max_pos(sofa)) == (r + vm.rmin, c + vm.cmin)


def test_index_goal_2d_equals_the_product_of_the_stand_alone_calls(ops, avmap):
    av = avmap[0]
    vm = av.vlmap
    win = (slice(int(vm.rmin), int(vm.rmax) + 1), slice(int(vm.cmin), int(vm.cmax) + 1))
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    combos = [
        (dict(obj="sofa"), lambda: [vm.get_distribution_map("sofa", 0.1)]),
        (dict(obj="sofa", sound="dog"), lambda: [vm.get_distribution_map("sofa", 0.1), av.index_sound_2d("dog")[win]]),
        (dict(obj="table", area="kitchen"), lambda: [vm.get_distribution_map("table", 0.1), av.index_area_2d("kitchen")[win]]),
        (dict(area="kitchen", sound="dog"), lambda: [av.index_area_2d("kitchen")[win], av.index_sound_2d("dog")[win]]),
        (dict(obj=["sofa", ("table", 0.01)], area=[("kitchen", 0.02), "bedroom"], sound="clock tick", decay_rates={"sound": 0.05}),
         lambda: [vm.get_distribution_map("sofa", 0.1), vm.get_distribution_map("table", 0.01), av.index_area_2d("kitchen", 0.02)[win],
                  av.index_area_2d("bedroom")[win], av.index_sound_2d("clock tick", 0.05)[win]]),
    ]
    for kwargs, parts in combos:
        parts = parts()
        want = f64(parts[0])
        for p in parts[1:]:
            want = want * f64(p)
        goal = av.index_goal_2d(**kwargs)
        assert goal.heat.dtype == np.float64 and goal.heat.shape == vm.obstacles_cropped.shape
        assert np.array_equal(goal.heat, want), kwargs
        r, c = np.unravel_index(np.argmax(want), want.shape)
        assert goal.cell.tolist() == [r + vm.rmin, c + vm.cmin] and goal.value == want[r, c]
        assert tuple(goal.cell) == tuple(vm.get_max_pos(want))
        lean = av.index_goal_2d(want_heat=False, **kwargs)
        assert lean.heat is None and lean.cell.tolist() == goal.cell.tolist() and lean.value == goal.value
    with pytest.raises(ValueError, match="at least one"):
        av.index_goal_2d()
    with pytest.raises(KeyError):
        av.index_goal_2d(obj="sofa", sound="zebra")


def test_plan_path_goal_2d(ops, avmap, capsys, monkeypatch):
    """--goal-2d hands AVLMap.index_goal_2d's cell to the planner; the default path does not call it"""
    from avlmaps_amd.apps import plan_path
    from avlmaps_amd.map import AVLMap, Goal2D
    from avlmaps_amd.navigator import Navigator
    from avlmaps_amd.utils.navigation_utils import NoPathError
    av, sc, cfg_path = avmap
    vm = av.vlmap
    free = np.argwhere(vm.obstacles_cropped) + np.array([vm.rmin, vm.cmin])
    nav = Navigator()
    nav.build_visgraph(vm.obstacles_cropped, vm.rmin, vm.cmin)
    found = None
    for k in range(0, len(free), max(1, len(free) // 40)):          # two free cells the planner connects
        a, b = free[k], free[(k + len(free) // 2) % len(free)]
        try:
            path = nav.plan_to([float(a[0]), float(a[1])], [float(b[0]), float(b[1])])
            if len(path) >= 2:
                found = (a, b, path)
                break
        except NoPathError:
            continue
    nav.close()
    assert found is not None, "no pair of free cells is connected"
    a, b, path = found
    seen = {}

    def fake(self, **kw):
        seen.update(kw)
        return Goal2D(None, 0.75, (int(b[0]), int(b[1])))
    monkeypatch.setattr(AVLMap, "index_goal_2d", fake)
    out = plan_path.main(["--data-dir", str(sc), "--config", str(cfg_path), "--text-model", "hash", "--query", "table", "--sound", "dog",
                          "--goal-2d", "--start", str(float(a[0])), str(float(a[1]))])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert seen == dict(obj="table", area=None, sound=["dog"], want_heat=False)
    assert out["goal"] == out["goal_cell"] == [float(b[0]), float(b[1])] and out["goal_value"] == 0.75
    assert out["path"] == [[float(p[0]), float(p[1])] for p in path] and "goal_voxel" not in out
