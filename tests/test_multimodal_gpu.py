"""Area, sound and image goal queries on the GPU (csrc/avl_field2d.hip through ops and AVLMap) against a NumPy + SciPy restatement
of the reference's loops (avlmaps/map/avlmap.py:78-163): one distance_transform_edt per pose or segment, the occupied_ids lift
loop.  Given the same peaks the kernels are bit-exact; end to end (scores from a GPU matmul) within 1e-5."""
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy.ndimage import distance_transform_edt

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent / "tools"))


# ------------------------------------------------------------------ restatement of the reference's loops
def ref_area_field(cells, peaks_f32, gs, decay):
    D = np.zeros((gs, gs), dtype=np.float32)
    for (r, c), s in zip(cells, peaks_f32):
        if r < 0 or r >= gs or c < 0 or c >= gs:
            continue
        tmp = np.zeros_like(D, dtype=np.float32)
        tmp[r, c] = s
        dists = distance_transform_edt(tmp == 0)
        t = np.clip(np.ones_like(dists) * s - dists * decay, 0, 1)
        D = np.where(D > t, D, t)
    return D


def ref_sound_field(cell_lists, probs_f32, gs, decay):
    D = np.zeros((gs, gs), dtype=np.float32)
    for cells, con in zip(cell_lists, probs_f32):
        tmp = np.zeros_like(D, dtype=np.float32)
        for r, c in cells:
            tmp[r, c] = con
        dists = distance_transform_edt(tmp == 0)
        t = np.ones_like(tmp) * con - con * dists * decay
        D += np.where(t < 0, np.zeros_like(t), t)
    return D


def ref_normalise(D):
    return (D - np.min(D)) / (np.max(D) - np.min(D))


def ref_lift(D2, occupied_ids, N):
    heat = np.zeros(N, dtype=np.float32)
    rows, cols, hs = np.where(occupied_ids != -1)
    for r, c, h in zip(rows, cols, hs):
        heat[occupied_ids[r, c, h]] = D2[r, c]
    return heat


def ref_image(grid_pos, row, col, height, decay):
    pos = np.array([row, col, height])
    d = np.linalg.norm((grid_pos - pos)[:, :2], axis=1)
    return np.clip(1.0 - decay * d, 0, 1)


def _gf(field):
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    mm = np.array([field.min(), field.max()], dtype=field.dtype)
    return ops.GoalField(DeviceArray.from_numpy(field), DeviceArray.from_numpy(mm))


# ------------------------------------------------------------------ ops level, bit-exact
def _area_case(rng, P, gs=1000):
    cells = rng.integers(0, gs, (P, 2)).astype(np.int32)
    peaks = rng.random(P).astype(np.float32)
    if P >= 8:
        peaks[: P // 8] = 0.0                                       # zero peaks: no background upstream, contribute 0
        peaks[P // 8] = 1.0
        cells[P // 4: P // 4 + P // 8] = cells[0]                   # duplicate cells
        cells[-3:] = [[-1, 5], [gs, 3], [7, 2 * gs]]                # out-of-grid poses are skipped
        cells[-4] = [gs - 1, gs - 1]
    return cells, peaks


@pytest.mark.parametrize("P,decay", [(0, 0.1), (1, 0.1), (37, 0.1), (300, 0.1), (300, 0.01), (64, 0.0), (120, 0.003)])
def test_area_field_bit_exact(P, decay):
    from avlmaps_amd import ops
    rng = np.random.default_rng(P * 7 + int(decay * 1000))
    cells, peaks = _area_case(rng, P)
    gf = ops.area_field(cells, peaks.astype(np.float64), 1000, decay)
    got = gf.field.numpy()
    want = ref_area_field(cells, peaks, 1000, decay).astype(np.float64)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    lo, hi = gf.bounds()
    assert lo == want.min() and hi == want.max()
    if hi > lo:
        assert np.array_equal(ops.field_normalize(gf).numpy(), ref_normalise(want))


def test_area_field_small_grid_many_poses():
    """tiles cut by the grid edge (gs not a multiple of 16), several chunks of 256 poses, peaks above 1 clipped"""
    from avlmaps_amd import ops
    rng = np.random.default_rng(5)
    gs, P = 101, 700
    cells = rng.integers(-5, gs + 5, (P, 2)).astype(np.int32)
    peaks = (rng.random(P) * 1.2).astype(np.float32)
    for decay in (0.05, 0.5, 0.0):
        gf = ops.area_field(cells, peaks.astype(np.float64), gs, decay)
        assert np.array_equal(gf.field.numpy(), ref_area_field(cells, peaks, gs, decay).astype(np.float64))


@pytest.mark.parametrize("S,decay", [(1, 0.01), (40, 0.01), (25, 0.1), (12, 0.0)])
def test_sound_field_bit_exact(S, decay):
    from avlmaps_amd import ops
    rng = np.random.default_rng(S)
    gs = 1000
    cell_lists = [rng.integers(0, gs, (int(rng.integers(1, 21)), 2)).astype(np.int32) for _ in range(S)]
    probs = rng.random(S).astype(np.float32)
    if S > 4:
        probs[::5] = 0.0
        probs[1] = 1.0
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in cell_lists])])
    gf = ops.sound_field(offsets, np.concatenate(cell_lists), probs, gs, decay)
    got = gf.field.numpy()
    want = ref_sound_field(cell_lists, probs, gs, decay)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    lo, hi = gf.bounds()
    assert lo == want.min() and hi == want.max()
    if hi > lo:
        assert np.array_equal(ops.field_normalize(gf).numpy(), ref_normalise(want))


def test_sound_field_rejects_bad_input():
    from avlmaps_amd import ops
    with pytest.raises(ValueError):
        ops.sound_field([0, 1], [[5, 1000]], [0.5], 1000, 0.01)        # location outside the grid
    with pytest.raises(ValueError):
        ops.sound_field([0, 0, 1], [[5, 5]], [0.5, 0.5], 1000, 0.01)   # a segment without locations
    with pytest.raises(ValueError):
        ops.sound_field([0, 1], [[5, 5]], [0.5], 1000, -0.01)
    with pytest.raises(ValueError):
        ops.area_field([[5, 5]], [0.5], 1000, float("nan"))


def test_normalise_and_lift_on_a_builder_map(golden, tmp_path):
    """the lift through grid_pos equals the reference's loop over occupied_ids on a map made by VLMapBuilder (golden g2a), in
    both precisions"""
    from test_api_gpu import MemoryBuilder
    from avlmaps_amd import ops
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    g = golden("g2a_builder_small.npz")
    b = MemoryBuilder.make(g, tmp_path)
    np.random.seed(1234)
    b.create_mobile_base_map()
    _, _, gp, _, occ, _ = load_3d_map(tmp_path / "vlmap" / "vlmaps.h5df")
    gs, vh = occ.shape[0], occ.shape[2]
    rng = np.random.default_rng(0)
    for dtype in (np.float64, np.float32):
        field = rng.random((gs, gs)).astype(dtype) * 3 + 0.25
        gf = _gf(field)
        heat = ops.field_lift(gf, gp, vh).numpy()
        assert heat.dtype == np.float32 and np.array_equal(heat, ref_lift(ref_normalise(field), occ, len(gp)))
        assert np.array_equal(ops.field_normalize(gf).numpy(), ref_normalise(field))
    # voxels outside the (gs, gs, vh) grid are never reached by the occupied_ids loop: heat 0
    odd = np.array([[-1, 0, 0], [0, gs, 0], [3, 3, vh], [3, 3, 0]], dtype=np.int32)
    field = rng.random((gs, gs))
    h = ops.field_lift(_gf(field), odd, vh).numpy()
    assert h[:3].tolist() == [0, 0, 0] and h[3] == np.float32(ref_normalise(field)[3, 3])


def test_planar_decay_float64():
    from avlmaps_amd import ops
    rng = np.random.default_rng(3)
    gp = np.concatenate([rng.integers(0, 1000, (200_000, 2)), rng.integers(0, 30, (200_000, 1))], 1).astype(np.int32)
    for row, col, decay in ((500, 480, 0.01), (-20, 1300, 0.001), (3, 7, 0.5)):
        sim = ops.planar_decay(gp, row, col, decay).numpy()
        assert sim.dtype == np.float64 and np.array_equal(sim, ref_image(gp, row, col, 30.0, decay))


# ------------------------------------------------------------------ end to end through AVLMap and the CLI
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map
    from avlmaps_amd.apps.common import HashImageEncoder, load_config
    from avlmaps_amd.map.area_map import AreaMap
    tmp = tmp_path_factory.mktemp("mm")
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
    return sc, cfg_path, load_config(str(cfg_path))


def _avlmap(scene):
    from avlmaps_amd.apps.common import HashAudioText, HashClip
    from avlmaps_amd.map import AVLMap
    sc, _, cfg = scene
    av = AVLMap(cfg, data_dir=str(sc), area_text_model=HashClip(768), audio_text_model=HashAudioText())
    assert av.load_map(str(sc))
    return av


def _ref_cells(tfs, sc, av):
    from test_multimodal_host import ref_full_map_pose
    poses = np.loadtxt(sc / "poses.txt")
    return [ref_full_map_pose(tf, poses[0], av.vlmap.base_transform, 400, 0.05)[:2] for tf in tfs]


def test_index_area_end_to_end(scene):
    from avlmaps_amd.apps.common import HashClip
    from avlmaps_amd.utils.clip_utils import get_text_feats
    from avlmaps_amd.utils.mapping_utils import cvt_pose_vec2tf
    sc, _, _ = scene
    av = _avlmap(scene)
    vm = av.vlmap
    sparse = av.area_map.clip_sparse_map
    cells = _ref_cells([cvt_pose_vec2tf(p) for p in np.loadtxt(sc / "poses.txt")], sc, av)
    for name, decay in (("kitchen", 0.1), ("bedroom", 0.01)):
        scores = sparse @ get_text_feats([name], HashClip(768), 768).T                        # CPU matmul
        scores = scores.flatten()
        s = (scores - np.min(scores)) / (np.max(scores) - np.min(scores))
        D2 = ref_normalise(ref_area_field(cells, s, 400, decay))
        want = ref_lift(D2, vm.occupied_ids, len(vm.grid_pos))
        heat = av.index_area(name, decay_rate=decay)
        assert heat.dtype == np.float32 and heat.shape == want.shape
        assert np.abs(heat - want).max() <= 1e-5 and np.argmax(heat) == np.argmax(want)
        m2 = av.index_area_2d(name, decay_rate=decay)
        assert m2.dtype == np.float64 and m2.shape == (400, 400) and np.abs(m2 - D2).max() <= 1e-5
    # categories preloaded: the category's column of scores_mat, exact lookup
    sm = av.area_map.init_categories(["kitchen", "bedroom"])
    assert sm.shape == (len(sparse), 2)
    assert np.abs(sm[:, 1] - (sparse @ get_text_feats(["bedroom"], HashClip(768), 768).T)[:, 0]).max() < 1e-5


def test_index_sound_end_to_end(scene):
    from avlmaps_amd.apps.common import HashAudioText
    sc, _, _ = scene
    av = _avlmap(scene)
    vm = av.vlmap
    db = pickle.loads((sc / "audio_video" / "audio_data_level_3.pkl").read_bytes())
    A = np.stack([db[i]["audio_features"] for i in range(len(db))])
    cats = av.sound_map.sound_categories
    T = HashAudioText().encode_text(cats)
    cell_lists = []
    for i in range(len(db)):
        tfs = []
        for p in db[i]["locations"]:
            tf = np.eye(4)
            tf[:3, 3] = p
            tfs.append(tf)
        cell_lists.append(_ref_cells(tfs, sc, av))
    for name, decay in (("dog", 0.01), ("clock tick", 0.05)):
        logits = (np.float32(100.0) * A) @ T.T                                                # CPU matmul
        p = logits[:, cats.index(name)]
        p = (p - np.min(p)) / (np.max(p) - np.min(p))
        D2 = ref_normalise(ref_sound_field(cell_lists, p, 400, decay))
        want = ref_lift(D2, vm.occupied_ids, len(vm.grid_pos))
        heat = av.index_sound(name, decay_rate=decay)
        assert heat.dtype == np.float32 and np.abs(heat - want).max() <= 1e-5 and np.argmax(heat) == np.argmax(want)
        m2 = av.index_sound_2d(name, decay_rate=decay)
        assert m2.dtype == np.float32 and np.abs(m2 - D2).max() <= 1e-5
    with pytest.raises(KeyError):
        av.index_sound("zebra")


def test_index_image_end_to_end(scene):
    from avlmaps_amd.apps.common import FixedPoseLocalizer
    from avlmaps_amd.utils.mapping_utils import cvt_pose_vec2tf
    sc, _, cfg = scene
    av = _avlmap(scene)
    poses = np.loadtxt(sc / "poses.txt")
    av.visual_map.localizer = FixedPoseLocalizer(poses[5], av.vlmap.base2cam_tf)
    sim = av.index_image(np.zeros((48, 64, 3), np.uint8))
    row, col = _ref_cells([cvt_pose_vec2tf(poses[5])], sc, av)[0]
    assert sim.dtype == np.float64 and np.array_equal(sim, ref_image(av.vlmap.grid_pos, row, col, 1.5 / 0.05, 0.01))
    av.visual_map.localizer = lambda img, K: None
    with pytest.raises(ValueError):
        av.index_image(np.zeros((4, 4, 3), np.uint8))


def test_cli_modalities(scene):
    from avlmaps_amd.apps import index_map
    sc, cfg_path, _ = scene
    av = _avlmap(scene)
    base = ["--data-dir", str(sc), "--config", str(cfg_path), "--text-model", "hash"]
    heat = index_map.main(base + ["--modality", "area", "--query", "kitchen"])
    assert np.array_equal(heat, av.index_area("kitchen", decay_rate=0.1))
    heat = index_map.main(base + ["--modality", "sound", "--query", "dog", "--decay-rate", "0.02"])
    assert np.array_equal(heat, av.index_sound("dog", decay_rate=0.02))
    img = sorted((sc / "rgb").glob("*.png"))[2]
    heat = index_map.main(base + ["--modality", "image", "--image", str(img), "--image-pose", "2"])
    from avlmaps_amd.apps.common import FixedPoseLocalizer
    av.visual_map.localizer = FixedPoseLocalizer(np.loadtxt(sc / "poses.txt")[2], av.vlmap.base2cam_tf)
    from avlmaps_amd.utils.mapping_utils import load_rgb_png
    assert heat.dtype == np.float64 and np.array_equal(heat, av.index_image(load_rgb_png(img)))
