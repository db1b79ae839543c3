"""Host side of the image localizer: the sampling hash restated in NumPy (ops.pnp_sample_indices), HLocLocalizer's bookkeeping and
its rules that need no GPU, VisualMap.localize_image's composition against the reference's three lines (visual_map.py:77-79), and
the SciPy yardstick of tests/test_localize_gpu.py run on the synthetic scenes of tests/_loc_synth.py."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import _loc_synth as S  # noqa: E402
from avlmaps_amd import ops  # noqa: E402
from avlmaps_amd.map.avlmap import AVLMap, MissingSubMap  # noqa: E402,F401
from avlmaps_amd.map.visual_map import VisualMap  # noqa: E402
from avlmaps_amd.utils import localization_utils as L  # noqa: E402

MAP_CONFIG = dict(pose_info=dict(base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1], camera_height=1.5))


# ------------------------------------------------------------------ the sampling hash
@pytest.mark.parametrize("m", [3, 4, 65])
def test_sample_indices_are_distinct_and_in_range(m):
    t = ops.pnp_sample_indices(5, 4096, m)
    assert t.shape == (4096, 3) and t.dtype == np.int32
    assert t.min() >= 0 and t.max() < m
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    if m == 3:
        assert (np.sort(t, axis=1) == np.arange(3)).all()
        assert len({tuple(r) for r in t.tolist()}) == 6          # every permutation turns up
    else:
        assert set(np.unique(t).tolist()) == set(range(m))       # every index is drawn, in every column
        for c in range(3):
            assert len(np.unique(t[:, c])) == m


def test_sample_indices_do_not_depend_on_the_number_of_hypotheses():
    full = ops.pnp_sample_indices(9, 9216, 401)
    for n in (1, 63, 64, 65, 1000):
        assert np.array_equal(ops.pnp_sample_indices(9, n, 401), full[:n])
    assert not np.array_equal(ops.pnp_sample_indices(10, 64, 401), full[:64])
    with pytest.raises(ValueError):
        ops.pnp_sample_indices(0, 4, 2)


def test_sample_hash_is_the_documented_one():
    """the first hypothesis by hand, in Python integers"""
    def mix(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xffffffff
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xffffffff
        return x ^ (x >> 16)
    for seed, h, m in ((0, 0, 7), (123456789, 77, 1000), (0xffffffff, 9215, 3)):
        w = [mix((mix((mix(seed ^ 0x9e3779b9) + h) & 0xffffffff) + d) & 0xffffffff) for d in range(3)]
        i0 = w[0] % m
        i1 = w[1] % (m - 1)
        i1 += i1 >= i0
        k = w[2] % (m - 2)
        k += k >= min(i0, i1)
        k += k >= max(i0, i1)
        assert ops.pnp_sample_indices(seed, h + 1, m)[h].tolist() == [i0, i1, k]


def test_default_trial_budget_is_the_derived_one():
    import math
    trials = math.log(1e-4) / math.log(1 - 0.1 ** 3)
    assert math.ceil(trials) == 9206 and ops.PNP_DEFAULT_HYPOTHESES == 64 * math.ceil(trials / 64) == 9216
    assert ops.PNP_MAX_ERROR == 12.0 and L.MIN_MATCHES == 100


# ------------------------------------------------------------------ HLocLocalizer bookkeeping
def _write_frames(data_dir, n, h=6, w=8):
    from PIL import Image
    (data_dir / "rgb").mkdir(parents=True)
    (data_dir / "depth").mkdir()
    rows = []
    for i in range(n):
        img = np.zeros((h, w, 3), np.uint8)
        img[0, 0, 0] = i
        Image.fromarray(img).save(data_dir / "rgb" / f"{i:06}.png")
        np.save(data_dir / "depth" / f"{i:06}.npy", np.full((h, w), 1.0 + i, np.float32))
        rows.append([0.1 * i, 0.0, -0.2 * i, 0.0, np.sin(0.05 * i), 0.0, np.cos(0.05 * i)])
    np.savetxt(data_dir / "poses.txt", np.array(rows))
    return np.array(rows)


def test_localizer_paths_and_descriptor_cache(tmp_path):
    data_dir = tmp_path / "scene_a"
    rows = _write_frames(data_dir, 11)
    calls = []

    def descriptor(img):
        calls.append(int(img[0, 0, 0]))
        v = np.zeros(16, np.float32)
        v[int(img[0, 0, 0])] = 1.0
        return v

    vm = VisualMap(MAP_CONFIG, localizer=None)
    vm.create_and_load_map(data_dir, global_descriptor=descriptor)
    loc = vm.localizer
    assert isinstance(loc, L.HLocLocalizer)
    assert vm.map_save_dir == data_dir / "visual_map" and vm.map_save_dir.is_dir()
    assert [Path(p).name for p in loc.image_paths_list] == [f"{i:06}.png" for i in range(11)]
    assert [Path(p).name for p in loc.depth_paths_list] == [f"{i:06}.npy" for i in range(11)]
    assert len(loc.pose_list) == 11 and np.allclose(loc.pose_list[3][:3, 3], rows[3, :3])
    cache = data_dir / "visual_map" / "scene_a_reference_features.npy"
    assert Path(loc.ref_features_path) == cache and cache.is_file()
    assert calls == list(range(11)) and np.array_equal(np.load(cache), np.eye(16, dtype=np.float32)[:11])
    # a second map over the same folder reads the cache instead of describing the frames again
    vm2 = VisualMap(MAP_CONFIG)
    vm2.create_and_load_map(data_dir, global_descriptor=descriptor)
    assert calls == list(range(11)) and np.array_equal(vm2.localizer.ref_desc, loc.ref_desc)
    # without cam_calib_mat the reference intrinsics are get_sim_cam_mat of the frame size; with it, the config's
    assert np.array_equal(vm.ref_cam_intrinsic_mat, np.array([[4.0, 0, 4.0], [0, 4.0, 3.0], [0, 0, 1.0]]))
    K = [300.0, 0, 320.0, 0, 300.0, 240.0, 0, 0, 1.0]
    assert np.array_equal(VisualMap(dict(MAP_CONFIG, cam_calib_mat=K)).ref_cam_intrinsic_mat, np.array(K).reshape(3, 3))


def test_default_folder_key_sorts_by_the_trailing_number(tmp_path):
    from PIL import Image
    for i in (10, 9, 100):
        Image.fromarray(np.zeros((2, 2, 3), np.uint8)).save(tmp_path / f"frame_{i}.png")
    loc = L.HLocLocalizer(tmp_path / "features")
    loc.init_video_with_images_folder(tmp_path)
    assert [Path(p).name for p in loc.image_paths_list] == ["frame_9.png", "frame_10.png", "frame_100.png"]
    # a folder whose path holds a "." or a "_" does not disturb the key
    dotted = tmp_path / ".hidden_v1.2" / "rgb_3"
    dotted.mkdir(parents=True)
    for i in (10, 9, 100):
        Image.fromarray(np.zeros((2, 2, 3), np.uint8)).save(dotted / f"frame_{i}.png")
        np.save(dotted / f"depth_{i}.npy", np.zeros((2, 2), np.float32))
    loc.init_video_with_images_folder(dotted)
    loc.init_depth_with_depth_folder(dotted)
    assert [Path(p).name for p in loc.image_paths_list] == ["frame_9.png", "frame_10.png", "frame_100.png"]
    assert [Path(p).name for p in loc.depth_paths_list] == ["depth_9.npy", "depth_10.npy", "depth_100.npy"]


def test_fewer_than_100_matches_is_none_without_the_gpu(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("the GPU path was entered")
    for name in ("loc_lift", "pnp_ransac", "pnp_refine"):
        monkeypatch.setattr(ops, name, no_gpu)
    pts = np.random.default_rng(0).uniform(0, 40, (99, 2))
    loc = L.HLocLocalizer.__new__(L.HLocLocalizer)
    loc.matcher = lambda a, b: (pts, pts + 1.0, np.ones(99))
    loc.last_estimate = "stale"
    assert loc._get_relative_pose_with_depth(None, None, np.ones((48, 64))) is None
    assert loc.last_estimate is None
    loc.matcher = lambda a, b: (np.zeros((100, 2)), np.zeros((100, 2)), np.ones(100))
    with pytest.raises(AssertionError, match="GPU path"):
        loc._get_relative_pose_with_depth(None, None, np.ones((48, 64)))


def test_missing_models_say_what_to_provide(tmp_path):
    loc = L.HLocLocalizer(tmp_path / "features")
    with pytest.raises(MissingSubMap, match="global_descriptor"):
        loc.compute_global_descriptor([np.zeros((4, 4, 3), np.uint8)], reference=False)
    with pytest.raises(MissingSubMap, match="matcher"):
        loc._get_relative_pose_with_depth(None, None, np.ones((4, 4)))
    with pytest.raises(MissingSubMap, match="reference frames"):
        loc.localize_agent(np.zeros((4, 4, 3), np.uint8))
    assert issubclass(MissingSubMap, NotImplementedError)


def test_habitat_pose_and_saved_transform(tmp_path):
    row = np.array([1.0, 2.0, 3.0, 0.0, np.sin(0.2), 0.0, np.cos(0.2)])
    (tmp_path / "p.txt").write_text(" ".join(str(v) for v in row))
    from scipy.spatial.transform import Rotation as R
    want = np.eye(4)
    want[:3, :3] = R.from_quat(row[3:]).as_matrix() @ np.diag([1.0, -1.0, -1.0])
    want[:3, 3] = [1.0, 3.5, 3.0]
    assert np.array_equal(L.get_cam_pose_habitat(tmp_path / "p.txt"), want) and np.array_equal(L.get_cam_pose_habitat(row), want)
    L.save_hab_tf(tmp_path / "tf.txt", want)
    assert np.array_equal(np.array([float(x) for x in (tmp_path / "tf.txt").read_text().split(",")]).reshape(4, 4), want)
    L.save_hab_tf(tmp_path / "none.txt", None)
    assert (tmp_path / "none.txt").read_text() == ""


# ------------------------------------------------------------------ VisualMap.localize_image
class FakeHLoc:
    """answers localize_agent_with_depth from a table; records what it was asked"""

    def __init__(self, pose_list, answer):
        self.pose_list, self.answer, self.asked = pose_list, answer, []

    def localize_agent_with_depth(self, img, ref_intr_mat=None, query_intr_mat=None, vis=False):
        self.asked.append((ref_intr_mat, query_intr_mat))
        return self.answer


def test_localize_image_composes_like_the_reference():
    rng = np.random.default_rng(3)
    from scipy.spatial.transform import Rotation as R

    def tf():
        m = np.eye(4)
        m[:3, :3] = R.from_rotvec(rng.standard_normal(3)).as_matrix()
        m[:3, 3] = rng.standard_normal(3)
        return m
    poses, transform = [tf() for _ in range(5)], tf()
    K = [300.0, 0, 320.0, 0, 300.0, 240.0, 0, 0, 1.0]
    fake = FakeHLoc(poses, (3, transform))
    vm = VisualMap(dict(MAP_CONFIG, cam_calib_mat=K), localizer=fake)
    cam_tf, base_tf = vm.localize_image(np.zeros((48, 64, 3), np.uint8))
    # visual_map.py:77-79
    tf_ref = poses[3] @ vm.tf_base2cam
    want_cam = tf_ref @ transform
    want_base = want_cam @ np.linalg.inv(vm.tf_base2cam)
    assert np.array_equal(cam_tf, want_cam) and np.array_equal(base_tf, want_base)
    ref_K, query_K = fake.asked[0]
    assert np.array_equal(ref_K, np.array(K).reshape(3, 3))
    assert np.allclose(query_K, [[32.0, 0, 32.0], [0, 32.0, 24.0], [0, 0, 1.0]])      # 90 degrees over 64 columns
    fake.answer = (-1, None)
    assert vm.localize_image(np.zeros((48, 64, 3), np.uint8)) is None


def test_a_plain_callable_localizer_still_works():
    seen = []

    def plain(img, K):
        seen.append(K)
        return "cam", "base"
    vm = VisualMap(MAP_CONFIG, localizer=plain)
    assert vm.localize_image(np.zeros((4, 8, 3), np.uint8)) == ("cam", "base") and seen[0].shape == (3, 3)


# ------------------------------------------------------------------ the yardstick on the helper's scenes
@pytest.mark.parametrize("case", S.E2E_CASES + ((400, 0.03, 13),))
def test_scenes_and_scipy_yardstick(case):
    y = S.yardstick(*case)
    sc = y["scene"]
    m, share, _ = case
    assert sc["planted"].sum() == round(share * m)
    d = np.linalg.norm(sc["pixels"] - sc["truth"], axis=1)
    assert d[sc["planted"]].max() <= 3.0 and d[~sc["planted"]].min() >= 48.0
    # rotation up to 30 degrees, translation up to 1 m, every point in front of both cameras
    angle, dist = S.pose_distance(sc["pose"], np.eye(3, 4))
    assert angle <= np.deg2rad(30.0) + 1e-12 and dist <= 1.0 + 1e-12
    assert S.project(sc["pose"], sc["points"], sc["K"])[1].min() > 0.5
    # the optimum keeps the planted inlier set, lowers the truth's cost, and does not depend on the start beyond the measured bound
    for pose in (y["pose"], y["pose_b"]):
        assert np.array_equal(S.inlier_mask(pose, sc["points"], sc["pixels"], sc["K"]), sc["planted"])
    e, _ = S.squared_errors(sc["pose"], sc["points"][sc["planted"]], sc["pixels"][sc["planted"]], sc["K"])
    assert y["cost"] <= e.sum() and abs(y["cost_b"] - y["cost"]) <= 1e-9 * y["cost"]
    rot, t = S.pose_distance(y["pose"], y["pose_b"])
    print(f"scipy optima from two starts: {rot:.3e} rad, {t:.3e} m apart; cost {y['cost']:.15g}")
    if case in S.E2E_CASES:
        assert rot <= S.POSE_BOUND_ROT and t <= S.POSE_BOUND_T


def test_numpy_lift_is_depth2pc_at_the_key_points():
    rng = np.random.default_rng(1)
    depth = rng.uniform(0.05, 11.0, (5, 7))
    K = S.camera(3.5, 7, 5)
    kp = np.stack([rng.uniform(0, 7, 30), rng.uniform(0, 5, 30)], axis=1)
    pts, pix, kept = S.numpy_lift(depth, K, kp, kp + 100.0)
    xi, yi = kp.astype(np.int32).T
    z = depth[yi, xi]
    assert np.array_equal(kept, (z > 0.1) & (z < 10))
    assert np.allclose(pts[:, 2], z[kept], rtol=1e-15) and np.array_equal(pix, kp[kept] + 100.0)
    assert np.allclose(pts[:, 0], (xi[kept] + 0.5 - 3.5) / 3.5 * z[kept], rtol=1e-13, atol=1e-15)
