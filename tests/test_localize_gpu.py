"""The localization kernels (csrc/avl_pnp.hip) through ops, HLocLocalizer and VisualMap.localize_image on an MI355X: the lift against
NumPy's depth2pc + indexing, the inlier test bit for bit against its NumPy restatement, the sampling hash against its host twin,
the P3P solver by its properties, RANSAC + refinement against scipy.optimize.least_squares on planted scenes (tests/_loc_synth.py),
and retrieval against np.argmax of the float64 product."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import _loc_synth as S  # noqa: E402
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.map.visual_map import VisualMap  # noqa: E402
from avlmaps_amd.utils import localization_utils as L  # noqa: E402

MAP_CONFIG = dict(pose_info=dict(base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1], camera_height=1.5))


# ------------------------------------------------------------------ lift
def lift_case(h, w, m, dtype, seed):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.5, 9.0, (h, w))
    # the edges of the kept interval, zero and NaN, at known pixels
    special = {(0, 0): 0.1, (1, 1): 10.0, (2, 2): 0.0, (3, 3): np.nan, (4, 4): np.nextafter(0.1, 1.0), (0, 5): np.nextafter(10.0, 0.0),
               (h - 1, w - 1): 2.5, (h - 1, 0): 11.0, (0, w - 1): -1.0}
    for (r, c), v in special.items():
        depth[r, c] = v
    depth = depth.astype(dtype)
    kp = np.stack([rng.uniform(0, w, m), rng.uniform(0, h, m)], axis=1)
    fixed = [(c + 0.99, r + 0.99) for (r, c) in special]                       # x.99 truncates; the last row and column among them
    fixed += [(w - 1 + 0.999, 0.0), (0.0, h - 1 + 0.999), (w - 0.5, h - 0.5), (0.0, 0.0), (3.0, 2.0)]
    kp[rng.permutation(m)[:len(fixed)]] = np.array(fixed)
    kq = rng.uniform(-50, 700, (m, 2))
    K = np.array([[0.5 * w + 0.3, 0.0, 0.5 * w - 0.2], [0.0, 0.5 * w - 0.1, 0.5 * h + 0.4], [0.0, 0.0, 1.0]])
    return depth, K, kp, kq


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("h,w,m", [(5, 7, 40), (64, 65, 700)])
def test_lift_equals_depth2pc_and_indexing(h, w, m, dtype):
    depth, K, kp, kq = lift_case(h, w, m, dtype, h + w)
    want_pts, want_pix, kept = S.numpy_lift(depth, K, kp, kq)
    got = ops.loc_lift(depth, K, kp, kq)
    pts, pix = got.numpy()
    assert got.count == kept.sum() and 0 < got.count < m
    assert np.array_equal(pix, want_pix)                      # mask and order
    if dtype == np.float64:                                   # depths of exactly 0.1 and 10 are excluded, their neighbours kept
        xi, yi = kp.astype(np.int32).T
        z = depth[yi, xi]
        assert not kept[z == 0.1].any() and not kept[z == 10.0].any() and (z == 0.1).any() and (z == 10.0).any()
        assert kept[z == np.nextafter(0.1, 1.0)].all() and kept[z == np.nextafter(10.0, 0.0)].all()
    # |error| <= 5 * 2^-53 * |z| * sum_j |Kinv_ij p_j|: a three-term dot product in any order, fused or not, then one multiply
    Kinv = np.linalg.inv(K)
    ki = kp.astype(np.int32)[kept]
    p = np.stack([ki[:, 0] + 0.5, ki[:, 1] + 0.5, np.ones(len(ki))], axis=1)
    z = depth[ki[:, 1], ki[:, 0]].astype(np.float64)
    bound = 5 * 2.0 ** -53 * np.abs(z)[:, None] * (np.abs(Kinv)[None, :, :] * np.abs(p)[:, None, :]).sum(axis=2)
    assert (np.abs(pts - want_pts) <= bound).all()
    # float32 key points (what a matcher returns) truncate alike
    got32 = ops.loc_lift(depth, K, kp.astype(np.float32), kq)
    want32 = S.numpy_lift(depth, K, kp.astype(np.float32), kq)
    assert np.array_equal(got32.numpy()[1], want32[1])


@pytest.mark.parametrize("bad", [(7.0, 1.0), (1.0, 5.0), (-1.5, 1.0), (np.nan, 1.0), (1.0, np.inf)])
def test_lift_rejects_a_key_point_outside_the_image(bad):
    depth, K, kp, kq = lift_case(5, 7, 40, np.float32, 1)
    kp[17] = bad
    with pytest.raises(_lib.AvlError, match="outside"):
        ops.loc_lift(depth, K, kp, kq)


# ------------------------------------------------------------------ scoring
def score_poses(sc, n, seed):
    rng = np.random.default_rng(seed)
    poses = [sc["pose"]]
    for k in range(n - 1):
        poses.append(S.perturbed(sc["pose"], eps=10.0 ** rng.uniform(-4, -1) * rng.choice([-1.0, 1.0])))
    poses = np.stack(poses)
    if n >= 3:
        poses[n // 2] = np.nan
        poses[n - 1] = -sc["pose"]               # every point behind the camera
    return poses


@pytest.mark.parametrize("n_poses", [1, 65])
@pytest.mark.parametrize("m", [1, 63, 64, 65, "stage+1"])
def test_score_equals_the_numpy_restatement(m, n_poses):
    m = ops.pnp_lds_stage() + 1 if m == "stage+1" else m
    sc = S.make_scene(m, 0.5, 100 + m)
    poses = score_poses(sc, n_poses, m)
    want = np.stack([S.inlier_mask(p, sc["points"], sc["pixels"], sc["K"]) for p in poses])
    # no squared residual within relative 1e-9 of max_error^2: the comparison cannot hinge on one rounding
    for p in poses:
        e, _ = S.squared_errors(p, sc["points"], sc["pixels"], sc["K"])
        e = e[np.isfinite(e)]
        assert (np.abs(e - S.MAX_ERROR ** 2) > 1e-9 * S.MAX_ERROR ** 2).all()
    counts, mask = ops.pnp_score(sc["points"], sc["pixels"], poses, sc["K"], want_mask=True)
    assert counts.dtype == np.int32 and np.array_equal(counts, want.sum(axis=1))
    assert np.array_equal(mask, want[0])
    if n_poses >= 3:
        assert counts[n_poses // 2] == 0 and counts[n_poses - 1] == 0
    if m >= 2:
        assert counts[0] == sc["planted"].sum()
    assert np.array_equal(ops.pnp_score(sc["points"], sc["pixels"], poses, sc["K"]), counts)


# ------------------------------------------------------------------ samples and P3P
@pytest.mark.parametrize("m,n_hyp,seed", [(3, 64, 0), (4, 65, 1), (65, 64, 2), (1026, 200, 0xfffffffe)])
def test_ransac_draws_the_documented_samples(m, n_hyp, seed):
    sc = S.make_scene(m, 1.0, 200 + m, noise=False)
    res = ops.pnp_ransac(sc["points"], sc["pixels"], sc["K"], n_hyp=n_hyp, seed=seed, want_triples=True)
    assert res.triples.dtype == np.int32 and np.array_equal(res.triples, ops.pnp_sample_indices(seed, n_hyp, m))


@pytest.mark.parametrize("m", [40, 1030])
def test_p3p_properties_without_noise(m):
    sc = S.make_scene(m, 1.0, 300 + m, noise=False)
    pts, pix, K = sc["points"], sc["pixels"], sc["K"]
    res = ops.pnp_ransac(pts, pix, K, n_hyp=64, seed=4, want_triples=True, want_poses=True)
    assert np.isfinite(res.hyp_poses).all() and np.isfinite(res.pose).all()
    solved = 0
    for h in range(64):
        if res.hyp_counts[h] >= 3:
            t = res.triples[h]
            assert S.inlier_mask(res.hyp_poses[h], pts[t], pix[t], K).all(), h
            assert S.inlier_mask(res.hyp_poses[h], pts, pix, K).sum() == res.hyp_counts[h]
            solved += 1
        else:
            assert res.hyp_counts[h] == 0 and np.array_equal(res.hyp_poses[h], np.eye(3, 4))
    assert solved >= 48                                      # three points in general position have a solution
    assert res.hyp_counts.max() == m == res.count
    assert S.inlier_mask(res.pose, pts, pix, K).sum() == res.count
    first = int(np.argmax(res.hyp_counts))                   # ties go to the smallest hypothesis
    assert np.array_equal(res.pose, res.hyp_poses[first])


def test_collinear_points_give_no_pose():
    K = S.camera()
    pts = np.array([[0.0, 0.0, 3.0], [0.5, 0.25, 3.5], [1.0, 0.5, 4.0]])
    pix, _ = S.project(np.eye(3, 4), pts, K)
    res = ops.pnp_ransac(pts, pix, K, n_hyp=64, seed=0, want_poses=True)
    assert res.count == 0 and not res.hyp_counts.any()
    assert np.array_equal(res.pose, np.eye(3, 4)) and np.isfinite(res.hyp_poses).all()
    pts[1] = pts[0]                                           # a repeated point
    res = ops.pnp_ransac(pts, pix, K, n_hyp=64, seed=0)
    assert res.count == 0 and np.isfinite(res.pose).all()
    assert ops.pnp_ransac(pts[:2], pix[:2], K, n_hyp=64).count == 0      # fewer than three: no launch


# ------------------------------------------------------------------ end to end
def estimate(sc, seed=0):
    est = ops.pnp_ransac(sc["points"], sc["pixels"], sc["K"], seed=seed)           # the default trial budget
    ref = ops.pnp_refine(sc["points"], sc["pixels"], est.pose_dev, sc["K"])
    return est, ref


@pytest.mark.parametrize("case", S.E2E_CASES)
def test_ransac_and_refinement_reach_scipys_optimum(case):
    y = S.yardstick(*case)
    sc = y["scene"]
    est, ref = estimate(sc)
    rot, t = S.pose_distance(ref.pose, y["pose"])
    print(f"case {case}: ransac count {est.count}, refined count {ref.count}, cost {ref.cost:.15g} (scipy {y['cost']:.15g}), "
          f"{ref.iterations} steps, {rot:.3e} rad and {t:.3e} m from scipy's optimum")
    assert np.array_equal(ref.mask, sc["planted"]) and ref.count == sc["planted"].sum() == ref.n_used
    assert ref.cost <= y["cost"] * (1 + 1e-6)
    assert ref.iterations <= ops.PNP_MAX_ITERATIONS
    # SciPy's optima from two starts lie (1.01e-10 rad, 3.77e-10 m) apart at most on these scenes; ten times that is allowed
    assert rot <= S.POSE_BOUND_ROT and t <= S.POSE_BOUND_T
    # the refined pose scored on its own gives the mask the refinement reports
    counts, mask = ops.pnp_score(sc["points"], sc["pixels"], ref.pose, sc["K"], want_mask=True)
    assert counts[0] == ref.count and np.array_equal(mask, ref.mask)
    # the same seed gives the same bits, another seed the same inliers
    est2, ref2 = estimate(sc)
    assert np.array_equal(est.pose, est2.pose) and np.array_equal(est.hyp_counts, est2.hyp_counts) and est.count == est2.count
    assert np.array_equal(ref.pose, ref2.pose) and ref.cost == ref2.cost and ref.iterations == ref2.iterations
    _, ref3 = estimate(sc, seed=12345)
    assert np.array_equal(ref3.mask, ref.mask)


# ------------------------------------------------------------------ retrieval
def retrieval_case(n, q, seed, d=4096):
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal((n, d)).astype(np.float32)
    ref /= np.linalg.norm(ref, axis=1, keepdims=True)
    target = rng.integers(0, n, q)
    query = ref[target] + 0.3 * rng.standard_normal((q, d)).astype(np.float32) / np.sqrt(d)
    query /= np.linalg.norm(query, axis=1, keepdims=True)
    return ref, query.astype(np.float32), target


@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_retrieval_is_the_float64_argmax(n, q):
    from avlmaps_amd.device import DeviceArray
    ref, query, target = retrieval_case(n, q, 10 * n + q)
    exact = query.astype(np.float64) @ ref.astype(np.float64).T
    if n > 1:
        top2 = np.sort(exact, axis=1)[:, -2:]
        assert (top2[:, 1] - top2[:, 0] > 1e-3).all()           # above the kernel's 1e-4 score contract
    resident = DeviceArray.from_numpy(ref)
    idx, val = ops.retrieve_frame(resident, query)
    assert idx.shape == (q,) and np.array_equal(idx, np.argmax(exact, axis=1)) and np.array_equal(idx, target)
    assert np.abs(val - exact.max(axis=1)).max() < 1e-4
    one_idx, one_val = ops.retrieve_frame(ref, query[0])         # a host matrix and a single (D,) query
    assert one_idx == idx[0] and abs(one_val - val[0]) < 1e-4


def test_retrieval_returns_the_first_of_two_equal_rows():
    ref, query, target = retrieval_case(65, 3, 5)
    target = np.minimum(target, 60)
    query = ref[target].copy()
    ref[64] = ref[target[0]]
    ref[target[1] + 1] = ref[target[1]]
    idx, _ = ops.retrieve_frame(ref, query)
    assert np.array_equal(idx, target)


# ------------------------------------------------------------------ HLocLocalizer and VisualMap on a synthetic scene
H, W, N_FRAMES = 48, 64, 12
K_REF = np.array([[32.0, 0.0, 32.0], [0.0, 32.0, 24.0], [0.0, 0.0, 1.0]])
K_QUERY = np.array([[40.0, 0.0, 31.0], [0.0, 40.0, 25.0], [0.0, 0.0, 1.0]])


class Scene:
    """12 frames of 48 x 64 depth with poses, written like a dataset folder; queries are images that carry an id, the descriptor
    stand-in returns planted vectors and the matcher fabricates matches from the known geometry"""

    def __init__(self, data_dir):
        from PIL import Image
        rng = np.random.default_rng(21)
        self.data_dir = data_dir
        (data_dir / "rgb").mkdir(parents=True)
        (data_dir / "depth").mkdir()
        yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
        self.depths, rows = [], []
        for i in range(N_FRAMES):
            depth = (3.0 + np.sin(2 * xx + 0.4 * i) * np.cos(1.5 * yy) + 0.3 * rng.random((H, W))).astype(np.float32)
            self.depths.append(depth)
            np.save(data_dir / "depth" / f"{i:06}.npy", depth)
            img = np.zeros((H, W, 3), np.uint8)
            img[0, 0] = (i, 0, 0)                                     # channel 1 = 0: a reference frame
            Image.fromarray(img).save(data_dir / "rgb" / f"{i:06}.png")
            rows.append([0.3 * i, 0.0, -0.1 * i, 0.0, np.sin(0.1 * i), 0.0, np.cos(0.1 * i)])
        np.savetxt(data_dir / "poses.txt", np.array(rows))
        self.desc = rng.standard_normal((N_FRAMES, 64)).astype(np.float32)
        self.desc /= np.linalg.norm(self.desc, axis=1, keepdims=True)
        self.queries = {}

    def add_query(self, qid, frame, n_matches, inlier_share, seed):
        """a query image seen from a planted pose relative to `frame`; returns the image"""
        rng = np.random.default_rng(seed)
        pose = S.random_pose(rng, max_angle_deg=20.0, max_t=0.5)
        cells = rng.permutation(H * W)[:n_matches]
        kp0 = np.stack([cells % W + rng.uniform(0.0, 0.99, n_matches), cells // W + rng.uniform(0.0, 0.99, n_matches)], axis=1)
        depth = self.depths[frame].astype(np.float64)
        pts, _, kept = S.numpy_lift(depth, K_REF, kp0, kp0)
        assert kept.all()
        kp1, z = S.project(pose, pts, K_QUERY)
        assert z.min() > 0.3
        n_in = int(round(inlier_share * n_matches))
        out = rng.permutation(n_matches)[n_in:]
        ang, dist = rng.uniform(0, 2 * np.pi, len(out)), rng.uniform(60.0, 200.0, len(out))
        kp1[out] += np.stack([dist * np.cos(ang), dist * np.sin(ang)], axis=1)
        self.queries[qid] = dict(frame=frame, pose=pose, kp0=kp0.astype(np.float32).astype(np.float64), kp1=kp1)
        # the float32 round trip of kp0 must not change a truncated pixel
        assert np.array_equal(self.queries[qid]["kp0"].astype(np.int32), kp0.astype(np.int32))
        img = np.zeros((H, W, 3), np.uint8)
        img[0, 0] = (qid, 1, 0)
        return img

    def descriptor(self, img):
        ident, is_query = int(img[0, 0, 0]), int(img[0, 0, 1])
        if not is_query:
            return self.desc[ident]
        v = self.desc[self.queries[ident]["frame"]] + 0.05 * np.random.default_rng(ident).standard_normal(64).astype(np.float32)
        return v / np.linalg.norm(v)

    def matcher(self, img_ref, img_query):
        q = self.queries[int(img_query[0, 0, 0])]
        assert int(img_ref[0, 0, 0]) == q["frame"] and int(img_ref[0, 0, 1]) == 0
        return q["kp0"], q["kp1"], np.ones(len(q["kp0"]))


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    sc = Scene(tmp_path_factory.mktemp("loc") / "scene_b")
    sc.images = {
        0: sc.add_query(0, frame=7, n_matches=300, inlier_share=0.6, seed=1),
        1: sc.add_query(1, frame=2, n_matches=50, inlier_share=1.0, seed=2),          # fewer than 100 matches
        2: sc.add_query(2, frame=11, n_matches=150, inlier_share=1.0, seed=3),
        3: sc.add_query(3, frame=4, n_matches=400, inlier_share=0.03, seed=4),        # 97 % outliers
    }
    vm = VisualMap(MAP_CONFIG, localizer=None)
    vm.create_and_load_map(sc.data_dir, global_descriptor=sc.descriptor, matcher=sc.matcher)
    sc.vm = vm
    return sc


def expected_cam_tf(sc, qid):
    q = sc.queries[qid]
    rel = np.eye(4)
    rel[:3, :4] = q["pose"]
    return sc.vm.localizer.pose_list[q["frame"]] @ sc.vm.tf_base2cam @ np.linalg.inv(rel)


def test_localize_image_finds_the_frame_and_the_planted_pose(scene):
    loc = scene.vm.localizer
    for qid in (0, 2):
        frame, sim = loc.localize_agent(scene.images[qid])
        assert frame == scene.queries[qid]["frame"] and sim > 0.8
        cam_tf, base_tf = scene.vm.localize_image(scene.images[qid], query_cam_intrinsic_mat=K_QUERY)
        est = loc.last_estimate
        assert est["inliers"] == round((0.6 if qid == 0 else 1.0) * est["matches"]) and est["lifted"] == est["matches"]
        want = expected_cam_tf(scene, qid)
        rot, t = S.pose_distance(cam_tf[:3], want[:3])
        print(f"query {qid}: {est['inliers']} inliers of {est['lifted']}, {est['iterations']} steps, {rot:.3e} rad, {t:.3e} m from the planted pose")
        assert rot <= S.POSE_BOUND_ROT and t <= S.POSE_BOUND_T
        assert np.allclose(base_tf, cam_tf @ np.linalg.inv(scene.vm.tf_base2cam), rtol=0, atol=1e-12)
        assert np.array_equal(cam_tf[3], [0, 0, 0, 1])


def test_unlocalizable_queries_return_none(scene, monkeypatch):
    loc = scene.vm.localizer
    # 97 % outliers: the count stays below min_inliers = ceil(0.1 M'); None, not an exception
    q = scene.queries[3]
    ref_img = np.zeros((H, W, 3), np.uint8)
    ref_img[0, 0] = (q["frame"], 0, 0)
    assert loc._get_relative_pose_with_depth(ref_img, scene.images[3], scene.depths[q["frame"]].astype(float), ref_intr_mat=K_REF,
                                             query_intr_mat=K_QUERY) is None
    est = loc.last_estimate
    assert est["min_inliers"] == 40 and est["inliers"] < 40 and est["lifted"] == 400
    assert scene.vm.localize_image(scene.images[3], query_cam_intrinsic_mat=K_QUERY) is None
    # 99 matches: None without touching the GPU
    def no_gpu(*a, **k):
        raise AssertionError("the GPU path was entered")
    for name in ("loc_lift", "pnp_ransac", "pnp_refine"):
        monkeypatch.setattr(ops, name, no_gpu)
    q99 = dict(scene.queries[0], kp0=scene.queries[0]["kp0"][:99], kp1=scene.queries[0]["kp1"][:99])
    monkeypatch.setitem(scene.queries, 0, q99)
    ref_img[0, 0] = (q99["frame"], 0, 0)
    assert loc._get_relative_pose_with_depth(ref_img, scene.images[0], scene.depths[q99["frame"]].astype(float)) is None


def test_get_frames_tfs_keeps_a_slot_for_every_frame(scene):
    loc = scene.vm.localizer
    rows = np.loadtxt(scene.data_dir / "poses.txt")
    init_tf_inv = np.linalg.inv(L.get_cam_pose_habitat(rows[0]))
    tfs = L.get_frames_tfs(loc, [scene.images[0], scene.images[1], scene.images[2]], rows, init_tf_inv, ref_cam_mat=K_REF,
                           query_cam_mat=K_QUERY)
    assert len(tfs) == 3 and tfs[1] is None
    for slot, qid in ((0, 0), (2, 2)):
        q = scene.queries[qid]
        rel = np.eye(4)
        rel[:3, :4] = q["pose"]
        want = init_tf_inv @ L.get_cam_pose_habitat(rows[q["frame"]]) @ np.linalg.inv(rel)      # localization_utils.py:580-581
        rot, t = S.pose_distance(tfs[slot][:3], want[:3])
        assert rot <= S.POSE_BOUND_ROT and t <= S.POSE_BOUND_T
