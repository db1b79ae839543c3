"""Synthetic geometry of the localization tests (tests/test_localize_host.py, tests/test_localize_gpu.py): 3-D points in front of a
reference camera, a known query pose, exact float64 projections, a planted share of inliers with sub-pixel noise and outliers
moved far away; NumPy restatements of the kernels' lift and inlier test; the SciPy yardstick of the refinement."""
import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation as R

MAX_ERROR = 12.0
INLIER_NOISE_PX = 1.0          # uniform, per axis
OUTLIER_MIN_PX = 60.0
OUTLIER_MAX_PX = 200.0


def camera(f=320.0, w=640, h=480):
    return np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])


def transform_rows(pose, pts):
    """(x, y, z) of every point, each row the left-to-right sum ((r0 X + r1 Y) + r2 Z) + t, the kernels' order"""
    P = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    X, Y, Z = pts[:, 0], pts[:, 1], pts[:, 2]
    return [((P[i, 0] * X + P[i, 1] * Y) + P[i, 2] * Z) + P[i, 3] for i in range(3)]


def project(pose, pts, K):
    x, y, z = transform_rows(pose, pts)
    f, cx, cy = K[0, 0], K[0, 2], K[1, 2]
    return np.stack([f * (x / z) + cx, f * (y / z) + cy], axis=1), z


def squared_errors(pose, pts, pix, K):
    """the squared reprojection error of every correspondence as the kernels compute it, and the camera-frame coordinates"""
    with np.errstate(all="ignore"):
        x, y, z = transform_rows(pose, pts)
        f, cx, cy = K[0, 0], K[0, 2], K[1, 2]
        du = (f * (x / z) + cx) - pix[:, 0]
        dv = (f * (y / z) + cy) - pix[:, 1]
        return du * du + dv * dv, (x, y, z)


def inlier_mask(pose, pts, pix, K, max_error=MAX_ERROR):
    """NumPy float64 restatement of the kernels' inlier test"""
    with np.errstate(all="ignore"):
        e, (x, y, z) = squared_errors(pose, pts, pix, K)
        return (z > 0) & np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (e <= max_error * max_error)


def random_pose(rng, max_angle_deg=30.0, max_t=1.0):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    angle = np.deg2rad(rng.uniform(0.3 * max_angle_deg, max_angle_deg))
    t = rng.standard_normal(3)
    t *= rng.uniform(0.3 * max_t, max_t) / np.linalg.norm(t)
    pose = np.zeros((3, 4))
    pose[:, :3] = R.from_rotvec(axis * angle).as_matrix()
    pose[:, 3] = t
    return pose


def make_scene(m, inlier_share, seed, K=None, noise=True):
    """dict(points (m, 3), pixels (m, 2), pose (3, 4) query camera from reference camera, K (3, 3), planted (m,) bool, truth (m, 2)).
    Asserts that every planted inlier is within 3 px and every planted outlier beyond 48 px of the true pose's projection, so the
    inlier set at 12 px is the planted one for any pose near the optimum."""
    rng = np.random.default_rng(seed)
    K = camera() if K is None else np.asarray(K, dtype=np.float64)
    for _ in range(100):
        pose = random_pose(rng)
        pts = np.stack([rng.uniform(-2.0, 2.0, m), rng.uniform(-1.5, 1.5, m), rng.uniform(2.0, 6.0, m)], axis=1)
        truth, z = project(pose, pts, K)
        if z.min() > 0.5:
            break
    else:
        raise AssertionError("no pose keeps the box in front of the query camera")
    n_in = int(round(inlier_share * m))
    planted = np.zeros(m, dtype=bool)
    planted[rng.permutation(m)[:n_in]] = True
    pix = truth.copy()
    if noise:
        pix[planted] += rng.uniform(-INLIER_NOISE_PX, INLIER_NOISE_PX, (n_in, 2))
    ang = rng.uniform(0.0, 2.0 * np.pi, m - n_in)
    dist = rng.uniform(OUTLIER_MIN_PX, OUTLIER_MAX_PX, m - n_in)
    pix[~planted] += np.stack([dist * np.cos(ang), dist * np.sin(ang)], axis=1)
    d = np.linalg.norm(pix - truth, axis=1)
    assert (d[planted] <= 3.0).all() and (d[~planted] >= 48.0).all()
    assert np.array_equal(inlier_mask(pose, pts, pix, K), planted)
    return dict(points=pts, pixels=pix, pose=pose, K=K, planted=planted, truth=truth)


# ------------------------------------------------------------------ the SciPy yardstick
def _pose_of(x):
    pose = np.zeros((3, 4))
    pose[:, :3] = R.from_rotvec(x[:3]).as_matrix()
    pose[:, 3] = x[3:]
    return pose


def _params_of(pose):
    return np.concatenate([R.from_matrix(pose[:, :3]).as_rotvec(), pose[:, 3]])


def scipy_refine(pts, pix, K, pose0):
    """(pose, sum of squared pixel residuals): scipy.optimize.least_squares in float64 with xtol = ftol = gtol = 1e-15"""
    def fun(x):
        uv, _ = project(_pose_of(x), pts, K)
        return (uv - pix).reshape(-1)
    res = least_squares(fun, _params_of(np.asarray(pose0, dtype=np.float64)), xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return _pose_of(res.x), float(np.sum(res.fun ** 2))


def perturbed(pose, eps=1e-3):
    """the pose with every rotation-vector and translation component moved by eps"""
    return _pose_of(_params_of(pose) + eps)


def pose_distance(a, b):
    """(rotation angle in radians, translation distance) between two 3 x 4 poses; the angle from the quaternion, accurate near 0"""
    a, b = np.asarray(a).reshape(3, 4), np.asarray(b).reshape(3, 4)
    return float(R.from_matrix(a[:, :3] @ b[:, :3].T).magnitude()), float(np.linalg.norm(a[:, 3] - b[:, 3]))


# The pose bound of the end-to-end tests.  Measured: SciPy's optimum from the true pose and from the true pose perturbed by 1e-3
# lie (1.01e-10 rad, 3.77e-10 m) apart on the (120, 0.5, 11) scene and (4.3e-11 rad, 1.78e-10 m) on (400, 0.15, 12): both runs stop
# at the rounding floor of the cost.  Ten times the larger pair is allowed, because the stopping rules differ.
E2E_CASES = ((120, 0.5, 11), (400, 0.15, 12))      # (M', planted inlier share, seed): 50 % and 85 % outliers
POSE_BOUND_ROT = 1.1e-9        # radians
POSE_BOUND_T = 3.8e-9          # metres

_YARDSTICK = {}


def yardstick(m, inlier_share, seed):
    """the scene, SciPy's optimum on the planted inliers from the true pose and from the perturbed true pose; computed once"""
    key = (m, inlier_share, seed)
    if key not in _YARDSTICK:
        sc = make_scene(m, inlier_share, seed)
        pts, pix = sc["points"][sc["planted"]], sc["pixels"][sc["planted"]]
        pose_a, cost_a = scipy_refine(pts, pix, sc["K"], sc["pose"])
        pose_b, cost_b = scipy_refine(pts, pix, sc["K"], perturbed(sc["pose"]))
        _YARDSTICK[key] = dict(scene=sc, pose=pose_a, cost=cost_a, pose_b=pose_b, cost_b=cost_b)
    return _YARDSTICK[key]


# ------------------------------------------------------------------ the lift
def numpy_lift(depth, K_ref, kp_ref, kp_query):
    """localization_utils.py:461-473 with mapping_utils.depth2pc:226-251, in NumPy: (points (M', 3), pixels (M', 2), kept mask)"""
    h, w = depth.shape
    Kinv = np.linalg.inv(K_ref)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x = x.reshape((1, -1)) + 0.5
    y = y.reshape((1, -1)) + 0.5
    z = depth.reshape((1, -1))
    pc = Kinv @ np.vstack([x, y, np.ones_like(x)])
    with np.errstate(invalid="ignore"):
        pc = pc * z
        mask = np.logical_and(pc[2, :] > 0.1, pc[2, :] < 10)
    mask = mask.reshape((h, w))
    pc = pc.reshape((3, h, w))
    ki = kp_ref.astype(np.int32)
    p3 = pc[:, ki[:, 1], ki[:, 0]]
    km = mask[ki[:, 1], ki[:, 0]]
    return p3[:, km].T.copy(), kp_query[km, :].copy(), km
