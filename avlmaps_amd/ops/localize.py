"""Image localization: key-point lifting, P3P RANSAC, refinement and frame retrieval (csrc/avl_pnp.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import DeviceArray, DeviceView, as_device
from ._args import _is_dev, _workspace
from .sim import argmax_f32, sim_scores

PNP_DEFAULT_HYPOTHESES = 9216     # trials for confidence 0.9999 at inlier ratio 0.1: ln(1e-4) / ln(1 - 0.1^3) = 9206, up to a multiple of 64
PNP_MAX_ERROR = 12.0              # localization_utils.py:485
PNP_MAX_ITERATIONS = 50
PNP_STEP_TOLERANCE = 1e-10


def pnp_lds_stage() -> int:
    """the number of correspondences the RANSAC and scoring kernels stage in LDS at a time"""
    return int(_lib.load().avl_pnp_lds_stage())


def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def pnp_sample_indices(seed, n_hyp, m) -> np.ndarray:
    """(n_hyp, 3) int32: the three distinct correspondence indices hypothesis h of pnp_ransac draws from [0, m), the hash of
    csrc/avl_pnp.hip restated in NumPy's wrapping uint32 arithmetic.  Row h depends on (seed, h, m) alone."""
    m = int(m)
    if m < 3:
        raise ValueError(f"three distinct samples need m >= 3, got {m}")
    with np.errstate(over="ignore"):
        h = np.arange(int(n_hyp), dtype=np.uint32)
        base = _mix32(_mix32(np.uint32((int(seed) ^ 0x9e3779b9) & 0xffffffff)) + h)
        w0, w1, w2 = (_mix32(base + np.uint32(d)) for d in range(3))
    i0 = (w0 % np.uint32(m)).astype(np.int64)
    i1 = (w1 % np.uint32(m - 1)).astype(np.int64)
    i1 += i1 >= i0
    k = (w2 % np.uint32(m - 2)).astype(np.int64)
    k += k >= np.minimum(i0, i1)
    k += k >= np.maximum(i0, i1)
    return np.stack([i0, i1, k], axis=1).astype(np.int32)


class Correspondences:
    """what loc_lift keeps: points (M', 3) in the reference camera's frame and pixels (M', 2) in the query image, float64 on the
    device (views of buffers this object owns), count = M'"""
    __slots__ = ("points", "pixels", "count", "_keep")

    def __init__(self, points, pixels, count, keep=()):
        self.points, self.pixels, self.count, self._keep = points, pixels, int(count), keep

    def numpy(self, stream=None):
        if self.count == 0:
            return np.zeros((0, 3)), np.zeros((0, 2))
        full_p, full_x = self._keep[0].numpy(stream), self._keep[1].numpy(stream)
        return full_p[:self.count].copy(), full_x[:self.count].copy()


def _f64_2d(x, cols, what, stream):
    if isinstance(x, np.ndarray) or not _is_dev(x):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    ptr, shape, keep = as_device(x, np.float64, stream)
    if len(shape) != 2 or shape[1] != cols:
        raise ValueError(f"{what}: expected (n, {cols}) float64, got shape {tuple(shape)}")
    return ptr, int(shape[0]), keep


def _camera3(K):
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"the query intrinsic matrix must be (3, 3), got {K.shape}")
    return float(K[0, 0]), float(K[0, 2]), float(K[1, 2])


def _corr_args(points, pixels, stream):
    if isinstance(points, Correspondences):
        points, pixels = points.points, points.pixels
    pp, m, k1 = _f64_2d(points, 3, "points", stream)
    xp, m2, k2 = _f64_2d(pixels, 2, "pixels", stream)
    if m != m2:
        raise ValueError(f"{m} points but {m2} pixels")
    return pp, xp, m, (k1, k2)


def loc_lift(depth, K_ref, kp_ref, kp_query, stream=None) -> Correspondences:
    """localization_utils.py:461-473: the matched key points of the reference frame lifted to 3-D with its depth image.
    depth (H, W) float32 or float64 metres, host or device; K_ref (3, 3); kp_ref, kp_query (M, 2) (x, y) pixel pairs.  kp_ref is
    truncated like astype(np.int32); the point is inv(K_ref) @ (x + 0.5, y + 0.5, 1) * z and is kept when 0.1 < p_z < 10.  The kept
    pairs come back in input order.  A key point outside the image raises AvlError (upstream's IndexError)."""
    lib = _lib.load()
    _lib.require_gpu()
    if not _is_dev(depth):
        depth = np.asarray(depth)
        if depth.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            depth = depth.astype(np.float64)
    dt = np.dtype(str(depth.dtype).replace("torch.", ""))
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"depth must be float32 or float64, got {dt}")
    dp, dshape, k0 = as_device(depth, dt, stream)
    if len(dshape) != 2:
        raise ValueError(f"depth must be (H, W), got shape {tuple(dshape)}")
    Kinv = np.ascontiguousarray(np.linalg.inv(np.asarray(K_ref, dtype=np.float64).reshape(3, 3)))
    rp, m, k1 = _f64_2d(kp_ref, 2, "kp_ref", stream)
    qp, m2, k2 = _f64_2d(kp_query, 2, "kp_query", stream)
    if m != m2:
        raise ValueError(f"{m} reference key points but {m2} query key points")
    pts, pix, counter = DeviceArray((max(m, 1), 3), np.float64), DeviceArray((max(m, 1), 2), np.float64), DeviceArray((2,), np.int32)
    n = C.c_int64(0)
    _lib.check(lib.avl_loc_lift(dp, int(dt == np.float64), int(dshape[0]), int(dshape[1]), Kinv.ctypes.data, rp, qp, m, pts.ptr, pix.ptr,
                                counter.ptr, C.byref(n), stream), "avl_loc_lift")
    return Correspondences(DeviceView(pts.ptr, (n.value, 3), np.float64), DeviceView(pix.ptr, (n.value, 2), np.float64), n.value,
                           keep=(pts, pix, k0, k1, k2))


class PnpRansacResult:
    """pose (3, 4) float64 [R|t] (query camera from reference camera), count, hyp_counts (n_hyp,) int32, triples (n_hyp, 3) int32 or
    None; hyp_poses (n_hyp, 3, 4) or None: the best pose of every hypothesis ([I|0] without a solution); pose_dev: the pose on the
    device"""
    __slots__ = ("pose", "count", "hyp_counts", "triples", "hyp_poses", "pose_dev")

    def __init__(self, pose, count, hyp_counts, triples, hyp_poses, pose_dev):
        self.pose, self.count, self.hyp_counts, self.triples, self.hyp_poses, self.pose_dev = pose, int(count), hyp_counts, triples, hyp_poses, pose_dev


def pnp_ransac(points, pixels, K_query, max_error=PNP_MAX_ERROR, n_hyp=PNP_DEFAULT_HYPOTHESES, seed=0, want_triples=False,
               want_poses=False, stream=None) -> PnpRansacResult:
    """n_hyp P3P hypotheses scored against all correspondences (the estimation half of pycolmap.absolute_pose_estimation,
    localization_utils.py:478-498).  points (M, 3) / pixels (M, 2) float64, host or device, or a Correspondences as `points`.
    The winner has the largest inlier count, ties to the smallest hypothesis index; the same seed gives the same bits.  Fewer
    than three correspondences: count 0 and the pose [I|0], without a launch."""
    lib = _lib.load()
    _lib.require_gpu()
    f, cx, cy = _camera3(K_query)
    n_hyp = int(n_hyp)
    pp, xp, m, keep = _corr_args(points, pixels, stream)
    if m < 3:
        return PnpRansacResult(np.eye(3, 4), 0, np.zeros(n_hyp, np.int32), None, None, None)
    ws, nws = _workspace(lib.avl_pnp_ransac_work_bytes, "avl_pnp_ransac_work_bytes", n_hyp)
    assert nws == n_hyp * 12 * 8                     # after the call: the best pose of every hypothesis, (n_hyp, 3, 4) float64
    counts, pose, count = DeviceArray((n_hyp,), np.int32), DeviceArray((3, 4), np.float64), DeviceArray((1,), np.int32)
    triples = DeviceArray((n_hyp, 3), np.int32) if want_triples else None
    _lib.check(lib.avl_pnp_ransac(pp, xp, m, f, cx, cy, float(max_error), int(seed) & 0xffffffff, n_hyp, triples.ptr if want_triples else None,
                                  counts.ptr, pose.ptr, count.ptr, ws.ptr, nws, stream), "avl_pnp_ransac")
    res = PnpRansacResult(pose.numpy(stream), int(count.numpy(stream)[0]), counts.numpy(stream),
                          triples.numpy(stream) if want_triples else None,
                          ws.numpy(stream).view(np.float64).reshape(n_hyp, 3, 4) if want_poses else None, pose)
    return res


def pnp_score(points, pixels, poses, K_query, max_error=PNP_MAX_ERROR, want_mask=False, stream=None):
    """inlier counts (P,) int32 of poses (P, 3, 4) (or one (3, 4) pose) with the RANSAC kernel's own inlier test; want_mask=True:
    (counts, mask) with the (M,) bool inlier mask of pose 0"""
    lib = _lib.load()
    _lib.require_gpu()
    f, cx, cy = _camera3(K_query)
    pp, xp, m, keep = _corr_args(points, pixels, stream)
    if isinstance(poses, (DeviceArray, DeviceView)):
        sp, sshape, k3 = as_device(poses, np.float64, stream)
    else:
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64))
        sp, sshape, k3 = as_device(poses.reshape(-1, 3, 4), np.float64, stream)
    P = int(np.prod(sshape, dtype=np.int64)) // 12
    counts = DeviceArray((P,), np.int32)
    mask = DeviceArray((max(m, 1),), np.uint8) if want_mask else None
    _lib.check(lib.avl_pnp_score(pp, xp, m, sp, P, f, cx, cy, float(max_error), counts.ptr, mask.ptr if want_mask else None, stream),
               "avl_pnp_score")
    c = counts.numpy(stream)
    if want_mask:
        return c, mask.numpy(stream)[:m].astype(bool)
    return c


class PnpRefineResult:
    """pose (3, 4), cost (sum of squared pixel residuals over the correspondences refined on), iterations, mask (M,) bool and count:
    the inliers of the refined pose, n_used: the inliers of the given pose, which the refinement ran on"""
    __slots__ = ("pose", "cost", "iterations", "mask", "count", "n_used")

    def __init__(self, pose, cost, iterations, mask, count, n_used):
        self.pose, self.cost, self.iterations, self.mask, self.count, self.n_used = pose, float(cost), int(iterations), mask, int(count), int(n_used)


def pnp_refine(points, pixels, pose, K_query, max_error=PNP_MAX_ERROR, max_iter=PNP_MAX_ITERATIONS, step_tol=PNP_STEP_TOLERANCE,
               stream=None) -> PnpRefineResult:
    """Levenberg-Marquardt on the inliers of `pose` ((3, 4), host or the device pose of pnp_ransac), focal length fixed, in one
    launch that iterates on the device; the refined pose is returned even if its inlier count dropped (upstream does not re-check)."""
    lib = _lib.load()
    _lib.require_gpu()
    f, cx, cy = _camera3(K_query)
    pp, xp, m, keep = _corr_args(points, pixels, stream)
    if m < 1:
        raise ValueError("pnp_refine needs at least one correspondence")
    if not isinstance(pose, (DeviceArray, DeviceView)):
        pose = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(3, 4))
    sp, _, k3 = as_device(pose, np.float64, stream)
    o13, o3, mask = DeviceArray((13,), np.float64), DeviceArray((3,), np.int32), DeviceArray((m,), np.uint8)
    _lib.check(lib.avl_pnp_refine(pp, xp, m, sp, f, cx, cy, float(max_error), int(max_iter), float(step_tol), o13.ptr, o3.ptr, mask.ptr, stream),
               "avl_pnp_refine")
    a, b = o13.numpy(stream), o3.numpy(stream)
    return PnpRefineResult(a[:12].reshape(3, 4).copy(), a[12], b[0], mask.numpy(stream).astype(bool), b[1], b[2])


def retrieve_frame(ref_desc, query_desc, stream=None):
    """localization_utils.py:432-447: the reference frame most similar to each query, (indices (Q,) int64, scores (Q,) float32), from
    the two existing calls: sim_scores in its exact float32 mode and argmax_f32 (the first maximum over the frames).  ref_desc (N, D)
    float32: pass a resident DeviceArray to upload a scene's descriptors once.  query_desc (D,) or (Q, D); a (D,) query returns
    scalars."""
    _lib.load()
    _lib.require_gpu()
    q = query_desc
    single = False
    if not _is_dev(q):
        q = np.ascontiguousarray(np.asarray(q, dtype=np.float32))
        single = q.ndim == 1
        q = q.reshape(1, -1) if single else q
    if not _is_dev(ref_desc):
        ref_desc = DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(ref_desc, dtype=np.float32)), stream)
    qp, qshape, qk = as_device(q, np.float32, stream)
    if len(qshape) != 2 or len(ref_desc.shape) != 2 or qshape[1] != ref_desc.shape[1]:
        raise ValueError(f"shape mismatch: reference descriptors {tuple(ref_desc.shape)}, queries {tuple(qshape)}")
    N, D = int(ref_desc.shape[0]), int(qshape[1])
    if N < 1:
        raise ValueError("no reference frames")
    idx, val = np.zeros(qshape[0], np.int64), np.zeros(qshape[0], np.float32)
    scores = DeviceArray((N, 1), np.float32)
    for j in range(int(qshape[0])):      # one (N, 1) score column per query: argmax_f32 takes a contiguous vector
        sim_scores(ref_desc, DeviceView(qp + j * D * 4, (1, D), np.float32), want_argmax=False, precision="exact", stream=stream,
                   out_scores=scores, col_support=None)
        idx[j], val[j] = argmax_f32(DeviceView(scores.ptr, (N,), np.float32), stream)
    return (int(idx[0]), float(val[0])) if single else (idx, val)
