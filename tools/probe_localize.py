"""GPU box: time the localization kernels (csrc/avl_pnp.hip) and frame retrieval against NumPy on the same box.
Prints one JSON object (and writes it to --out).

    probe_localize.py [--reps 30] [--warmup 3] [--out profiles/localize_probe.txt]

Synthetic scenes of tests/_loc_synth.py with 30 % planted inliers, the default trial budget (ops.PNP_DEFAULT_HYPOTHESES) and
max_error 12, at M' = 200 / 1 000 / 4 000 correspondences:
  lift_<M>               ops.loc_lift of M key points on a 480 x 640 float32 depth image that is already resident
  ransac_<M>             ops.pnp_ransac on resident correspondences (pose, count and per-hypothesis counts copied back)
  refine_<M>             ops.pnp_refine from the RANSAC pose (one launch; mask copied back)
  localize_<M>           lift + RANSAC + refinement as HLocLocalizer._get_relative_pose_with_depth chains them, host arrays in
  numpy_score_loop_<M>   NumPy's inlier count of the SAME hypotheses' poses (the per-hypothesis poses the kernel found), one pose at a
                         time: the scoring half of a NumPy RANSAC over these hypotheses, without its P3P solves (a lower bound);
                         "same" compares its counts with the kernel's wherever the triple had a P3P solution
Retrieval at N = 1 000 / 10 000 reference frames x 4 096-D, one query:
  retrieve_<N>           ops.retrieve_frame on resident descriptors
  retrieve_numpy_<N>     np.argmax(ref @ query) in float32
Every path ends synchronised, so a host clock around each call is a valid time; every figure is the median of `reps` calls after
`warmup`, with the minimum and maximum next to it."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import _loc_synth as S  # noqa: E402
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_morph2d import stats  # noqa: E402


def numpy_score_loop(poses, pts, pix, K):
    return np.array([S.inlier_mask(p, pts, pix, K).sum() for p in poses])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    res = {"n_hyp": ops.PNP_DEFAULT_HYPOTHESES, "max_error": ops.PNP_MAX_ERROR, "inlier_share": 0.3,
           "method": "host clock around synchronised calls, median of reps", "cases": {}, "same": {}}
    c = res["cases"]
    rng = np.random.default_rng(0)
    H, W = 480, 640
    depth = rng.uniform(1.0, 6.0, (H, W)).astype(np.float32)
    ddepth = DeviceArray.from_numpy(depth)
    K_ref = S.camera()
    for m in (200, 1000, 4000):
        sc = S.make_scene(m, 0.3, m)
        pts, pix, K = sc["points"], sc["pixels"], sc["K"]
        dpts, dpix = DeviceArray.from_numpy(pts), DeviceArray.from_numpy(pix)
        kp = np.stack([rng.uniform(0, W, m), rng.uniform(0, H, m)], axis=1)
        c[f"lift_{m}"] = stats(lib, lambda: ops.loc_lift(ddepth, K_ref, kp, pix), a.reps, a.warmup)
        est = ops.pnp_ransac(dpts, dpix, K, want_poses=True)
        c[f"ransac_{m}"] = stats(lib, lambda: ops.pnp_ransac(dpts, dpix, K), a.reps, a.warmup)
        c[f"refine_{m}"] = stats(lib, lambda: ops.pnp_refine(dpts, dpix, est.pose_dev, K), a.reps, a.warmup)
        ref = ops.pnp_refine(dpts, dpix, est.pose_dev, K)

        def localize():
            # key points whose lifted points are the scene's: the lift is timed on the same count, the estimate on the scene
            ops.loc_lift(ddepth, K_ref, kp, pix)
            e = ops.pnp_ransac(pts, pix, K)
            return ops.pnp_refine(pts, pix, e.pose_dev, K)
        c[f"localize_{m}"] = stats(lib, localize, a.reps, a.warmup)
        want = numpy_score_loop(est.hyp_poses, pts, pix, K)
        solved = ~(est.hyp_poses == np.eye(3, 4)).all(axis=(1, 2))      # a triple without a P3P solution keeps [I|0] and count 0
        res["same"][f"counts_{m}"] = bool(np.array_equal(want[solved], est.hyp_counts[solved]) and not est.hyp_counts[~solved].any())
        res["same"][f"solved_{m}"] = int(solved.sum())
        res["same"][f"mask_{m}"] = bool(np.array_equal(ref.mask, sc["planted"]))
        res["cases"][f"refine_{m}"]["iterations"] = ref.iterations
        c[f"numpy_score_loop_{m}"] = stats(lib, lambda: numpy_score_loop(est.hyp_poses, pts, pix, K), max(3, a.reps // 10), 1)
    for n in (1000, 10000):
        refd = rng.standard_normal((n, 4096)).astype(np.float32)
        refd /= np.linalg.norm(refd, axis=1, keepdims=True)
        q = refd[n // 3] + 0.005 * rng.standard_normal(4096).astype(np.float32)
        resident = DeviceArray.from_numpy(refd)
        res["same"][f"retrieve_{n}"] = bool(ops.retrieve_frame(resident, q)[0] == int(np.argmax(refd @ q)) == n // 3)
        c[f"retrieve_{n}"] = stats(lib, lambda: ops.retrieve_frame(resident, q), a.reps, a.warmup)
        c[f"retrieve_numpy_{n}"] = stats(lib, lambda: int(np.argmax(refd @ q)), a.reps, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
