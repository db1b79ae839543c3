"""Scalar restatement of the sight ray that the carver, the audit and the vote share (csrc/avl_sightray.h, DESIGN.md 4.14 steps 1 - 10
up to the end points), and the scene helpers of their tests.

A ray's points come from the oracle's pinned depth2pc_pixels and transform_points (oracle/avl_oracle.py); the slab and the end
points are scalar Python in the order the header writes them down.  `stats`, when given, counts what the rays of a call did, so
that a test can assert that its scene really contains the cases it claims to cover."""
import numpy as np

from oracle import avl_oracle as O


def _bump(stats, key, value=None):
    if stats is None:
        return
    if value is None:
        stats[key] = stats.get(key, 0) + 1
    else:
        stats.setdefault(key, set()).add(value)


def ray_segment(z_f32, u, v, Kinv, T, h_min, h_max, min_depth, max_depth, stats=None):
    """-> the reason (a str, also bumped in stats) why the ray of depth z_f32 at pixel (v, u) is skipped whole, or
    (far, t0, t1, O, P, A, B): the ray's kind, its part inside the height band and the points X(0), X(1), X(t0), X(t1)"""
    depth = np.zeros((v + 1, u + 1), np.float32)        # depth2pc_pixels takes pixel v * W + u of an image: one just large enough
    depth[v, u] = z_f32
    pc, _ = O.depth2pc_pixels(depth, Kinv, [v * (u + 1) + u], min_depth, max_depth)
    p = pc[0]

    def skipped(why):
        _bump(stats, why)
        return why
    if not p[2] > min_depth:
        return skipped("dropped")
    far = bool(p[2] >= max_depth)
    if far:
        with np.errstate(invalid="ignore"):                 # an infinite depth gives inf * 0: not finite, skipped below
            s = max_depth / p[2]
            p = np.array([p[0] * s, p[1] * s, p[2] * s])
    Ov = np.array([T[0, 3], T[1, 3], T[2, 3]], dtype=np.float64)
    P = O.transform_points(T, p[None])[0]
    if not (np.all(np.isfinite(Ov)) and np.all(np.isfinite(P))):
        return skipped("not_finite")
    t0, t1 = 0.0, 1.0
    dz = P[2] - Ov[2]
    if Ov[2] == h_max:
        _bump(stats, "camera_at_h_max")
    if dz == 0.0:
        if not (h_min <= Ov[2] <= h_max):
            return skipped("level_outside")
        _bump(stats, "level_inside")
    else:
        ta, tb = (h_min - Ov[2]) / dz, (h_max - Ov[2]) / dz
        t0, t1 = max(0.0, min(ta, tb)), min(1.0, max(ta, tb))
        if not t0 <= t1:
            return skipped("slab_empty")
        if t0 > 0.0:
            _bump(stats, "slab_enters")
            _bump(stats, "enters_from_above" if Ov[2] > h_max else "enters_from_below")
        if t1 < 1.0:
            _bump(stats, "slab_leaves")
        if t0 == 0.0 and t1 == 1.0:
            _bump(stats, "slab_inside")
    dx, dy = P[0] - Ov[0], P[1] - Ov[1]
    A = tuple(Ov) if t0 == 0.0 else (Ov[0] + t0 * dx, Ov[1] + t0 * dy, Ov[2] + t0 * dz)
    B = tuple(P) if t1 == 1.0 else (Ov[0] + t1 * dx, Ov[1] + t1 * dy, Ov[2] + t1 * dz)
    if not all(np.isfinite(w) for w in A[:2] + B[:2]):      # (the z of A and B is for the caller that reads it)
        return skipped("not_finite")
    return far, t0, t1, Ov, P, A, B


# ------------------------------------------------------------------ scene helpers
BASE_FROM_CAM = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])     # camera x right, y down, z forward -> base x forward, y left, z up


def rot_z(deg):
    q = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}.get(deg % 360 if float(deg).is_integer() else None)
    c, s = q if q else (np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg)))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rot_y(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def rot_x(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def camera(origin, yaw=0, pitch=0.0, roll=0.0):
    """camera -> map transform of a camera at `origin` (base frame, metres) looking along the base x axis turned by yaw (about z, to the
    left), pitch (about y, positive = down) and roll (about x).  Quarter-turn yaws are exact."""
    T = np.eye(4)
    R = rot_z(yaw)
    if pitch:
        R = R @ rot_y(pitch)
    if roll:
        R = R @ rot_x(roll)
    T[:3, :3] = R @ BASE_FROM_CAM
    T[:3, 3] = origin
    return T


def calib(f, cx, cy):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
