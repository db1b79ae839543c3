"""NumPy / scalar restatement of the free-space carver (csrc/avl_explore.hip) and of the frontier mask, for the tests.

A ray's points come from the oracle's pinned depth2pc_pixels, transform_points and base_pos2grid_id_3d (oracle/avl_oracle.py); the
slab and the walk are a scalar Python loop in the order DESIGN.md 4.14 writes them down.  `stats`, when given, counts what the rays
of a call did, so that a test can assert that its scene really contains the cases it claims to cover."""
import numpy as np

from oracle import avl_oracle as O

NEVER = -1
MAX_CELL = 1 << 29


def cell(gs, cs, x, y):
    row, col, _ = O.base_pos2grid_id_3d(gs, cs, x, y, 0.0)
    return int(row), int(col)


def walk(a, b, gs, mark_end):
    """the cells the all-octant integer Bresenham from a to b marks, in order; it stops at the first cell outside the grid"""
    (r, c), (br, bc) = a, b
    dr, dc = abs(br - r), abs(bc - c)
    sr, sc = (1 if br > r else -1), (1 if bc > c else -1)
    err = dc - dr
    out = []
    for _ in range(2 * gs + 1):
        if not (0 <= r < gs and 0 <= c < gs):
            break
        if (r, c) == (br, bc):
            if mark_end:
                out.append((r, c))
            break
        out.append((r, c))
        e2 = 2 * err
        if e2 > -dr:
            err -= dr
            c += sc
        if e2 < dc:
            err += dc
            r += sr
    return out


def _bump(stats, key, value=None):
    if stats is None:
        return
    if value is None:
        stats[key] = stats.get(key, 0) + 1
    else:
        stats.setdefault(key, set()).add(value)


def ray_cells(z_f32, u, v, Kinv, T, gs, cs, h_min, h_max, min_depth, max_depth, stats=None):
    """the cells one ray marks (the camera cell not included)"""
    depth = np.zeros((v + 1, u + 1), np.float32)        # depth2pc_pixels takes pixel v * W + u of an image: one just large enough
    depth[v, u] = z_f32
    pc, _ = O.depth2pc_pixels(depth, Kinv, [v * (u + 1) + u], min_depth, max_depth)
    p = pc[0]
    if not p[2] > min_depth:
        _bump(stats, "dropped")
        return []
    far = bool(p[2] >= max_depth)
    if far:
        with np.errstate(invalid="ignore"):                 # an infinite depth gives inf * 0: not finite, skipped below
            s = max_depth / p[2]
            p = np.array([p[0] * s, p[1] * s, p[2] * s])
    Ov = np.array([T[0, 3], T[1, 3], T[2, 3]], dtype=np.float64)
    P = O.transform_points(T, p[None])[0]
    if not (np.all(np.isfinite(Ov)) and np.all(np.isfinite(P))):
        _bump(stats, "not_finite")
        return []
    t0, t1 = 0.0, 1.0
    dz = P[2] - Ov[2]
    if dz == 0.0:
        if not (h_min <= Ov[2] <= h_max):
            _bump(stats, "level_outside")
            return []
        _bump(stats, "level_inside")
    else:
        ta, tb = (h_min - Ov[2]) / dz, (h_max - Ov[2]) / dz
        t0, t1 = max(0.0, min(ta, tb)), min(1.0, max(ta, tb))
        if not t0 <= t1:
            _bump(stats, "slab_empty")
            return []
        if t0 > 0.0:
            _bump(stats, "slab_enters")
        if t1 < 1.0:
            _bump(stats, "slab_leaves")
        if t0 == 0.0 and t1 == 1.0:
            _bump(stats, "slab_inside")
    dx, dy = P[0] - Ov[0], P[1] - Ov[1]
    ax, ay = (Ov[0], Ov[1]) if t0 == 0.0 else (Ov[0] + t0 * dx, Ov[1] + t0 * dy)
    bx, by = (P[0], P[1]) if t1 == 1.0 else (Ov[0] + t1 * dx, Ov[1] + t1 * dy)
    if not all(np.isfinite(w) for w in (ax, ay, bx, by)):
        _bump(stats, "not_finite")
        return []
    a, b = cell(gs, cs, ax, ay), cell(gs, cs, bx, by)
    if not (0 <= a[0] < gs and 0 <= a[1] < gs):
        _bump(stats, "starts_outside")
        return []
    if abs(b[0]) > MAX_CELL or abs(b[1]) > MAX_CELL:
        _bump(stats, "too_far")
        return []
    hit_end = (not far) and t1 == 1.0
    _bump(stats, "far" if far else "hit")
    dr, dc = abs(b[0] - a[0]), abs(b[1] - a[1])
    kind = ("point" if dr == 0 and dc == 0 else "along_row" if dr == 0 else "along_col" if dc == 0 else "diagonal" if dr == dc else None)
    if kind:
        _bump(stats, kind)
    else:
        _bump(stats, "octants", (b[0] > a[0], b[1] > a[1], dr > dc))
    if not (0 <= b[0] < gs and 0 <= b[1] < gs):
        _bump(stats, "leaves_grid")
    return walk(a, b, gs, not hit_end)


def carve_ref(first_seen, depth, calib, transforms, frame_ids, gs, cs, stride=4, h_min=0.0, h_max=1.5, min_depth=0.1, max_depth=6.0,
              stats=None):
    """-> a new (gs, gs) int32 map: first_seen (None = all NEVER) with the frames folded in"""
    out = np.full((gs, gs), NEVER, np.int32) if first_seen is None else np.array(first_seen, dtype=np.int32)
    depth = np.asarray(depth, dtype=np.float32)
    depth = depth[None] if depth.ndim == 2 else depth
    Kinv = np.linalg.inv(np.asarray(calib, dtype=np.float64).reshape(3, 3))
    Ts = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4)

    def mark(r, c, fid):
        if out[r, c] == NEVER or fid < out[r, c]:
            out[r, c] = fid

    for f in range(depth.shape[0]):
        T, fid = Ts[f], int(frame_ids[f])
        cam = cell(gs, cs, T[0, 3], T[1, 3])
        if 0 <= cam[0] < gs and 0 <= cam[1] < gs:
            mark(cam[0], cam[1], fid)
        H, W = depth.shape[1:]
        for v in range(stride // 2, H, stride):
            for u in range(stride // 2, W, stride):
                for r, c in ray_cells(depth[f, v, u], u, v, Kinv, T, gs, cs, h_min, h_max, min_depth, max_depth, stats):
                    mark(r, c, fid)
    return out


def frontier_ref(free, explored):
    free, explored = np.asarray(free).astype(bool), np.asarray(explored).astype(bool)
    unknown = np.pad(~explored & free, 1)
    near = unknown[:-2, 1:-1] | unknown[2:, 1:-1] | unknown[1:-1, :-2] | unknown[1:-1, 2:]
    return (free & explored & near).astype(np.uint8)


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
