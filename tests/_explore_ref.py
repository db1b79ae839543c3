"""NumPy / scalar restatement of the free-space carver (csrc/avl_explore.hip) and of the frontier mask, for the tests.

A ray up to its end points is _ray_ref.ray_segment (the oracle's pinned depth2pc_pixels and transform_points, the slab in scalar
Python), shared with _audit_ref.py; its cells come from the oracle's base_pos2grid_id_3d and the walk is a scalar Python loop in the
order DESIGN.md 4.14 writes it down.  `stats`, when given, counts what the rays of a call did, so that a test can assert that its
scene really contains the cases it claims to cover.  The scene helpers of _ray_ref.py are re-exported here."""
import numpy as np

from oracle import avl_oracle as O

from _ray_ref import BASE_FROM_CAM, _bump, calib, camera, ray_segment, rot_x, rot_y, rot_z  # noqa: F401

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


def ray_cells(z_f32, u, v, Kinv, T, gs, cs, h_min, h_max, min_depth, max_depth, stats=None):
    """the cells one ray marks (the camera cell not included)"""
    seg = ray_segment(z_f32, u, v, Kinv, T, h_min, h_max, min_depth, max_depth, stats)
    if isinstance(seg, str):
        return []
    far, _, t1, _, _, A, B = seg
    a, b = cell(gs, cs, A[0], A[1]), cell(gs, cs, B[0], B[1])
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
