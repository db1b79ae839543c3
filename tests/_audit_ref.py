"""Scalar restatement of the visibility audit (csrc/avl_audit.hip) for the tests: the cell index as a dict, the ray
and its 3-D walk as a Python loop in the order DESIGN writes them down.

A ray up to its end points is _ray_ref.ray_segment, the one _explore_ref.py starts from; its cells come from the oracle's pinned
base_pos2grid_id_3d (oracle/avl_oracle.py).  The scene helpers of _ray_ref.py are re-exported here.  `stats`, when given, counts
what the rays of a call did, so that a test can assert that its scene really contains the cases it claims to cover."""
import numpy as np

from oracle import avl_oracle as O

from _explore_ref import walk as walk2d  # noqa: F401
from _ray_ref import _bump, calib, camera, ray_segment, rot_x, rot_y, rot_z  # noqa: F401

NEVER = -1
MAX_CELL = 1 << 28


def cell_dict(grid_pos, gs, vh):
    """{(row, col, h): voxel row}: rows outside the grid are left out, the largest row of a cell owns it"""
    index = {}
    for i, (r, c, h) in enumerate(np.asarray(grid_pos).reshape(-1, 3).tolist()):
        if 0 <= r < gs and 0 <= c < gs and 0 <= h < vh:
            index[(r, c, h)] = i            # rows come in increasing order: the last one written is the largest
    return index


def lookup_ref(grid_pos, gs, vh, cells):
    index = cell_dict(grid_pos, gs, vh)
    return np.array([index.get(tuple(c), -1) for c in np.asarray(cells).reshape(-1, 3).tolist()], dtype=np.int32).reshape(-1)


def walk3(a, b):
    """the n + 1 cells of the driving-axis walk from a to b, not clipped to any grid"""
    x = list(a)
    d = [abs(b[k] - a[k]) for k in range(3)]
    s = [1 if b[k] > a[k] else -1 for k in range(3)]
    n = max(d)
    drive = d.index(n)                      # the first of (row, col, h) with d == n
    e = [2 * d[k] - n for k in range(3)]
    out = []
    for _ in range(n + 1):
        out.append(tuple(x))
        for k in range(3):
            if k == drive:
                continue
            if e[k] > 0:
                x[k] += s[k]
                e[k] -= 2 * n
            e[k] += 2 * d[k]
        x[drive] += s[drive]
    return out


def ray(z_f32, u, v, Kinv, T, gs, vh, cs, h_min, h_max, min_depth, max_depth, stats=None):
    """-> None for a ray that is skipped whole, else (cells, n, has_end, is_hit): the cells the walk visits inside the grid, in
    order (cells[k] is step k), the walk's length n, and the ray's kind"""
    seg = ray_segment(z_f32, u, v, Kinv, T, h_min, h_max, min_depth, max_depth, stats)
    if isinstance(seg, str):
        return None
    far, _, t1, _, P, A, B = seg
    if not (np.isfinite(A[2]) and np.isfinite(B[2])):
        _bump(stats, "not_finite")
        return None

    def cell(X):
        row, col, _ = O.base_pos2grid_id_3d(gs, cs, X[0], X[1], 0.0)
        hu = int(X[2] / cs)                                 # truncating: the builder's base_pos2grid_id_3d
        assert hu == O.base_pos2grid_id_3d(gs, cs, 0.0, 0.0, X[2])[2]
        return (int(row), int(col), min(max(hu, 0), vh - 1)), hu
    (a, _), (b, bhu) = cell(A), cell(B)
    if not (0 <= a[0] < gs and 0 <= a[1] < gs):
        _bump(stats, "starts_outside")
        return None
    if abs(b[0]) > MAX_CELL or abs(b[1]) > MAX_CELL:
        _bump(stats, "too_far")
        return None
    has_end = (not far) and t1 == 1.0
    b_in = 0 <= b[0] < gs and 0 <= b[1] < gs
    is_hit = has_end and 0 <= bhu < vh and b_in
    _bump(stats, "far" if far else "has_end" if has_end else "cut")
    if is_hit:
        _bump(stats, "hit")
        if -cs < P[2] < 0.0:
            _bump(stats, "hit_below_zero")
    if has_end and b_in and bhu >= vh:
        _bump(stats, "end_above_grid")
    d = [abs(b[k] - a[k]) for k in range(3)]
    n = max(d)
    if n == 0:
        _bump(stats, "point")
    elif sorted(d)[1] == 0:
        _bump(stats, "axis_aligned", d.index(n))
    elif sorted(d)[1] == n:
        _bump(stats, "diagonal")
    if min(d) > 0:
        _bump(stats, "octants", (d.index(n), b[0] > a[0], b[1] > a[1], b[2] > a[2]))
    cells = []
    for x in walk3(a, b):
        if not (0 <= x[0] < gs and 0 <= x[1] < gs):
            _bump(stats, "leaves_grid")
            break
        assert 0 <= x[2] < vh
        cells.append(x)
    else:
        assert cells[-1] == b and len(cells) == n + 1
    return cells, n, has_end, is_hit


def lattice(H, W, stride):
    return [(v, u) for v in range(stride // 2, H, stride) for u in range(stride // 2, W, stride)]


def hit_cells(rays):
    """the end cells of the hit rays of a trace, a sorted list without repeats (a hit ray starts and ends inside the grid, and a
    walk between two cells of a box never leaves the box: its last cell is its end cell)"""
    return sorted({cells[-1] for _, cells, n, has_end, is_hit in rays if is_hit})


def trace(gs, vh, depth, calib_mat, transforms, frame_ids, cs, stride=4, h_min=None, h_max=None, min_depth=0.1, max_depth=6.0,
          stats=None):
    """the rays of the frames that are not skipped, in frame and lattice order: a list of (frame id, cells, n, has_end, is_hit).
    It does not depend on the voxels: a test traces a scene once and folds it as often as it likes."""
    h_min = -cs if h_min is None else h_min
    h_max = vh * cs if h_max is None else h_max
    depth = np.asarray(depth, dtype=np.float32)
    depth = depth[None] if depth.ndim == 2 else depth
    Kinv = np.linalg.inv(np.asarray(calib_mat, dtype=np.float64).reshape(3, 3))
    Ts = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4)
    out = []
    for f in range(depth.shape[0]):
        for v, u in lattice(depth.shape[1], depth.shape[2], stride):
            got = ray(depth[f, v, u], u, v, Kinv, Ts[f], gs, vh, cs, h_min, h_max, min_depth, max_depth, stats)
            if got is not None:
                out.append((int(frame_ids[f]),) + got)
    return out


def fold(rays, grid_pos, gs, vh, end_margin=2, last_hit=None, through=None, after=None, stats=None):
    """-> (last_hit, through): copies of the given arrays with the traced rays folded in, None where None was given"""
    index = cell_dict(grid_pos, gs, vh)
    last_hit = None if last_hit is None else np.array(last_hit, dtype=np.int32)
    through = None if through is None else np.array(through, dtype=np.uint32)
    for fid, cells, n, has_end, is_hit in rays:
        for k, x in enumerate(cells):
            i = index.get(x)
            if i is None:
                continue
            if k == n and is_hit:
                _bump(stats, "hit_recorded")
                if last_hit is not None:
                    last_hit[i] = max(int(last_hit[i]), fid)
            if (not has_end) or k < n - end_margin:
                if after is None or fid > int(after[i]):
                    _bump(stats, "through_counted")
                    if after is not None:
                        _bump(stats, "after_never" if int(after[i]) == NEVER else "after_next" if fid == int(after[i]) + 1 else "after_later")
                    if through is not None:
                        through[i] += np.uint32(1)
                else:
                    _bump(stats, "after_equal" if fid == int(after[i]) else "after_earlier")
            elif k < n:
                _bump(stats, "inside_margin")
    return last_hit, through


def audit_ref(grid_pos, gs, vh, depth, calib_mat, transforms, frame_ids, cs, stride=4, h_min=None, h_max=None, min_depth=0.1,
              max_depth=6.0, end_margin=2, last_hit=None, through=None, after=None, stats=None):
    """ops.audit_rays restated: trace, then fold"""
    rays = trace(gs, vh, depth, calib_mat, transforms, frame_ids, cs, stride, h_min, h_max, min_depth, max_depth, stats)
    return fold(rays, grid_pos, gs, vh, end_margin, last_hit, through, after, stats)
