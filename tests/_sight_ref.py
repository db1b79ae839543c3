"""Scalar restatement of the cell-to-cell line of sight (csrc/avl_sight.hip) for the tests: the cell index as
_audit_ref.cell_dict's dict, the sight line as _audit_ref.walk3 from the eye to the target, the blockers as a Python loop in the
order DESIGN writes them down.

`stats`, when given, counts what the pairs of a call did (as _audit_ref.fold's does), so that a test can assert that its scene
really contains the cases it claims to cover."""
import numpy as np

from _audit_ref import cell_dict, walk3
from _ray_ref import _bump

VISIBLE, INVALID = -1, -2


def inside(x, gs, vh):
    return 0 <= x[0] < gs and 0 <= x[1] < gs and 0 <= x[2] < vh


def first_blocker(index, gs, vh, e, t, transparent=None, end_margin=0, stats=None, shared=()):
    """one pair: VISIBLE, INVALID or the voxel row of the blocker with the smallest k.  shared: the cells more than one row lies in"""
    e, t = tuple(int(v) for v in e), tuple(int(v) for v in t)
    if not (inside(e, gs, vh) and inside(t, gs, vh)):
        _bump(stats, "invalid")
        for which, x in (("eye", e), ("target", t)):
            for k, lim in enumerate((gs, gs, vh)):
                if not 0 <= x[k] < lim:
                    _bump(stats, "invalid_kinds", (which, k, "low" if x[k] < 0 else "high"))
        return INVALID
    cells = walk3(e, t)
    d = [abs(t[k] - e[k]) for k in range(3)]
    n = max(d)
    assert len(cells) == n + 1 and cells[0] == e and cells[-1] == t and all(inside(x, gs, vh) for x in cells)
    if n == 0:
        _bump(stats, "point")
    elif sorted(d)[1] == 0:
        _bump(stats, "axis_aligned", d.index(n))
    elif sorted(d)[0] == n or (sorted(d)[0] == 0 and sorted(d)[1] == n):
        _bump(stats, "diagonal")
    if min(d) > 0:
        _bump(stats, "octants", (d.index(n), t[0] > e[0], t[1] > e[1], t[2] > e[2]))
    if e in index and n > 0:
        _bump(stats, "eye_occupied")
    if n <= end_margin + 1:
        _bump(stats, "nothing_tested")
    skipped = 0
    for k in range(1, n - end_margin):
        i = index.get(cells[k])
        if i is None:
            continue
        if transparent is not None and transparent[i] != 0:
            skipped += 1
            continue
        _bump(stats, "blocked")
        if skipped:
            _bump(stats, "blocked_behind_transparent")
        if cells[k] in shared:
            _bump(stats, "blocked_by_shared_cell")
        if any(index.get(x) is not None and (transparent is None or transparent[index[x]] == 0) for x in cells[k + 1:n - end_margin]):
            _bump(stats, "second_blocker_behind")
        return i
    _bump(stats, "visible")
    if skipped:
        _bump(stats, "visible_through_transparent")
    if any(x in index for x in cells[max(n - end_margin, 1):n]):
        _bump(stats, "occupied_inside_margin")
    if t in index:
        _bump(stats, "target_occupied")
    return VISIBLE


def _shared_cells(grid_pos, gs, vh):
    seen, shared = set(), set()
    for x in map(tuple, np.asarray(grid_pos).reshape(-1, 3).tolist()):
        (shared if x in seen else seen).add(x)
    return shared


def los_ref(grid_pos, gs, vh, eyes, targets, transparent=None, end_margin=0, stats=None):
    """ops.line_of_sight restated: (M,) int32"""
    index, shared = cell_dict(grid_pos, gs, vh), _shared_cells(grid_pos, gs, vh)
    eyes, targets = np.asarray(eyes).reshape(-1, 3).tolist(), np.asarray(targets).reshape(-1, 3).tolist()
    assert len(eyes) == len(targets)
    return np.array([first_blocker(index, gs, vh, e, t, transparent, end_margin, stats, shared) for e, t in zip(eyes, targets)],
                    dtype=np.int32).reshape(-1)


def counts_ref(grid_pos, gs, vh, eyes, targets, transparent=None, end_margin=0, max_range2=-1, stats=None):
    """ops.visible_counts restated: (visible (E,) uint32, first (E,) int32); max_range2 < 0 = unlimited, Python integers throughout"""
    index = cell_dict(grid_pos, gs, vh)
    eyes, targets = np.asarray(eyes).reshape(-1, 3).tolist(), np.asarray(targets).reshape(-1, 3).tolist()
    visible, first = np.zeros(len(eyes), np.uint32), np.full(len(eyes), -1, np.int32)
    for k, e in enumerate(eyes):
        if not inside(e, gs, vh):
            _bump(stats, "eye_outside")
            continue
        for j, t in enumerate(targets):
            if not inside(t, gs, vh):
                _bump(stats, "target_outside")
                continue
            d2 = sum((int(t[a]) - int(e[a])) ** 2 for a in range(3))
            if max_range2 >= 0:
                _bump(stats, "beyond_range" if d2 > max_range2 else "at_range" if d2 == max_range2 else "within_range")
                if d2 > max_range2:
                    continue
            if first_blocker(index, gs, vh, e, t, transparent, end_margin, stats) == VISIBLE:
                visible[k] += 1
                if first[k] < 0:
                    first[k] = j
    return visible, first
