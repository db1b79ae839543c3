"""CPU-side checks of the 2-D viewshed: the octant rule of ops.octant_of and of the restatement against atan2 and
against each other, the walk of the restatement (it ends on the target and stays in the box), ops.best_heading on hand-made rows,
the argument errors of ops.viewshed_gain / ops.viewshed_seen and of the C entry points, all raised before any device work, and
ExplorationViews' selection on a synthetic table."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import _viewshed_ref as R  # noqa: E402

SYMBOLS = ("avl_viewshed_gain", "avl_viewshed_seen")
N = 33
OFFSETS = [(dr, dc) for dr in range(-N, N + 1) for dc in range(-N, N + 1) if (dr, dc) != (0, 0)]


def test_the_octant_rule_puts_every_offset_in_one_sector_and_agrees_with_atan2():
    from avlmaps_amd import ops
    dr, dc = np.array(OFFSETS).T
    got = ops.octant_of(dr, dc)
    assert got.dtype == np.int64 and got.shape == (len(OFFSETS),) and got.min() == 0 and got.max() == 7
    assert got.tolist() == [R.octant(a, b) for a, b in OFFSETS]                 # the host form and the restatement are one rule
    boundaries = 0
    for (a, b), k in zip(OFFSETS, got.tolist()):
        on_boundary = a == 0 or b == 0 or abs(a) == abs(b)
        if on_boundary:
            # lower-inclusive: the boundary at k * 45 degrees belongs to sector k.  Its direction in integers:
            want = {(0, 1): 0, (1, 1): 1, (1, 0): 2, (1, -1): 3, (0, -1): 4, (-1, -1): 5, (-1, 0): 6, (-1, 1): 7}[(np.sign(a), np.sign(b))]
            boundaries += 1
        else:
            want = int(math.floor((math.degrees(math.atan2(a, b)) % 360.0) / 45.0))
        assert k == want, ((a, b), k, want)
    assert boundaries == 8 * N
    # a quarter turn (dr, dc) -> (dc, -dr) advances two sectors
    assert np.array_equal(ops.octant_of(dc, -dr), (got + 2) % 8)
    # shapes broadcast, the zero offset has no sector, floats are refused
    assert ops.octant_of(np.array([[0], [1]]), np.array([1, 0, -1])).tolist() == [[0, -1, 4], [1, 2, 3]]
    assert int(ops.octant_of(-1, 5)) == 7
    with pytest.raises(TypeError):
        ops.octant_of(1.0, 2)


def test_the_walk_ends_on_the_target_after_n_steps_and_stays_in_the_box():
    assert R.walk((0, 0), (2, 1)) == [(0, 0), (1, 0), (2, 1)]                      # not symmetric: the reverse passes (1, 1)
    assert R.walk((2, 1), (0, 0)) == [(2, 1), (1, 1), (0, 0)]
    assert R.walk((4, 4), (4, 4)) == [(4, 4)]
    e = (40, 50)
    for dr, dc in OFFSETS:
        t = (e[0] + dr, e[1] + dc)
        cells = R.walk(e, t)
        n = max(abs(dr), abs(dc))
        assert len(cells) == n + 1 and cells[0] == e and cells[-1] == t
        assert all(min(e[0], t[0]) <= r <= max(e[0], t[0]) and min(e[1], t[1]) <= c <= max(e[1], t[1]) for r, c in cells)
        steps = {(b[0] - a[0], b[1] - a[1]) for a, b in zip(cells[:-1], cells[1:])}
        assert all(max(abs(s[0]), abs(s[1])) == 1 for s in steps) and len(steps) <= 2          # 8-connected, towards t only


def test_best_heading_on_hand_made_rows():
    from avlmaps_amd import ops
    rows = np.array([[0, 0, 5, 7, 0, 0, 0, 0],           # a plain maximum: sectors 2 + 3
                     [9, 0, 0, 0, 0, 0, 0, 4],           # the run wraps around: sectors 7 + 0
                     [3, 3, 0, 0, 3, 3, 0, 0],           # two equal runs: the first
                     [0, 0, 0, 0, 0, 0, 0, 0],           # nothing anywhere: sector 0, sum 0
                     [1, 0, 0, 0, 0, 0, 0, 1]], np.int32)
    start, total = ops.best_heading(rows)
    assert start.tolist() == [2, 7, 0, 0, 7] and total.tolist() == [12, 13, 6, 0, 2]
    assert start.dtype == np.int64 and total.dtype == np.int64
    assert [R.best_heading_ref(r) for r in rows] == list(zip(start.tolist(), total.tolist()))
    start, total = ops.best_heading(rows, fov_octants=1)
    assert start.tolist() == [3, 0, 0, 0, 0] and total.tolist() == [7, 9, 3, 0, 1]
    start, total = ops.best_heading(rows, fov_octants=8)
    assert start.tolist() == [0] * 5 and total.tolist() == rows.sum(1).tolist()
    assert ops.best_heading(rows[1]) == (7, 13)                                 # one row: two scalars
    start, total = ops.best_heading(np.zeros((0, 8), np.int32))
    assert start.shape == total.shape == (0,)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            ops.best_heading(rows, fov_octants=bad)
    with pytest.raises(ValueError):
        ops.best_heading(np.zeros((3, 7), np.int32))


def test_python_argument_errors_come_before_any_device_work():
    from avlmaps_amd import ops
    ok = np.ones((6, 7), bool)
    eyes = np.array([[1, 2]], np.int32)
    assert ops.VIEWSHED_MAX_RADIUS == 127
    for call in (ops.viewshed_gain, ops.viewshed_seen):
        with pytest.raises(TypeError):
            call(ok.astype(np.int32), ok, eyes, 3)
        with pytest.raises(TypeError):
            call(ok, ok.astype(np.float32), eyes, 3)
        with pytest.raises(ValueError):
            call(ok, np.ones((6, 8), bool), eyes, 3)
        with pytest.raises(ValueError):
            call(np.ones((6,), bool), np.ones((6,), bool), eyes, 3)
        with pytest.raises(ValueError):
            call(np.ones((0, 7), bool), np.ones((0, 7), bool), eyes, 3)
        for radius in (0, 128, -1):
            with pytest.raises(ValueError):
                call(ok, ok, eyes, radius)
        with pytest.raises(TypeError):
            call(ok, ok, eyes, 2.5)
        for bad_eyes in (np.zeros((4, 3), np.int32), np.zeros((2,), np.int32), np.zeros((2, 2, 2), np.int32)):
            with pytest.raises(ValueError):
                call(ok, ok, bad_eyes, 3)
        with pytest.raises(TypeError):
            call(ok, ok, np.zeros((4, 2), np.float32), 3)
        with pytest.raises(TypeError):
            call(ok, ok, np.array([[2 ** 31, 0]], np.int64), 3)
    with pytest.raises(TypeError):
        ops.viewshed_seen(ok, ok, eyes, 3, out=np.zeros((6, 7), bool))
    with pytest.raises(ValueError):
        ops.viewshed_seen(ok, ok, eyes, 3, out=np.zeros((7, 6), np.uint8))


def test_c_entry_points_check_their_arguments_before_any_device_work():
    """made-up (never dereferenced) pointers: every check comes before any device work"""
    from avlmaps_amd import _lib
    lib = _lib.load()
    assert all(s in _lib.EXPORTED_SYMBOLS for s in SYMBOLS)

    def gain(free=1, explored=1, H=8, W=9, eyes=1, E=2, radius=3, ou=0, out=1):
        return lib.avl_viewshed_gain(free, explored, H, W, eyes, E, radius, ou, out, None)

    def seen(free=1, explored=1, H=8, W=9, eyes=1, M=2, radius=3, ou=0, acc=0, out=1):
        return lib.avl_viewshed_seen(free, explored, H, W, eyes, M, radius, ou, acc, out, None)

    for call, name in ((gain, b"avl_viewshed_gain"), (seen, b"avl_viewshed_seen")):
        for kw, word in ((dict(H=0), b"bad shape"), (dict(W=16385), b"bad shape"), (dict(radius=0), b"radius"), (dict(radius=128), b"radius"),
                         (dict(free=None), b"null"), (dict(explored=None), b"null"), (dict(eyes=None), b"null"), (dict(out=None), b"null")):
            assert call(**kw) != 0, kw
            err = lib.avl_last_error()
            assert name in err and word in err, (kw, err)
    assert gain(E=-1) != 0 and b"eyes" in lib.avl_last_error()
    assert seen(M=2 ** 31) != 0 and b"eyes" in lib.avl_last_error()
    assert gain(E=0, free=None, explored=None, eyes=None, out=None) == 0          # no eye: nothing to do, no pointer touched
    assert gain(E=0, radius=0) != 0                                                # but the arguments are still looked at


def test_exploration_views_select_on_a_synthetic_table():
    from avlmaps_amd.map.map import ExplorationViews
    gain = np.zeros((6, 8), np.int32)
    gain[0, 1] = 4
    gain[1, 7], gain[1, 0] = 6, 4           # total 10, heading 7 (wraps)
    gain[2, 3] = 5
    gain[3, 2], gain[3, 3] = 5, 5           # total 10 again
    gain[5, 4] = 1
    cells = np.array([[10, 10], [10, 14], [14, 10], [14, 14], [18, 10], [18, 14]])
    distance = np.array([[3, 0], [9, 1], [0, 2], [2, 6], [1, 1], [0, 0]], np.int32)
    v = ExplorationViews(cells, gain, distance, (8, 8, 20, 20), 12)
    assert len(v) == 6 and v.total.tolist() == [4, 10, 5, 10, 0, 1] and v.heading.tolist() == [0, 7, 2, 2, 0, 3]
    assert v.select().tolist() == [1, 2, 3] and v.select(1.0).tolist() == [1, 3] and v.select(0.0).tolist() == [0, 1, 2, 3, 5]
    assert v.select(0.41).tolist() == [1, 2, 3]                                  # ceil(4.1) = 5: the cell with 4 is out
    assert v.select(0.4).tolist() == [0, 1, 2, 3]
    assert v.best() == 1                                                         # the first of the two tens
    # the nearest selected cell: 0 + 2 sqrt(2) = 2.83 against 9 + sqrt(2) = 10.41 and 2 + 6 sqrt(2) = 10.49
    assert v.nearest() == 2 and v.nearest(1.0) == 1 and v.nearest(0.0) == 5
    with pytest.raises(ValueError):
        v.select(1.5)
    # the order of the pairs is a + b sqrt(2)'s, decided in integers: 7 + 0 sqrt(2) against 0 + 5 sqrt(2) = 7.07
    tie = ExplorationViews(cells[:2], gain[[1, 3]], np.array([[0, 5], [7, 0]], np.int32), (8, 8, 20, 20), 12)
    assert tie.nearest() == 1
    same = ExplorationViews(cells[:2], gain[[1, 3]], np.array([[4, 4], [4, 4]], np.int32), (8, 8, 20, 20), 12)
    assert same.nearest() == 0                                                   # raster order among equals
    none = ExplorationViews(cells, np.zeros((6, 8), np.int32), distance, (8, 8, 20, 20), 12)
    assert none.select().tolist() == [] and none.best() is None and none.nearest() is None
    outside = ExplorationViews(cells[:1], -np.ones((1, 8), np.int32), distance[:1], (8, 8, 20, 20), 12)
    assert outside.select().tolist() == [] and outside.best() is None
    empty = ExplorationViews(np.zeros((0, 2)), np.zeros((0, 8)), np.zeros((0, 2)), (8, 8, 20, 20), 12)
    assert len(empty) == 0 and empty.select().tolist() == [] and empty.best() is None
    with pytest.raises(ValueError):
        ExplorationViews(cells, gain[:5], distance, (8, 8, 20, 20), 12)
