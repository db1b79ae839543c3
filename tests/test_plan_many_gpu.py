"""Many goals from one start on the GPU (avl_navmany_* of csrc/avl_nav.hip through NavGraph.snap / plan_many, navigation_utils,
Navigator and Map.get_nearest_reachable_pos).

The oracle for distances and paths is the single-goal NavGraph.plan, goal by goal, compared with ==: the batch answers every goal
against one shortest-path tree in which no goal node took part, and DESIGN.md 4.6 argues that this changes neither a goal's
distance nor its predecessor chain.  The oracle for snapping is navigation_utils._in_obstacle / _nearest_free."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers (the shapes of tests/test_navigator_gpu.py, restated)
def _graph(free):
    from avlmaps_amd import ops
    return ops.nav_graph(free)


def _ring(door=True):
    free = np.ones((40, 40), bool)
    free[10, 10:31] = free[30, 10:31] = False
    free[10:31, 10] = free[10:31, 30] = False
    if door:
        free[20, 30] = True
    return free


def _block():
    free = np.ones((30, 30), bool)
    free[10:20, 10:20] = False
    return free


def _random_map(seed, H=90, W=96, blocks=22, walls=26, noise=0.05):
    rng = np.random.default_rng(seed)
    free = np.ones((H, W), bool)
    for _ in range(blocks):
        r, c = rng.integers(0, H - 3), rng.integers(0, W - 3)
        free[r:r + rng.integers(2, 7), c:c + rng.integers(2, 7)] = False
    for _ in range(walls):                                     # thin walls, axis and diagonal
        r, c, n = rng.integers(0, H), rng.integers(0, W), rng.integers(3, 15)
        dr, dc = [(0, 1), (1, 0), (1, 1), (1, -1)][rng.integers(0, 4)]
        for k in range(n):
            rr, cc = r + k * dr, c + k * dc
            if 0 <= rr < H and 0 <= cc < W:
                free[rr, cc] = False
    free[rng.random((H, W)) < noise] = False
    return free


def _half_free_point(rng, free):
    H, W = free.shape
    while True:
        r, c = rng.integers(0, H - 1), rng.integers(0, W - 1)
        if free[r:r + 2, c:c + 2].all():
            return [r + 0.5, c + 0.5]


def _len(a, b):
    dr, dc = float(b[0]) - float(a[0]), float(b[1]) - float(a[1])
    return math.sqrt(dr * dr + dc * dc)


def _first_min(dist):
    """the smallest k with the smallest finite distance, -1 when there is none"""
    best = -1
    for k, d in enumerate(dist):
        if d < math.inf and (best < 0 or d < dist[best]):
            best = k
    return best


def _check_against_single_plans(g, s, goals, pm):
    """dist, via and the whole path of every goal against NavGraph.plan, exactly"""
    assert len(pm.dist) == len(pm.via) == len(goals)
    for k, t in enumerate(goals):
        d, ids = g.plan(s, t)
        assert pm.dist[k] == d, (k, list(t), pm.dist[k], d)
        assert pm.path(k) == ids, (k, list(t), pm.path(k), ids)
        assert pm.via[k] == (ids[-2] if ids else -1), (k, list(t), pm.via[k], ids)
    assert pm.best == _first_min(pm.dist)


# ------------------------------------------------------------------ edge sizes
@pytest.mark.parametrize("M", [0, 1, 64, 65])
def test_no_vertices_every_goal_is_a_straight_line(M):
    free = np.ones((8, 8), bool)
    g = _graph(free)
    assert g.V == 0
    rng = np.random.default_rng(M)
    s = [3.25, 4.5]
    goals = rng.uniform(0.0, 7.0, size=(M, 2))
    if M >= 64:
        goals[7] = goals[40] = [0.5, 0.25]                  # the minimum twice: the first index is the best
        goals[63] = [0.0, 7.0]
    pm = g.plan_many(s, goals)
    assert pm.dist.shape == (M,) and pm.dist.dtype == np.float64 and pm.via.shape == (M,) and pm.via.dtype == np.int32
    assert pm.dist.tolist() == [0.0 + _len(s, t) for t in goals]
    assert (pm.via == 0).all()                                # V = 0: the start
    assert pm.best == (int(np.argmin(pm.dist)) if M else -1)
    assert all(pm.path(k) == [0, 1] for k in range(M))
    if M:
        _check_against_single_plans(g, s, goals[:8], g.plan_many(s, goals[:8]))
    g.close()


def _bars_map(n_vertices):
    """separated horizontal two-pixel bars (two vertices each) and, for an odd count, one three-pixel L (three vertices) in the
    first slot; the last bar is the last in raster order -> (free, the last bar's left pixel)"""
    n_l = n_vertices % 2
    n_bars = (n_vertices - 3 * n_l) // 2
    slots = n_bars + n_l
    rows = (slots + 7) // 8
    free = np.ones((4 * rows + 4, 8 * 5 + 4), bool)
    last = None
    for k in range(slots):
        r, c = 2 + 4 * (k // 8), 2 + 5 * (k % 8)
        if k == 0 and n_l:
            free[r, c] = free[r + 1, c] = free[r + 1, c + 1] = False
        else:
            free[r + 1, c] = free[r + 1, c + 1] = False
            last = (r + 1, c)
    return free, last


@pytest.mark.parametrize("V", [63, 64, 65])
def test_word_edges_the_last_vertex_attains(V):
    free, (r, c) = _bars_map(V)
    g = _graph(free)
    assert g.V == V
    verts = g.vertices()
    assert tuple(verts[V - 1]) == (r, c + 1)                   # the right pixel of the last bar
    # from just above the last bar, right of its middle, to just below it: the straight line crosses the bond, the way round the
    # right tip is the shorter one
    s = [r - 1.0, c + 0.75]
    goals = np.array([[r + 1.0, c + 0.75], [r + 1.5, c + 0.75], [r + 1.0, c + 0.25], [0.0, 0.0], [r + 1.0, c + 0.5]])
    pm = g.plan_many(s, goals)
    assert pm.via[0] == V - 1 and pm.via[1] == V - 1 and pm.via[2] == V - 2, pm.via
    assert pm.dist[0] == _len(s, verts[V - 1]) + _len(verts[V - 1], goals[0])
    _check_against_single_plans(g, s, goals, pm)
    g.close()


# ------------------------------------------------------------------ reachability, start and goal cases
def test_a_goal_inside_a_closed_ring_is_never_the_best():
    g = _graph(_ring(door=False))
    s = [20.5, 5.0]
    goals = np.array([[20.0, 12.0], [20.0, 38.0], [20.5, 20.5]])        # the first is the nearest as the crow flies, but inside
    pm = g.plan_many(s, goals)
    assert pm.dist[0] == math.inf and pm.via[0] == -1 and pm.path(0) == []
    assert pm.dist[2] == math.inf and pm.via[2] == -1
    assert pm.best == 1 and pm.dist[1] < math.inf
    _check_against_single_plans(g, s, goals, pm)
    inside = g.plan_many(s, goals[[0, 2]])
    assert inside.best == -1 and np.isinf(inside.dist).all()
    g.close()
    g = _graph(_ring(door=True))
    pm = g.plan_many(s, goals)
    assert np.isfinite(pm.dist).all() and pm.best == 1
    _check_against_single_plans(g, s, goals, pm)
    pm = g.plan_many([20.5, 20.5], goals)                     # from inside, through the door
    assert pm.best == 2 and pm.dist[2] == 0.0
    _check_against_single_plans(g, [20.5, 20.5], goals, pm)
    g.close()


def test_start_equals_goal_duplicates_and_half_integers():
    free = _block()
    g = _graph(free)
    s = [15.0, 2.0]
    goals = np.array([[15.0, 27.0], [15.0, 2.0], [14.5, 27.5], [15.0, 27.0], [21.5, 21.5], [14.5, 27.5], [9.0, 9.0]])
    pm = g.plan_many(s, goals)
    assert pm.dist[1] == 0.0 and pm.via[1] == g.V and pm.best == 1
    assert pm.dist[0] == pm.dist[3] and pm.via[0] == pm.via[3] and pm.path(0) == pm.path(3)
    assert pm.dist[2] == pm.dist[5] and pm.path(2) == pm.path(5)
    _check_against_single_plans(g, s, goals, pm)
    g.close()


def test_a_start_that_snaps_is_listed_twice():
    from avlmaps_amd.utils.navigation_utils import path_lengths, plan_to_nearest_pos, plan_to_pos_v2
    free = _block()
    g = _graph(free)
    s = [12.2, 11.0]                                          # on the block: snaps to (12, 9)
    goals = [[25.0, 25.0], [18.6, 14.0], [12.0, 9.0], [2.0, 27.0]]
    want = [plan_to_pos_v2(s, t, free, g) for t in goals]
    assert all(p[0] == p[1] == [12.0, 9.0] for p in want)
    assert want[2] == [[12.0, 9.0], [12.0, 9.0]]             # the goal is the snapped start
    k, path = plan_to_nearest_pos(s, goals, free, g)
    assert k == 2 and path == want[2]
    for j in (0, 1, 3):
        k, path = plan_to_nearest_pos(s, [goals[j]], free, g)
        assert k == 0 and path == want[j]
    lens = path_lengths(s, goals, free, g)
    for j, p in enumerate(want):
        d = 0.0
        for a, b in zip(p[:-1], p[1:]):
            d += _len(a, b)
        assert lens[j] == d
    g.close()


# ------------------------------------------------------------------ ties
def test_ties_go_to_the_lower_index_and_the_smaller_vertex():
    free = _block()                                           # mirror-symmetric about row 14.5
    g = _graph(free)
    s = [14.5, 2.0]
    up, down, axis = [3.0, 27.0], [26.0, 27.0], [14.5, 27.0]
    for goals in ([up, down], [down, up]):
        pm = g.plan_many(s, np.array(goals))
        assert pm.dist[0] == pm.dist[1] and pm.best == 0
        _check_against_single_plans(g, s, goals, pm)
    pm = g.plan_many(s, np.array([axis]))
    verts = g.vertices()
    ids = pm.path(0)
    assert [tuple(verts[k]) for k in ids[1:-1]] == [(10, 10), (10, 19)]      # both ways are equal: the smaller ids (upper corners)
    lower = _len(s, [19, 10]) + 9.0 + _len([19, 19], axis)
    assert pm.dist[0] == lower                                # the lower way attains the same value
    _check_against_single_plans(g, s, [axis], pm)
    g.close()


# ------------------------------------------------------------------ snapping
def _snap_map():
    free = np.ones((40, 44), bool)
    free[3:18, 20:35] = False                                 # a 15 x 15 block
    free[24, 5] = free[25, 4] = free[25, 5] = False           # window (24, 4): free corner (24, 4), hypotenuse u + v = 1
    free[30, 20] = False                                      # a lone pixel
    free[0:3, 0:3] = False                                    # the map corner
    free[37:40, 41:44] = False                                # the opposite corner
    free[30:33, 30] = False                                   # a short wall
    return free


def _snap_oracle(free, pts):
    from avlmaps_amd.utils.navigation_utils import _in_obstacle, _nearest_free
    moved = [bool(_in_obstacle(free, p)) for p in pts]
    out = [_nearest_free(free, list(p)) if m else [float(p[0]), float(p[1])] for p, m in zip(pts, moved)]
    return np.array(out, np.float64).reshape(-1, 2), np.array(moved, bool)


def test_snap_matches_nearest_free_case_by_case():
    free = _snap_map()
    g = _graph(free)
    cases = {
        "obstacle cell": [30.0, 20.0],
        "obstacle cell, float": [30.3, 20.6],
        "inside the fill, int() cell free": [24.9, 4.9],
        "inside the fill, near the hypotenuse": [24.6, 4.5],
        "on the hypotenuse": [24.5, 4.5],
        "before the hypotenuse": [24.25, 4.5],
        "grid line through the free corner": [24.0, 4.7],
        "grid line, column": [24.6, 4.0],
        "grid line inside the block": [10.0, 27.5],
        "two equally near free cells": [31.0, 30.0],          # (31, 29) and (31, 31): raster-first wins
        "four equally near free cells": [30.0, 20.0],
        "deep inside the block": [10.0, 27.0],               # the centre: 8 cells away from every side
        "deep inside, off centre": [10.4, 26.7],
        "map corner": [0.0, 0.0],
        "map corner, inside": [1.0, 1.0],
        "opposite corner": [39.0, 43.0],
        "opposite corner, inside": [38.5, 42.5],
        "free half-integer point": [20.5, 10.5],
        "free cell": [22.0, 10.0],
    }
    pts = np.array(list(cases.values()))
    want, want_moved = _snap_oracle(free, pts)
    got, moved = g.snap(pts)
    assert got.dtype == np.float64 and moved.dtype == bool
    for k, name in enumerate(cases):
        assert moved[k] == want_moved[k], name
        assert got[k].tolist() == want[k].tolist(), (name, got[k], want[k])
    names = list(cases)
    assert not moved[names.index("on the hypotenuse")] and moved[names.index("inside the fill, near the hypotenuse")]
    assert got[names.index("two equally near free cells")].tolist() == [31.0, 29.0]
    assert got[names.index("map corner")].tolist() == [0.0, 3.0]
    # M = 0 and a batch across several blocks: random points, half of them drawn on obstacle cells
    e, em = g.snap(np.zeros((0, 2)))
    assert e.shape == (0, 2) and em.shape == (0,)
    rng = np.random.default_rng(5)
    rnd = rng.uniform([0, 0], [39, 43], size=(300, 2))
    cells = np.argwhere(~free)
    on = cells[rng.integers(0, len(cells), 300)] + rng.uniform(0, 1, size=(300, 2)) * (rng.random((300, 1)) < 0.5)
    on = np.minimum(on, [39.0, 43.0])
    pts = np.vstack([rnd, on])
    want, want_moved = _snap_oracle(free, pts)
    got, moved = g.snap(pts)
    assert np.array_equal(moved, want_moved) and np.array_equal(got, want)
    g.close()


def test_snap_without_a_free_cell_is_an_error():
    from avlmaps_amd import _lib
    from avlmaps_amd.utils.navigation_utils import NoPathError, path_lengths
    free = np.zeros((6, 7), bool)
    g = _graph(free)
    with pytest.raises(_lib.AvlError, match="no free cell"):
        g.snap([[2.0, 2.0]])
    assert g.snap(np.zeros((0, 2)))[0].shape == (0, 2)
    with pytest.raises(NoPathError):
        path_lengths([1, 1], [[2, 2]], free, g)
    g.close()


# ------------------------------------------------------------------ random maps
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_maps_match_single_plans(seed):
    from avlmaps_amd.utils.navigation_utils import NoPathError, path_lengths, plan_to_pos_v2
    free = _random_map(seed)
    g = _graph(free)
    assert 200 <= g.V <= 400, g.V
    rng = np.random.default_rng(200 + seed)
    s = _half_free_point(rng, free)
    cells = np.argwhere(~free)
    goals = np.array([_half_free_point(rng, free) for _ in range(100)]
                     + cells[rng.integers(0, len(cells), 100)].astype(np.float64).tolist())
    snapped, moved = g.snap(goals)
    want, want_moved = _snap_oracle(free, goals)
    assert np.array_equal(moved, want_moved) and np.array_equal(snapped, want)
    assert not moved[:100].any() and moved[100:].all()
    pm = g.plan_many(s, snapped)
    _check_against_single_plans(g, s, snapped, pm)
    assert np.isfinite(pm.dist).any()
    lens = path_lengths(s, goals, free, g)
    assert np.array_equal(lens, pm.dist)
    for k, t in enumerate(goals):
        try:
            p = plan_to_pos_v2(s, list(t), free, g)
        except NoPathError:
            assert lens[k] == math.inf
            continue
        d = 0.0
        for a, b in zip(p[:-1], p[1:]):
            d += _len(a, b)
        assert lens[k] == d, (k, list(t))
    g.close()


# ------------------------------------------------------------------ interleaving
def test_single_plans_and_batches_interleave():
    free = _random_map(7)
    g = _graph(free)
    rng = np.random.default_rng(7)
    s, t = _half_free_point(rng, free), _half_free_point(rng, free)
    s2 = _half_free_point(rng, free)
    from avlmaps_amd import _lib
    with pytest.raises(_lib.AvlError, match="no batch"):
        g.many_stats()
    d0, ids0 = g.plan(s, t)
    lp0 = g.last_plan()
    goals = np.array([_half_free_point(rng, free) for _ in range(3000)])
    small = g.plan_many(s2, goals[:5])
    lp1 = g.last_plan()                                       # still the single plan
    assert all(np.array_equal(lp0[k], lp1[k]) for k in ("dist", "pred", "qvis")) and lp0["sg"] == lp1["sg"]
    assert g.plan(s, t) == (d0, ids0)
    assert small.path(0) == g.plan(s2, goals[0])[1]           # the batch's tree survived the single plans
    with pytest.raises(_lib.AvlError, match="did not count"):
        g.many_stats()                                        # counting is off by default
    g.count_walks(True)
    big = g.plan_many(s2, goals)                              # grows the buffers
    g.count_walks(False)
    with pytest.raises(ValueError):
        small.path(0)                                         # a newer batch owns the tree
    assert np.array_equal(big.dist[:5], small.dist) and np.array_equal(big.via[:5], small.via)
    assert big.best == _first_min(big.dist)
    stats = g.many_stats()
    assert 0 < stats["walks"] <= stats["candidates"] <= 3000 * g.V
    tail = g.plan_many(s2, goals[-2:])                        # and shrinks again
    assert np.array_equal(tail.dist, big.dist[-2:]) and np.array_equal(tail.via, big.via[-2:])
    _check_against_single_plans(g, s2, goals[-2:], tail)
    with pytest.raises(IndexError):
        tail.path(2)
    assert g.plan(s, t) == (d0, ids0)
    g.close()


# ------------------------------------------------------------------ Map.get_nearest_reachable_pos
def test_nearest_reachable_object_is_not_the_one_behind_the_wall():
    from avlmaps_amd.map.map import Map
    from avlmaps_amd.navigator import Navigator, NoPathError
    rmin, cmin = 100, 200

    def island(r0, c0):                                        # the ring of a 5 x 5 square, full-map coordinates
        pts = [(r0, c0 + k) for k in range(4)] + [(r0 + k, c0 + 4) for k in range(4)] + [(r0 + 4, c0 + 4 - k) for k in range(4)] \
            + [(r0 + 4 - k, c0) for k in range(4)]
        return np.array(pts, np.int64) + [rmin, cmin]

    walled, open_ = island(18, 12), island(2, 33)
    small = np.array([[0, 0], [0, 2], [2, 2], [2, 0]], np.int64) + [rmin + 20, cmin + 3]    # next to the start, too small

    class FixedMap(Map):
        def get_pos(self, name):
            cs = [small, walled, open_] if name == "sofa" else []
            boxes = [[c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max()] for c in cs]
            return cs, [[(b[0] + b[1]) / 2, (b[2] + b[3]) / 2] for b in boxes], boxes

    m = FixedMap.__new__(FixedMap)
    m.cs = 0.05
    nav = Navigator()
    nav.build_visgraph(_ring(door=False), rmin, cmin)
    start = [rmin + 20.0, cmin + 5.0]
    assert m.get_nearest_pos(start, "sofa") == [rmin + 20, cmin + 12]                        # as the crow flies: behind the wall
    pos, path = m.get_nearest_reachable_pos(start, "sofa", nav)
    cand = np.concatenate([walled, open_])
    lens = nav.path_lengths(start, cand)
    assert np.isinf(lens[:len(walled)]).all() and np.isfinite(lens[len(walled):]).all()
    k = int(np.argmin(lens))
    assert pos == cand[k].tolist() and any((open_ == pos).all(axis=1))
    assert path == nav.plan_to(start, pos) and path[0] == start and path[-1] == [float(pos[0]), float(pos[1])]
    assert nav.plan_to_nearest(start, cand) == (k, path)
    with pytest.raises(NoPathError):
        nav.plan_to_nearest(start, walled)
    assert m.get_nearest_reachable_pos(start, "lamp", nav) == (start, [start])
    nav.close()
