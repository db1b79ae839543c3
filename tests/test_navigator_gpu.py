"""Visibility-graph navigation on the GPU (csrc/avl_nav.hip through ops.NavGraph, utils.navigation_utils and Navigator) against
hand-built maps with known answers and an independent NumPy oracle.

The oracle does not walk cells.  It lists every primitive of the obstacle set -- every bond (segment between 8-adjacent obstacle
pixels), every fill (triangle or unit square of a 2 x 2 window with 3 or 4 obstacles), every axis bond with fills on both sides
-- and tests every segment against all of them with exact orientation predicates (int64 for vertex pairs, float64 for half-integer
query points, where they are exact too), plus the obstacle pixels lying strictly inside the segment, grouped into bonded runs.
Shortest paths come from a heap Dijkstra in Python floats."""
import heapq
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(ROOT / "tools"))

_NB = [(0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1)]     # E, NE, N, NW, W, SW, S, SE


# ------------------------------------------------------------------ oracle
def oracle_vertices(free):
    """obstacle pixels with >= 1 obstacle 8-neighbour, all within 135 degrees, in raster order -> (V, 2) int64"""
    obs = np.asarray(free) == 0
    H, W = obs.shape
    pad = np.zeros((H + 2, W + 2), bool)
    pad[1:-1, 1:-1] = obs
    nb = [pad[1 + dr:1 + dr + H, 1 + dc:1 + dc + W] for dr, dc in _NB]
    out = []
    for r, c in zip(*np.nonzero(obs)):
        m = [bool(n[r, c]) for n in nb]
        if not any(m):
            continue
        # the occupied directions fit in 4 consecutive ones <=> 4 consecutive free ones
        if any(not any(m[(k + q) % 8] for q in range(4)) for k in range(8)):
            out.append((r, c))
    return np.array(out, np.int64).reshape(-1, 2)


class Primitives:
    def __init__(self, free):
        obs = np.asarray(free) == 0
        self.obs = obs
        H, W = obs.shape
        A, B = [], []
        for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
            for r, c in zip(*np.nonzero(obs)):
                rr, cc = r + dr, c + dc
                if 0 <= rr < H and 0 <= cc < W and obs[rr, cc]:
                    A.append((r, c))
                    B.append((rr, cc))
        self.bA = np.array(A, np.int64).reshape(-1, 2)
        self.bB = np.array(B, np.int64).reshape(-1, 2)
        tris, squares = [], []
        cnt = np.zeros((H + 1, W + 1), int)          # cnt[r + 1, c + 1] = obstacles of the window with top-left (r, c)
        for r in range(H - 1):
            for c in range(W - 1):
                corners = [(r, c), (r, c + 1), (r + 1, c + 1), (r + 1, c)]   # ring order
                on = [p for p in corners if obs[p]]
                cnt[r + 1, c + 1] = len(on)
                if len(on) == 4:
                    squares.append(corners)
                elif len(on) == 3:
                    tris.append(on)
        self.polys = [np.array(p, np.int64) for p in tris + squares]
        # axis bonds with a fill on both sides: their open segment is interior to the union of the fills
        ie = []
        for (r, c), (rr, cc) in zip(self.bA, self.bB):
            if rr == r and cc == c + 1:
                if cnt[r, c + 1] >= 3 and cnt[r + 1, c + 1] >= 3:
                    ie.append(((r, c), (rr, cc)))
            elif cc == c and rr == r + 1:
                if cnt[r + 1, c] >= 3 and cnt[r + 1, c + 1] >= 3:
                    ie.append(((r, c), (rr, cc)))
        self.ie = np.array(ie, np.int64).reshape(-1, 2, 2)
        self.obs_pts = np.argwhere(obs).astype(np.int64)
        P = self.polys
        if P:
            # polygons as (K, 4, 2) with triangles padded by repeating their last corner, oriented counter-clockwise in (r, c)
            arr = np.array([np.vstack([p, p[-1:]]) if len(p) == 3 else p for p in P])
            area = np.array([_area(p) for p in P])
            arr[area < 0] = arr[area < 0][:, ::-1]
            self.poly_arr = arr
            self.poly_n = np.array([len(p) for p in P])
        else:
            self.poly_arr = np.zeros((0, 4, 2), np.int64)
            self.poly_n = np.zeros(0, int)


def _area(p):
    s = 0
    for k in range(len(p)):
        a, b = p[k], p[(k + 1) % len(p)]
        s += a[0] * b[1] - a[1] * b[0]
    return s


def _orient(a, b, c):
    """(b - a) x (c - a), broadcasting over leading axes; last axis = (r, c)"""
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])


def oracle_blocked(prim: Primitives, P, Q):
    """P (2,), Q (n, 2) -> (n,) bool blocked, the segment P -> Q[k] against every primitive"""
    P = np.asarray(P)
    Q = np.asarray(Q)
    n = len(Q)
    dtype = np.float64 if (P.dtype.kind == "f" or Q.dtype.kind == "f") else np.int64
    P = P.astype(dtype)
    Q = Q.astype(dtype)
    Pb = np.broadcast_to(P, Q.shape)
    blocked = np.zeros(n, bool)
    # (b) proper crossings of bonds
    if len(prim.bA):
        A = prim.bA.astype(dtype)[None]
        B = prim.bB.astype(dtype)[None]
        p, q = Pb[:, None], Q[:, None]
        o1, o2 = np.sign(_orient(p, q, A)), np.sign(_orient(p, q, B))
        o3, o4 = np.sign(_orient(A, B, p)), np.sign(_orient(A, B, q))
        blocked |= ((o1 * o2 < 0) & (o3 * o4 < 0)).any(axis=1)
    # (a) open interiors of the fills: separated by an edge line or by the segment's line, else they meet
    if len(prim.poly_arr):
        V = prim.poly_arr.astype(dtype)                       # (K, 4, 2), ccw; padded triangles repeat a corner
        K = len(V)
        sep = np.zeros((n, K), bool)
        p, q = Pb[:, None, None], Q[:, None, None]
        Vi, Vj = V[None, :, :, :], np.roll(V, -1, axis=1)[None]
        degenerate = (Vi == Vj).all(-1)                       # the padding edge
        e_sep = (_orient(Vi, Vj, p) <= 0) & (_orient(Vi, Vj, q) <= 0) & ~degenerate
        sep |= e_sep.any(-1)
        ov = _orient(Pb[:, None, None], Q[:, None, None], V[None])
        sep |= (ov >= 0).all(-1) | (ov <= 0).all(-1)
        blocked |= (~sep).any(axis=1)
    # (a) interior edges: collinear overlap of positive length
    if len(prim.ie):
        A = prim.ie[:, 0].astype(dtype)[None]
        B = prim.ie[:, 1].astype(dtype)[None]
        p, q = Pb[:, None], Q[:, None]
        col = (_orient(p, q, A) == 0) & (_orient(p, q, B) == 0)
        d = q - p
        L = (d * d).sum(-1)
        tA = ((A - p) * d).sum(-1)
        tB = ((B - p) * d).sum(-1)
        lo = np.maximum(np.minimum(tA, tB), 0)
        hi = np.minimum(np.maximum(tA, tB), L)
        blocked |= (col & (lo < hi)).any(axis=1)
    # (c) runs of obstacle pixels strictly inside the segment with obstacle neighbours strictly on both sides
    X = prim.obs_pts.astype(dtype)[None]
    p, q = Pb[:, None], Q[:, None]
    d = q - p
    L = (d * d).sum(-1)
    t = ((X - p) * d).sum(-1)
    on = (_orient(p, q, X) == 0) & (t > 0) & (t < L)
    H, W = prim.obs.shape
    for k in np.nonzero(on.any(axis=1) & ~blocked)[0]:
        idx = np.nonzero(on[k])[0]
        pts = prim.obs_pts[idx][np.argsort(t[k, idx])]
        run_sides, prev = set(), None
        for x in pts:
            if prev is None or np.abs(x - prev).max() > 1:
                run_sides = set()
            for dr, dc in _NB:
                rr, cc = x[0] + dr, x[1] + dc
                if 0 <= rr < H and 0 <= cc < W and prim.obs[rr, cc]:
                    o = _orient(P, Q[k], np.array([rr, cc], dtype))
                    if o != 0:
                        run_sides.add(o > 0)
            if len(run_sides) == 2:
                blocked[k] = True
                break
            prev = x
    return blocked


def oracle_visibility(free, verts):
    prim = Primitives(free)
    V = len(verts)
    vis = np.zeros((V, V), bool)
    for a in range(V - 1):
        b = np.arange(a + 1, V)
        vis[a, b] = ~oracle_blocked(prim, verts[a], verts[b])
    return vis | vis.T, prim


def _len(a, b):
    dr, dc = float(b[0]) - float(a[0]), float(b[1]) - float(a[1])
    return math.sqrt(dr * dr + dc * dc)


def oracle_spans(free, verts):
    """per vertex the clockwise-most and counter-clockwise-most obstacle-neighbour directions (at most 135 degrees apart)"""
    obs = np.asarray(free) == 0
    H, W = obs.shape
    out = []
    for r, c in verts:
        occ = [0 <= r + dr < H and 0 <= c + dc < W and obs[r + dr, c + dc] for dr, dc in _NB]
        e1 = [k for k in range(8) if occ[k] and not any(occ[(k - q) % 8] for q in range(1, 5))][0]
        e2 = [k for k in range(8) if occ[k] and not any(occ[(k + q) % 8] for q in range(1, 5))][0]
        out.append((_NB[e1], _NB[e2]))
    return out


def _in_span(span, d):
    """direction d strictly between the span's extreme directions (the span is < 180 degrees)"""
    (ar, ac), (br, bc) = span
    return ar * d[1] - ac * d[0] > 0 and d[0] * bc - d[1] * br > 0


def _run_bad(obs, a, b):
    """the edge from vertex a towards b lies along a wall from a: a, then obstacle pixels one unit step apart on the segment (up to
    b), and their obstacle neighbours off the segment's line are on both sides of it.  A path bends at a on the side away from
    a's neighbours, so such an edge could only carry it through the wall."""
    H, W = obs.shape
    dr, dc = float(b[0]) - float(a[0]), float(b[1]) - float(a[1])
    if not (dr == 0 or dc == 0 or abs(dr) == abs(dc)):
        return False
    sr, sc = int(np.sign(dr)), int(np.sign(dc))
    m = int(math.floor(max(abs(dr), abs(dc))))
    first = (int(a[0]) + sr, int(a[1]) + sc)
    if m < 1 or not (0 <= first[0] < H and 0 <= first[1] < W and obs[first]):
        return False                         # the edge leaves a without running along a bond: a contact at a only
    sides = set()
    for p in range(m + 1):
        x = (int(a[0]) + p * sr, int(a[1]) + p * sc)
        if not (0 <= x[0] < H and 0 <= x[1] < W and obs[x]):
            break
        for er, ec in _NB:
            rr, cc = x[0] + er, x[1] + ec
            o = sr * ec - sc * er
            if o != 0 and 0 <= rr < H and 0 <= cc < W and obs[rr, cc]:
                sides.add(o > 0)
    return len(sides) == 2


def oracle_plan(prim, verts, vis, s, g):
    """heap Dijkstra over vertices + start (id V) + goal (id V + 1) -> dist (V + 2,), pred (smallest id among ties), qvis, sg.
    An edge is used only where it leaves each of its vertices outside the span of that vertex's obstacle neighbours, and not along
    a wall whose neighbours lie on both sides of it (_run_bad)."""
    V = len(verts)
    s, g = np.array(s, np.float64), np.array(g, np.float64)
    qvis = np.zeros((2, V), bool)
    if V:
        qvis[0] = ~oracle_blocked(prim, s, verts.astype(np.float64))
        qvis[1] = ~oracle_blocked(prim, g, verts.astype(np.float64))
    sg = bool(~oracle_blocked(prim, s, g[None])[0])
    pos = [tuple(v) for v in verts] + [tuple(s), tuple(g)]
    spans = oracle_spans(~prim.obs, verts)

    def leaves(a, b):                        # the edge a -> b leaves vertex a outside its span and not along a wall it crosses
        if a >= V:                           # (the start and the goal: always)
            return True
        return not _in_span(spans[a], (pos[b][0] - pos[a][0], pos[b][1] - pos[a][1])) and not _run_bad(prim.obs, pos[a], pos[b])
    adj = [[] for _ in range(V + 2)]
    for a in range(V):
        for b in np.nonzero(vis[a])[0]:
            if leaves(a, int(b)) and leaves(int(b), a):
                adj[a].append(int(b))
    for k, node in ((0, V), (1, V + 1)):
        for b in np.nonzero(qvis[k])[0]:
            if leaves(int(b), node):
                adj[node].append(int(b))
                adj[int(b)].append(node)
    if sg:
        adj[V].append(V + 1)
        adj[V + 1].append(V)
    dist = [math.inf] * (V + 2)
    dist[V] = 0.0
    heap = [(0.0, V)]
    done = [False] * (V + 2)
    while heap:
        d, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for v in adj[u]:
            nd = d + _len(pos[u], pos[v])
            if nd < dist[v]:
                dist[v] = nd
                heapq.heappush(heap, (nd, v))
    pred = [-1] * (V + 2)
    for v in range(V + 2):
        if v == V or dist[v] == math.inf:
            continue
        for u in sorted(adj[v]):
            if dist[u] + _len(pos[u], pos[v]) == dist[v]:
                pred[v] = u
                break
    return np.array(dist), np.array(pred), qvis, sg


# ------------------------------------------------------------------ helpers
def _graph(free):
    from avlmaps_amd import ops
    return ops.nav_graph(free)


def _id(g, rc):
    v = g.vertices()
    hit = np.nonzero((v[:, 0] == rc[0]) & (v[:, 1] == rc[1]))[0]
    assert len(hit) == 1, (rc, "is not a vertex")
    return int(hit[0])


def _path_len(path):
    d = 0.0
    for a, b in zip(path[:-1], path[1:]):
        d += _len(a, b)
    return d


def _check_path(free, path, dist=None):
    """consecutive points see each other (oracle) and the float64 sum of the legs equals the reported distance"""
    prim = Primitives(free)
    for a, b in zip(path[:-1], path[1:]):
        if a == b:
            continue
        assert not oracle_blocked(prim, np.array(a, np.float64), np.array([b], np.float64))[0], (a, b)
    if dist is not None:
        assert _path_len(path) == dist


# ------------------------------------------------------------------ hand-built maps
def test_empty_map_is_a_straight_line():
    from avlmaps_amd.utils.navigation_utils import plan_to_pos_v2
    free = np.ones((20, 30), bool)
    g = _graph(free)
    assert g.V == 0
    path = plan_to_pos_v2([2.5, 3.5], [17.5, 26.5], free, g)
    assert path == [[2.5, 3.5], [17.5, 26.5]]
    dist, ids = g.plan([2.5, 3.5], [17.5, 26.5])
    assert ids == [0, 1] and dist == math.sqrt(15.0 * 15.0 + 23.0 * 23.0)
    g.close()


def test_solid_block_wraps_two_corners():
    free = np.ones((30, 30), bool)
    free[10:20, 10:20] = False
    g = _graph(free)
    assert sorted(map(tuple, g.vertices().tolist())) == [(10, 10), (10, 19), (19, 10), (19, 19)]
    dist, ids = g.plan([15, 2], [15, 27])
    d1 = math.sqrt(4.0 * 4.0 + 8.0 * 8.0)                     # (15, 2) -> (19, 10): the lower corners are nearer
    assert dist == (d1 + 9.0) + d1
    v = g.vertices()
    assert [tuple(v[k]) for k in ids[1:-1]] == [(19, 10), (19, 19)]
    # a symmetric start and goal: equal lengths both ways, the smaller predecessor id (raster order: the upper corners) wins
    dist, ids = g.plan([14.5, 2], [14.5, 27])
    assert [tuple(v[k]) for k in ids[1:-1]] == [(10, 10), (10, 19)]
    g.close()


def _ring(door=True):
    free = np.ones((40, 40), bool)
    free[10, 10:31] = free[30, 10:31] = False
    free[10:31, 10] = free[10:31, 30] = False
    if door:
        free[20, 30] = True
    return free


def test_ring_wall_with_a_door():
    from avlmaps_amd.navigator import Navigator, NoPathError
    free = _ring(door=True)
    nav = Navigator()
    nav.build_visgraph(free, 100, 200)
    path = nav.plan_to([112, 212], [136, 236])                # start inside the room, goal outside (full-map cells)
    local = [[p[0] - 100, p[1] - 200] for p in path]
    assert local[0] == [12.0, 12.0] and local[-1] == [36.0, 36.0]
    assert any(p in ([19.0, 30.0], [21.0, 30.0]) for p in local), local     # through the door, round one of its tips
    prim = Primitives(free)
    verts = oracle_vertices(free)
    vis, _ = oracle_visibility(free, verts)
    dist, pred, _, _ = oracle_plan(prim, verts, vis, [12, 12], [36, 36])
    _check_path(free, local, dist[-1])
    nav.close()
    nav.build_visgraph(_ring(door=False), 0, 0)
    with pytest.raises(NoPathError):
        nav.plan_to([12, 12], [36, 36])
    with pytest.raises(ValueError):                            # NoPathError is a ValueError
        nav.plan_to([12, 12], [36, 36])
    nav.close()


def test_jogged_closed_ring_is_not_crossable():
    """a closed one-pixel ring whose bottom wall jogs down one row half way: the two pixels of the jog are adjacent vertices, and an
    edge along the bond between them would carry a path from inside to outside"""
    from avlmaps_amd.navigator import Navigator, NoPathError
    free = _ring(door=False)
    free[30, 20:31] = True
    free[31, 20:31] = False
    free[10:32, 30] = False
    nav = Navigator()
    nav.build_visgraph(free, 0, 0)
    for goal in ([36.5, 15.5], [36.5, 25.5], [35, 38], [2, 2]):
        with pytest.raises(NoPathError):
            nav.plan_to([20.5, 20.5], goal)
    assert nav.plan_to([20.5, 20.5], [12, 28])[-1] == [12.0, 28.0]      # inside to inside still plans
    nav.close()


def _line8(free, a, b):
    (r0, c0), (r1, c1) = a, b
    n = max(abs(r1 - r0), abs(c1 - c0), 1)
    for k in range(n + 1):
        free[r0 + round(k * (r1 - r0) / n), c0 + round(k * (c1 - c0) / n)] = False


def _closed_wall_map(seed, H=48, W=48):
    """a closed 8-connected one-pixel polygon (random corners, so jogs and staircases of every slope) plus a few blocks"""
    rng = np.random.default_rng(seed)
    free = np.ones((H, W), bool)
    n = rng.integers(5, 9)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(9, 20, n)
    pts = [(int(H / 2 + r * np.sin(a)), int(W / 2 + r * np.cos(a))) for a, r in zip(ang, rad)]
    for k in range(n):
        _line8(free, pts[k], pts[(k + 1) % n])
    for _ in range(rng.integers(2, 6)):
        r, c = rng.integers(2, H - 6), rng.integers(2, W - 6)
        free[r:r + rng.integers(2, 4), c:c + rng.integers(2, 4)] = False
    return free


@pytest.mark.parametrize("seed", range(10))
def test_paths_never_leave_their_region(seed):
    """free cells in different 4-connected regions are separated by 8-connected walls: the goal must be unreachable.  In the same
    region it must be reached, with the oracle's distance"""
    from scipy import ndimage
    free = _closed_wall_map(seed)
    lab, _ = ndimage.label(free)
    g = _graph(free)
    verts = oracle_vertices(free)
    want, prim = oracle_visibility(free, verts)
    rng = np.random.default_rng(1000 + seed)
    cells = np.argwhere(free)
    for _ in range(6):
        s, t = cells[rng.integers(len(cells))].astype(float), cells[rng.integers(len(cells))].astype(float)
        if (s == t).all():
            continue
        dist, ids = g.plan(s, t)
        same = lab[tuple(s.astype(int))] == lab[tuple(t.astype(int))]
        assert (dist < math.inf) == same, (s.tolist(), t.tolist(), dist)
        odist, opred, _, _ = oracle_plan(prim, verts, want, list(s), list(t))
        lp = g.last_plan()
        assert np.array_equal(lp["dist"], odist) and np.array_equal(lp["pred"], opred)
    g.close()


@pytest.mark.parametrize("kind", ["diagonal", "bent", "staircase"])
def test_thin_8_connected_wall_is_not_crossable(kind):
    """a one-pixel diagonal wall; one with a 135-degree bend, whose bend pixel is a vertex a path must not bend through from the
    concave side (tangent rule); a 2:1 staircase, where every pixel is a vertex and a path must not run along a step's bond from
    one side to the other"""
    free = np.ones((40, 40), bool)
    if kind == "diagonal":
        for k in range(5, 31):
            free[k, k] = False
        s, t, tips = [22, 8], [8, 22], [(5, 5), (30, 30)]
    elif kind == "bent":
        for k in range(5, 16):
            free[k, k] = False
        free[15, 16:31] = False
        s, t, tips = [8, 20], [22, 8], [(5, 5), (15, 30)]
    else:
        for k in range(3, 18):                                 # (k, 2k), (k, 2k + 1): 8-connected between the steps
            free[k, 2 * k] = free[k, 2 * k + 1] = False
        s, t, tips = [15, 12], [6, 30], [(3, 6), (17, 35)]
    from avlmaps_amd.utils.navigation_utils import plan_to_pos_v2
    g = _graph(free)
    path = plan_to_pos_v2(s, t, free, g)
    lp = g.last_plan()
    assert not lp["sg"]                                        # the straight segment crosses the wall
    assert any(tuple(map(int, p)) in tips for p in path), path
    verts = oracle_vertices(free)
    vis, prim = oracle_visibility(free, verts)
    dist, _, _, _ = oracle_plan(prim, verts, vis, s, t)
    _check_path(free, path, dist[-1])
    g.close()


def _degenerate_map():
    free = np.ones((64, 64), bool)
    free[2:6, 15:19] = False        # B0: bottom-left corner (5, 15)
    free[10:14, 10:14] = False      # B1: top-left corner (10, 10), grazed by (5, 15)-(15, 5)
    free[15:19, 2:6] = False        # B2: top-right corner (15, 5)
    free[20, 30:41] = False         # a straight wall: tips (20, 30) and (20, 40)
    free[30:41, 30] = False         # a wall hanging down from its tip (30, 30)
    free[30, 24:26] = False         # domino: tip (30, 25)
    free[30, 35:37] = False         # domino: tip (30, 35)
    free[25, 24:26] = False         # domino: tip (25, 25)
    free[35, 35:37] = False         # domino: tip (35, 35)
    free[40:61, 50] = False         # a wall crossed at (50, 50)
    free[45, 44:46] = False         # domino: tip (45, 45)
    free[55, 55:57] = False         # domino: tip (55, 55)
    return free


def test_degenerate_visibility_pinned():
    free = _degenerate_map()
    g = _graph(free)
    vis = g.visibility()
    assert np.array_equal(vis, vis.T) and not vis.diagonal().any()
    i = lambda rc: _id(g, rc)                                                # noqa: E731
    assert vis[i((5, 15)), i((15, 5))]                          # grazes the block corner (10, 10)
    assert vis[i((10, 10)), i((10, 13))]                        # runs along the block's top edge
    assert vis[i((20, 30)), i((20, 40))]                        # runs along a thin wall, tip to tip
    assert vis[i((30, 25)), i((30, 35))]                        # passes the wall tip (30, 30) along a row
    assert vis[i((25, 25)), i((35, 35))]                        # passes the wall tip (30, 30) diagonally
    assert not vis[i((45, 45)), i((55, 55))]                    # crosses the wall at the pixel centre (50, 50)
    verts = oracle_vertices(free)
    assert np.array_equal(g.vertices(), verts)
    want, _ = oracle_visibility(free, verts)
    assert np.array_equal(vis, want)
    g.close()


def test_start_and_goal_cases():
    from avlmaps_amd.utils.navigation_utils import plan_to_pos_v2
    free = np.ones((30, 30), bool)
    free[10:20, 10:20] = False
    g = _graph(free)
    # start == goal: pyvisgraph's shortest_path returns the origin alone
    assert plan_to_pos_v2([3, 4], [3, 4], free, g) == [[3.0, 4.0]]
    # start on an obstacle: the nearest free cell (first in np.where order among the nearest), listed twice
    path = plan_to_pos_v2([12.2, 11.0], [25, 25], free, g)
    assert path[0] == path[1] == [12.0, 9.0]
    _check_path(free, path[1:])
    # goal on an obstacle: the same snap
    path = plan_to_pos_v2([2, 2], [18.6, 14.0], free, g)
    assert path[-1] == [20.0, 14.0] and path[0] == [2.0, 2.0]
    _check_path(free, path)
    with pytest.raises(ValueError):
        plan_to_pos_v2([-1, 2], [3, 3], free, g)
    g.close()
    # a map with obstacles but 0 vertices (isolated pixels block nothing)
    free = np.ones((16, 16), bool)
    free[4, 4] = free[8, 9] = False
    g = _graph(free)
    assert g.V == 0
    path = plan_to_pos_v2([0, 0], [12, 13.5], free, g)
    assert path == [[0.0, 0.0], [12.0, 13.5]]
    g.close()


def test_vertex_cap_is_an_error_not_a_crash():
    from avlmaps_amd import _lib, ops
    free = np.ones((420, 480), bool)
    free[::2, ::3] = False                                     # horizontal dominoes: both pixels are wall tips
    free[::2, 1::3] = False
    assert len(oracle_vertices(free[:40, :48])) == 2 * 20 * 16
    with pytest.raises(_lib.AvlError, match="65536"):
        ops.nav_graph(free)


# ------------------------------------------------------------------ random maps against the oracle
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


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_maps_match_the_oracle(seed):
    free = _random_map(seed)
    g = _graph(free)
    verts = oracle_vertices(free)
    assert 200 <= len(verts) <= 400, len(verts)
    assert np.array_equal(g.vertices(), verts)
    want, prim = oracle_visibility(free, verts)
    got = g.visibility()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(tuple(verts[a]), tuple(verts[b]), bool(got[a, b])) for a, b in bad[:10]]
    rng = np.random.default_rng(100 + seed)
    for q in range(4):
        s = _half_free_point(rng, free)
        t = _half_free_point(rng, free) if q % 2 == 0 else list(map(float, np.argwhere(free)[rng.integers(0, free.sum())]))
        dist, ids = g.plan(s, t)
        lp = g.last_plan()
        odist, opred, oq, osg = oracle_plan(prim, verts, want, s, t)
        assert np.array_equal(lp["qvis"], oq)
        assert lp["sg"] == osg
        assert np.array_equal(lp["dist"], odist)               # exactly: the fixpoint of the rounds is Dijkstra's
        assert np.array_equal(lp["pred"], opred)
        if dist < math.inf:
            pts = [s if k == g.V else (t if k == g.V + 1 else verts[k].astype(float).tolist()) for k in ids]
            _check_path(free, pts, dist)
    g.close()


@pytest.mark.parametrize("seed", range(8))
def test_dense_clutter_matches_the_oracle(seed):
    """small maps with 25 % noise: touching blocks, stubs and diagonal contacts everywhere -- the degenerate cases in bulk"""
    free = _random_map(seed, H=14, W=16, blocks=2, walls=3, noise=0.25)
    g = _graph(free)
    verts = oracle_vertices(free)
    assert np.array_equal(g.vertices(), verts)
    want, prim = oracle_visibility(free, verts)
    assert np.array_equal(g.visibility(), want)
    rng = np.random.default_rng(seed)
    s, t = _half_free_point(rng, free), _half_free_point(rng, free)
    g.plan(s, t)
    lp = g.last_plan()
    odist, opred, oq, osg = oracle_plan(prim, verts, want, s, t)
    assert np.array_equal(lp["qvis"], oq) and lp["sg"] == osg
    assert np.array_equal(lp["dist"], odist) and np.array_equal(lp["pred"], opred)
    g.close()


def test_vertices_over_two_compaction_blocks():
    """33 x 37 = 1221 pixels: a second block of the vertex compaction (1024 pixels each) whose only round ends inside a wave"""
    free = _random_map(11, H=33, W=37, blocks=6, walls=8, noise=0.1)
    g = _graph(free)
    verts = oracle_vertices(free)
    assert len(verts) > 64 and (verts[:, 0] * 37 + verts[:, 1] >= 1024).any()
    assert np.array_equal(g.vertices(), verts)
    g.close()


def test_vertices_over_two_rounds_of_the_block_count_scan():
    """520 x 512 = 266 240 pixels are 260 compaction blocks of 1024, more than the 256 threads of the one-workgroup scan of the block
    counts: the vertices of the last four blocks (rows 512 and below) are written behind the total that the first round carries"""
    free = _random_map(12, H=520, W=512, noise=0.0)           # the seed puts five of the 140 vertices there
    verts = oracle_vertices(free)
    assert (verts[:, 0] * 512 + verts[:, 1] >= 256 * 1024).any()
    g = _graph(free)
    assert np.array_equal(g.vertices(), verts)
    g.close()


def test_plans_reuse_the_graph():
    free = _random_map(7)
    rng = np.random.default_rng(7)
    from avlmaps_amd.navigator import Navigator
    nav = Navigator()
    nav.build_visgraph(free, 5, 9)
    pairs = [(_half_free_point(rng, free), _half_free_point(rng, free)) for _ in range(5)]
    pairs = [([s[0] + 5, s[1] + 9], [t[0] + 5, t[1] + 9]) for s, t in pairs]
    from avlmaps_amd.utils.navigation_utils import NoPathError

    def run(n, s, t):
        try:
            return n.plan_to(s, t)
        except NoPathError:
            return None
    reused = [run(nav, s, t) for s, t in pairs]
    for (s, t), want in zip(pairs, reused):
        fresh = Navigator()
        fresh.build_visgraph(free, 5, 9)
        assert run(fresh, s, t) == want
        fresh.close()
    nav.close()


# ------------------------------------------------------------------ end to end
def _scene(tmp_path):
    import yaml
    from make_synth_dataset import make
    scene = make(tmp_path / "scene", frames=6, H=96, W=128)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                  "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    from avlmaps_amd.apps import create_map
    create_map.main(["--data-dir", str(scene), "--config", str(cfg), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    return scene, cfg


def test_end_to_end_name_to_path(tmp_path):
    from avlmaps_amd.apps.common import HashClip, load_config
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.navigator import Navigator
    scene, cfg = _scene(tmp_path)
    vm = VLMap(load_config(str(cfg)).map_config, data_dir=str(scene))
    assert vm.load_map(str(scene))
    vm.clip_feat_dim = vm.grid_feat.shape[1]
    vm.clip_model = HashClip(vm.clip_feat_dim)
    vm.init_categories(["sofa", "other"])
    vm.generate_obstacle_map()
    obs = vm.obstacles_cropped
    free_cells = np.argwhere(obs)
    start = [float(free_cells[0][0] + vm.rmin), float(free_cells[0][1] + vm.cmin)]
    goal = vm.get_nearest_pos(start, "sofa")
    nav = Navigator()
    nav.build_visgraph(obs, vm.rmin, vm.cmin)
    path = nav.plan_to(start, goal)
    assert path[0] == start and len(path) >= 1                # the start is a free cell: no snap, listed once
    local = [[p[0] - vm.rmin, p[1] - vm.cmin] for p in path]
    _check_path(obs, local)
    nav.close()
    r = subprocess.run([sys.executable, "-m", "avlmaps_amd.apps.plan_path", "--data-dir", str(scene), "--config", str(cfg),
                        "--query", "sofa", "--start", str(start[0]), str(start[1]), "--text-model", "hash"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["path"] == [[float(a), float(b)] for a, b in path] and out["goal"] == [float(goal[0]), float(goal[1])]
