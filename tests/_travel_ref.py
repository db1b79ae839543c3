"""The reference of the travel-distance field, written from the definition alone: the legal-step rule as one
function, the exact integer order of the pairs, a heap Dijkstra on pairs, and the NumPy restatement of the decay map."""
import heapq

import numpy as np

UNREACHED = -1
# (d_row, d_col) of the eight neighbours in the order TravelField.descend looks at them: E, NE, N, NW, W, SW, S, SE
NEIGHBOURS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))


def legal_step(free, sources, u, v):
    """may a walk step from cell u to its 8-neighbour v?  v is free; u is free or a source; for a diagonal step both cells that
    share an edge with u and with v are free"""
    H, W = free.shape
    (ur, uc), (vr, vc) = u, v
    if not (0 <= ur < H and 0 <= uc < W and 0 <= vr < H and 0 <= vc < W):
        return False
    if max(abs(ur - vr), abs(uc - vc)) != 1:
        return False
    if not free[vr, vc] or not (free[ur, uc] or sources[ur, uc]):
        return False
    if ur != vr and uc != vc:
        return bool(free[ur, vc] and free[vr, uc])
    return True


def pair_less(p, q):
    """a1 + b1 sqrt(2) < a2 + b2 sqrt(2) in integers (Python's are unbounded)"""
    da, db = p[0] - q[0], p[1] - q[1]
    if da <= 0 and db <= 0:
        return (da, db) != (0, 0)
    if da >= 0 and db >= 0:
        return False
    return da * da > 2 * db * db if da < 0 else da * da < 2 * db * db


class _Key:
    """a heap entry ordered by pair_less"""
    __slots__ = ("pair", "cell")

    def __init__(self, pair, cell):
        self.pair, self.cell = pair, cell

    def __lt__(self, other):
        return pair_less(self.pair, other.pair)


def travel_ref(free, sources):
    """-> (straight, diagonal) int32 (H, W): the pair of the shortest legal walk from any source, (0, 0) on a source,
    UNREACHED where no walk ends"""
    free = np.asarray(free) != 0
    sources = np.asarray(sources) != 0
    H, W = free.shape
    A = np.full((H, W), UNREACHED, dtype=np.int32)
    B = np.full((H, W), UNREACHED, dtype=np.int32)
    done = np.zeros((H, W), dtype=bool)
    heap = []
    for r, c in np.argwhere(sources):
        A[r, c] = B[r, c] = 0
        heap.append(_Key((0, 0), (int(r), int(c))))
    heapq.heapify(heap)
    while heap:
        k = heapq.heappop(heap)
        r, c = k.cell
        if done[r, c]:
            continue
        done[r, c] = True
        for dr, dc in NEIGHBOURS:
            v = (r + dr, c + dc)
            if not legal_step(free, sources, (r, c), v) or done[v]:
                continue
            cand = (k.pair[0] + (dr == 0 or dc == 0), k.pair[1] + (dr != 0 and dc != 0))
            if A[v] < 0 or pair_less(cand, (int(A[v]), int(B[v]))):
                A[v], B[v] = cand
                heapq.heappush(heap, _Key(cand, v))
    return A, B


def distance_ref(A, B):
    """float64(a) + float64(b) * sqrt(2), inf where unreached"""
    d = A.astype(np.float64) + B.astype(np.float64) * np.sqrt(2.0)
    d[A < 0] = np.inf
    return d


def decay_ref(A, B, decay_rate, cell_size=1.0, normalize=False):
    """t = 1 - (d / cell_size) * decay_rate, negative and unreached cells 0; normalize: (t - t.min()) / (t.max() - t.min())"""
    reached = A >= 0
    d = np.where(reached, A.astype(np.float64) + B.astype(np.float64) * np.sqrt(2.0), 0.0)
    t = 1.0 - (d / np.float64(cell_size)) * np.float64(decay_rate)
    t[t < 0] = 0.0
    t[~reached] = 0.0
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (t - t.min()) / (t.max() - t.min())
    return t


def check_walk(free, sources, A, B, walk):
    """a descend() walk: starts with the cell's pair, every step (taken backwards) is legal, the step counts add up, and it ends on
    a source"""
    free = np.asarray(free) != 0
    sources = np.asarray(sources) != 0
    straight = diagonal = 0
    for v, u in zip(walk[:-1], walk[1:]):
        assert legal_step(free, sources, u, v), (u, v)
        if u[0] != v[0] and u[1] != v[1]:
            diagonal += 1
        else:
            straight += 1
    assert (straight, diagonal) == (int(A[walk[0]]), int(B[walk[0]])), (straight, diagonal, walk[0])
    assert sources[walk[-1]], walk[-1]


def serpentine(H, W):
    """free map of width-1 corridors: every other row free, joined alternately at the right and the left end"""
    free = np.zeros((H, W), dtype=np.uint8)
    free[0::2] = 1
    for k, r in enumerate(range(1, H, 2)):
        free[r, W - 1 if k % 2 == 0 else 0] = 1
    return free


def spiral(n):
    """an n x n free map of concentric width-1 rings at offsets 0, 2, 4, ..., each cut below its top-left corner and joined to the
    next one there: one corridor that winds inwards"""
    free = np.zeros((n, n), dtype=np.uint8)
    for k in range(0, (n + 1) // 2, 2):
        lo, hi = k, n - 1 - k
        free[lo, lo:hi + 1] = free[hi, lo:hi + 1] = 1
        free[lo:hi + 1, lo] = free[lo:hi + 1, hi] = 1
        if hi - lo >= 4:
            free[lo + 1, lo] = 0                           # the cut
            free[lo + 2, lo + 1] = 1                       # the way into the next ring
    return free
