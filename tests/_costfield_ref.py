"""The reference of the cost-weighted travel field and of the layered costmap, written from the definition alone:
a heap Dijkstra on integer pairs (A, B) = (summed price of the straight steps, summed price of the diagonal steps) ordered exactly
by _travel_ref.pair_less in Python integers, _travel_ref.legal_step with "passable" in place of "free", the price of a step being
that of the cell it enters; the NumPy restatement of avl_costmap2d; and the check of a descend() walk under prices."""
import heapq

import numpy as np

from _travel_ref import NEIGHBOURS, UNREACHED, _Key, legal_step, pair_less


def passable_ref(free, cost):
    """free and not lethal: price 0 on a free cell makes it impassable"""
    return (np.asarray(free) != 0) & (np.asarray(cost) != 0)


def cost_ref(free, cost, sources):
    """-> (A, B) int32 (H, W): the pair of the cheapest legal walk from any source, (0, 0) on a source, UNREACHED where no walk ends"""
    ok = passable_ref(free, cost)
    price = np.asarray(cost).astype(np.int64)
    sources = np.asarray(sources) != 0
    H, W = ok.shape
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
            if not legal_step(ok, sources, (r, c), v) or done[v]:
                continue
            p = int(price[v])
            cand = (k.pair[0] + p, k.pair[1]) if dr == 0 or dc == 0 else (k.pair[0], k.pair[1] + p)
            if A[v] < 0 or pair_less(cand, (int(A[v]), int(B[v]))):
                A[v], B[v] = cand
                heapq.heappush(heap, _Key(cand, v))
    return A, B


def price_ref(A, B):
    """float64(A) + float64(B) * sqrt(2), inf where unreached"""
    d = A.astype(np.float64) + B.astype(np.float64) * np.sqrt(2.0)
    d[A < 0] = np.inf
    return d


def costmap_ref(free, layers):
    """avl_costmap2d in NumPy.  layers: [(distance plane (H, W) float64, table uint8), ...].  0 where not free or where any layer's
    entry is 255; else min(254, 1 + the sum of table[min(rint(d * d), len(table) - 1)] over the layers)"""
    free = np.asarray(free) != 0
    total = np.ones(free.shape, dtype=np.int64)
    lethal = np.zeros(free.shape, dtype=bool)
    for plane, table in layers:
        d = np.asarray(plane, dtype=np.float64)
        table = np.asarray(table, dtype=np.uint8)
        d2 = np.minimum(np.rint(d * d).astype(np.int64), len(table) - 1)
        t = table[d2].astype(np.int64)
        lethal |= t == 255
        total += t
    out = np.minimum(total, 254)
    out[lethal | ~free] = 0
    return out.astype(np.uint8)


def check_walk(free, cost, sources, A, B, walk):
    """a descend() walk: every step (taken backwards, from the source to the cell) is legal on the passable map, the prices of the
    cells entered add up to the start's pair, straight and diagonal apart, and the walk ends on a source"""
    ok = passable_ref(free, cost)
    sources = np.asarray(sources) != 0
    straight = diagonal = 0
    for v, u in zip(walk[:-1], walk[1:]):
        assert legal_step(ok, sources, u, v), (u, v)
        if u[0] != v[0] and u[1] != v[1]:
            diagonal += int(cost[v])
        else:
            straight += int(cost[v])
    assert (straight, diagonal) == (int(A[walk[0]]), int(B[walk[0]])), (straight, diagonal, walk[0])
    assert sources[walk[-1]], walk[-1]
