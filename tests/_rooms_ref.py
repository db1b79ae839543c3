"""The reference of label growth and of the room segmentation, written from the definitions alone: a lexicographic
heap Dijkstra ordered by (pair_less, then label) on the legal-step rule of _travel_ref, the tight-predecessor fixed point it must
equal, SciPy's distance_transform_edt and label for the seeds, and plain Python loops for the room and door tables."""
import heapq

import numpy as np
from scipy import ndimage

from _travel_ref import NEIGHBOURS, UNREACHED, legal_step, pair_less


class _Key:
    """a heap entry ordered by pair_less, then by label"""
    __slots__ = ("pair", "label", "cell")

    def __init__(self, pair, label, cell):
        self.pair, self.label, self.cell = pair, label, cell

    def __lt__(self, other):
        if self.pair != other.pair:
            return pair_less(self.pair, other.pair)
        return self.label < other.label


def grow_ref(free, seeds):
    """-> (owner int32, A, B): the heap Dijkstra on (pair, label).  A cell is settled when it is popped first; among the entries
    of its final pair the smallest label is popped first, because every tight predecessor has a strictly shorter pair and was
    settled -- with its own smallest label -- before."""
    free = np.asarray(free) != 0
    seeds = np.asarray(seeds).astype(np.int64)
    sources = seeds > 0
    H, W = free.shape
    A = np.full((H, W), UNREACHED, dtype=np.int32)
    B = np.full((H, W), UNREACHED, dtype=np.int32)
    owner = np.zeros((H, W), dtype=np.int32)
    done = np.zeros((H, W), dtype=bool)
    heap = [_Key((0, 0), int(seeds[r, c]), (int(r), int(c))) for r, c in np.argwhere(sources)]
    heapq.heapify(heap)
    while heap:
        k = heapq.heappop(heap)
        r, c = k.cell
        if done[r, c]:
            continue
        done[r, c] = True
        A[r, c], B[r, c] = k.pair
        owner[r, c] = k.label
        for dr, dc in NEIGHBOURS:
            v = (r + dr, c + dc)
            if not legal_step(free, sources, (r, c), v) or done[v]:
                continue
            cand = (k.pair[0] + (dr == 0 or dc == 0), k.pair[1] + (dr != 0 and dc != 0))
            heapq.heappush(heap, _Key(cand, k.label, v))
    return owner, A, B


def tight_fixed_point(free, seeds, A, B):
    """owner[c] = min(owner[u]) over the tight predecessors u, iterated from the seeds until nothing changes (rule 3)"""
    free = np.asarray(free) != 0
    seeds = np.asarray(seeds).astype(np.int64)
    sources = seeds > 0
    H, W = free.shape
    NONE = np.iinfo(np.int64).max
    owner = np.where(sources, seeds, NONE)
    changed = True
    while changed:
        changed = False
        for r in range(H):
            for c in range(W):
                if sources[r, c] or A[r, c] < 0:
                    continue
                best = owner[r, c]
                for dr, dc in NEIGHBOURS:
                    u = (r + dr, c + dc)                     # the step u -> (r, c) is the reverse of direction (dr, dc)
                    if not legal_step(free, sources, u, (r, c)) or A[u] < 0:
                        continue
                    diag = dr != 0 and dc != 0
                    if A[u] + (not diag) != A[r, c] or B[u] + diag != B[r, c]:
                        continue
                    best = min(best, owner[u])
                if best != owner[r, c]:
                    owner[r, c] = best
                    changed = True
    owner[owner == NONE] = 0
    return owner.astype(np.int32)


def seeds_ref(free, radius, min_seed_cells):
    """-> (seeds int32, K, E): the islands of E > radius with SciPy's numbering, the small ones dropped, the rest renumbered"""
    free = np.asarray(free) != 0
    E = ndimage.distance_transform_edt(free)
    lab, n = ndimage.label(E > np.float64(radius), structure=np.ones((3, 3)))
    seeds = np.zeros(free.shape, dtype=np.int32)
    k = 0
    for old in range(1, n + 1):
        cells = lab == old
        if int(cells.sum()) >= min_seed_cells:
            k += 1
            seeds[cells] = k
    return seeds, k, E


def room_table_ref(labels, seeds, E, K):
    table = np.zeros((K, 10), dtype=np.int64)
    H, W = labels.shape
    for k in range(1, K + 1):
        cells = [(r, c) for r in range(H) for c in range(W) if labels[r, c] == k]
        rows, cols = [r for r, _ in cells], [c for _, c in cells]
        best = None
        for r, c in cells:                                   # raster order: the first of the largest E
            if best is None or E[r, c] > E[best]:
                best = (r, c)
        table[k - 1] = [len(cells), min(rows), max(rows), min(cols), max(cols), sum(rows), sum(cols),
                        sum(1 for r, c in cells if seeds[r, c] == k), best[0], best[1]]
    return table


def door_table_ref(labels, E):
    H, W = labels.shape
    pairs = {}
    for r in range(H):
        for c in range(W):
            for vr, vc in ((r, c + 1), (r + 1, c)):
                if vr >= H or vc >= W:
                    continue
                lu, lv = int(labels[r, c]), int(labels[vr, vc])
                if lu == 0 or lv == 0 or lu == lv:
                    continue
                pairs.setdefault((min(lu, lv), max(lu, lv)), []).append(((r, c), (vr, vc)))
    table = np.zeros((len(pairs), 10), dtype=np.int64)
    for d, (i, j) in enumerate(sorted(pairs)):
        cells = sorted({cell for contact in pairs[(i, j)] for cell in contact})          # raster order
        best = None
        for cell in cells:
            if best is None or E[cell] > E[best]:
                best = cell
        rows, cols = [r for r, _ in cells], [c for _, c in cells]
        table[d] = [i, j, len(pairs[(i, j)]), min(rows), max(rows), min(cols), max(cols), best[0], best[1], 0]
    return table


def rooms_ref(free, radius, min_seed_cells):
    """-> dict(n, labels, rooms, doors, seeds, clearance)"""
    free = np.asarray(free) != 0
    seeds, K, E = seeds_ref(free, radius, min_seed_cells)
    labels = grow_ref(free, seeds)[0] if K else np.zeros(free.shape, dtype=np.int32)
    return dict(n=K, labels=labels, rooms=room_table_ref(labels, seeds, E, K), doors=door_table_ref(labels, E), seeds=seeds, clearance=E)


def three_rooms():
    """the 70 x 100 map of three rooms: 2-cell outer walls, inner walls at columns 33-34 and 66-67 with doors at rows 30-33 and
    40-43, and a 4 x 6 block of furniture in the middle room"""
    free = np.ones((70, 100), dtype=np.uint8)
    free[:2] = free[-2:] = 0
    free[:, :2] = free[:, -2:] = 0
    free[:, 33:35] = 0
    free[:, 66:68] = 0
    free[30:34, 33:35] = 1
    free[40:44, 66:68] = 1
    free[12:16, 45:51] = 0
    return free


def route_ref(n, doors, a, b):
    """the fewest-doors room sequence from a to b by BFS over the door table, neighbours in ascending id; None when not connected"""
    nb = {k: set() for k in range(1, n + 1)}
    for i, j in np.asarray(doors)[:, :2].tolist():
        nb[i].add(j)
        nb[j].add(i)
    prev, queue = {a: None}, [a]
    while queue:
        k = queue.pop(0)
        if k == b:
            out = []
            while k is not None:
                out.append(k)
                k = prev[k]
            return out[::-1]
        for m in sorted(nb[k]):
            if m not in prev:
                prev[m] = k
                queue.append(m)
    return None

