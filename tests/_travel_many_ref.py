"""The reference of the batched travel fields, written from the definition alone: a loop of _travel_ref.travel_ref
per set, the arrival rule as plain loops, the sound sum as NumPy float64 / float32 step by step, and a brute force over
permutations for tours."""
import itertools

import numpy as np

from _travel_ref import NEIGHBOURS, UNREACHED, pair_less, travel_ref


def csr(sets):
    """[[(r, c), ...], ...] -> (offsets int64 (K + 1,), cells int32 (L, 2))"""
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    cells = np.array([c for s in sets for c in s], dtype=np.int32).reshape(-1, 2)
    return offsets, cells


def set_mask(shape, cells):
    m = np.zeros(shape, np.uint8)
    for r, c in cells:
        m[r, c] = 1
    return m


def fields_ref(free, sets):
    """-> (A, B) int32 (K, H, W): travel_ref once per set"""
    planes = [travel_ref(free, set_mask(np.asarray(free).shape, s)) for s in sets]
    return np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])


def arrive_cell_ref(free, A, B, t):
    """-> ((a, b), direction) of one field's arrival at cell t, or (None, -1): (0, 0) with direction -1 on a source; else the exact
    minimum over the neighbours u = t + NEIGHBOURS[d] of pair(u) + step(u -> t), over reached u and, on a diagonal step, with both
    cells that share an edge with u and t free; the first direction among ties; t itself need not be free"""
    H, W = A.shape
    r, c = t
    if A[r, c] == 0 and B[r, c] == 0:
        return (0, 0), -1
    best, best_d = None, -1
    for d, (dr, dc) in enumerate(NEIGHBOURS):
        ur, uc = r + dr, c + dc
        if not (0 <= ur < H and 0 <= uc < W) or A[ur, uc] < 0:
            continue
        diag = dr != 0 and dc != 0
        if diag and not (free[ur, c] and free[r, uc]):
            continue
        cand = (int(A[ur, uc]) + (not diag), int(B[ur, uc]) + diag)
        if best is None or pair_less(cand, best):
            best, best_d = cand, d
    return best, best_d


def arrivals_ref(free, A, B, sets):
    """-> a, b, cell, from_ int32 (K, M): per field and target set the minimum over the set's cells in CSR order (the first cell
    among ties; cell is the index into the concatenated cells), -1 in all four where nothing arrives"""
    free = np.asarray(free) != 0
    K, M = len(A), len(sets)
    out = [np.full((K, M), -1, np.int32) for _ in range(4)]
    for k in range(K):
        at = 0
        for j, s in enumerate(sets):
            best = None
            for i, t in enumerate(s):
                pair, d = arrive_cell_ref(free, A[k], B[k], t)
                if pair is not None and (best is None or pair_less(pair, best[0])):
                    best = (pair, at + i, d)
            at += len(s)
            if best is not None:
                out[0][k, j], out[1][k, j], out[2][k, j], out[3][k, j] = best[0][0], best[0][1], best[1], best[2]
    return out


def sound_ref(A, B, peaks, decay):
    """float32 (H, W): for the segments in order, t = p - (p * d) * decay in float64 with d = float64(a) + float64(b) * sqrt(2),
    clipped at 0 and 0 where unreached; acc = float32(float64(acc) + t)"""
    acc = np.zeros(A.shape[1:], np.float32)
    for s, p in enumerate(np.asarray(peaks, np.float32)):
        pd = np.float64(p)
        reached = A[s] >= 0
        d = np.where(reached, A[s].astype(np.float64) + B[s].astype(np.float64) * np.float64(1.4142135623730951), 0.0)
        t = pd - (pd * d) * np.float64(decay)
        t[t < 0] = 0.0
        t[~reached] = 0.0
        acc = (acc.astype(np.float64) + t).astype(np.float32)
    return acc


def tour_ref(a, b, closed=False):
    """Brute force over the permutations of the goals 1 .. n of the (n + 1, n + 1) integer matrices a, b (row / column 0 = the
    start): goals with a[0, g] < 0 are skipped; among the orders of the others the smallest sum of pairs (pair_less on Python
    ints), ties to the lexicographically smallest order; an order that uses an unreachable leg is out.  -> (order, (A, B), skipped);
    order [] with (0, 0) when nothing is left"""
    n = len(a) - 1
    goals = [g for g in range(1, n + 1) if a[0, g] >= 0]
    skipped = [g for g in range(1, n + 1) if a[0, g] < 0]
    best = None
    for perm in itertools.permutations(goals):
        legs = list(zip((0,) + perm, perm + ((0,) if closed else ())))
        if any(a[u, v] < 0 for u, v in legs):
            continue
        tot = (sum(int(a[u, v]) for u, v in legs), sum(int(b[u, v]) for u, v in legs))
        if best is None or pair_less(tot, best[1]):
            best = (list(perm), tot)
    if best is None:
        return [], (0, 0), skipped
    return best[0], best[1], skipped


__all__ = ["UNREACHED", "arrivals_ref", "arrive_cell_ref", "csr", "fields_ref", "set_mask", "sound_ref", "tour_ref"]
