"""Goal tours on the set-to-set matrix of batched travel fields (Map.plan_tour): the exact order of a handful of
goals by Held-Karp on integer pairs, and the legs driven along the fields.  Host code: the matrix comes from ops.travel_arrivals."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

TOUR_MAX_GOALS = 10      # Held-Karp keeps n * 2^n states: 10 240 at the limit


def pair_less(p, q) -> bool:
    """a1 + b1 sqrt(2) < a2 + b2 sqrt(2) in Python integers: the kernel's travel_less on sums of pairs, without a float"""
    da, db = p[0] - q[0], p[1] - q[1]
    if da <= 0 and db <= 0:
        return (da, db) != (0, 0)
    if da >= 0 and db >= 0:
        return False
    return da * da > 2 * db * db if da < 0 else da * da < 2 * db * db


def held_karp(a, b, closed: bool = False):
    """The best order of the goals 1 .. n of the (n + 1, n + 1) integer matrices a, b (TravelArrivals.a / .b over [start] + goals;
    row and column 0 are the start, -1 = no walk).  Goals with a[0, g] < 0 are left out.  Among the orders of the others that use
    no missing leg, the one whose legs' pairs sum to the smallest a + b sqrt(2) -- sums and comparisons in Python ints
    (pair_less) -- and among equal sums the lexicographically smallest order; closed adds the leg back to the start.
    -> (order, (A, B), skipped): goal indices 1 .. n.  ([], (0, 0), skipped) when no goal is left; ValueError when the goals that
    are left admit no order (a leg between two of them is missing), and above TOUR_MAX_GOALS goals."""
    a, b = np.asarray(a), np.asarray(b)
    n = len(a) - 1
    if a.shape != (n + 1, n + 1) or b.shape != a.shape or n < 0:
        raise ValueError(f"held_karp: square matrices of one size, got {a.shape} and {b.shape}")
    if n > TOUR_MAX_GOALS:
        raise ValueError(f"a tour has at most {TOUR_MAX_GOALS} goals, got {n}")
    goals = [g for g in range(1, n + 1) if a[0, g] >= 0]
    skipped = [g for g in range(1, n + 1) if a[0, g] < 0]
    m = len(goals)
    if m == 0:
        return [], (0, 0), skipped

    def leg(u, v):
        return None if a[u, v] < 0 else (int(a[u, v]), int(b[u, v]))

    def better(x, y):                                    # (pair, order) x before y
        return y is None or pair_less(x[0], y[0]) or (x[0] == y[0] and x[1] < y[1])
    best = {}
    for i, g in enumerate(goals):
        best[(1 << i, i)] = (leg(0, g), (g,))
    for mask in range(1, 1 << m):
        for last in range(m):
            cur = best.get((mask, last))
            if cur is None:
                continue
            for nxt in range(m):
                if mask >> nxt & 1:
                    continue
                step = leg(goals[last], goals[nxt])
                if step is None:
                    continue
                cand = ((cur[0][0] + step[0], cur[0][1] + step[1]), cur[1] + (goals[nxt],))
                key = (mask | 1 << nxt, nxt)
                if better(cand, best.get(key)):
                    best[key] = cand
    final = None
    for last in range(m):
        cur = best.get(((1 << m) - 1, last))
        if cur is None:
            continue
        if closed:
            back = leg(goals[last], 0)
            if back is None:
                continue
            cur = ((cur[0][0] + back[0], cur[0][1] + back[1]), cur[1])
        if better(cur, final):
            final = cur
    if final is None:
        raise ValueError("plan_tour: the goals that can be reached from the start cannot all be reached from one another")
    return list(final[1]), final[0], skipped


class Tour:
    """Map.plan_tour's answer.  order: the goals' indices (into the `goals` argument) in visiting order; skipped: the goals no walk
    from the start reaches.  matrix_pair = (A, B) and matrix_length = A + B sqrt(2): the sum of the set-to-set distances along the
    order (and back to the start when closed), for which the order is optimal.  legs: one walk per leg, full-map (row, col) cells
    from where the last leg ended to the goal; driven_pairs: each leg's own (straight, diagonal) step counts, driven_length their
    total in cells."""

    def __init__(self, order, skipped, matrix_pair, legs, driven_pairs, closed):
        self.order, self.skipped, self.closed = list(order), list(skipped), bool(closed)
        self.matrix_pair = (int(matrix_pair[0]), int(matrix_pair[1]))
        self.matrix_length = self.matrix_pair[0] + self.matrix_pair[1] * float(np.sqrt(2.0))
        self.legs: List[List[Tuple[int, int]]] = legs
        self.driven_pairs: List[Tuple[int, int]] = driven_pairs
        self.driven_length = sum(p[0] for p in driven_pairs) + sum(p[1] for p in driven_pairs) * float(np.sqrt(2.0))


def step_counts(walk) -> Tuple[int, int]:
    """(straight, diagonal) steps of a walk of 8-neighbour cells"""
    diag = sum(1 for u, v in zip(walk[:-1], walk[1:]) if u[0] != v[0] and u[1] != v[1])
    return len(walk) - 1 - diag, diag


def drive_leg(field, free, cell, neighbours):
    """The walk from `cell` to the sources of `field` (an ops.TravelField): field.descend(cell), trimmed to its last free cell (a
    goal's cells may be obstacles -- the robot stops in front of the sofa).  A cell the field does not reach -- the start on an
    obstacle cell -- first steps to the neighbour the arrival rule names: the smallest pair + step over the reached neighbours, a
    diagonal step only past two free cells, the first in `neighbours` order among ties.  ValueError when nothing is reached."""
    a, b = field.planes()
    H, W = field.shape
    r, c = int(cell[0]), int(cell[1])
    head = []
    if a[r, c] < 0:
        best = None
        for dr, dc in neighbours:
            ur, uc = r + dr, c + dc
            if not (0 <= ur < H and 0 <= uc < W) or a[ur, uc] < 0:
                continue
            diag = dr != 0 and dc != 0
            if diag and not (free[ur, c] and free[r, uc]):
                continue
            cand = (int(a[ur, uc]) + (not diag), int(b[ur, uc]) + diag)
            if best is None or pair_less(cand, best[0]):
                best = (cand, (ur, uc))
        if best is None:
            raise ValueError(f"plan_tour: no walk from cell {(r, c)} to the goal")
        head, (r, c) = [(r, c)], best[1]
    walk = head + field.descend((r, c))
    while len(walk) > 1 and not free[walk[-1]]:
        walk.pop()
    return walk
