"""The reference of the 2-D viewshed, written from the definition alone in scalar Python: the walk, the octant
rule, gain and seen per eye, the candidate table of Map.get_exploration_views and the greedy tour of Map.plan_exploration on host
arrays.  Nothing here looks at the kernel; the travel distances come from tests/_travel_ref.py."""
import math

import numpy as np

import _travel_ref as T


def walk(e, t):
    """the cells k = 0 .. n of the sight line from e to t, both (row, col)"""
    (r, c), (tr, tc) = (int(e[0]), int(e[1])), (int(t[0]), int(t[1]))
    dr, dc = abs(tr - r), abs(tc - c)
    sr, sc = (1 if tr > r else -1), (1 if tc > c else -1)
    n = max(dr, dc)
    er, ec = 2 * dr - n, 2 * dc - n
    cells = [(r, c)]
    for _ in range(n):
        if er > 0:
            r += sr
            er -= 2 * n
        er += 2 * dr
        if ec > 0:
            c += sc
            ec -= 2 * n
        ec += 2 * dc
        cells.append((r, c))
    return cells


def octant(dr, dc):
    """the sector of a nonzero offset"""
    dr, dc = int(dr), int(dc)
    assert (dr, dc) != (0, 0)
    k = 0
    while not (dc > 0 and dr >= 0):
        dr, dc = -dc, dr
        k += 2
    return k + (0 if dr < dc else 1)


def classes(free, explored, opaque_unknown=False):
    """(blocking, unknown) as lists of lists of bools"""
    free, explored = np.asarray(free) != 0, np.asarray(explored) != 0
    unknown = free & ~explored
    blocking = ~free | (unknown if opaque_unknown else False)
    return blocking.tolist(), unknown.tolist()


def visible_from(blocking, H, W, eye, radius):
    """the visible targets of one eye as a list of (row, col), None for an eye outside the image"""
    er, ec = int(eye[0]), int(eye[1])
    if not (0 <= er < H and 0 <= ec < W):
        return None
    out = []
    R2 = radius * radius
    for tr in range(max(er - radius, 0), min(er + radius, H - 1) + 1):
        for tc in range(max(ec - radius, 0), min(ec + radius, W - 1) + 1):
            dr, dc = tr - er, tc - ec
            if (dr, dc) == (0, 0) or dr * dr + dc * dc > R2:
                continue
            # the walk, with an exit at the first blocker among the cells 1 <= k < n
            ar, ac = abs(dr), abs(dc)
            n = max(ar, ac)
            sr, sc = (1 if dr > 0 else -1), (1 if dc > 0 else -1)
            e_r, e_c, r, c = 2 * ar - n, 2 * ac - n, er, ec
            free_line = True
            for _ in range(1, n):
                if e_r > 0:
                    r += sr
                    e_r -= 2 * n
                e_r += 2 * ar
                if e_c > 0:
                    c += sc
                    e_c -= 2 * n
                e_c += 2 * ac
                if blocking[r][c]:
                    free_line = False
                    break
            if free_line:
                out.append((tr, tc))
    return out


def _visible(cache, blocking, H, W, eye, radius):
    """visible_from, looked up in `cache` (a dict that belongs to one free map, explored map and opaque_unknown) when one is given"""
    if cache is None:
        return visible_from(blocking, H, W, eye, radius)
    key = (int(eye[0]), int(eye[1]), radius)
    if key not in cache:
        cache[key] = visible_from(blocking, H, W, eye, radius)
    return cache[key]


def gain_ref(free, explored, eyes, radius, opaque_unknown=False, cache=None):
    """(E, 8) int32"""
    H, W = np.asarray(free).shape
    blocking, unknown = classes(free, explored, opaque_unknown)
    eyes = np.asarray(eyes).reshape(-1, 2)
    gain = np.zeros((len(eyes), 8), np.int32)
    for i, eye in enumerate(eyes):
        vis = _visible(cache, blocking, H, W, eye, int(radius))
        if vis is None:
            gain[i] = -1
            continue
        for tr, tc in vis:
            if unknown[tr][tc]:
                gain[i, octant(tr - int(eye[0]), tc - int(eye[1]))] += 1
    return gain


def seen_ref(free, explored, eyes, radius, opaque_unknown=False, out=None, cache=None):
    """(H, W) uint8, OR-ed into a copy of `out` when that is given"""
    H, W = np.asarray(free).shape
    blocking, _ = classes(free, explored, opaque_unknown)
    seen = np.zeros((H, W), np.uint8) if out is None else np.array(out, dtype=np.uint8)
    for eye in np.asarray(eyes).reshape(-1, 2):
        vis = _visible(cache, blocking, H, W, eye, int(radius))
        if vis is None:
            continue
        seen[int(eye[0]), int(eye[1])] = 1
        for tr, tc in vis:
            seen[tr, tc] = 1
    return seen


def best_heading_ref(row, fov_octants=2):
    """(start, sum) of the cyclic run of fov_octants sectors with the largest sum, the first among equals"""
    best = (0, -1)
    for s in range(8):
        total = sum(int(row[(s + j) % 8]) for j in range(fov_octants))
        if total > best[1]:
            best = (s, total)
    return best


def frontier_centres_ref(free, explored, min_cells=5):
    """the centres of Map.get_frontiers in crop coordinates, as a set: explored free cells with an unknown 4-neighbour, grouped
    into 8-connected islands of at least min_cells cells; an island's centre is its own cell nearest to its centroid, the first in
    raster order among equals"""
    from scipy import ndimage
    free, explored = np.asarray(free) != 0, np.asarray(explored) != 0
    unknown = np.pad(free & ~explored, 1)
    near = unknown[:-2, 1:-1] | unknown[2:, 1:-1] | unknown[1:-1, :-2] | unknown[1:-1, 2:]
    labels, n = ndimage.label(free & explored & near, structure=np.ones((3, 3), int))
    centres = set()
    for k in range(1, n + 1):
        cells = np.argwhere(labels == k)
        if len(cells) >= min_cells:
            d2 = np.sum((cells - cells.mean(axis=0)) ** 2, axis=1)
            centres.add(tuple(int(v) for v in cells[int(np.argmin(d2))]))
    return centres


def views_ref(free, explored, pos, radius, stride=4, opaque_unknown=False, min_cells=5):
    """The candidate table over a crop, everything in crop coordinates: the known-free cells on the lattice of `stride` cells and
    the frontier centres, in raster order; with `pos` (a crop cell) only those a legal walk from pos over known-free cells reaches.
    -> dict(cells (n, 2), gain (n, 8), total (n,), heading (n,), distance (n, 2))"""
    free, explored = np.asarray(free) != 0, np.asarray(explored) != 0
    H, W = free.shape
    known = free & explored
    cand = np.zeros((H, W), bool)
    cand[::stride, ::stride] = known[::stride, ::stride]
    for r, c in frontier_centres_ref(free, explored, min_cells):
        cand[r, c] = True
    A = B = np.full((H, W), -1, np.int32)
    if pos is not None:
        src = np.zeros((H, W), bool)
        src[int(pos[0]), int(pos[1])] = True
        A, B = T.travel_ref(known, src)
        cand &= A >= 0
    cells = np.argwhere(cand)
    gain = gain_ref(free, explored, cells, radius, opaque_unknown)
    heading = np.array([best_heading_ref(g)[0] for g in gain], np.int64).reshape(-1)
    return dict(cells=cells, gain=gain, total=gain.astype(np.int64).sum(axis=1), heading=heading,
                distance=np.stack([A[cells[:, 0], cells[:, 1]], B[cells[:, 0], cells[:, 1]]], axis=1).reshape(-1, 2))


def select_ref(total, min_fraction=0.5):
    total = [int(t) for t in total]
    if not total or max(total) == 0:
        return []
    need = max(1, math.ceil(float(min_fraction) * max(total)))
    return [i for i, t in enumerate(total) if t >= need]


def next_view_ref(views, min_fraction=0.5):
    """the row of the selected candidate with the shortest travel distance, the first in raster order among equals; None when no
    candidate gains anything"""
    best = None
    for i in select_ref(views["total"], min_fraction):
        pair = (int(views["distance"][i, 0]), int(views["distance"][i, 1]))
        if best is None or T.pair_less(pair, best[1]):
            best = (i, pair)
    return None if best is None else best[0]


def tour_ref(free, explored, pos, radius, k, stride=4, opaque_unknown=False, min_fraction=0.5):
    """the greedy tour in crop coordinates -> [(cell, heading, gain), ...] and the explored map after it"""
    explored = (np.asarray(explored) != 0).copy()
    tour = []
    for _ in range(k):
        views = views_ref(free, explored, pos, radius, stride, opaque_unknown)
        i = next_view_ref(views, min_fraction)
        if i is None:
            break
        cell = tuple(int(v) for v in views["cells"][i])
        tour.append((cell, int(views["heading"][i]), int(views["total"][i])))
        explored |= seen_ref(free, explored, [cell], radius, opaque_unknown) != 0
        pos = cell
    return tour, explored
