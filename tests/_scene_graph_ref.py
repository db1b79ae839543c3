"""The brute-force restatement of avl_object_relations (include/avlmaps_hip.h (24)) in NumPy: a dense owner array
padded by R, one vectorised step per offset, a dict of pairs.  Shared by the scene-graph tests; nothing here is fast or clever."""
import numpy as np


def owner_array(pos, gs, vh, R):
    """(gs + 2R, gs + 2R, vh + 2R) int64: the largest row of every cell of the grid, -1 where there is none; the padding stays -1"""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    inside = np.all((pos >= 0) & (pos < np.array([gs, gs, vh])), axis=1)
    owner = np.full((gs + 2 * R, gs + 2 * R, vh + 2 * R), -1, np.int64)
    rows = np.flatnonzero(inside)
    q = pos[rows] + R
    np.maximum.at(owner, (q[:, 0], q[:, 1], q[:, 2]), rows)
    return owner, inside


def reference_relations(pos, labels, n, R, gs, vh):
    """-> (table (P, 8) int64 sorted by (lo, hi), P)"""
    pos, labels = np.asarray(pos, np.int64).reshape(-1, 3), np.asarray(labels, np.int64).reshape(-1)
    owner, inside = owner_array(pos, gs, vh, R)
    scan = np.flatnonzero(inside & (labels >= 1) & (labels <= n))            # ascending rows
    a_all = labels[scan]
    pairs = {}                                                               # (lo, hi) -> [d2, i, code, j, lo_on_hi, hi_on_lo, contacts]
    side = 2 * R + 1
    for dr in range(-R, R + 1):
        for dc in range(-R, R + 1):
            for dh in range(-R, R + 1):
                d2 = dr * dr + dc * dc + dh * dh
                if d2 > R * R or len(scan) == 0:
                    continue
                code = ((dr + R) * side + (dc + R)) * side + (dh + R)
                q = pos[scan] + R + np.array([dr, dc, dh])
                j_all = owner[q[:, 0], q[:, 1], q[:, 2]]                     # the padding answers for every cell outside the grid
                b_all = np.where(j_all >= 0, labels[np.maximum(j_all, 0)], 0)
                ok = (j_all >= 0) & (b_all >= 1) & (b_all <= n) & (b_all != a_all)
                if not ok.any():
                    continue
                i, j, a, b = scan[ok], j_all[ok], a_all[ok], b_all[ok]
                lo, hi = np.minimum(a, b), np.maximum(a, b)
                key = lo * (n + 1) + hi
                uniq, first, counts = np.unique(key, return_index=True, return_counts=True)     # first: the smallest scanning row of a key
                for k, f, cnt in zip(uniq.tolist(), first.tolist(), counts.tolist()):
                    rec = pairs.setdefault((k // (n + 1), k % (n + 1)), [1 << 60, -1, -1, -1, 0, 0, 0])
                    cand = (d2, int(i[f]), code)
                    if cand < tuple(rec[:3]):
                        rec[:4] = [d2, int(i[f]), code, int(j[f])]
                    if 1 <= d2 <= 3:
                        rec[6] += cnt
                if (dr, dc, dh) == (0, 0, -1):
                    for k, scanner_is_lo in zip(key.tolist(), (a < b).tolist()):
                        pairs[(k // (n + 1), k % (n + 1))][4 if scanner_is_lo else 5] += 1
    table = np.zeros((len(pairs), 8), np.int64)
    for t, (lo, hi) in enumerate(sorted(pairs)):
        d2, i, _, j, lo_on_hi, hi_on_lo, contacts = pairs[(lo, hi)]
        table[t] = [lo, hi, d2, i, j, lo_on_hi, hi_on_lo, contacts]
    return table, len(pairs)


def offset_code(dr, dc, dh, R):
    return ((dr + R) * (2 * R + 1) + (dc + R)) * (2 * R + 1) + (dh + R)
