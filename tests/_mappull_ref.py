"""Scalar restatement of the backward resampling of a voxel map (include/avlmaps_hip.h section 32), written from the
definition in plain Python and elementwise NumPy float64 (never `@`: no BLAS, no fused multiply-add) and sharing no code with the
package.  Python floats are float64 and every operation below rounds once."""
import math

import numpy as np


def centre(k, cs):
    """the centre of the base-coordinate interval of the horizontal cell k = gs // 2 - index: the cell k = 0 is two cells wide"""
    return (k + (0.5 if k > 0 else -0.5 if k < 0 else 0.0)) * cs


def bracket(s):
    """(k0, t) of s = coordinate / cs on the lattice of centres 0, +-1.5, +-2.5, ..: the centre of k0 lies at or below s, the centre
    of k0 + 1 above it, t is the fraction of the way"""
    a = abs(s)
    if a < 1.5:
        j0, u = 0, a / 1.5
    else:
        b = a - 0.5
        j0 = math.floor(b)
        u = b - j0
    if s >= 0.0:
        return j0, u
    if u == 0.0:
        return -j0, 0.0
    return -(j0 + 1), 1.0 - u


def bracket_h(q):
    """(h0, t) of q = z / cs on the lattice of centres h + 0.5"""
    s = q - 0.5
    h0 = math.floor(s)
    return h0, s - h0


def corners(qx, qy, qz, gs):
    """the eight (cell, lambda) of the point (qx, qy, qz) = base coordinates / cs, corner j with dz = j & 1, dy = j >> 1 & 1, dx = j >> 2 & 1"""
    (kx, tx), (ky, ty), (h0, tz) = bracket(qx), bracket(qy), bracket_h(qz)
    out = []
    for j in range(8):
        dz, dy, dx = j & 1, j >> 1 & 1, j >> 2 & 1
        lx, ly, lz = (tx if dx else 1.0 - tx), (ty if dy else 1.0 - ty), (tz if dz else 1.0 - tz)
        out.append(((gs // 2 - (kx + dx), gs // 2 - (ky + dy), h0 + dz), (lx * ly) * lz))
    return out


def pulled_back(cell, gs, cs, P):
    """(qx, qy, qz): the centre of the cell through the inverse transform P (4 x 4 nested floats), divided by cs; None when a quotient
    is not finite or not below 2^31"""
    x, y, z = centre(gs // 2 - cell[0], cs), centre(gs // 2 - cell[1], cs), (cell[2] + 0.5) * cs
    q = [(((P[k][0] * x + P[k][1] * y) + P[k][2] * z) + P[k][3]) / cs for k in range(3)]
    return q if all(math.isfinite(v) and abs(v) < 2.0 ** 31 for v in q) else None


def selected_rows(cells_b, w_b, gs, vh, use_b=None):
    """({cell: row} of the selected rows, rows that use or weight unselects, further rows outside); ValueError for two in one cell"""
    owner, unselected, outside = {}, 0, 0
    for i, cell in enumerate(np.asarray(cells_b).reshape(-1, 3).tolist()):
        w = float(w_b[i])
        if not ((use_b is None or use_b[i]) and math.isfinite(w) and w > 0.0):
            unselected += 1
        elif not (0 <= cell[0] < gs and 0 <= cell[1] < gs and 0 <= cell[2] < vh):
            outside += 1
        elif tuple(cell) in owner:
            raise ValueError("two selected rows of map B share a cell")
        else:
            owner[tuple(cell)] = i
    return owner, unselected, outside


def ref_pull_plan(cells_b, w_b, gs, cs, vh, P=None, shift=(0, 0, 0), use_b=None, interp="linear", min_support=0.5):
    """dict of n_out, cells (n, 3) int32, members (n, 8) int32, lam (n, 8) float64, counts (4,) int32, occupied (gs, gs, vh) int32.
    P: the sixteen doubles of the INVERSE transform, or None"""
    owner, unselected, outside = selected_rows(cells_b, w_b, gs, vh, use_b)
    P = None if P is None else [[float(v) for v in row] for row in np.asarray(P, np.float64).reshape(4, 4)]
    cs, min_support = float(cs), float(min_support)
    cells, members, lam, below, used = [], [], [], 0, set()
    occupied = np.full((gs, gs, vh), -1, np.int32)
    for r in range(gs):
        for c in range(gs):
            for h in range(vh):
                moved = (r - int(shift[0]), c - int(shift[1]), h - int(shift[2]))
                if P is None:
                    cand = [(moved, 1.0)]
                else:
                    q = pulled_back(moved, gs, cs, P)
                    if q is None:
                        cand = []
                    elif interp == "nearest":
                        cand = [((int(gs / 2 - int(q[0])), int(gs / 2 - int(q[1])), int(q[2])), 1.0)]
                    else:
                        cand = corners(q[0], q[1], q[2], gs)
                m, l, support = [-1] * 8, [0.0] * 8, 0.0
                for j, (cell, weight) in enumerate(cand):
                    if weight > 0.0 and cell in owner:
                        m[j], l[j] = owner[cell], weight
                        support = support + weight
                if support > 0.0 and support >= min_support:
                    occupied[r, c, h] = len(cells)
                    cells.append((r, c, h))
                    members.append(m)
                    lam.append(l)
                    used.update(v for v in m if v >= 0)
                elif support > 0.0:
                    below += 1
    n = len(cells)
    return dict(n_out=n, cells=np.array(cells, np.int32).reshape(n, 3), members=np.array(members, np.int32).reshape(n, 8),
                lam=np.array(lam, np.float64).reshape(n, 8), counts=np.array([unselected, outside, below, len(owner) - len(used)], np.int32),
                occupied=occupied)


def ref_pull_rows(plan, feat_b, w_b, rgb_b):
    """(grid_feat, weight, grid_rgb) of a ref_pull_plan dict: the first product starts a sum, every later one is added to it"""
    feat_b = np.asarray(feat_b, np.float32)
    n, D = plan["n_out"], feat_b.shape[1]
    feat, weight, rgb = np.zeros((n, D), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.uint8)
    with np.errstate(all="ignore"):
        for v in range(n):
            W = S = acc = col = None
            for j in range(8):
                m = int(plan["members"][v, j])
                if m < 0:
                    continue
                l = np.float64(plan["lam"][v, j])
                om = l * np.float64(w_b[m])
                p, pc = om * feat_b[m].astype(np.float64), om * np.asarray(rgb_b[m]).astype(np.float64)
                W, S, acc, col = (om, l, p, pc) if W is None else (W + om, S + l, acc + p, col + pc)
            feat[v] = (acc / W).astype(np.float32)
            weight[v] = np.float32(W / S)
            rgb[v] = np.trunc(col / W).astype(np.uint8)
    return feat, weight, rgb


def pinholes(cells, gs, vh):
    """the number of empty cells between four filled in-plane neighbours (row +- 1 and col +- 1 at the same height)"""
    grid = np.zeros((gs + 2, gs + 2, vh), bool)
    cells = np.asarray(cells).reshape(-1, 3)
    grid[cells[:, 0] + 1, cells[:, 1] + 1, cells[:, 2]] = True
    mid = grid[1:-1, 1:-1]
    return int((~mid & grid[:-2, 1:-1] & grid[2:, 1:-1] & grid[1:-1, :-2] & grid[1:-1, 2:]).sum())
