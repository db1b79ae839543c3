"""Scalar restatements of the three definitions of the map fusion (include/avlmaps_hip.h section 31), written from the definitions in
plain Python and elementwise NumPy float64 (never `@`: no BLAS, no fused multiply-add) and sharing no code with the package."""
import math

import numpy as np


def _centre(k, cs):
    return (k + (0.5 if k > 0 else -0.5 if k < 0 else 0.0)) * cs


def ref_move_cells(cells, gs, cs, vh, transform=None, shift=(0, 0, 0)):
    """(moved (n, 3) int32, inside (n,) uint8): Python floats are float64 and every operation below rounds once"""
    cells = np.asarray(cells).reshape(-1, 3)
    out = np.full((len(cells), 3), -1, np.int32)
    inside = np.zeros(len(cells), np.uint8)
    T = None if transform is None else [[float(v) for v in row] for row in np.asarray(transform, np.float64)]
    cs = float(cs)
    for i, (r, c, h) in enumerate(cells.tolist()):
        if T is not None:
            x, y, z = _centre(gs // 2 - r, cs), _centre(gs // 2 - c, cs), (h + 0.5) * cs
            moved = [((T[k][0] * x + T[k][1] * y) + T[k][2] * z) + T[k][3] for k in range(3)]
            q = [m / cs for m in moved]
            if not all(math.isfinite(v) and abs(v) < 2.0 ** 31 for v in q):
                continue
            r, c, h = int(gs / 2 - int(q[0])), int(gs / 2 - int(q[1])), int(q[2])
        r, c, h = r + int(shift[0]), c + int(shift[1]), h + int(shift[2])
        if 0 <= r < gs and 0 <= c < gs and 0 <= h < vh:
            out[i] = (r, c, h)
            inside[i] = 1
    return out, inside


def _weight_ok(w):
    w = float(w)
    return math.isfinite(w) and w > 0.0


def ref_fuse_plan(cells_a, w_a, cells_b, w_b, gs, vh, inside_b=None, use_a=None, use_b=None):
    """dict of n_out, a_row, b_start, b_rows, out_of_a, out_of_b, counts (6,), error (bit 0: a selected A row outside the grid, bit
    1: two selected A rows in one cell)"""
    cells_a, cells_b = np.asarray(cells_a).reshape(-1, 3).tolist(), np.asarray(cells_b).reshape(-1, 3).tolist()
    n_a, n_b = len(cells_a), len(cells_b)

    def within(cell):
        return 0 <= cell[0] < gs and 0 <= cell[1] < gs and 0 <= cell[2] < vh

    error = 0
    voxel_of_cell, members_b, a_row = {}, [], []
    out_of_a, out_of_b = [-1] * n_a, [-1] * n_b
    for i, cell in enumerate(cells_a):
        if (use_a is None or use_a[i]) and _weight_ok(w_a[i]):
            if not within(cell):
                error |= 1
                continue
            if tuple(cell) in voxel_of_cell:
                error |= 2
            out_of_a[i] = len(a_row)
            voxel_of_cell[tuple(cell)] = len(a_row)         # of two rows in a cell the later one owns it
            a_row.append(i)
            members_b.append([])
    n_sel_a = len(a_row)
    counts = [n_a - n_sel_a, 0, 0, 0, 0, 0]
    for j, cell in enumerate(cells_b):
        if not ((use_b is None or use_b[j]) and _weight_ok(w_b[j])):
            counts[1] += 1
        elif not ((inside_b is None or inside_b[j]) and within(cell)):
            counts[2] += 1
        else:
            v = voxel_of_cell.get(tuple(cell))
            if v is None:                                   # ascending j: a new cell is numbered at its smallest row
                v = voxel_of_cell[tuple(cell)] = len(a_row)
                a_row.append(-1)
                members_b.append([])
                counts[4] += 1
            elif v < n_sel_a:
                counts[3] += 1
            else:
                counts[5] += 1
            out_of_b[j] = v
            members_b[v].append(j)
    b_start = np.zeros(len(a_row) + 1, np.int32)
    b_start[1:] = np.cumsum([len(m) for m in members_b])
    b_rows = np.array([j for m in members_b for j in m], np.int32)
    return dict(n_out=len(a_row), a_row=np.array(a_row, np.int32), b_start=b_start, b_rows=b_rows, out_of_a=np.array(out_of_a, np.int32),
                out_of_b=np.array(out_of_b, np.int32), counts=np.array(counts, np.int32), error=error)


def ref_fuse_rows(plan, cells_a, feat_a, w_a, rgb_a, cells_b, feat_b, w_b, rgb_b, gs, vh, gain_a=1.0, gain_b=1.0):
    """(grid_pos, grid_feat, weight, grid_rgb, occupied_ids) of a ref_fuse_plan dict; cells_b are the MOVED cells.  Member order: the
    A row, then the B rows ascending; the first product starts the sum, every later one is added to it."""
    feat_a, feat_b = np.asarray(feat_a, np.float32), np.asarray(feat_b, np.float32)
    D = feat_a.shape[1] if feat_a.ndim == 2 and feat_a.shape[0] else feat_b.shape[1]
    n = plan["n_out"]
    pos, feat = np.full((n, 3), -1, np.int32), np.zeros((n, D), np.float32)
    weight, rgb = np.zeros(n, np.float32), np.zeros((n, 3), np.uint8)
    occ = np.full((gs, gs, vh), -1, np.int32)
    for v in range(n):
        members = []
        a = int(plan["a_row"][v])
        if a >= 0:
            members.append((np.float64(w_a[a]) * np.float64(gain_a), feat_a[a], rgb_a[a], cells_a[a]))
        for j in plan["b_rows"][plan["b_start"][v]:plan["b_start"][v + 1]]:
            members.append((np.float64(w_b[j]) * np.float64(gain_b), feat_b[j], rgb_b[j], cells_b[j]))
        W, acc, col = None, None, None
        for w, f, c, _ in members:
            p, pc = w * f.astype(np.float64), w * np.asarray(c).astype(np.float64)
            W, acc, col = (w, p, pc) if W is None else (W + w, acc + p, col + pc)
        feat[v] = (acc / W).astype(np.float32)
        weight[v] = np.float32(W)
        rgb[v] = np.trunc(col / W).astype(np.uint8)
        pos[v] = members[0][3]
        occ[tuple(pos[v])] = v
    return pos, feat, weight, rgb, occ
