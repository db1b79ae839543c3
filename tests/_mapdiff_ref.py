"""Scalar and NumPy restatements of the three definitions of the map comparison (include/avlmaps_hip.h section 30), written from the
definitions and sharing no code with the package."""
import numpy as np


def ref_match_cells(pos_b, cells_a, gs, vh, radius, shift=(0, 0, 0)):
    """(match, d2): a dict from cell to its largest row, and a triple loop over offsets ordered by (d2, linear cell)"""
    owner = {}
    for row, (r, c, h) in enumerate(np.asarray(pos_b).reshape(-1, 3).tolist()):
        if 0 <= r < gs and 0 <= c < gs and 0 <= h < vh:
            owner[(r, c, h)] = row                      # ascending rows: the largest stays
    cells_a = np.asarray(cells_a).reshape(-1, 3)
    match = np.full(len(cells_a), -1, np.int32)
    d2 = np.full(len(cells_a), -1, np.int32)
    for i, (r, c, h) in enumerate(cells_a.tolist()):
        r, c, h = r + int(shift[0]), c + int(shift[1]), h + int(shift[2])
        if not (0 <= r < gs and 0 <= c < gs and 0 <= h < vh):
            continue
        best = None
        for dr in range(-radius, radius + 1):
            for dc in range(-radius, radius + 1):
                for dh in range(-radius, radius + 1):
                    cell = (r + dr, c + dc, h + dh)
                    if cell in owner:                   # a cell outside the grid is never in the dict
                        key = (dr * dr + dc * dc + dh * dh, (cell[0] * gs + cell[1]) * vh + cell[2])
                        if best is None or key < best[0]:
                            best = (key, owner[cell])
        if best is not None:
            match[i], d2[i] = best[1], best[0][0]
    return match, d2


def _butterfly(v):
    """the xor butterfly of 64 float64 lane values: six rounds of pairwise additions, v = v + partner"""
    v = np.asarray(v, np.float64).copy()
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ off]
    assert np.all(v.view(np.int64) == v.view(np.int64)[0]) or np.isnan(v).any()
    return v[0]


def _lane_sums(x, y):
    """x, y (D,) float32 -> the float64 sum of x * y in the pinned order: rows zero-padded to a multiple of 256, lane l owns the
    elements d with (d // 4) % 64 == l and adds their exact float64 products in ascending d from +0.0, then the butterfly"""
    D = len(x)
    P = -(-D // 256) * 256
    px, py = np.zeros(P, np.float64), np.zeros(P, np.float64)
    px[:D], py[:D] = x, y
    prod = (px * py).reshape(P // 256, 64, 4)           # [chunk, lane, j]: d = 256 chunk + 4 lane + j; a float32 product is exact
    acc = np.zeros(64, np.float64)
    for chunk in range(P // 256):
        for j in range(4):
            acc = acc + prod[chunk, :, j]
    return _butterfly(acc)


def ref_row_dots(feat_a, feat_b, match):
    feat_a, feat_b = np.asarray(feat_a, np.float32), np.asarray(feat_b, np.float32)
    out = np.zeros((len(match), 3), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for i, m in enumerate(np.asarray(match).tolist()):
            if m >= 0:
                a, b = feat_a[i], feat_b[m]
                out[i] = (_lane_sums(a, b), _lane_sums(a, a), _lane_sums(b, b))
    return out


def ref_status(match, sums, threshold, through=None, min_rays=3):
    """(status uint8, counts int32[4]); t2 = threshold * threshold in float64, the products grouped as ab * ab >= t2 * (aa * bb)"""
    match, sums = np.asarray(match), np.asarray(sums, np.float64).reshape(-1, 3)
    ab, aa, bb = sums[:, 0], sums[:, 1], sums[:, 2]
    t2 = np.float64(threshold) * np.float64(threshold)
    with np.errstate(over="ignore", invalid="ignore"):
        same = (aa > 0) & (bb > 0) & (ab > 0) & (ab * ab >= t2 * (aa * bb))
    status = np.where(same, 0, 1).astype(np.uint8)
    status[match < 0] = 2
    if through is not None:
        status[(match < 0) & (np.asarray(through).astype(np.int64) < int(min_rays))] = 3
    return status, np.bincount(status, minlength=4).astype(np.int32)


def ref_map_diff(pos_a, feat_a, pos_b, feat_b, gs, vh, radius, threshold, shift=(0, 0, 0), through_a=None, through_b=None, min_rays=3):
    """both directions: [(match, d2, sums, status, counts)] for A against B and for B against A under the negated shift"""
    out = []
    neg = tuple(-int(s) for s in shift)
    for pa, fa, pb, fb, sh, th in ((pos_a, feat_a, pos_b, feat_b, shift, through_a), (pos_b, feat_b, pos_a, feat_a, neg, through_b)):
        match, d2 = ref_match_cells(pb, pa, gs, vh, radius, sh)
        sums = ref_row_dots(fa, fb, match)
        status, counts = ref_status(match, sums, threshold, th, min_rays)
        out.append((match, d2, sums, status, counts))
    return out
