"""Scalar / NumPy restatement of the ground-truth label map (csrc/avl_gtmap.hip) for the tests: the vote pass, the majority labels,
the label-valued top-down pool, the confusion matrix and map_scores.

A vote's point comes from the oracle's pinned depth2pc_pixels, transform_points and base_pos2grid_id_3d (oracle/avl_oracle.py), as
tests/_explore_ref.py builds its rays; everything after the cell is integer bookkeeping in the order DESIGN.md 4.16 writes it down.
`stats`, when given, counts which cases the pixels of a call fell into, so that a test can assert that its scene really contains
the cases it claims to cover."""
import numpy as np

from oracle import avl_oracle as O

from _ray_ref import _bump, calib, camera  # noqa: F401  (the scene helpers, re-exported)

UNLABELLED = -1


def vote_ref(votes, depth, semantic, calib_mat, transforms, occupied, n_voxels, C, cs, stride=1, min_depth=0.1, max_depth=6.0, obj2cls=None,
             counts=None, stats=None):
    """-> (votes (n_voxels, C) uint32, counts (4,) uint64): new arrays, `votes` / `counts` (None = zero) with the frames folded in.
    counts = pixels dropped by depth or grid, by class, for want of a voxel, and votes cast.  An index entry >= n_voxels raises."""
    out = np.zeros((n_voxels, C), np.int64) if votes is None else np.array(votes, dtype=np.int64)
    cnt = [0, 0, 0, 0] if counts is None else [int(c) for c in counts]
    depth = np.asarray(depth, dtype=np.float32)
    depth = depth[None] if depth.ndim == 2 else depth
    semantic = np.asarray(semantic).reshape(depth.shape)
    Kinv = np.linalg.inv(np.asarray(calib_mat, dtype=np.float64).reshape(3, 3))
    Ts = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4)
    gs, _, vh = occupied.shape
    F, H, W = depth.shape
    lattice = [(v, u) for v in range(stride // 2, H, stride) for u in range(stride // 2, W, stride)]
    for f in range(F):
        frame_votes = {}
        if not lattice:
            break
        pcs, masks = O.depth2pc_pixels(depth[f], Kinv, [v * W + u for v, u in lattice], min_depth, max_depth)      # (1)
        gpts = O.transform_points(Ts[f], pcs)                                                         # (2) (used where the mask holds)
        for (v, u), pc, ok, g in zip(lattice, pcs, masks, gpts):
            z = depth[f, v, u]
            if not ok:
                cnt[0] += 1
                _bump(stats, "depth_nan" if np.isnan(z) else "depth_inf" if np.isinf(z) else "depth_zero" if z == 0 else
                      "depth_far" if pc[2] >= max_depth else "depth_near")
                continue
            row, col, h = O.base_pos2grid_id_3d(gs, cs, g[0], g[1], g[2])
            if not (0 <= row < gs and 0 <= col < gs and 0 <= h < vh):
                cnt[0] += 1
                for name, x, n in (("row", row, gs), ("col", col, gs), ("h", h, vh)):
                    if x < 0:
                        _bump(stats, name + "_low")
                    if x >= n:
                        _bump(stats, name + "_high")
                continue
            o = int(semantic[f, v, u])                                                                # (3)
            if obj2cls is not None:
                if o < 0 or o >= len(obj2cls):
                    cnt[1] += 1
                    _bump(stats, "obj_negative" if o < 0 else "obj_beyond")
                    continue
                c = int(obj2cls[o])
            else:
                c = o
            if c < 0 or c >= C:
                cnt[1] += 1
                _bump(stats, "cls_negative" if c < 0 else "cls_beyond")
                continue
            r = int(occupied[row, col, h])                                                            # (4)
            if r < 0:
                cnt[2] += 1
                _bump(stats, "no_voxel")
                continue
            if r >= n_voxels:
                raise IndexError(f"voxel id {r} >= {n_voxels}")
            out[r, c] += 1                                                                            # (5)
            cnt[3] += 1
            frame_votes[(r, c)] = frame_votes.get((r, c), 0) + 1
        if stats is not None and frame_votes:
            stats["max_votes_one_counter_one_frame"] = max(stats.get("max_votes_one_counter_one_frame", 0), max(frame_votes.values()))
    return (out % (1 << 32)).astype(np.uint32), np.array(cnt, dtype=np.uint64)


def labels_ref(votes):
    """-> (label (N,) int32: np.argmax of the row -- the lowest class at the maximum -- or UNLABELLED for an all-zero row;
    support (N,) uint32: the row sum, wrapping at 2^32)"""
    votes = np.asarray(votes, dtype=np.uint32)
    if votes.shape[0] == 0:
        return np.zeros((0,), np.int32), np.zeros((0,), np.uint32)
    label = np.argmax(votes, axis=1).astype(np.int32)
    label[~(votes != 0).any(axis=1)] = UNLABELLED
    support = (votes.astype(np.uint64).sum(axis=1) % (1 << 32)).astype(np.uint32)
    return label, support


def pool_ref(labels, occupied, window=None):
    """the label of the highest voxel of every column of the window (r0, r1, c0, c1, inclusive) that has one; UNLABELLED when none has"""
    gs, _, vh = occupied.shape
    r0, r1, c0, c1 = (0, gs - 1, 0, gs - 1) if window is None else window
    out = np.full((r1 - r0 + 1, c1 - c0 + 1), UNLABELLED, np.int32)
    for r in range(r0, r1 + 1):
        for c in range(c0, c1 + 1):
            for h in range(vh - 1, -1, -1):
                i = occupied[r, c, h]
                if i >= 0 and labels[i] >= 0:
                    out[r - r0, c - c0] = labels[i]
                    break
    return out


def confusion_ref(gt, pred, Cg, Cp, conf=None, skipped=None):
    """-> (conf (Cg, Cp) int64 by np.add.at, skipped (2,) int64: gt < 0; gt >= 0 and pred < 0)"""
    gt, pred = np.asarray(gt).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)
    conf = np.zeros((Cg, Cp), np.int64) if conf is None else np.array(conf, dtype=np.int64)
    skipped = np.zeros(2, np.int64) if skipped is None else np.array(skipped, dtype=np.int64)
    no_gt = gt < 0
    no_pred = ~no_gt & (pred < 0)
    keep = ~no_gt & ~no_pred
    if np.any(gt[keep] >= Cg) or np.any(pred[keep] >= Cp):
        raise IndexError("label out of range")
    np.add.at(conf, (gt[keep], pred[keep]), 1)
    skipped += (int(no_gt.sum()), int(no_pred.sum()))
    return conf, skipped


def scores_ref(conf):
    """map_scores term by term, in the formulas' order -> dict(pixel_acc, mean_acc, miou, fwiou, acc, iou)"""
    conf = np.asarray(conf).astype(np.int64)
    Cg, Cp = conf.shape
    total = int(conf.sum())
    acc, iou, classes = [np.nan] * Cg, [np.nan] * Cg, []
    trace = 0
    for k in range(Cg):
        row_sum = int(conf[k].sum())
        col_sum = int(conf[:, k].sum()) if k < Cp else 0
        hit = int(conf[k, k]) if k < Cp else 0
        trace += hit
        if row_sum > 0:
            classes.append(k)
            acc[k] = hit / row_sum
            iou[k] = hit / (row_sum + col_sum - hit)
    if total == 0:
        return dict(pixel_acc=np.nan, mean_acc=np.nan, miou=np.nan, fwiou=np.nan, acc=np.array(acc), iou=np.array(iou))
    weighted = 0.0
    for k in classes:
        weighted += float(int(conf[k].sum())) * iou[k]
    return dict(pixel_acc=trace / total, mean_acc=float(np.mean([acc[k] for k in classes])), miou=float(np.mean([iou[k] for k in classes])),
                fwiou=weighted / total, acc=np.array(acc), iou=np.array(iou))


# ------------------------------------------------------------------ the voting scene of the tests
H, W, GS, VH, CS = 24, 32, 64, 8, 0.05
K = calib(32.0, 16.0, 12.0)                # 24 x 32 frames: +-0.5 per metre of depth sideways, +-0.375 up and down
DEPTHS = dict(min_depth=0.1, max_depth=6.0)


def vote_scene(F, C, n_obj=12, seed=0, class_ids=False):
    """(depth (F, H, W) float32, semantic (F, H, W) int32, transforms (F, 4, 4), obj2cls (n_obj,) int32 | None).  Frame 0 looks at a
    flat wall 0.3 m ahead from the middle of the grid (nearly every pixel of it falls into a handful of voxels: the contended
    counter) and carries the depths that drop a pixel; the other frames stand near the four borders, level, pitched up and pitched
    down, with depths up to 2.5 m, so that points leave the grid on every side.  Object ids run from -1 to n_obj, table entries
    from -1 to C: one below and one above each range.  class_ids: no table, the frames hold class ids from -1 to C."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.15, 2.5, (F, H, W)).astype(np.float32)
    depth[0] = 0.3
    depth[0, 0, :6] = [0.0, np.nan, np.inf, 6.0, 7.5, 0.05]
    poses = [((0.0125, 0.0125, 0.2125), 0, 0.0), ((1.3, 0.2, 0.2), 0, 0.0), ((-1.3, -0.2, 0.2), 180, 0.0), ((0.2, 1.3, 0.2), 90, 0.0),
             ((-0.2, -1.3, 0.2), 270, 0.0), ((0.3, -0.4, 0.2), 45.0, 25.0), ((-0.5, 0.6, 0.2), 200.0, -25.0)]
    Ts = np.stack([camera(poses[f % len(poses)][0], yaw=poses[f % len(poses)][1], pitch=poses[f % len(poses)][2]) for f in range(F)])
    if class_ids:
        return depth, rng.integers(-1, C + 1, (F, H, W)).astype(np.int32), Ts, None
    semantic = rng.integers(-1, n_obj + 1, (F, H, W)).astype(np.int32)
    semantic[0, 12:, :] = 3                                      # half the wall is one object
    table = rng.integers(-1, C + 1, n_obj).astype(np.int32)
    table[3], table[0], table[1] = C - 1, -1, C                  # the wall's class; one entry below and one above the classes
    return depth, semantic, Ts, table


def voxel_index(fill=0.7, seed=1):
    """(occupied_ids (GS, GS, VH) int32, N): a voxel in `fill` of the cells, ids in a shuffled order, -1 elsewhere"""
    rng = np.random.default_rng(seed)
    has = rng.random((GS, GS, VH)) < fill
    has[26:38, 26:38, :] = True                                  # the wall's voxels exist ...
    has[30, 30, :] = False                                       # ... but for one column
    occupied = np.full((GS, GS, VH), -1, np.int32)
    N = int(has.sum())
    occupied[has] = rng.permutation(N).astype(np.int32)
    return occupied, N
