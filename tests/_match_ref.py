"""Restatement of the correlative pose search (csrc/avl_match.hip) for the tests: a point and its cells as scalar
Python in the order the source writes them down, the scores by slicing a dense bool volume, the winner by a plain lexicographic
sort.

A point comes from the oracle's pinned depth2pc_pixels and transform_points, its cell from the pinned base_pos2grid_id_3d
(oracle/avl_oracle.py), as tests/_gtmap_ref.py builds the vote's; the rotation between them is Python float arithmetic, which is
IEEE float64 and never fused.  The scene helpers of _ray_ref.py are re-exported here."""
import numpy as np

from oracle import avl_oracle as O

from _ray_ref import calib, camera  # noqa: F401  (the scene helpers, re-exported)


def lattice(H, W, stride):
    return [(v, u) for v in range(stride // 2, H, stride) for u in range(stride // 2, W, stride)]


def frame_points(depth_f32, Kinv, T, cs, stride, min_depth, max_depth, h_lo, h_hi):
    """steps 1 - 2: the (x, y, h) of the lattice pixels of one frame that are hit points, finite and inside the height band"""
    H, W = depth_f32.shape
    lat = lattice(H, W, stride)
    if not lat:
        return []
    pcs, masks = O.depth2pc_pixels(depth_f32, Kinv, [v * W + u for v, u in lat], min_depth, max_depth)
    gpts = O.transform_points(T, pcs)
    out = []
    for ok, g in zip(masks, gpts):
        if not ok or not np.all(np.isfinite(g)):
            continue
        h = O.base_pos2grid_id_3d(1, cs, 0.0, 0.0, g[2])[2]
        if h_lo <= h <= h_hi:
            out.append((float(g[0]), float(g[1]), int(h)))
    return out


def rotate(x, y, c, s, px, py):
    """step 3, in the source's order; the zero angle is the point itself"""
    if c == 1.0 and s == 0.0:
        return x, y
    dx, dy = x - px, y - py
    return px + (c * dx - s * dy), py + (s * dx + c * dy)


def cells_of(points, c, s, px, py, gs, cs, R):
    """steps 3 - 4: (n, 3) int64 cells (row, col, h) of the points under one angle, NOT clipped to the grid; a point that no shift
    of [-R, R] can bring in is left out"""
    out = []
    for x, y, h in points:
        qx, qy = rotate(x, y, float(c), float(s), float(px), float(py))
        row, col, _ = O.base_pos2grid_id_3d(gs, cs, qx, qy, 0.0)
        if -R <= row <= gs - 1 + R and -R <= col <= gs - 1 + R:
            out.append((int(row), int(col), h))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def volumes(depth, calib_mat, transforms, cs, vh, stride=4, min_depth=0.1, max_depth=6.0, h_band=(2, None), joint=False, pivot=None):
    """-> [(points, (px, py))] per volume: every frame on its own with its origin as the pivot, or all frames in one"""
    depth = np.asarray(depth, dtype=np.float32)
    depth = depth[None] if depth.ndim == 2 else depth
    Kinv = np.linalg.inv(np.asarray(calib_mat, dtype=np.float64).reshape(3, 3))
    Ts = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4)
    h_lo = 0 if h_band[0] is None else int(h_band[0])
    h_hi = vh - 1 if h_band[1] is None else int(h_band[1])
    per_frame = [frame_points(depth[f], Kinv, Ts[f], cs, stride, min_depth, max_depth, h_lo, h_hi) for f in range(depth.shape[0])]
    if joint:
        if pivot is None:
            pivot = (Ts[0, 0, 3], Ts[0, 1, 3]) if len(Ts) else (0.0, 0.0)
        return [([p for pts in per_frame for p in pts], (float(pivot[0]), float(pivot[1])))]
    return [(pts, (float(Ts[f, 0, 3]), float(Ts[f, 1, 3]))) for f, pts in enumerate(per_frame)]


def dense(grid_pos, gs, vh):
    """the occupancy of a voxel list as a (gs, gs, vh) bool volume; rows outside the grid are left out"""
    occ = np.zeros((gs, gs, vh), bool)
    g = np.asarray(grid_pos, dtype=np.int64).reshape(-1, 3)
    ok = (g[:, 0] >= 0) & (g[:, 0] < gs) & (g[:, 1] >= 0) & (g[:, 1] < gs) & (g[:, 2] >= 0) & (g[:, 2] < vh)
    occ[g[ok, 0], g[ok, 1], g[ok, 2]] = True
    return occ


def score_cells(occ, cells, R):
    """step 5: (S, S) uint32.  The volume is padded by 2R cells of nothing on every side of rows and cols; the window of a point
    at (row, col, h) is the S x S slice of layer h that starts at padded (row + R, col + R): its entry (di + R, dj + R) is the
    cell (row + di, col + dj).  One slice per point, summed: a point counts once per point."""
    S = 2 * R + 1
    if len(cells) == 0:
        return np.zeros((S, S), np.uint32)
    padded = np.pad(occ, ((2 * R, 2 * R), (2 * R, 2 * R), (0, 0)))
    windows = np.lib.stride_tricks.sliding_window_view(padded, (S, S), axis=(0, 1))          # (gs + 2R, gs + 2R, vh, S, S)
    total = np.zeros((S, S), np.uint64)
    step = max(1, (1 << 24) // (S * S))
    for lo in range(0, len(cells), step):
        c = cells[lo:lo + step]
        total += windows[c[:, 0] + R, c[:, 1] + R, c[:, 2]].sum(axis=0, dtype=np.uint64)
    return total.astype(np.uint32)


def winner(scores, k0):
    """step 6 for one volume's (K, S, S) scores: (k, di, dj, score), the first of a lexicographic sort"""
    K, S, _ = scores.shape
    R = (S - 1) // 2
    k, a, b = (x.reshape(-1) for x in np.meshgrid(np.arange(K), np.arange(S), np.arange(S), indexing="ij"))
    di, dj = a - R, b - R
    sc = scores.reshape(-1).astype(np.int64)
    order = np.lexsort((dj, di, k, np.abs(k - k0), di * di + dj * dj, -sc))                   # (the last key sorts first)
    i = order[0]
    return int(k[i]), int(di[i]), int(dj[i]), int(sc[i])


def match_ref(grid_pos, gs, vh, depth, calib_mat, transforms, cs, angles, radius, stride=4, min_depth=0.1, max_depth=6.0, h_band=(2, None),
              joint=False, pivot=None, k0=None):
    """ops.match_frames restated -> (scores (V, K, S, S) uint32, best (V, 4) int32, valid (V,) uint32)"""
    angles = np.asarray(angles, dtype=np.float64).reshape(-1, 2)
    if k0 is None:
        k0 = int(np.flatnonzero((angles[:, 0] == 1.0) & (angles[:, 1] == 0.0))[0])
    occ = dense(grid_pos, gs, vh)
    vols = volumes(depth, calib_mat, transforms, cs, vh, stride, min_depth, max_depth, h_band, joint, pivot)
    S = 2 * radius + 1
    scores = np.zeros((len(vols), len(angles), S, S), np.uint32)
    best = np.zeros((len(vols), 4), np.int32)
    valid = np.zeros((len(vols),), np.uint32)
    for v, (points, (px, py)) in enumerate(vols):
        valid[v] = len(points)
        for k, (c, s) in enumerate(angles):
            scores[v, k] = score_cells(occ, cells_of(points, c, s, px, py, gs, cs, radius), radius)
        best[v] = winner(scores[v], k0)
    return scores, best, valid


def correction_ref(k, di, dj, cs, angles, pivot):
    """the 4 x 4 correction of a winner, built entry by entry: a rotation by angle k about the pivot, then -di, -dj cells"""
    c, s = np.asarray(angles, dtype=np.float64).reshape(-1, 2)[k]
    px, py = pivot
    C = np.eye(4)
    C[0, :2], C[1, :2] = (c, -s), (s, c)
    C[0, 3] = px - (c * px - s * py) - di * cs
    C[1, 3] = py - (s * px + c * py) - dj * cs
    return C


# ------------------------------------------------------------------ the scenes of the tests
H, W, GS, CS = 24, 32, 64, 0.05
K = calib(32.0, 16.0, 12.0)                # 24 x 32 frames: +-0.5 per metre of depth sideways, +-0.375 up and down
DEPTHS = dict(min_depth=0.125, max_depth=6.0)       # (both exact in float32: a pixel AT a limit is dropped)


def room_depth(T, box, posts=(), H=H, W=W, Kmat=K):
    """(H, W) float32 depth of a camera at T inside the room box = (x0, x1, y0, y1): per pixel the z of the nearest wall along the
    pixel's ray, walls being the four vertical planes of the box and the square posts (cx, cy, half side)"""
    Kinv = np.linalg.inv(Kmat)
    depth = np.zeros((H, W), np.float32)
    o = T[:3, 3]
    for v in range(H):
        for u in range(W):
            d = T[:3, :3] @ (Kinv @ np.array([u + 0.5, v + 0.5, 1.0]))         # the ray of depth 1
            best = np.inf
            rects = [(box, False)] + [((cx - hw, cx + hw, cy - hw, cy + hw), True) for cx, cy, hw in posts]
            for (x0, x1, y0, y1), solid in rects:
                for axis, planes, lo, hi in ((0, (x0, x1), y0, y1), (1, (y0, y1), x0, x1)):
                    for w in planes:
                        if d[axis] == 0.0:
                            continue
                        t = (w - o[axis]) / d[axis]
                        other = o[1 - axis] + t * d[1 - axis]
                        if t > 1e-9 and lo - 1e-9 <= other <= hi + 1e-9 and t < best:
                            best = t
            depth[v, u] = best if np.isfinite(best) else 0.0
    return depth


def scene(F, seed=0):
    """(depth (F, H, W) float32, transforms (F, 4, 4)): cameras 0.4 m up inside an L-shaped corner of walls, near the grid's middle
    and near its borders (so that shifted and rotated cells leave and enter the grid), looking in all directions; frame 0 carries
    the depths that drop a pixel and the two range limits themselves"""
    rng = np.random.default_rng(seed)
    box = (-1.45, 1.75, -1.1, 1.52)
    poses = [((0.1, -0.2, 0.4), 30.0), ((1.0, 1.2, 0.4), 20.0), ((-1.2, -0.9, 0.4), 200.0), ((0.9, -0.8, 0.4), 300.0),
             ((-1.1, 1.3, 0.4), 120.0), ((0.3, 0.4, 0.4), 75.0), ((-0.4, 0.1, 0.4), 250.0)]
    Ts = np.stack([camera(poses[f % len(poses)][0], yaw=poses[f % len(poses)][1] + 3.0 * (f // len(poses))) for f in range(F)])
    depth = np.stack([room_depth(Ts[f], box, posts=((0.7, 0.1, 0.1),)) for f in range(F)])
    depth += rng.uniform(-0.02, 0.02, depth.shape).astype(np.float32)
    depth[0, 0, :8] = [0.0, np.nan, np.inf, 6.0, 7.5, 0.125, 0.05, -1.0]
    return depth.astype(np.float32), Ts


def voxels(vh, fill=0.35, seed=1):
    """(N, 3) int32 cells of a random map with some rows outside the grid and a cell that two rows share"""
    rng = np.random.default_rng(seed)
    pos = np.argwhere(rng.random((GS, GS, vh)) < fill).astype(np.int32)
    pos = pos[rng.permutation(len(pos))]
    extra = np.array([[-1, 3, 1], [GS, 3, 1], [3, -1, 1], [3, GS, 0], [5, 5, vh], [5, 5, -1], pos[0], pos[0]], np.int32)
    return np.ascontiguousarray(np.concatenate([pos, extra]))


PLANT_BOX = (-1.2, 1.3, -1.1, 1.25)        # a room whose walls stay inside the grid under every planted shift


def planted(angles, k_star, di_star, dj_star, vh, radius, origin=(0.1, -0.2, 0.4), yaw=30.0, stride=1, h_band=(2, None)):
    """(depth (1, H, W), T (1, 4, 4), pos (N, 3) int32): a frame of the asymmetric room seen from `origin`, and a map made of the
    restatement's own cells of that frame under angle k_star, moved by (di_star, dj_star) cells -- so that the frame under its
    prior T scores every valid point at (k_star, di_star, dj_star)"""
    T = camera(origin, yaw=yaw)[None]
    depth = room_depth(T[0], PLANT_BOX, posts=((0.7, 0.1, 0.1),))[None]
    (points, (px, py)), = volumes(depth, K, T, CS, vh, stride, h_band=h_band, **DEPTHS)
    cells = cells_of(points, *np.asarray(angles)[k_star], px, py, GS, CS, radius)
    assert len(cells) == len(points)
    pos = np.unique(cells + (di_star, dj_star, 0), axis=0).astype(np.int32)
    return depth, T, pos


def recording(sc, cfg, n_frames, angles, plant, vh, used, radius=3):
    """Write a recording of n_frames frames of the asymmetric room under `sc` (poses.txt, depth/*.npy: the dataset's layout) ->
    (depth, Ts, pos, n_points, (min_depth, max_depth)): its frames, its camera -> map transforms as the builder derives them, and
    the voxels of a map in which the recording is off by plant = (k, di, dj): the restatement's cells of the frames `used`, as one
    joint volume about the first frame's origin, under angle k, moved by (di, dj)"""
    from scipy.spatial.transform import Rotation
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.map.vlmap_builder import VLMapBuilder
    (sc / "depth").mkdir(parents=True)
    vm = VLMap(cfg)
    vecs = np.array([[0.1 * i, 0.0, 0.05 * i, *Rotation.from_euler("y", 25.0 + 10.0 * i, degrees=True).as_quat()] for i in range(n_frames)])
    np.savetxt(sc / "poses.txt", vecs)
    builder = VLMapBuilder(sc, cfg, sc / "poses.txt", [], [], vm.base2cam_tf, vm.base_transform)
    Ts = np.stack(builder.frame_transforms(vecs))
    depth = np.stack([room_depth(T, PLANT_BOX, posts=((0.7, 0.1, 0.1),)) for T in Ts])
    for i, d in enumerate(depth):
        np.save(sc / "depth" / f"{i:06d}.npy", d)
    mn, mx = float(builder.min_depth), float(builder.max_depth)
    pivot = (Ts[0, 0, 3], Ts[0, 1, 3])
    (points, _), = volumes(depth[used], K, Ts[used], CS, vh, 1, mn, mx, (2, None), joint=True, pivot=pivot)
    cells = cells_of(points, *np.asarray(angles)[plant[0]], *pivot, GS, CS, radius) + (plant[1], plant[2], 0)
    pos = np.unique(cells, axis=0).astype(np.int32)
    assert len(cells) == len(points) > 300 and pos[:, :2].min() >= 0 and pos[:, :2].max() < GS
    return depth, Ts, pos, len(points), (mn, mx)


def recording_config(camera_height=0.4):
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": GS, "map_config.cell_size": CS,
                                  "map_config.cam_calib_mat": [float(x) for x in K.reshape(-1)],
                                  "map_config.pose_info.camera_height": camera_height}).map_config
