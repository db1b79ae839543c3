"""GPU parity of the multi-floor (global) builder, vlmap_builder_multi_floor.py:60-199: pass 1 (ops.points_bbox -> bbox_kernel) and
pass 2 (VoxelAccumulator.integrate_frame_global -> K1 in global mode: np.round((p - pcd_min) / cs) on an (n0, n1, n2) grid, uint16
depth / depth_div, points outside the pass-1 box dropped) against the sequential oracle (C, float64, the reference's order) and the
reference's own run on a scene built for exact arithmetic (G10)."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import avl_oracle as O

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_api_gpu import check_multi_floor_builder  # noqa: E402
from test_builder_gpu import FEAT_RTOL, compare_maps, ops  # noqa: E402,F401  (ops: the module's GPU fixture)

H2C = O.HABITAT2CAM_ROT


def run_gpu_global(ops, grid_size, cs, pcd_min, calib, Ts, depths, rgbs, feats_chw, samples, depth_div=1000.0, capacity=None,
                   replay=False, deferred=False, calib_inv=None):
    """one integrate_frame_global call per frame on a (x, y, z) = (n0, n2, n1) grid -- what VLMapBuilderMultiFloor issues"""
    n0, n2, n1 = (int(v) for v in grid_size)
    D = feats_chw[0].shape[0]
    acc = ops.VoxelAccumulator(n1, cs, n2, D, capacity=capacity, n_rows=n0, deferred_fuse=deferred)
    if replay:
        acc.enable_replay_log(sum(len(s) for s in samples))
    for i in range(len(depths)):
        acc.integrate_frame_global(depths[i], calib, Ts[i], samples[i], np.ascontiguousarray(np.transpose(feats_chw[i], (1, 2, 0))),
                                   rgbs[i], frame_idx=i, pcd_min=pcd_min, depth_div=depth_div, calib_inv=calib_inv)
    return acc


def run_oracle_global(pcd_min, pcd_max, cs, calib, Ts, depths_m, rgbs, feats_chw, samples, calib_inv=None):
    m = O.OracleGlobalMap(pcd_min, pcd_max, cs, feats_chw[0].shape[0])
    pts = sum(m.integrate(depths_m[i], calib, Ts[i], samples[i], feats_chw[i], rgbs[i], calib_inv=calib_inv) for i in range(len(depths_m)))
    return m, m.export(), pts


def same_bounds(a, b):
    return bool(np.all(a == b))          # (== : -0.0 and +0.0 are the same bound)


def grid_of(minmax, cs):
    return np.ceil((minmax[3:] - minmax[:3]) / cs + 1).astype(int)        # vlmap_builder_multi_floor.py:222


# ---------------------------------------------------------------------------------------------------------------- pass 1
def test_points_bbox_matches_the_oracle_at_the_edges(ops):
    """pass 1 folded over 21 frames: uint16 raw values 0, 1, 32767, 32768, 65535 (a sign-extended or float-converted uint16 moves
    the box), depth_div 1000 and 5000, float32 metres with NaN, +-inf and values on both strict bounds, and frames without a
    single valid sample (the box must not move).  Six bounds and the grid size equal after every frame."""
    rng = np.random.default_rng(2024)
    H, W, cs = 24, 32, 0.25
    calib = np.array([20.0, 0, 15.5, 0, 20.0, 11.5, 0, 0, 1])
    from scipy.spatial.transform import Rotation as R
    gpu = np.array([np.inf] * 3 + [-np.inf] * 3)
    ref = gpu.copy()
    f32_lo = float(np.float32(0.1))          # 0.1 itself is no float32: this is the value a float32 depth can sit exactly on
    for i in range(21):
        T = np.eye(4)
        T[:3, :3] = R.from_euler("yxz", rng.uniform(-np.pi, np.pi, 3)).as_matrix()
        T[:3, 3] = rng.uniform(-3, 3, 3)
        T = T @ H2C
        samples = rng.permutation(H * W)[: H * W // (1 + i % 3)].astype(np.int32)
        min_depth, max_depth = 0.1, 100.0
        if i < 10:                           # uint16 millimetres / fifths of a millimetre
            div = 1000.0 if i % 2 == 0 else 5000.0
            d = rng.integers(500, 6000, (H, W)).astype(np.uint16)
            special = np.array([0, 1, 32767, 32768, 65535, 65535, 32768, 100, 99], dtype=np.uint16)
            d.reshape(-1)[rng.choice(H * W, 60, replace=False)] = np.resize(special, 60)
            if i == 7:
                d[:] = 0                     # no valid sample: minmax unchanged
            depth, depth_m = d, d / div
        else:
            div = 1000.0
            d = rng.uniform(0.2, 8.0, (H, W)).astype(np.float32)
            special = np.array([np.nan, np.inf, -np.inf, 0.1, 100.0, np.nextafter(np.float32(0.1), np.float32(1)),
                                np.nextafter(np.float32(100), np.float32(0)), -1.0, 0.0, 99.5], dtype=np.float32)
            d.reshape(-1)[rng.choice(H * W, 80, replace=False)] = np.resize(special, 80)
            if i == 12:
                min_depth = f32_lo           # the lower bound exactly on float32(0.1): those samples are dropped (strict)
            if i == 15:
                d[:] = np.float32(np.nan)
            if i == 18:
                d[:] = np.float32(100.0)     # all on the strict upper bound
            depth, depth_m = d, d.astype(np.float64)
        before = gpu.copy()
        ops.points_bbox(gpu, depth, calib, T, samples, depth_div=div, min_depth=min_depth, max_depth=max_depth)
        O.points_bbox(ref, depth_m, calib, T, samples, min_depth=min_depth, max_depth=max_depth)
        assert same_bounds(gpu, ref), (i, gpu, ref)
        if i in (7, 15, 18):
            assert same_bounds(gpu, before), i
        if np.isfinite(gpu).all():
            assert np.array_equal(grid_of(gpu, cs), grid_of(ref, cs))
    assert np.isfinite(gpu).all() and (gpu[3:] - gpu[:3]).min() > 10      # 65.535 m and 32.768 m points are in the box


def test_depth_must_be_uint16_or_float32(ops):
    """a float64 depth in metres (what the reference's PNG / 1000.0 is) used to be rounded to float32 on the way in -- a different
    box and different voxel ids at cell edges; both passes now refuse every dtype but the two the kernels read"""
    H, W = 4, 6
    calib = np.array([2.0, 0, 3, 0, 2.0, 2, 0, 0, 1])
    mm = np.array([np.inf] * 3 + [-np.inf] * 3)
    idx = np.arange(H * W, dtype=np.int32)
    acc = ops.VoxelAccumulator(8, 0.25, 8, 4, n_rows=8)
    feat, rgb = np.zeros((2, 2, 4), np.float32), np.zeros((H, W, 3), np.uint8)
    for bad in (np.full((H, W), 1.1), np.full((H, W), 1100, np.int32), np.full((H, W), 1100, np.int16)):
        with pytest.raises(TypeError, match="uint16 .* or float32"):
            ops.points_bbox(mm, bad, calib, np.eye(4), idx)
        with pytest.raises(TypeError, match="uint16 .* or float32"):
            acc.integrate_frame_global(bad, calib, np.eye(4), idx, feat, rgb, frame_idx=0, pcd_min=np.zeros(3))
    assert np.isinf(mm).all() and acc.num_voxels() == 0
    import torch
    t64 = torch.full((H, W), 1.1, dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError, match="uint16 .* or float32"):
        ops.points_bbox(mm, t64, calib, np.eye(4), idx)
    with pytest.raises(TypeError, match="uint16 .* or float32"):      # (its bytes used to be read as float32 here)
        acc.integrate_frame_global(t64, calib, np.eye(4), idx, feat, rgb, frame_idx=0, pcd_min=np.zeros(3))
    # the accepted forms still work: 1.125 m as uint16 millimetres and as float32 metres give the same box
    a, b = mm.copy(), mm.copy()
    ops.points_bbox(a, np.full((H, W), 1125, np.uint16), calib, np.eye(4), idx)
    ops.points_bbox(b, torch.full((H, W), 1.125, dtype=torch.float32, device="cuda"), calib, np.eye(4), idx)
    assert same_bounds(a, b) and np.isfinite(a).all()


# ---------------------------------------------------------------------------------------------------------------- pass 2
@pytest.mark.parametrize("replay", [False, True], ids=["sums", "replay"])
@pytest.mark.parametrize("deferred", [False, True], ids=["frame_calls", "deferred"])
def test_g10_through_the_gpu(ops, golden, deferred, replay):
    """the reference's run on a scene full of exact halves (tools/gen_golden.py G10): voxel ids, their order and occupied_ids bit
    for bit, every fused point counted; with the replay log weight and grid_rgb are the reference's, bit for bit, across the
    dtype switch (5 186 voxels > the grid_size[0] * grid_size[2] = 1 890 rows the reference reserves)"""
    g = golden("g10_multi_floor_edges.npz")
    nfr = len(g["depths_u16"])
    Ts = [g["poses"][i] @ H2C for i in range(nfr)]
    feats = list(g["feats"])
    acc = run_gpu_global(ops, g["grid_size"], float(g["cs"]), g["pcd_min"], g["calib"], Ts, g["depths_u16"], g["rgbs"], feats,
                         g["samples_pass2"], replay=replay, deferred=deferred)
    _, ref, pts = run_oracle_global(g["pcd_min"], g["pcd_max"], float(g["cs"]), g["calib"], Ts, g["depths_u16"] / 1000.0, g["rgbs"],
                                    feats, g["samples_pass2"])
    assert np.array_equal(ref["grid_pos"], g["grid_pos"])
    assert acc.num_voxels() == int(g["max_id"]) and acc.num_points() == pts
    assert acc.capacity >= int(g["max_id"]) > int(g["grid_size"][0] * g["grid_size"][2])
    out = acc.finalize()
    assert np.array_equal(out["grid_pos"], g["grid_pos"])
    occ = -np.ones(tuple(g["occ_shape"]), dtype=np.int32)
    nz = g["occ_nz"]
    occ[nz[:, 0], nz[:, 1], nz[:, 2]] = g["occ_nz_vals"]
    assert np.array_equal(out["occupied_ids"], occ)
    np.testing.assert_allclose(out["grid_feat"], g["grid_feat"], rtol=FEAT_RTOL, atol=FEAT_RTOL * 14.3)
    if replay:
        assert np.array_equal(out["weight"], g["weight"].astype(np.float32))
        assert np.array_equal(out["grid_rgb"], np.floor(g["grid_rgb"]).astype(np.uint8))
    else:
        compare_maps(out, dict(ref, grid_rgb=np.floor(ref["grid_rgb"]).astype(np.uint8)), 14.3)


def exact_coord(q, pmin, cs):
    """a float64 coordinate g with (g - pmin) / cs == q exactly, in float64 (the kernel's and np.round's input)"""
    g = pmin + q * cs
    cands = [g]
    lo = hi = g
    for _ in range(16):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cands += [lo, hi]
    for c in cands:
        if (c - pmin) / cs == q:
            return float(c)
    raise AssertionError(f"no float64 coordinate reaches {q!r}")


@pytest.mark.parametrize("grid", [(6, 7, 4), (7, 4, 5)], ids=["even_odd_even", "odd_even_odd"])
def test_half_way_rounding_on_every_axis(ops, grid):
    """exact camera-frame points (calib_inv and the pose place each one on a chosen float64 coordinate) at (p - pcd_min) / cs =
    -0.5 (np.round -> -0.0: kept, index 0), -0.5 - 1 ulp (dropped), 0.5, 1.5, 2.5, 3.5 (half to even), n - 0.5 (even n: rounds to
    n, dropped; odd n: n - 1, kept), n - 0.5 - 1 ulp (kept) on one axis at a time, against np.round and the oracle"""
    cs, D = 0.25, 4
    pcd_min = np.array([0.125, 0.0625, 0.125])
    n = np.array(grid)                                   # (x, y, z) sizes
    pcd_max = pcd_min + (n - 1) * cs
    H, W = 2, 2
    kinv = np.array([0.0, 0, 0, 0, 0, 0, 0, 0, 1])        # every pixel -> camera point (0, 0, depth)
    calib = np.array([1.0, 0, 1, 0, 1.0, 1, 0, 0, 1])
    pts, Ts = [], []
    for axis in range(3):
        m = int(n[axis])
        for q in (-0.5, np.nextafter(-0.5, -np.inf), np.nextafter(-0.5, np.inf), 0.5, 1.5, 2.5, 3.5, m - 0.5,
                  np.nextafter(m - 0.5, -np.inf)):
            p = pcd_min + 1.0 * cs                       # index 1 on the other axes
            p[axis] = exact_coord(q, pcd_min[axis], cs)
            T = np.eye(4)
            T[:3, :3] = 0.0
            T[:3, 3] = p                                 # global point = translation, exactly
            pts.append(p)
            Ts.append(T)
    pts = np.array(pts)
    want = np.round((pts - pcd_min) / cs).astype(int)    # vlmap_builder_multi_floor.py:146, literally
    kept = np.all((want >= 0) & (want < n), axis=1)
    assert 0 < kept.sum() < len(pts)
    nfr = len(Ts)
    rng = np.random.default_rng(5)
    depths = [np.ones((H, W), np.float32)] * nfr
    rgbs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(nfr)]
    feats = [rng.standard_normal((D, 2, 2)).astype(np.float32) for _ in range(nfr)]
    samples = [np.array([3], np.int32)] * nfr
    acc = run_gpu_global(ops, n, cs, pcd_min, calib, Ts, depths, rgbs, feats, samples, calib_inv=kinv)
    _, ref, ref_pts = run_oracle_global(pcd_min, pcd_max, cs, calib, Ts, [d.astype(np.float64) for d in depths], rgbs, feats,
                                        samples, calib_inv=kinv)
    out = acc.finalize()
    # (row, col, height) = (x, z, y) index, first-touch order
    first = list(dict.fromkeys(tuple(w) for w in want[kept][:, [0, 2, 1]].tolist()))
    assert out["grid_pos"].tolist() == [list(t) for t in first]
    assert acc.num_points() == ref_pts == kept.sum()
    compare_maps(out, dict(ref, grid_rgb=np.floor(ref["grid_rgb"]).astype(np.uint8)), 4.0)


def two_floor_scene(rng, nfr, H, W, Hf, Wf, D):
    """uint16 depth in fifths of a millimetre (raw values past 32 767 from 6.55 m on), generic poses on two floors 2.6 m apart"""
    from scipy.spatial.transform import Rotation as R
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    depths, rgbs, feats, Ts = [], [], [], []
    for i in range(nfr):
        d = 4.5 + 2.5 * np.sin(2.1 * xx + 0.5 * i) * np.cos(1.4 * yy) + 0.8 * yy + rng.normal(0, 0.01, xx.shape)
        u = np.round(d * 5000).clip(0, 65535).astype(np.uint16)
        u[rng.random(u.shape) < 0.03] = 0
        depths.append(u)
        rgbs.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        f = rng.standard_normal((D, Hf, Wf)).astype(np.float32)
        feats.append((f / np.linalg.norm(f, axis=0, keepdims=True) * 14.2857).astype(np.float32))
        T = np.eye(4)
        T[:3, :3] = R.from_euler("yxz", [0.9 * i, 0.1 * np.sin(i), 0.05 * i]).as_matrix()
        T[:3, 3] = [0.4 * i, 1.5 + 2.6 * (i >= nfr // 2), -0.3 * i]
        Ts.append(T @ H2C)
    return depths, rgbs, feats, Ts


@pytest.mark.parametrize("D,H,W,deferred,capacity", [
    (5, 48, 64, False, 8),
    (64, 256, 384, True, None),        # 32 768 samples in one deferred frame: the compacted-owner K3
    (257, 48, 64, True, 8),
    (1600, 48, 64, False, 8),          # D > 1536: fuse_generic_kernel
], ids=["D5_cap8", "D64_32k_deferred", "D257_deferred_cap8", "D1600_generic_cap8"])
def test_two_floor_scene_drops_points_outside_the_box(ops, D, H, W, deferred, capacity):
    """depth_sample_rate 3: pass 2 samples other pixels than pass 1, so some of its points fall outside the pass-1 box -- the
    reference would wrap or raise there, the library drops them (flag 8) and does not count them; the oracle drops them too.
    Feature image smaller than the depth image; capacity 8 doubles nine times and more."""
    rng = np.random.default_rng(D)
    nfr, rate, cs, div = 6, 3, 0.25, 5000.0
    Hf, Wf = H // 3 + 1, W // 3 - 1
    depths, rgbs, feats, Ts = two_floor_scene(rng, nfr, H, W, Hf, Wf, D)
    calib = np.array([W / 2, 0, W / 2, 0, W / 2, H / 2, 0, 0, 1])
    rs = np.random.RandomState(D)
    s1 = [O.sample_indices(rs, H * W, rate) for _ in range(nfr)]
    s2 = [O.sample_indices(rs, H * W, rate) for _ in range(nfr)]
    assert len(s2[0]) >= (32768 if H * W >= 98304 else 1)
    for i in range(nfr):                 # 13.1 m spikes only pass 2 samples: they lie beyond the pass-1 box
        depths[i].reshape(-1)[np.setdiff1d(s2[i], s1[i])[:20]] = 65535
    assert max(int(d.max()) for d in depths) == 65535 and sum(int(((d > 32767) & (d < 65535)).sum()) for d in depths) > 100
    depths_m = [d / div for d in depths]
    mm, mm_ref = np.array([np.inf] * 3 + [-np.inf] * 3), np.array([np.inf] * 3 + [-np.inf] * 3)
    for i in range(nfr):
        ops.points_bbox(mm, depths[i], calib, Ts[i], s1[i], depth_div=div)
        O.points_bbox(mm_ref, depths_m[i], calib, Ts[i], s1[i])
    assert same_bounds(mm, mm_ref)
    grid = grid_of(mm, cs)
    assert len(set(grid.tolist())) == 3
    # how many pass-2 points lie outside the box (the test is only worth something if there are some)
    kinv = np.linalg.inv(calib.reshape(3, 3))
    outside = 0
    for i in range(nfr):
        v, u = np.divmod(s2[i], W)
        z = depths_m[i].reshape(-1)[s2[i]]
        pc = (kinv @ np.stack([u + 0.5, v + 0.5, np.ones(len(u))])) * z
        pc = pc[:, (pc[2] > 0.1) & (pc[2] < 100)]
        idx = np.round(((Ts[i] @ np.vstack([pc, np.ones(pc.shape[1])]))[:3].T - mm[:3]) / cs)
        outside += int((~np.all((idx >= 0) & (idx < grid), axis=1)).sum())
    assert outside > 0
    acc = run_gpu_global(ops, grid, cs, mm[:3], calib, Ts, depths, rgbs, feats, s2, depth_div=div, capacity=capacity,
                         deferred=deferred, replay=True)
    _, ref, pts = run_oracle_global(mm[:3], mm[3:], cs, calib, Ts, depths_m, rgbs, feats, s2)
    assert acc.num_voxels() == len(ref["grid_pos"]) and acc.num_points() == pts
    assert capacity is None or acc.capacity >= len(ref["grid_pos"]) > 8 << 8
    out = acc.finalize()
    rgb = np.floor(ref["grid_rgb"]).astype(np.uint8)
    compare_maps(out, dict(ref, grid_rgb=rgb), 14.3)
    # the replay log gives the oracle's sequential weight and colour (the reference's dtype semantics) bit for bit
    assert np.array_equal(out["weight"], ref["weight"].astype(np.float32)) and np.array_equal(out["grid_rgb"], rgb)


def test_multi_floor_builder_reproduces_g10(golden, tmp_path):
    """VLMapBuilderMultiFloor end to end on G10: both passes from the global RNG, bbox bit for bit, the map of the reference run"""
    check_multi_floor_builder(golden("g10_multi_floor_edges.npz"), tmp_path)
