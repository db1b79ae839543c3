"""The backward resampling of a voxel map on the GPU (csrc/avl_mappull.hip through ops.pull_plan, ops.pull_rows, ops.pull_map,
VLMap.resample(method=...) and apps/audit_map.py --fuse-resample) against the restatement of tests/_mappull_ref.py.

Every comparison is of bytes: the pulled-back point and the corner weights are float64 with every operation rounded once, the members
and their order are fixed, a gathered element is a float64 sum in corner order.  The restatement is fed the same sixteen doubles of
the inverse transform that the kernels get (ops.inverse_transform)."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
import _mappull_ref as R  # noqa: E402

CS = 0.05
MODES = ("nearest", "linear")


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def all_cells(gs, vh):
    return np.stack(np.meshgrid(np.arange(gs), np.arange(gs), np.arange(vh), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)


def rot_z(deg, t=(0.0, 0.0, 0.0), scale=1.0):
    a = np.radians(deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, :3] *= scale
    T[:3, 3] = t
    return T


def tilt_x(deg, t=(0.0, 0.0, 0.0)):
    a = np.radians(deg)
    T = np.eye(4)
    T[1:3, 1:3] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = t
    return T


def box(r0, r1, c0, c1, h0, h1):
    return np.array([(r, c, h) for r in range(r0, r1 + 1) for c in range(c0, c1 + 1) for h in range(h0, h1 + 1)], np.int32)


@functools.lru_cache(maxsize=None)
def scene(gs):
    """(cells, weights, vh): 8 -> every cell of the 8 x 8 x 5 grid but each seventh, in a shuffled order; 33 -> a 25 x 25 x 8 block around
    the double-width cell of the 33 x 33 x 31 grid (more than one scan block of the target's bit plane, 1055 words) and a slab above it"""
    if gs == 8:
        cells, vh = all_cells(8, 5), 5
        cells = cells[np.arange(len(cells)) % 7 != 3]
    else:
        cells, vh = np.concatenate([box(4, 28, 4, 28, 0, 7), box(10, 20, 12, 30, 27, 30)]), 31
    rng = np.random.default_rng(gs)
    cells = cells[rng.permutation(len(cells))]
    w = rng.uniform(0.5, 40.0, len(cells)).astype(np.float32)
    cells.setflags(write=False), w.setflags(write=False)
    return cells, w, vh


def check_plan(ops, cells, w, gs, vh, T=None, shift=(0, 0, 0), use=None, interp="linear", min_support=0.5, cs=CS):
    cells = np.asarray(cells, np.int32).reshape(-1, 3)
    want = R.ref_pull_plan(cells, w, gs, cs, vh, ops.inverse_transform(T, "test"), shift, use, interp, min_support)
    got = ops.pull_plan(cells, w, gs, cs, vh, transform=T, shift=shift, use_b=use, interp=interp, min_support=min_support)
    print(f"gs {gs} {interp} support {min_support}: n_out {got.n_out} (restated {want['n_out']}), counts {got.counts.tolist()} ({want['counts'].tolist()})")
    assert got.n_out == want["n_out"]
    for name, key in (("cells", "cells"), ("members", "members"), ("lam", "lam"), ("counts", "counts"), ("occupied_ids", "occupied")):
        g = getattr(got, name)
        assert same_bytes(g, want[key]), (name, interp, None if name != "members" else (g[(g != want[key]).any(1)][:4], want[key][(g != want[key]).any(1)][:4]))
    return got


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("interp", MODES)
@pytest.mark.parametrize("gs", (8, 33))
def test_plan_without_a_transform_is_the_cell_moved_by_the_shift(ops, gs, interp):
    cells, w, vh = scene(gs)
    p = check_plan(ops, cells, w, gs, vh, None, (0, 0, 0), interp=interp)
    assert p.n_out == len(cells) and p.counts.tolist() == [0, 0, 0, 0] and (p.lam[:, 0] == 1.0).all() and (p.members[:, 1:] == -1).all()
    assert same_bytes(p.cells, cells[p.members[:, 0]])
    p = check_plan(ops, cells, w, gs, vh, None, (1, -2, 0), interp=interp)
    assert same_bytes(p.cells, cells[p.members[:, 0]] + np.array([1, -2, 0], np.int32))
    pushed = check_plan(ops, cells, w, gs, vh, None, (0, gs // 4, 2), interp=interp)              # a part of the rows leaves the grid
    assert 0 < pushed.n_out < len(cells) and pushed.counts.tolist() == [0, 0, 0, len(cells) - pushed.n_out]


@pytest.mark.parametrize("interp", MODES)
@pytest.mark.parametrize("gs", (8, 33))
def test_plan_the_identity_as_a_matrix_returns_every_cell(ops, gs, interp):
    cells, w, vh = scene(gs)
    p = check_plan(ops, cells, w, gs, vh, np.eye(4), interp=interp)
    # a quotient (k + 0.5) cs / cs may come out one rounding off the centre: the neighbour then is a member with a lambda of 1e-16
    assert p.n_out == len(cells) and (np.abs(p.lam.sum(1) - 1.0) <= 1e-9).all() and same_bytes(p.cells, cells[p.members[np.arange(p.n_out), p.lam.argmax(1)]])
    if interp == "nearest":
        assert (p.counts == 0).all() and (p.lam[:, 0] == 1.0).all()


@pytest.mark.parametrize("interp", MODES)
@pytest.mark.parametrize("deg", (0.5, 3.0, 45.0, 180.0))
@pytest.mark.parametrize("gs", (8, 33))
def test_plan_rotations_with_a_sub_cell_translation(ops, gs, deg, interp):
    cells, w, vh = scene(gs)
    p = check_plan(ops, cells, w, gs, vh, rot_z(deg, (0.013, -0.02, 0.007)), interp=interp)
    assert 0 < p.n_out and (interp == "nearest" or (p.members >= 0).sum(1).max() == 8)


@pytest.mark.parametrize("interp", MODES)
@pytest.mark.parametrize("gs", (8, 33))
def test_plan_a_tilt_clips_at_the_height_band_and_a_scale_is_not_rigid(ops, gs, interp):
    cells, w, vh = scene(gs)
    tilted = check_plan(ops, cells, w, gs, vh, tilt_x(20.0, (0.0, 0.01, 0.02)), interp=interp)
    assert 0 < tilted.n_out and tilted.counts[3] > 0                        # rows of B that no cell of the band reaches
    grown = check_plan(ops, cells, w, gs, vh, rot_z(7.0, (0.004, 0.0, 0.0), scale=1.5), interp=interp)
    assert grown.n_out > 0
    if gs == 33:
        assert grown.n_out > len(cells)                                     # every voxel covers 1.5^3 cells


@pytest.mark.parametrize("min_support", (0.25, 0.5, 1.0))
def test_plan_min_support(ops, min_support):
    for gs in (8, 33):
        cells, w, vh = scene(gs)
        p = check_plan(ops, cells, w, gs, vh, rot_z(3.0, (0.013, -0.02, 0.0)), min_support=min_support)
        assert (p.lam.sum(1) >= min_support - 1e-15).all()
    loose = ops.pull_plan(cells, w, 33, CS, vh, transform=rot_z(3.0, (0.013, -0.02, 0.0)), min_support=0.01, want_occupied=False)
    assert loose.n_out > p.n_out and loose.occupied_ids is None and loose.n_out + loose.counts[2] == p.n_out + p.counts[2]


@pytest.mark.parametrize("interp", MODES)
def test_plan_a_random_sparse_map_with_masks_weights_and_rows_outside(ops, interp):
    rng = np.random.default_rng(12)
    every = all_cells(33, 31)
    cells = np.concatenate([every[rng.choice(len(every), 292, replace=False)], [(33, 0, 0), (0, -1, 0), (5, 5, 31), (-1, -1, -1), (2 ** 31 - 1, 0, 0),
                                                                                  (0, 33, 30), (16, 16, 0), (16, 16, 1)]]).astype(np.int32)
    w = rng.uniform(0.5, 40.0, 300).astype(np.float32)
    w[3], w[50], w[100], w[150], w[298] = 0.0, np.nan, -1.0, np.inf, 0.0    # (16, 16, 0) is unselected by its weight
    use = rng.random(300) < 0.85
    use[292], use[299] = False, True
    p = check_plan(ops, cells, w, 33, 31, rot_z(10.0, (0.013, -0.02, 0.007)), (0, 0, 0), use, interp, 0.125)
    sel = use & np.isfinite(w) & (w > 0)
    assert p.counts[0] == (~sel).sum() and p.counts[1] == sel[292:298].sum() and p.n_out > 0
    assert sel[p.members[p.members >= 0]].all() and not np.isin(p.members, np.arange(292, 299)).any()
    # the same list whatever the order of B's rows
    order = rng.permutation(300)
    q = ops.pull_plan(cells[order], w[order], 33, CS, 31, transform=rot_z(10.0, (0.013, -0.02, 0.007)), use_b=use[order], interp=interp, min_support=0.125)
    assert same_bytes(q.cells, p.cells) and same_bytes(q.lam, p.lam) and same_bytes(np.where(q.members >= 0, order[q.members], -1).astype(np.int32), p.members)
    assert same_bytes(q.counts, p.counts)


@pytest.mark.parametrize("interp", MODES)
def test_plan_no_row_one_row_and_two_rows_in_one_cell(ops, interp):
    none = check_plan(ops, np.zeros((0, 3), np.int32), np.zeros(0, np.float32), 8, 5, rot_z(3.0), interp=interp)
    assert none.n_out == 0 and none.cells.shape == (0, 3) and none.members.shape == (0, 8) and (none.occupied_ids == -1).all()
    check_plan(ops, np.zeros((0, 3), np.int32), np.zeros(0, np.float32), 33, 31, None, interp=interp)
    one = check_plan(ops, [(3, 4, 2)], np.array([2.5], np.float32), 8, 5, rot_z(45.0, (0.01, 0.0, 0.0)), interp=interp, min_support=0.1)
    assert one.n_out >= 1 and (one.members[one.members >= 0] == 0).all()
    check_plan(ops, [(3, 4, 2)], np.array([2.5], np.float32), 8, 5, None, (1, 1, 1), interp=interp)
    unselected = check_plan(ops, [(3, 4, 2)], np.array([np.nan], np.float32), 8, 5, None, interp=interp)
    assert unselected.n_out == 0 and unselected.counts.tolist() == [1, 0, 0, 0]
    twice = np.array([(1, 1, 1), (2, 2, 2), (1, 1, 1)], np.int32)
    for T in (None, rot_z(3.0)):
        with pytest.raises(ValueError, match="share a cell"):
            ops.pull_plan(twice, np.ones(3, np.float32), 8, CS, 5, transform=T, interp=interp)
    # a masked or weightless twin does not count
    assert ops.pull_plan(twice, np.ones(3, np.float32), 8, CS, 5, use_b=np.array([1, 1, 0], bool), interp=interp).n_out == 2
    assert ops.pull_plan(twice, np.array([0, 1, 1], np.float32), 8, CS, 5, interp=interp).members[:, 0].tolist() == [2, 1]


# ------------------------------------------------------------------ the rows
GS, VH, N_B = 8, 5, 240


@functools.lru_cache(maxsize=None)
def rows_inputs():
    """three quarters of the cells of the 8 x 8 x 5 grid under 10 degrees and a low support: voxels with one to eight members"""
    rng = np.random.default_rng(1)
    cells = all_cells(GS, VH)[rng.permutation(GS * GS * VH)][:N_B]
    w, rgb = rng.uniform(0.5, 40.0, N_B).astype(np.float32), rng.integers(0, 256, (N_B, 3)).astype(np.uint8)
    w[:4] = [1e-40, 3e38, 1.0, 0.75]                                          # a denormal and a huge weight among them
    T = rot_z(10.0, (0.013, -0.02, 0.007))
    for x in (cells, w, rgb, T):
        x.setflags(write=False)
    return cells, w, rgb, T


@functools.lru_cache(maxsize=None)
def rows_feats(D):
    feat = np.random.default_rng(100 + D).standard_normal((N_B, D)).astype(np.float32)
    feat[:6, 0] = np.array([-0.0, 1e-45, -3.4e38, np.inf, 0.0, 1.17549435e-38], np.float32)
    feat[6:12, D - 1] = feat[:6, 0]
    feat.setflags(write=False)
    return feat


@functools.lru_cache(maxsize=None)
def rows_want(D, interp):
    from avlmaps_amd import ops
    cells, w, rgb, T = rows_inputs()
    plan = R.ref_pull_plan(cells, w, GS, CS, VH, ops.inverse_transform(T, "test"), (0, 0, 0), None, interp, 0.05)
    return plan, R.ref_pull_rows(plan, rows_feats(D), w, rgb)


def off_by_one_float(ops, a):
    """`a` on the device at an address that is 4 bytes past a 16-byte boundary: (the owner, a DeviceView of a's shape)"""
    from avlmaps_amd import _lib
    a = np.ascontiguousarray(a, np.float32)
    buf = ops.DeviceArray((a.size + 1,), np.float32)
    assert buf.ptr % 16 == 0
    if a.size:
        _lib.check(_lib.load().avl_memcpy_h2d(buf.ptr + 4, a.ctypes.data, a.nbytes, None), "avl_memcpy_h2d")
    _lib.check(_lib.load().avl_stream_sync(None), "avl_stream_sync")
    return buf, ops.DeviceView(buf.ptr + 4, a.shape, np.float32)


@pytest.mark.parametrize("D", (1, 3, 4, 5, 256, 260, 512))
def test_rows_equal_the_restatement_on_both_load_paths(ops, D):
    from avlmaps_amd import _lib
    cells, w, rgb, T = rows_inputs()
    feat = rows_feats(D)
    ref_plan, want = rows_want(D, "linear")
    plan = ops.pull_plan(cells, w, GS, CS, VH, transform=T, min_support=0.05)
    assert plan.n_out == ref_plan["n_out"] and same_bytes(plan.members, ref_plan["members"]) and same_bytes(plan.lam, ref_plan["lam"])
    assert set((plan.members >= 0).sum(1).tolist()) == set(range(1, 9))                         # voxels with 1 .. 8 members
    got = ops.pull_rows(plan, feat, w, rgb)
    for g, wnt, name in zip(got, want, ("grid_feat", "weight", "grid_rgb")):
        assert same_bytes(g, wnt), (D, name)
    # every matrix one float past a 16-byte boundary, the output too: the scalar path, the same bytes
    keep_b, view_b = off_by_one_float(ops, feat)
    keep_o, view_o = off_by_one_float(ops, np.zeros((plan.n_out, D), np.float32))
    again = ops.pull_rows(plan, view_b, w, rgb, feat_out=view_o)
    assert again[0] is view_o
    back = np.empty((plan.n_out, D), np.float32)
    _lib.check(_lib.load().avl_memcpy_d2h(back.ctypes.data, view_o.ptr, back.nbytes, None), "avl_memcpy_d2h")
    assert same_bytes(back, want[0]) and same_bytes(again[1], want[1]) and same_bytes(again[2], want[2])
    # one side aligned, the other not; a caller's aligned feat_out
    assert same_bytes(ops.pull_rows(plan, view_b, w, rgb)[0], want[0])
    mine = ops.DeviceArray((plan.n_out, D), np.float32)
    out = ops.pull_rows(plan, feat, w, rgb, feat_out=mine, device=True)
    assert out[0] is mine and same_bytes(mine.numpy(), want[0]) and same_bytes(out[1].numpy(), want[1])


def test_rows_a_view_that_is_not_contiguous(ops):
    cells, w, rgb, T = rows_inputs()
    feat = rows_feats(512)
    plan = ops.pull_plan(cells, w, GS, CS, VH, transform=T, min_support=0.05)
    wide, tall = np.zeros((N_B, 1024), np.float32), np.zeros((2 * N_B, 512), np.float32)
    wide[:, 1::2], tall[::2] = feat, feat
    want = rows_want(512, "linear")[1]
    assert same_bytes(ops.pull_rows(plan, wide[:, 1::2], w, rgb)[0], want[0]) and same_bytes(ops.pull_rows(plan, tall[::2], w, rgb)[0], want[0])


@pytest.mark.parametrize("D", (5, 512))
def test_rows_in_nearest_mode_are_the_members_rows_bit_for_bit(ops, D):
    cells, w, rgb, T = rows_inputs()
    feat = rows_feats(D)
    plan = ops.pull_plan(cells, w, GS, CS, VH, transform=T, interp="nearest")
    ref_plan, want = rows_want(D, "nearest")
    assert same_bytes(plan.members, ref_plan["members"]) and (plan.members[:, 1:] == -1).all() and plan.n_out > N_B // 2
    m = plan.members[:, 0]
    # rows 0, 1 and 3 hold -0.0, a denormal and inf in column 0, rows 6, 7 and 9 in column D - 1, row 0 a denormal weight: all are members
    assert {0, 1, 3, 6, 7, 9} <= set(m.tolist())
    got = ops.pull_rows(plan, feat, w, rgb)
    assert same_bytes(got[0], feat[m]) and same_bytes(got[1], w[m]) and same_bytes(got[2], rgb[m])
    at = {row: int(np.flatnonzero(m == row)[0]) for row in (0, 1, 3, 6, 7, 9)}
    for col, (zero, tiny, inf) in ((0, (0, 1, 3)), (D - 1, (6, 7, 9))):
        assert got[0][at[zero], col] == 0.0 and np.signbit(got[0][at[zero], col])
        assert got[0][at[tiny], col].tobytes() == np.float32(1e-45).tobytes() and got[0][at[tiny], col] > 0.0
        assert got[0][at[inf], col] == np.inf
    assert got[1][at[0]].tobytes() == np.float32(1e-40).tobytes() and got[1][at[1]] == np.float32(3e38)
    for g, wnt in zip(got, want):
        assert same_bytes(g, wnt)


def test_rows_rgb_truncates_at_a_quotient_just_below_a_whole_number(ops):
    # the point between the centres of two cells in height: lambda 0.5 each, weights 1 and 999
    cells = np.array([(3, 3, 1), (3, 3, 2)], np.int32)
    w, rgb = np.array([1, 999], np.float32), np.array([(0, 10, 255), (1, 11, 254)], np.uint8)
    feat = np.ones((2, 4), np.float32)
    T = np.eye(4)
    T[2, 3] = 0.5 * CS
    plan = ops.pull_plan(cells, w, GS, CS, VH, transform=T, min_support=0.9)
    ref = R.ref_pull_plan(cells, w, GS, CS, VH, ops.inverse_transform(T, "test"), min_support=0.9)
    assert plan.n_out == ref["n_out"] == 1 and plan.cells.tolist() == [[3, 3, 2]] and same_bytes(plan.lam, ref["lam"])
    assert (plan.members[0] >= 0).sum() == 2 and np.abs(plan.lam[0][plan.members[0] >= 0] - 0.5).max() <= 1e-9
    got, want = ops.pull_rows(plan, feat, w, rgb), R.ref_pull_rows(ref, feat, w, rgb)
    assert got[2].tolist() == [[0, 10, 254]] and same_bytes(got[2], want[2]) and same_bytes(got[1], want[1]) and abs(float(got[1][0]) - 500.0) <= 1e-3
    assert same_bytes(got[0], want[0])


# ------------------------------------------------------------------ pull_map, the point of the feature, the map layer
MGS, MVH, MD, MCS = 24, 8, 128, 0.1


def map_arrays(seed, cells):
    rng = np.random.default_rng(seed)
    n = len(cells)
    return (np.asarray(cells, np.int32).reshape(-1, 3), rng.standard_normal((n, MD)).astype(np.float32), rng.uniform(1, 30, n).astype(np.float32),
            rng.integers(0, 256, (n, 3)).astype(np.uint8))


def make_vlmap(arrays):
    from test_host_mirror import Cfg
    from avlmaps_amd.map import VLMap
    cfg = Cfg(map_type="vlmap", grid_size=MGS, cell_size=MCS,
              pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                            base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0]))
    vm = VLMap(cfg)
    vm.prefetch_device = False
    pos, feat, weight, rgb = (x.copy() for x in arrays)
    vm.grid_pos, vm.grid_feat, vm.weight, vm.grid_rgb, vm.mapped_iter_list = pos, feat, weight, rgb, [0, 1, 2]
    vm.occupied_ids = -np.ones((MGS, MGS, MVH), np.int32)
    vm.occupied_ids[tuple(pos.T)] = np.arange(len(pos))
    vm.scores_mat = None
    return vm


@pytest.mark.parametrize("interp", MODES)
def test_without_a_transform_pull_map_is_the_forward_fuse_maps_in_linear_cell_order(ops, interp):
    b = map_arrays(4, np.random.default_rng(6).permutation(box(2, 12, 3, 12, 0, 7))[:500])
    use = np.random.default_rng(7).random(500) < 0.9
    empty = (np.zeros((0, 3), np.int32), np.zeros((0, MD), np.float32), np.zeros(0, np.float32), np.zeros((0, 3), np.uint8))
    for shift in ((0, 0, 0), (3, -2, 1), (0, 14, 0)):
        fwd = ops.fuse_maps(*empty, *b, MGS, MCS, MVH, shift=shift, use_b=use)
        got = ops.pull_map(*b, MGS, MCS, MVH, shift=shift, use_b=use, interp=interp)
        order = np.argsort((fwd.grid_pos[:, 0].astype(np.int64) * MGS + fwd.grid_pos[:, 1]) * MVH + fwd.grid_pos[:, 2])
        assert got.n_out == fwd.n_out == len(order) and 0 < got.n_out
        assert same_bytes(got.grid_pos, fwd.grid_pos[order]) and same_bytes(got.grid_feat, fwd.grid_feat[order])
        assert same_bytes(got.weight, fwd.weight[order]) and same_bytes(got.grid_rgb, fwd.grid_rgb[order])
        inverse = np.empty(len(order), np.int32)
        inverse[order] = np.arange(len(order), dtype=np.int32)
        assert same_bytes(got.occupied_ids, np.where(fwd.occupied_ids >= 0, inverse[fwd.occupied_ids], -1).astype(np.int32))
        assert got.counts["unselected_b"] == fwd.counts["unselected_b"] and got.counts["outside_b"] + got.counts["unused_b"] == fwd.counts["outside_b"]
    on_device = ops.pull_map(*b, MGS, MCS, MVH, interp=interp, want_occupied=False, device=True)
    assert not on_device.plan._host                                                             # nothing of the plan was read back yet
    order_b = np.argsort((b[0][:, 0] * MGS + b[0][:, 1]) * MVH + b[0][:, 2]).astype(np.int32)
    assert same_bytes(on_device.members[:, 0], order_b) and (on_device.members[:, 1:] == -1).all() and same_bytes(on_device.lam, (on_device.members >= 0) * 1.0)
    assert on_device.occupied_ids is None and same_bytes(on_device.grid_feat.numpy(), b[1][np.argsort((b[0][:, 0] * MGS + b[0][:, 1]) * MVH + b[0][:, 2])])
    assert same_bytes(on_device.grid_pos.numpy(), b[0][np.argsort((b[0][:, 0] * MGS + b[0][:, 1]) * MVH + b[0][:, 2])])


@pytest.mark.parametrize("deg", (3.0, 45.0))
def test_a_turned_block_comes_out_without_pinholes(ops, deg):
    """the block of DESIGN.md 4.33: 25 x 25 x 8 cells at rows and columns 4 .. 28 and heights 0 .. 7 of a 33 x 33 x 10 grid"""
    gs, vh = 33, 10
    block = box(4, 28, 4, 28, 0, 7)
    w = np.ones(len(block), np.float32)
    T = rot_z(deg, (0.013, -0.02, 0.0))
    moved, inside = ops.move_cells(block, gs, CS, vh, transform=T)
    forward = np.unique(moved[inside.astype(bool)], axis=0)
    holes = R.pinholes(forward, gs, vh)
    print(f"{deg} degrees: forward {len(forward)} cells, {holes} pinholes")
    assert holes > 0 and len(forward) < len(block)
    # the figures of DESIGN.md 4.33 and 4.34, which the restatements give: (forward cells, forward pinholes, backward cells)
    figures = {3.0: (4856, 8, 5000), 45.0: (3904, 816, 4864)}[deg]
    assert (len(forward), holes) == figures[:2]
    for interp in MODES:
        p = ops.pull_plan(block, w, gs, CS, vh, transform=T, interp=interp)
        print(f"{deg} degrees: {interp} {p.n_out} cells, {R.pinholes(p.cells, gs, vh)} pinholes")
        assert R.pinholes(p.cells, gs, vh) == 0 and p.n_out >= len(forward)
        assert p.n_out == figures[2]


def test_resample_methods_equal_the_restatement_and_the_default_stays_forward(ops):
    from avlmaps_amd.apps.common import HashClip
    b = map_arrays(5, np.random.default_rng(8).permutation(box(3, 14, 4, 15, 0, 6))[:700])
    vm = make_vlmap(b)
    vm.categories = ["chair", "table"]
    T, shift = rot_z(12.0, (0.03, -0.02, 0.0)), (1, 0, 0)
    default, forward = vm.resample(T, shift), vm.resample(T, shift, method="forward")
    for name in ("grid_pos", "grid_feat", "weight", "grid_rgb", "occupied_ids"):
        assert same_bytes(getattr(default, name), getattr(forward, name)), name
    assert default.resample_counts == forward.resample_counts and "new_cells" in default.resample_counts
    q = np.random.default_rng(9).standard_normal((4, MD)).astype(np.float32)
    for method, support in (("nearest", 0.5), ("linear", 0.5), ("linear", 0.3)):
        out = vm.resample(T, shift, method=method, min_support=support)
        plan = R.ref_pull_plan(b[0], b[2], MGS, MCS, MVH, ops.inverse_transform(T, "test"), shift, None, method, support)
        want = R.ref_pull_rows(plan, b[1], b[2], b[3])
        assert same_bytes(out.grid_pos, plan["cells"]) and same_bytes(out.occupied_ids, plan["occupied"]) and len(out.grid_pos) > 300
        for name, wnt in zip(("grid_feat", "weight", "grid_rgb"), want):
            assert same_bytes(getattr(out, name), wnt), (method, name)
        assert out.resample_counts == dict(zip(ops.PULL_COUNTS, plan["counts"].tolist()))
        assert out is not vm and type(out) is type(vm) and out.mapped_iter_list == [0, 1, 2] and out.categories == ["chair", "table"] and out.scores_mat is None
        fresh = make_vlmap((plan["cells"], *want))
        fresh.categories = ["chair", "table"]
        am, sc = out.index_queries(q, want_scores=True)
        am_fresh, sc_fresh = fresh.index_queries(q, want_scores=True)
        assert len(am) == plan["n_out"] and np.array_equal(am, am_fresh) and np.array_equal(sc, sc_fresh)
        for m in (out, fresh):
            m.clip_feat_dim, m.clip_model = MD, HashClip(MD)
        assert np.array_equal(out.index_map("chair", with_init_cat=False), fresh.index_map("chair", with_init_cat=False))
    assert len(vm.grid_pos) == 700 and same_bytes(vm.grid_feat, b[1])
    no_rgb = make_vlmap(b)
    no_rgb.grid_rgb = None
    assert no_rgb.resample(T, method="linear").grid_rgb is None
    # a turned copy compared against the original: nothing vanishes inside the block
    turned = vm.resample(rot_z(2.0, (0.013, -0.02, 0.0)), method="linear")
    assert vm.compare(turned, radius=1).summary()["voxels_b"] == len(turned.grid_pos)


# ------------------------------------------------------------------ the app
from test_audit_gpu import _config, _config_file, EG, EVH, visit  # noqa: E402,F401  (the rendered scene of the audit's end-to-end test)


def test_the_app_fuses_a_later_map_resampled_backward(ops, visit, tmp_path):
    from avlmaps_amd.apps import audit_map
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.utils.mapping_utils import save_3d_map
    root, _, pos = visit

    def load(where):
        vm = VLMap(_config())
        vm.prefetch_device = False
        assert vm.load_map(str(where))
        return vm
    a = load(root / "a")
    n, rng = len(pos), np.random.default_rng(8)
    keep = np.arange(n) % 5 != 0
    feat_b = a.grid_feat[keep].copy()
    feat_b[::3] *= -1
    pos_b = pos[keep]
    occupied = -np.ones((EG, EG, EVH), np.int32)
    occupied[tuple(pos_b.T)] = np.arange(len(pos_b))
    (root / "b" / "vlmap").mkdir(exist_ok=True)
    save_3d_map(root / "b" / "vlmap" / "vlmaps.h5df", feat_b, pos_b, np.full(len(pos_b), 2.0, np.float32), occupied, [0, 1, 2, 3],
                rng.integers(0, 255, (len(pos_b), 3)).astype(np.uint8))
    before_a, before_b = load(root / "a"), load(root / "b")
    res = audit_map.main(["--data-dir", str(root / "a"), "--fuse", str(root / "b"), "--fuse-out", str(tmp_path / "both"), "--stride", "1",
                          "--compare-radius", "0", "--fuse-resample", "linear", "--fuse-min-support", "0.75", "--config", _config_file(tmp_path)])
    assert res["fuse"]["resample"] == "linear" and res["fuse"]["min_support"] == 0.75
    # the same steps through the map layer
    b = load(root / "b")
    T = a.transform_from(root / "b")
    moved = b.resample(T, method="linear", min_support=0.75)
    assert res["fuse"]["resampled"] == moved.resample_counts and set(moved.resample_counts) == set(ops.PULL_COUNTS) and len(moved.grid_pos) > 0
    changes = a.compare(moved, radius=0)
    counts = a.fuse(moved, changes=changes)
    assert res["fuse"]["counts"] == counts and res["fuse"]["summary"] == changes.summary()
    fused = load(tmp_path / "both")
    for name in ("grid_pos", "grid_feat", "weight", "grid_rgb", "occupied_ids"):
        assert same_bytes(np.asarray(getattr(fused, name)), np.asarray(getattr(a, name))), name
    for where, before in ((root / "a", before_a), (root / "b", before_b)):
        again = load(where)
        for name in ("grid_pos", "grid_feat", "weight", "grid_rgb", "occupied_ids"):
            assert same_bytes(np.asarray(getattr(again, name)), np.asarray(getattr(before, name))), (where, name)
