"""The map fusion on the GPU (csrc/avl_mapfuse.hip through ops.move_cells, ops.fuse_plan, ops.fuse_rows, ops.fuse_maps, VLMap.resample
and VLMap.fuse) against the restatements of tests/_mapfuse_ref.py.

Every comparison is of bytes: the move is float64 with every operation rounded once, the plan is integer, a fused element is a
float64 sum in member order."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
import _mapfuse_ref as R  # noqa: E402


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


def rot_z(deg, t=(0.0, 0.0, 0.0)):
    a = np.radians(deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = t
    return T


# ------------------------------------------------------------------ move_cells
def check_move(ops, cells, gs, cs, vh, T=None, shift=(0, 0, 0)):
    cells = np.asarray(cells, np.int32).reshape(-1, 3)
    want = R.ref_move_cells(cells, gs, cs, vh, T, shift)
    got = ops.move_cells(cells, gs, cs, vh, transform=T, shift=shift)
    assert same_bytes(got[0], want[0]), (got[0][(got[0] != want[0]).any(1)][:5], want[0][(got[0] != want[0]).any(1)][:5])
    assert same_bytes(got[1], want[1])
    return got


@pytest.mark.parametrize("gs,vh,cs", [(8, 5, 0.05), (33, 31, 0.05), (33, 31, 1 / 3)])
def test_move_the_identity_returns_every_cell(ops, gs, vh, cs):
    cells = all_cells(gs, vh)
    for T in (None, np.eye(4)):
        moved, inside = ops.move_cells(cells, gs, cs, vh, transform=T)
        assert same_bytes(moved, cells) and inside.dtype == np.uint8 and (inside == 1).all()


@pytest.mark.parametrize("gs", (8, 33))
def test_move_next_to_the_double_width_cell(ops, gs):
    vh, cs, m = 5, 0.05, gs // 2
    cells = [(r, c, h) for r in (m - 2, m - 1, m, m + 1, m + 2) for c in (m - 1, m, m + 1) for h in (0, vh - 1)]
    for f in (-1.6, -1.0, -0.6, -0.4, 0.4, 0.6, 1.0, 1.6):                  # fractions of a cell, both ways across the axes
        got = check_move(ops, cells, gs, cs, vh, rot_z(0.0, (f * cs, -f * cs, 0.0)))
        assert got[1].all() == (gs == 33 or f > -1.6)                       # on the 8-grid -1.6 cells push row 6 (x = -2.5 cells) to row 8
    # a whole-cell shift is added to the indices: next to the axes a translation by two cells in metres is something else (from
    # k = -1, centre -1.5 cells, it reaches 0.5 cells, which is the cell k = 0)
    by_shift = check_move(ops, cells, gs, cs, vh, np.eye(4), shift=(-2, 0, 0))[0]
    by_metres = check_move(ops, cells, gs, cs, vh, rot_z(0.0, (2 * cs, 0.0, 0.0)))[0]
    assert np.array_equal(by_shift[:, 0], np.asarray(cells)[:, 0] - 2) and not np.array_equal(by_shift, by_metres)


@functools.lru_cache(maxsize=None)
def block_cells():
    return np.ascontiguousarray(all_cells(33, 31).reshape(33, 33, 31, 3)[4:29, 4:29, 2:10].reshape(-1, 3))          # 25 x 25 x 8


@pytest.mark.parametrize("deg", (0.5, 3.0, 45.0, 180.0))
def test_move_rotations_with_a_sub_cell_translation(ops, deg):
    moved, inside = check_move(ops, block_cells(), 33, 0.05, 31, rot_z(deg, (0.013, -0.02, 0.0)))
    assert 0 < inside.sum() <= len(inside)
    per_cell = np.unique(moved[inside == 1], axis=0, return_counts=True)[1]
    assert per_cell.max() <= 3


def test_move_a_translation_pushes_a_third_of_the_rows_outside_and_a_tilt_clips_at_the_band(ops):
    cells = all_cells(33, 31)[::7]
    inside = check_move(ops, cells, 33, 0.05, 31, rot_z(0.0, (11 * 0.05, 0.0, 0.0)))[1]
    assert abs(int((inside == 0).sum()) - len(cells) // 3) <= len(cells) // 30
    tilt = np.eye(4)
    tilt[:3, :3] = [[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]]
    inside = check_move(ops, cells, 33, 0.05, 31, tilt)[1]
    assert 0 < inside.sum() < len(cells)


@pytest.mark.parametrize("shift", [(1, -2, 1), (100000, 0, 0), (0, 0, -2 ** 31 + 1), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)])
def test_move_whole_cell_shifts_do_not_wrap(ops, shift):
    cells = all_cells(8, 5)
    for T in (None, rot_z(3.0)):
        inside = check_move(ops, cells, 8, 0.05, 5, T, shift)[1]
        assert inside.any() == (shift == (1, -2, 1))


@pytest.mark.parametrize("n", (0, 1, 65))
def test_move_sizes(ops, n):
    moved, inside = check_move(ops, all_cells(8, 5)[:n], 8, 0.05, 5, rot_z(45.0, (0.01, 0.02, 0.0)), (0, 1, 0))
    assert moved.shape == (n, 3) and inside.shape == (n,)


def test_move_rejects_a_transform_that_is_not_finite_or_not_affine(ops):
    T = np.eye(4)
    T[1, 2] = np.nan
    with pytest.raises(ValueError):
        ops.move_cells(all_cells(8, 5), 8, 0.05, 5, transform=T)
    T = np.eye(4)
    T[3, 0] = 0.5
    with pytest.raises(ValueError):
        ops.move_cells(all_cells(8, 5), 8, 0.05, 5, transform=T)


# ------------------------------------------------------------------ fuse_plan
def check_plan(ops, cells_a, w_a, cells_b, w_b, gs, vh, inside_b=None, use_a=None, use_b=None):
    cells_a, cells_b = np.asarray(cells_a, np.int32).reshape(-1, 3), np.asarray(cells_b, np.int32).reshape(-1, 3)
    w_a, w_b = np.asarray(w_a, np.float32), np.asarray(w_b, np.float32)
    want = R.ref_fuse_plan(cells_a, w_a, cells_b, w_b, gs, vh, inside_b, use_a, use_b)
    assert want["error"] == 0
    got = ops.fuse_plan(cells_a, w_a, cells_b, w_b, gs, vh, inside_b=inside_b, use_a=use_a, use_b=use_b)
    assert got.n_out == want["n_out"]
    for name in ("a_row", "b_start", "b_rows", "out_of_a", "out_of_b", "counts"):
        assert same_bytes(getattr(got, name), want[name]), (name, getattr(got, name), want[name])
    c = got.counts
    assert c[1:].sum() == len(cells_b) and c[0] + got.n_sel_a == len(cells_a) and got.n_out == got.n_sel_a + c[4]
    assert got.n_sel_b == len(cells_b) - c[1] - c[2] == len(got.b_rows) == c[3] + c[4] + c[5]
    return got


def ones(n):
    return np.ones(n, np.float32)


def test_plan_empty_sides(ops):
    a = [(1, 1, 1), (2, 2, 2), (0, 0, 0)]
    assert check_plan(ops, a, ones(3), np.zeros((0, 3)), ones(0), 8, 5).a_row.tolist() == [0, 1, 2]
    p = check_plan(ops, np.zeros((0, 3)), ones(0), a, ones(3), 8, 5)
    assert p.a_row.tolist() == [-1, -1, -1] and p.out_of_b.tolist() == [0, 1, 2]
    assert check_plan(ops, np.zeros((0, 3)), ones(0), np.zeros((0, 3)), ones(0), 8, 5).n_out == 0


def test_plan_b_inside_a_b_new_and_three_rows_in_one_new_cell(ops):
    a = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (7, 7, 4)]
    p = check_plan(ops, a, ones(4), [(3, 3, 3), (1, 1, 1), (3, 3, 3)], ones(3), 8, 5)
    assert p.n_out == 4 and p.out_of_b.tolist() == [2, 0, 2] and p.counts.tolist() == [0, 0, 0, 3, 0, 0]
    p = check_plan(ops, a, ones(4), [(0, 0, 0), (5, 5, 0)], ones(2), 8, 5)
    assert p.n_out == 6 and p.a_row.tolist() == [0, 1, 2, 3, -1, -1] and p.counts.tolist() == [0, 0, 0, 0, 2, 0]
    # the first row of a new cell decides its number: (6, 6, 1) is met at row 1, (0, 1, 0) at row 0
    p = check_plan(ops, a, ones(4), [(0, 1, 0), (6, 6, 1), (2, 2, 2), (6, 6, 1), (0, 1, 0), (6, 6, 1)], ones(6), 8, 5)
    assert p.out_of_b.tolist() == [4, 5, 1, 5, 4, 5] and p.b_rows.tolist() == [2, 0, 4, 1, 3, 5] and p.b_start.tolist() == [0, 0, 1, 1, 1, 3, 6]
    assert p.counts.tolist() == [0, 0, 0, 1, 2, 3]


def test_plan_masks_weights_and_rows_outside(ops):
    a = [(1, 1, 1), (2, 2, 2), (3, 3, 3)]
    # A's row 1 is masked out and B refills its cell: the voxel moves to the tail
    p = check_plan(ops, a, ones(3), [(2, 2, 2), (3, 3, 3)], ones(2), 8, 5, use_a=np.array([1, 0, 1], bool))
    assert p.a_row.tolist() == [0, 2, -1] and p.out_of_a.tolist() == [0, -1, 1] and p.out_of_b.tolist() == [2, 1]
    # weights 0, NaN, -1 and inf unselect a row on either side; an unselected row of A may lie outside the grid or share a cell
    wa = np.array([1, 0, np.nan, -1, np.inf, 2], np.float32)
    p = check_plan(ops, a + [(1, 1, 1), (9, 9, 9), (0, 0, 0)], wa, [(1, 1, 1)] * 5, np.array([0, np.nan, -1, np.inf, 3], np.float32), 8, 5)
    assert p.out_of_a.tolist() == [0, -1, -1, -1, -1, 1] and p.out_of_b.tolist() == [-1, -1, -1, -1, 0] and p.counts.tolist() == [4, 4, 0, 1, 0, 0]
    # outside: by move_cells' flag, and by the cell itself
    b = [(1, 1, 1), (8, 0, 0), (0, 0, 5), (-1, -1, -1), (4, 4, 4)]
    p = check_plan(ops, a, ones(3), b, ones(5), 8, 5, inside_b=np.array([1, 1, 1, 0, 0], np.uint8), use_b=np.array([1, 1, 0, 1, 1], bool))
    assert p.out_of_b.tolist() == [0, -1, -1, -1, -1] and p.counts.tolist() == [0, 1, 3, 1, 0, 0]


def test_plan_two_selected_rows_of_a_in_one_cell_or_one_outside_raise(ops):
    with pytest.raises(ValueError, match="share a cell"):
        ops.fuse_plan(np.array([(1, 1, 1), (2, 2, 2), (1, 1, 1)], np.int32), ones(3), np.zeros((0, 3), np.int32), ones(0), 8, 5)
    with pytest.raises(ValueError, match="outside"):
        ops.fuse_plan(np.array([(1, 1, 1), (8, 2, 2)], np.int32), ones(2), np.zeros((0, 3), np.int32), ones(0), 8, 5)


def test_plan_random_under_a_rotation_and_more_than_one_scan_block(ops):
    rng = np.random.default_rng(3)
    every = all_cells(33, 31)
    cells_a, cells_b = every[rng.choice(len(every), 300, replace=False)], every[rng.choice(len(every), 300, replace=False)]
    cells_b[:40] = cells_a[100:140]
    moved, inside = ops.move_cells(cells_b, 33, 0.05, 31, transform=rot_z(10.0, (0.013, -0.02, 0.0)))
    w = rng.uniform(0.0, 3.0, (2, 300)).astype(np.float32)
    w[:, ::17] = 0
    p = check_plan(ops, cells_a, w[0], moved, w[1], 33, 31, inside_b=inside, use_a=rng.random(300) < 0.9, use_b=rng.random(300) < 0.9)
    assert p.counts[2] > 0 and p.counts[4] > 0
    # 2500 and 3000 rows: more than one block of the scans (1024 rows each), rows of B piled up in few cells
    cells_a = every[rng.choice(len(every), 2500, replace=False)]
    cells_b = np.concatenate([cells_a[rng.integers(0, 2500, 1500)], every[rng.integers(0, 400, 1500)]])[rng.permutation(3000)]
    p = check_plan(ops, cells_a, ones(2500), cells_b, ones(3000), 33, 31)
    assert p.counts[3] >= 1500 and p.counts[5] > 0


# ------------------------------------------------------------------ fuse_rows
GS, VH = 8, 5
N_A, N_B = 40, 150


@functools.lru_cache(maxsize=None)
def rows_plan_inputs():
    """40 rows of A; of B, rows 0 .. 39 fall into A's cells 0 .. 19 twice over (members 3), rows 40 .. 49 into A's cells 20 .. 29
    (members 2), rows 50 .. 59 into new cells of their own (sole members, like A's rows 30 .. 39), rows 60 .. 79 pairwise into ten
    new cells, rows 80 .. 149 into ONE new cell (70 members)"""
    every = all_cells(GS, VH)[np.random.default_rng(1).permutation(GS * GS * VH)]
    cells_a = every[:N_A]
    b = [cells_a[k % 20] for k in range(40)] + [cells_a[20 + k] for k in range(10)] + [every[40 + k] for k in range(10)]
    b += [every[50 + k % 10] for k in range(20)] + [every[60]] * 70
    cells_b = np.asarray(b, np.int32)
    rng = np.random.default_rng(2)
    w_a, w_b = rng.uniform(0.5, 40.0, N_A).astype(np.float32), rng.uniform(0.5, 40.0, N_B).astype(np.float32)
    rgb_a, rgb_b = rng.integers(0, 256, (N_A, 3)).astype(np.uint8), rng.integers(0, 256, (N_B, 3)).astype(np.uint8)
    for x in (cells_a, cells_b, w_a, w_b, rgb_a, rgb_b):
        x.setflags(write=False)
    return cells_a, cells_b, w_a, w_b, rgb_a, rgb_b


@functools.lru_cache(maxsize=None)
def rows_feats(D):
    rng = np.random.default_rng(100 + D)
    feat_a, feat_b = rng.standard_normal((N_A, D)).astype(np.float32), rng.standard_normal((N_B, D)).astype(np.float32)
    special = np.array([-0.0, 1e-45, -3.4e38, np.inf, 0.0, 1.17549435e-38], np.float32)      # sole members: these come back as they are
    feat_a[30:36, 0], feat_b[50:56, D - 1] = special, special
    feat_a.setflags(write=False), feat_b.setflags(write=False)
    return feat_a, feat_b


@functools.lru_cache(maxsize=None)
def rows_want(D, gain_b=1.0):
    cells_a, cells_b, w_a, w_b, rgb_a, rgb_b = rows_plan_inputs()
    feat_a, feat_b = rows_feats(D)
    plan = R.ref_fuse_plan(cells_a, w_a, cells_b, w_b, GS, VH)
    return plan, R.ref_fuse_rows(plan, cells_a, feat_a, w_a, rgb_a, cells_b, feat_b, w_b, rgb_b, GS, VH, 1.0, gain_b)


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
    cells_a, cells_b, w_a, w_b, rgb_a, rgb_b = rows_plan_inputs()
    feat_a, feat_b = rows_feats(D)
    ref_plan, want = rows_want(D)
    plan = ops.fuse_plan(cells_a, w_a, cells_b, w_b, GS, VH)
    assert plan.n_out == ref_plan["n_out"] == 61 and np.bincount(1 * (plan.a_row >= 0) + plan.b_count).tolist()[1:4] == [20, 20, 20]
    assert plan.b_count.max() == 70
    got = ops.fuse_rows(plan, feat_a, w_a, rgb_a, feat_b, w_b, rgb_b)
    for g, w, name in zip(got, want, ("grid_pos", "grid_feat", "weight", "grid_rgb", "occupied_ids")):
        assert same_bytes(g, w), (D, name)
    # sole members come back bit for bit: A's rows 30 .. 39 and B's rows 50 .. 59
    assert same_bytes(got[1][30:40], feat_a[30:40]) and same_bytes(got[2][30:40], w_a[30:40]) and same_bytes(got[3][30:40], rgb_a[30:40])
    sole_b = plan.out_of_b[50:60]
    assert same_bytes(got[1][sole_b], feat_b[50:60]) and same_bytes(got[2][sole_b], w_b[50:60]) and same_bytes(got[3][sole_b], rgb_b[50:60])
    # every matrix one float past a 16-byte boundary, the output too: the scalar path, the same bytes
    keep_a, view_a = off_by_one_float(ops, feat_a)
    keep_b, view_b = off_by_one_float(ops, feat_b)
    keep_o, view_o = off_by_one_float(ops, np.zeros((plan.n_out, D), np.float32))
    again = ops.fuse_rows(plan, view_a, w_a, rgb_a, view_b, w_b, rgb_b, feat_out=view_o, want_occupied=False)
    assert again[4] is None and again[1] is view_o
    back = np.empty((plan.n_out, D), np.float32)
    _lib.check(_lib.load().avl_memcpy_d2h(back.ctypes.data, view_o.ptr, back.nbytes, None), "avl_memcpy_d2h")
    assert same_bytes(back, want[1]) and same_bytes(again[2], want[2]) and same_bytes(again[3], want[3]) and same_bytes(again[0], want[0])
    # one side aligned, the other not
    mixed = ops.fuse_rows(plan, feat_a, w_a, rgb_a, view_b, w_b, rgb_b, want_occupied=False)
    assert same_bytes(mixed[1], want[1])


def test_rows_a_view_that_is_not_contiguous_and_a_gain(ops):
    cells_a, cells_b, w_a, w_b, rgb_a, rgb_b = rows_plan_inputs()
    feat_a, feat_b = rows_feats(512)
    plan = ops.fuse_plan(cells_a, w_a, cells_b, w_b, GS, VH)
    wide_a, wide_b = np.zeros((N_A, 1024), np.float32), np.zeros((2 * N_B, 512), np.float32)
    wide_a[:, 1::2], wide_b[::2] = feat_a, feat_b
    got = ops.fuse_rows(plan, wide_a[:, 1::2], w_a, rgb_a, wide_b[::2], w_b, rgb_b)
    assert same_bytes(got[1], rows_want(512)[1][1])
    want = rows_want(512, 0.25)[1]
    got = ops.fuse_rows(plan, feat_a, w_a, rgb_a, feat_b, w_b, rgb_b, gain_b=0.25)
    for g, w in zip(got, want):
        assert same_bytes(g, w)
    assert not same_bytes(want[1], rows_want(512)[1][1])


def test_rows_rgb_truncates_at_a_quotient_just_below_a_whole_number(ops):
    cells = np.array([(1, 1, 1)], np.int32)
    w_a, w_b = np.array([1], np.float32), np.array([999], np.float32)
    rgb_a, rgb_b = np.array([(0, 10, 255)], np.uint8), np.array([(1, 11, 254)], np.uint8)
    feat = np.ones((1, 4), np.float32)
    plan = ops.fuse_plan(cells, w_a, cells, w_b, GS, VH)
    got = ops.fuse_rows(plan, feat, w_a, rgb_a, feat, w_b, rgb_b)
    ref_plan = R.ref_fuse_plan(cells, w_a, cells, w_b, GS, VH)
    want = R.ref_fuse_rows(ref_plan, cells, feat, w_a, rgb_a, cells, feat, w_b, rgb_b, GS, VH)
    assert got[3].tolist() == [[0, 10, 254]] and same_bytes(got[3], want[3]) and got[2].tolist() == [1000.0]


# ------------------------------------------------------------------ fuse_maps and the map layer
MGS, MVH, MD, MCS = 24, 8, 128, 0.1


def map_arrays(seed, cells):
    rng = np.random.default_rng(seed)
    n = len(cells)
    return (np.asarray(cells, np.int32).reshape(-1, 3), rng.standard_normal((n, MD)).astype(np.float32), rng.uniform(1, 30, n).astype(np.float32),
            rng.integers(0, 256, (n, 3)).astype(np.uint8))


def make_vlmap(arrays, scores=None):
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
    vm.scores_mat = scores
    return vm


def box(r0, r1, c0, c1, h0, h1):
    return [(r, c, h) for r in range(r0, r1 + 1) for c in range(c0, c1 + 1) for h in range(h0, h1 + 1)]


def test_fuse_maps_with_an_empty_b_returns_a_and_resample_returns_the_map(ops):
    a = map_arrays(1, np.random.default_rng(0).permutation(np.asarray(box(2, 9, 3, 12, 0, 7)))[:300])
    empty = (np.zeros((0, 3), np.int32), np.zeros((0, MD), np.float32), np.zeros(0, np.float32), np.zeros((0, 3), np.uint8))
    got = ops.fuse_maps(*a, *empty, MGS, MCS, MVH)
    vm = make_vlmap(a)
    for g, w in zip((got.grid_pos, got.grid_feat, got.weight, got.grid_rgb, got.occupied_ids), a + (vm.occupied_ids,)):
        assert same_bytes(g, w)
    assert got.a_row.tolist() == list(range(300)) and not got.b_count.any() and sum(got.counts.values()) == 0
    on_device = ops.fuse_maps(*a, *empty, MGS, MCS, MVH, want_occupied=False, device=True)
    assert on_device.occupied_ids is None and same_bytes(on_device.grid_feat.numpy(), a[1])
    same = vm.resample()
    assert same is not vm and type(same) is type(vm) and same.mapped_iter_list == [0, 1, 2] and same.scores_mat is None
    for name in ("grid_pos", "grid_feat", "weight", "grid_rgb", "occupied_ids"):
        assert same_bytes(getattr(same, name), getattr(vm, name)), name
    # a rotated copy compares against the original: the limit of the comparison is gone
    turned = vm.resample(rot_z(2.0, (0.013, -0.02, 0.0)))
    assert 0 < len(turned.grid_pos) <= 300 and vm.compare(turned, radius=1).summary()["voxels_b"] == len(turned.grid_pos)


def test_fuse_in_place_equals_the_restatement_and_drops_the_caches(ops):
    from avlmaps_amd.apps.common import HashClip
    cells = np.random.default_rng(5).permutation(np.asarray(box(2, 12, 2, 12, 0, 7)))
    a, b = map_arrays(2, cells[:400]), map_arrays(3, cells[250:700])                    # 150 cells in common
    vm, other = make_vlmap(a, scores=np.zeros((400, 3), np.float32)), make_vlmap(b)
    q = np.random.default_rng(7).standard_normal((5, MD)).astype(np.float32)
    before = vm.index_queries(q)                                                        # makes the resident copy that fusing has to drop
    shift = (1, 0, -1)                                                                  # compare's meaning: A's c is B's c + shift
    counts = vm.fuse(other, shift=shift, gain=2.0)
    moved, inside = R.ref_move_cells(b[0], MGS, MCS, MVH, None, tuple(-s for s in shift))
    plan = R.ref_fuse_plan(a[0], a[2], moved, b[2], MGS, MVH, inside)
    want = R.ref_fuse_rows(plan, a[0], a[1], a[2], a[3], moved, b[1], b[2], b[3], MGS, MVH, 1.0, 2.0)
    for name, w in zip(("grid_pos", "grid_feat", "weight", "grid_rgb", "occupied_ids"), want):
        assert same_bytes(getattr(vm, name), w), name
    assert counts["voxels"] == plan["n_out"] == len(vm.grid_pos) and counts["merged_b"] == plan["counts"][3] > 0 and counts["outside_b"] > 0
    assert vm.scores_mat is None and vm.mapped_iter_list == [0, 1, 2] and len(before) == 400
    fresh = make_vlmap(want[:4])
    am, sc = vm.index_queries(q, want_scores=True)
    am_fresh, sc_fresh = fresh.index_queries(q, want_scores=True)
    assert len(am) == plan["n_out"] and np.array_equal(am, am_fresh) and np.array_equal(sc, sc_fresh)
    for m in (vm, fresh):
        m.clip_feat_dim, m.clip_model = MD, HashClip(MD)
    assert np.array_equal(vm.index_map("chair", with_init_cat=False), fresh.index_map("chair", with_init_cat=False))
    with pytest.raises(ValueError):
        vm.fuse(make_vlmap((b[0], np.zeros((450, MD + 1), np.float32), b[2], b[3])))


def test_fuse_with_changes_drops_a_vanished_block_and_replaces_a_changed_one(ops):
    rng = np.random.default_rng(11)
    base = {k: rng.standard_normal(MD) for k in ("wall", "x", "y", "y2", "z")}
    base["y2"] = -base["y"]
    wall, bx, by, bz = [(2, c, h) for c in range(2, 22) for h in range(1, 6)], box(8, 10, 8, 10, 2, 4), box(15, 17, 5, 7, 1, 2), box(15, 17, 15, 17, 3, 6)

    def part(cells, kind, seed):
        pos, feat, weight, rgb = map_arrays(seed, cells)
        return pos, (base[kind][None, :] + 0.05 * feat).astype(np.float32), weight, rgb

    def join(parts):
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
    a = join([part(wall, "wall", 1), part(bx, "x", 2), part(by, "y", 3)])                # B: X gone, Y replaced, Z new
    b = join([part(wall, "wall", 4), part(by, "y2", 5), part(bz, "z", 6)])
    vm, other = make_vlmap(a), make_vlmap(b)
    changes = vm.compare(other, radius=0)
    nw, nx, ny, nz = len(wall), len(bx), len(by), len(bz)
    assert changes.vanished.sum() == nx and changes.changed_a.sum() == ny == changes.changed.sum() and changes.appeared.sum() == nz
    with pytest.raises(ValueError):
        vm.fuse(other, changes=changes, transform=np.eye(4))
    with pytest.raises(ValueError):
        vm.fuse(other, changes=changes, shift=(1, 0, 0))
    kept = make_vlmap(a)
    kept_counts = kept.fuse(other, changes=changes, drop_vanished=False, replace_changed=False)
    assert kept_counts["voxels"] == nw + nx + ny + nz and kept_counts["dropped_a"] == 0
    counts = vm.fuse(other, changes=changes)
    assert counts["dropped_a"] == nx + ny and counts["merged_b"] == nw and counts["new_cells"] == ny + nz and counts["voxels"] == nw + ny + nz
    use_a = ~(changes.vanished | changes.changed_a)
    plan = R.ref_fuse_plan(a[0], a[2], b[0], b[2], MGS, MVH, None, use_a, None)
    want = R.ref_fuse_rows(plan, a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], MGS, MVH)
    for name, w in zip(("grid_pos", "grid_feat", "weight", "grid_rgb", "occupied_ids"), want):
        assert same_bytes(getattr(vm, name), w), name
    # X's cells are empty, Y's cells hold B's rows as they were
    assert (vm.occupied_ids[tuple(np.asarray(bx).T)] == -1).all()
    rows_y = vm.occupied_ids[tuple(b[0][nw:nw + ny].T)]
    assert (rows_y >= nw).all() and same_bytes(vm.grid_feat[rows_y], b[1][nw:nw + ny]) and same_bytes(vm.weight[rows_y], b[2][nw:nw + ny])


# ------------------------------------------------------------------ the app
from test_audit_gpu import _config, _config_file, EG, EVH, visit  # noqa: E402,F401  (the rendered scene of the audit's end-to-end test)


def test_the_app_fuses_a_later_map_and_writes_over_neither_input(ops, visit, tmp_path):
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
    # the later map: a fifth of A's voxels gone, every third of the rest replaced by its negative, ten voxels in free cells
    keep = np.arange(n) % 5 != 0
    free = np.argwhere(a.occupied_ids < 0)[::97][:10].astype(np.int32)
    feat_b = a.grid_feat[keep].copy()
    feat_b[::3] *= -1
    pos_b = np.concatenate([pos[keep], free])
    feat_b = np.concatenate([feat_b, rng.standard_normal((len(free), feat_b.shape[1])).astype(np.float32)])
    occupied = -np.ones((EG, EG, EVH), np.int32)
    occupied[tuple(pos_b.T)] = np.arange(len(pos_b))
    (root / "b" / "vlmap").mkdir(exist_ok=True)
    save_3d_map(root / "b" / "vlmap" / "vlmaps.h5df", feat_b, pos_b, np.full(len(pos_b), 2.0, np.float32), occupied, [0, 1, 2, 3],
                rng.integers(0, 255, (len(pos_b), 3)).astype(np.uint8))
    res = audit_map.main(["--data-dir", str(root / "a"), "--fuse", str(root / "b"), "--fuse-out", str(tmp_path / "both"), "--stride", "1",
                          "--compare-radius", "0", "--fuse-gain", "2", "--fuse-json", str(tmp_path / "fuse.json"), "--config", _config_file(tmp_path)])
    # the same steps through the map layer
    b = load(root / "b")
    T = a.transform_from(root / "b")
    assert np.abs(T - np.eye(4)).max() <= 1e-12                               # both recordings start at one pose
    moved = b.resample(T)
    changes = a.compare(moved, radius=0)
    assert changes.vanished.sum() == n - keep.sum() and changes.appeared.sum() == len(free) and changes.changed.sum() == len(feat_b[:keep.sum():3])
    counts = a.fuse(moved, changes=changes, gain=2.0)
    assert res["fuse"]["counts"] == counts and res["fuse"]["summary"] == changes.summary() and counts["voxels"] == len(pos_b)
    fused = load(tmp_path / "both")
    for name in ("grid_pos", "grid_feat", "weight", "grid_rgb", "occupied_ids"):
        assert same_bytes(np.asarray(getattr(fused, name)), np.asarray(getattr(a, name))), name
    assert (tmp_path / "fuse.json").exists() and str(tmp_path / "both" / "vlmap" / "vlmaps.h5df") in res["files"]
    assert len(load(root / "a").grid_pos) == n and same_bytes(np.asarray(load(root / "b").grid_feat), feat_b)
