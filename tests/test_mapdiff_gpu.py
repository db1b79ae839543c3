"""The map comparison on the GPU (csrc/avl_mapdiff.hip through ops.match_cells, ops.row_dots, ops.diff_status, ops.map_diff,
VLMap.compare, MapChanges.objects and AVLMap.index_changes) against the restatements of tests/_mapdiff_ref.py.

Every comparison is np.array_equal: the join is integer, the sums are float64 additions in a pinned order (compared as bytes), the
status is a float64 predicate in a pinned grouping."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
import _mapdiff_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ match_cells
def check_match(ops, pos_b, cells_a, gs, vh, shift=(0, 0, 0)):
    pos_b, cells_a = np.asarray(pos_b, np.int32).reshape(-1, 3), np.asarray(cells_a, np.int32).reshape(-1, 3)
    out = {}
    with ops.cell_index(pos_b, gs, vh) as index:
        for r in (0, 1, 2):
            want = R.ref_match_cells(pos_b, cells_a, gs, vh, r, shift)
            got = ops.match_cells(index, cells_a, radius=r, shift=shift)
            assert got[0].dtype == np.int32 and got[1].dtype == np.int32
            assert np.array_equal(got[0], want[0]), (r, got[0], want[0])
            assert np.array_equal(got[1], want[1]), (r, got[1], want[1])
            out[r] = got
    return out


def test_match_cells_at_the_corners_of_the_grid_probes_leave_the_grid(ops):
    gs, vh = 8, 5
    corners = [(r, c, h) for r in (0, gs - 1) for c in (0, gs - 1) for h in (0, vh - 1)]
    # B: cells one and two steps inside every corner, so that every corner voxel of A looks outside the grid on three sides
    pos_b = [(min(max(r + dr, 1), gs - 2), min(max(c + dc, 1), gs - 2), min(max(h, 1), vh - 2)) for r, c, h in corners for dr in (0,) for dc in (0,)]
    pos_b += [(0, 3, 0), (gs - 1, 4, vh - 1), (3, 0, vh - 1), (4, gs - 1, 0)]
    cells_a = corners + [(0, 4, 0), (gs - 1, 3, vh - 1), (1, 1, 1), (0, 0, 2)]
    got = check_match(ops, pos_b, cells_a, gs, vh)
    assert (got[0][0][:8] == -1).all() and (got[1][0][:8] >= 0).all() and (got[1][1][:8] == 3).all()


def test_match_cells_two_rows_in_one_cell_the_largest_row_owns_it(ops):
    pos_b = [(2, 2, 2), (5, 5, 1), (2, 2, 2), (9, 9, 9)]            # rows 0 and 2 share a cell; row 3 lies outside the grid
    got = check_match(ops, pos_b, [(2, 2, 2), (2, 3, 2), (7, 7, 4), (5, 5, 1)], 8, 5)
    assert got[0][0].tolist() == [2, -1, -1, 1] and got[1][0].tolist() == [2, 2, -1, 1] and got[1][1].tolist() == [0, 1, -1, 0]


def test_match_cells_ties_of_equal_distance_go_to_the_smaller_linear_cell(ops):
    # neighbours on both sides of the voxel along every axis, and diagonal ones: the winner is the smallest linear cell at the least d2
    centre = (4, 4, 2)
    for axis in range(3):
        lo, hi = list(centre), list(centre)
        lo[axis] -= 1
        hi[axis] += 1
        got = check_match(ops, [tuple(hi), tuple(lo)], [centre], 8, 5)
        assert got[1][0].tolist() == [1] and got[1][1].tolist() == [1]
        lo[axis] -= 1
        hi[axis] += 1
        got = check_match(ops, [tuple(hi), tuple(lo)], [centre], 8, 5)
        assert got[1][0].tolist() == [-1] and got[2][0].tolist() == [1] and got[2][1].tolist() == [4]
    check_match(ops, [(5, 5, 3), (3, 3, 1), (5, 3, 1), (3, 5, 3), (4, 5, 3), (4, 3, 1)], [centre], 8, 5)
    check_match(ops, [(6, 4, 2), (4, 6, 2), (4, 4, 4), (4, 4, 0), (4, 2, 2), (2, 4, 2), (5, 5, 3)], [centre], 8, 5)


def test_match_cells_a_shift_pushes_rows_out_of_the_grid(ops):
    pos_b = [(r, c, h) for r in range(8) for c in (0, 7) for h in (0, 4)]
    cells_a = [(0, 0, 0), (7, 7, 4), (3, 0, 0), (6, 7, 4), (1, 1, 1), (7, 0, 0)]
    for shift in ((2, 0, 0), (-2, 0, 0), (0, 1, 0), (0, 0, -1), (1, -1, 1), (100000, 0, 0), (0, 0, -2 ** 31 + 1)):
        check_match(ops, pos_b, cells_a, 8, 5, shift)
    got = check_match(ops, pos_b, cells_a, 8, 5, (2, 0, 0))
    assert got[2][0][[1, 3, 5]].tolist() == [-1, -1, -1] and got[2][0][0] >= 0


def test_match_cells_empty_sides_and_more_than_one_wave(ops):
    rng = np.random.default_rng(5)
    pos_b = np.stack([rng.integers(0, 8, 40), rng.integers(0, 8, 40), rng.integers(0, 5, 40)], axis=1)
    for n in (0, 1, 65):
        cells = np.stack([rng.integers(-1, 9, n), rng.integers(-1, 9, n), rng.integers(-1, 6, n)], axis=1).reshape(n, 3)
        got = check_match(ops, pos_b, cells, 8, 5)
        assert got[1][0].shape == (n,)
        got = check_match(ops, np.zeros((0, 3), np.int32), cells, 8, 5)                # N_b = 0: nothing matches
        assert (got[2][0] == -1).all() and (got[2][1] == -1).all()


def test_match_cells_random_odd_grid(ops):
    rng = np.random.default_rng(11)
    gs, vh = 33, 31
    def cells(n):
        return np.stack([rng.integers(-1, gs + 1, n), rng.integers(-1, gs + 1, n), rng.integers(-1, vh + 1, n)], axis=1)
    pos_b, cells_a = cells(300), cells(300)
    cells_a[:60] = pos_b[:60] + rng.integers(-2, 3, (60, 3))                           # near misses, so that every radius finds some
    cells_a[60:80] = pos_b[60:80]                                                      # and exact hits
    got = check_match(ops, pos_b, cells_a, gs, vh)
    assert (got[2][1] > 0).sum() > 20 and (got[0][0] >= 0).sum() > 5
    check_match(ops, pos_b, cells_a, gs, vh, (1, -2, 1))


# ------------------------------------------------------------------ row_dots
DIMS = (1, 3, 4, 63, 64, 65, 255, 256, 257, 512, 1028, 1537)


@functools.lru_cache(maxsize=None)
def dots_case(D, n_a, n_b=37, seed=0):
    """seeded float32 rows with the edge cases planted where n_a allows: magnitudes 1e-15 and 1e+15, a zero row, a row equal to its
    partner, a negative dot, some unmatched rows"""
    rng = np.random.default_rng(seed + 1000 * D + n_a)
    a = rng.standard_normal((n_a, D)).astype(np.float32)
    b = rng.standard_normal((n_b, D)).astype(np.float32)
    match = rng.integers(0, n_b, n_a).astype(np.int32)
    b[1] *= np.float32(1e15)
    b[2] *= np.float32(1e-15)
    b[3] = 0
    a[0] = b[match[0]]                                   # ab == aa == bb
    if n_a > 8:
        a[1] = -b[match[1]]                              # a negative dot
        a[2] *= np.float32(1e15)
        a[3] *= np.float32(1e-15)
        a[4] = 0
        match[2:5] = (2, 1, 3)                           # large against small, small against large, zero against zero
        match[5] = 1
        match[6] = 3
        match[7::9] = -1
        match[-1] = n_b - 1
    for x in (a, b, match):
        x.setflags(write=False)
    return a, b, match, R.ref_row_dots(a, b, match)


@pytest.mark.parametrize("D", DIMS)
def test_row_dots_equal_the_restatement_bit_for_bit(ops, D):
    for n_a in (1, 64, 65, 257):
        a, b, match, want = dots_case(D, n_a)
        got = ops.row_dots(a, b, match)
        assert got.dtype == np.float64 and got.shape == (n_a, 3)
        bad = np.flatnonzero((got.view(np.int64) != want.view(np.int64)).any(axis=1))
        assert bad.size == 0, (D, n_a, bad[:5], got[bad[:5]], want[bad[:5]])
        assert (got[match < 0] == 0).all()
    a, b, match, want = dots_case(D, 257)
    assert same_bytes(got[0], np.array([want[0, 0]] * 3))                              # a row equal to its partner: one value three times
    perm = np.random.default_rng(D).permutation(257)                                   # the rows of A permuted together with match
    assert same_bytes(ops.row_dots(a[perm], b, match[perm]), want[perm])


@pytest.mark.parametrize("D", (4, 64, 256, 512, 1028))
def test_row_dots_do_not_depend_on_the_load_path(ops, D):
    """feat_a one float off 16-byte alignment with D % 4 == 0 takes the scalar loads, feat_b the 16-byte ones, and the other way round"""
    from avlmaps_amd.device import DeviceArray, DeviceView
    a, b, match, want = dots_case(D, 65)
    for shift_a, shift_b in ((1, 0), (0, 1), (1, 1), (2, 3)):
        ha, hb = np.zeros(65 * D + 4, np.float32), np.zeros(37 * D + 4, np.float32)
        ha[shift_a:shift_a + 65 * D], hb[shift_b:shift_b + 37 * D] = a.ravel(), b.ravel()
        da, db = DeviceArray.from_numpy(ha), DeviceArray.from_numpy(hb)
        va, vb = DeviceView(da.ptr + 4 * shift_a, (65, D), np.float32), DeviceView(db.ptr + 4 * shift_b, (37, D), np.float32)
        assert (va.ptr % 16 != 0) == (shift_a != 0) and (vb.ptr % 16 != 0) == (shift_b != 0)
        got = ops.row_dots(va, vb, match)
        assert same_bytes(got, want), (D, shift_a, shift_b)
        da.free()
        db.free()


def test_row_dots_streams_a_host_matrix_in_pieces(ops, monkeypatch):
    from avlmaps_amd.ops import mapdiff
    a, b, match, want = dots_case(65, 257)
    monkeypatch.setattr(mapdiff, "DIFF_STREAM_ROWS", 100)
    assert same_bytes(ops.row_dots(a, b, match), want)
    sums = ops.row_dots(a, b, match, device=True)
    assert same_bytes(sums.numpy(), want)
    assert ops.row_dots(np.zeros((0, 8), np.float32), b[:, :8], np.zeros(0, np.int32)).shape == (0, 3)


# ------------------------------------------------------------------ diff_status
def test_diff_status_every_branch_and_the_counts(ops):
    x = np.float64(3.0)
    rows = [
        (0, (x, x, x)),                      # a == b: ab * ab == 1 * (aa * bb) exactly -> SAME at threshold 1
        (0, (np.nextafter(x, 0), x, x)),     # just below -> CHANGED at threshold 1
        (1, (-x, x, x)),                     # opposite rows: ab * ab passes, ab > 0 does not
        (2, (0.0, 0.0, x)),                  # a zero row of A
        (3, (0.0, x, 0.0)),                  # a zero row of B
        (4, (0.0, x, x)),                    # orthogonal rows
        (-1, (0.0, 0.0, 0.0)),
        (-1, (0.0, 0.0, 0.0)),
        (-1, (0.0, 0.0, 0.0)),
        (5, (1e300, 1e300, 1e300)),          # aa * bb overflows to inf, and so does ab * ab: inf >= inf
        (6, (np.nan, x, x)),
        (7, (0.8, 1.0, 1.0)),                # cosine 0.8 exactly
        (8, (np.nextafter(0.8, 0), 1.0, 1.0)),
    ]
    match = np.array([m for m, _ in rows], np.int32)
    sums = np.array([s for _, s in rows], np.float64)
    through = np.array([0] * 6 + [2, 3, 4] + [0] * 4, np.int32)
    for threshold in (1.0, 0.8, 0.5, 1e-3):
        for th, min_rays in ((None, 3), (through, 3), (through, 4), (through.astype(np.uint32), 1)):
            want = R.ref_status(match, sums, threshold, th, min_rays)
            status, counts = ops.diff_status(match, sums, threshold, th, min_rays)
            assert status.dtype == np.uint8 and counts.dtype == np.int32 and counts.shape == (4,)
            assert np.array_equal(status, want[0]), (threshold, min_rays, status, want[0])
            assert np.array_equal(counts, np.bincount(status, minlength=4)) and np.array_equal(counts, want[1])
    status, _ = ops.diff_status(match, sums, 1.0, through, 3)
    assert status.tolist() == [0, 1, 1, 1, 1, 1, 3, 2, 2, 0, 1, 1, 1]
    # more than one block, and nothing at all
    rng = np.random.default_rng(2)
    n = 3000
    match = rng.integers(-1, 50, n).astype(np.int32)
    sums = np.abs(rng.standard_normal((n, 3)))
    sums[:, 0] *= rng.choice([-1.0, 1.0, 1.0], n)
    through = rng.integers(0, 6, n).astype(np.int32)
    want = R.ref_status(match, sums, 0.7, through, 3)
    status, counts = ops.diff_status(match, sums, 0.7, through, 3)
    assert np.array_equal(status, want[0]) and np.array_equal(counts, want[1]) and counts.sum() == n and (counts > 0).all()
    status, counts = ops.diff_status(np.zeros(0, np.int32), np.zeros((0, 3)), 0.7)
    assert status.shape == (0,) and counts.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------ map_diff and the map layer
GS, VH, D, CS = 24, 8, 16, 0.1
NAMES = ["wall", "chair", "plant"]
BOX_X, BOX_Y, BOX_Z, BOX_M = (8, 10, 8, 10, 2, 4), (15, 17, 5, 7, 1, 2), (15, 17, 15, 17, 3, 6), (19, 21, 10, 12, 2, 4)


def _box_cells(box):
    r0, r1, c0, c1, h0, h1 = box
    return [(r, c, h) for r in range(r0, r1 + 1) for c in range(c0, c1 + 1) for h in range(h0, h1 + 1)]


@functools.lru_cache(maxsize=None)
def scene():
    """Map A: a wall (row 2, cols 2 .. 21, heights 1 .. 5) and the blocks X and Y, every object with one base feature row plus a
    little noise per voxel.  Map B: A with X deleted, Z added, Y's rows replaced by another object's, and the wall's cols 2 .. 11
    moved one cell to row 3.  Map C: A with X deleted and an equal block of the same category at BOX_M.  Blocks keep three cells
    of air to everything else, so that no radius <= 2 joins them to a neighbour."""
    rng = np.random.default_rng(7)
    base = {k: rng.standard_normal(D) for k in ("wall", "x", "y", "y2", "z")}
    base["y2"] = -base["y"] + 0.3 * base["y2"]

    def rows(cells, kind, cat):
        feat = (base[kind][None, :] + 0.05 * rng.standard_normal((len(cells), D))).astype(np.float32)
        scores = np.full((len(cells), len(NAMES)), 0.1, np.float32)
        scores[:, cat] = 0.9
        return np.asarray(cells, np.int32).reshape(-1, 3), feat, scores

    wall = [(2, c, h) for c in range(2, 22) for h in range(1, 6)]
    a_parts = [rows(wall, "wall", 0), rows(_box_cells(BOX_X), "x", 1), rows(_box_cells(BOX_Y), "y", 1)]
    wall_b = [(3, c, h) if c <= 11 else (2, c, h) for (_, c, h) in wall]
    pw, fw, sw = a_parts[0]
    b_parts = [(np.asarray(wall_b, np.int32), fw.copy(), sw.copy()), rows(_box_cells(BOX_Y), "y2", 2), rows(_box_cells(BOX_Z), "z", 2)]
    xm = rows(_box_cells(BOX_M), "x", 1)
    c_parts = [a_parts[0], a_parts[2], xm]
    maps = {}
    for name, parts in (("a", a_parts), ("b", b_parts), ("c", c_parts)):
        pos, feat, scores = (np.concatenate([p[k] for p in parts]) for k in range(3))
        perm = np.random.default_rng(len(pos)).permutation(len(pos))                   # a voxel list in no particular order
        maps[name] = tuple(np.ascontiguousarray(x[perm]) for x in (pos, feat, scores))
        for x in maps[name]:
            x.setflags(write=False)
    return maps


def in_box(pos, box):
    r0, r1, c0, c1, h0, h1 = box
    return (pos[:, 0] >= r0) & (pos[:, 0] <= r1) & (pos[:, 1] >= c0) & (pos[:, 1] <= c1) & (pos[:, 2] >= h0) & (pos[:, 2] <= h1)


def make_avlmap(which):
    from test_host_mirror import Cfg
    from avlmaps_amd.map import AVLMap
    pos, feat, scores = scene()[which]
    cfg = Cfg(map_config=Cfg(map_type="vlmap", grid_size=GS, cell_size=CS,
                             pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                                           base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0])),
              params=Cfg(cs=CS))
    av = AVLMap(cfg)
    vm = av.vlmap
    vm.prefetch_device = False
    vm.grid_pos, vm.grid_feat, vm.scores_mat, vm.categories = pos.copy(), feat.copy(), scores.copy(), list(NAMES)
    vm.occupied_ids = -np.ones((GS, GS, VH), np.int32)
    vm.occupied_ids[tuple(pos.T)] = np.arange(len(pos))
    return av


@pytest.mark.parametrize("radius", (0, 1, 2))
def test_map_diff_both_directions_equal_the_restatement(ops, radius):
    (pa, fa, _), (pb, fb, _) = scene()["a"], scene()["b"]
    rng = np.random.default_rng(radius)
    ta, tb = rng.integers(0, 6, len(pa)).astype(np.int32), rng.integers(0, 6, len(pb)).astype(np.int32)
    for shift, through in (((0, 0, 0), (None, None)), ((0, 0, 0), (ta, tb)), ((1, -1, 0), (ta, None))):
        want = R.ref_map_diff(pa, fa, pb, fb, GS, VH, radius, 0.8, shift, through[0], through[1], 3)
        diff = ops.map_diff(pa, fa, pb, fb, GS, VH, radius=radius, threshold=0.8, shift=shift, through_a=through[0], through_b=through[1])
        for side, ref in zip((diff.a, diff.b), want):
            for name, w in zip(("match", "d2", "sums", "status", "counts"), ref):
                assert same_bytes(getattr(side, name), w), (radius, shift, name)
            cos = side.cosine
            assert cos.dtype == np.float64 and np.array_equal(np.isnan(cos), (ref[0] < 0) | (ref[2][:, 1] <= 0) | (ref[2][:, 2] <= 0))
            ok = ~np.isnan(cos)
            assert np.array_equal(cos[ok], ref[2][ok, 0] / np.sqrt(ref[2][ok, 1] * ref[2][ok, 2]))
    # the jittered part of the wall: vanished and appeared at radius 0, the same wall from radius 1 on
    diff = ops.map_diff(pa, fa, pb, fb, GS, VH, radius=radius)
    wall_a, wall_b = (pa[:, 0] == 2) & (pa[:, 1] <= 11), pb[:, 0] == 3
    assert wall_a.sum() == wall_b.sum() == 50
    if radius == 0:
        assert (diff.a.status[wall_a] == ops.DIFF_NO_MATCH).all() and (diff.b.status[wall_b] == ops.DIFF_NO_MATCH).all()
    else:
        assert (diff.a.status[wall_a] == ops.DIFF_SAME).all() and (diff.b.status[wall_b] == ops.DIFF_SAME).all()
        assert (diff.a.d2[wall_a] == 1).all()
    assert (diff.a.status[in_box(pa, BOX_X)] == ops.DIFF_NO_MATCH).all() and (diff.b.status[in_box(pb, BOX_Z)] == ops.DIFF_NO_MATCH).all()
    assert (diff.a.status[in_box(pa, BOX_Y)] == ops.DIFF_CHANGED).all() and (diff.b.status[in_box(pb, BOX_Y)] == ops.DIFF_CHANGED).all()


def test_map_diff_takes_device_inputs_and_keeps_results_on_the_device(ops):
    from avlmaps_amd.device import DeviceArray
    (pa, fa, _), (pb, fb, _) = scene()["a"], scene()["b"]
    want = R.ref_map_diff(pa, fa, pb, fb, GS, VH, 1, 0.8)
    dev = [DeviceArray.from_numpy(x) for x in (pa, fa, pb, fb)]
    with ops.cell_index(dev[0], GS, VH) as ia, ops.cell_index(dev[2], GS, VH) as ib:
        diff = ops.map_diff(*dev, GS, VH, index_a=ia, index_b=ib, device=True)
        for side, ref in zip((diff.a, diff.b), want):
            for name, w in zip(("match", "d2", "sums", "status", "counts"), ref):
                got = getattr(side, name)
                assert isinstance(got, DeviceArray) and same_bytes(got.numpy(), w), name
        assert np.array_equal(np.isnan(diff.a.cosine), want[0][0] < 0)
        assert ia.buf is not None and ib.buf is not None                               # the caller's indices are not closed
    for d in dev:
        d.free()


def test_compare_finds_the_three_planted_changes_with_their_boxes(ops):
    from avlmaps_amd.map.changes import MapChanges
    a, b = make_avlmap("a").vlmap, make_avlmap("b").vlmap
    ch = a.compare(b, radius=1)
    assert isinstance(ch, MapChanges)
    pa, pb = scene()["a"][0], scene()["b"][0]
    assert np.array_equal(ch.vanished, in_box(pa, BOX_X)) and np.array_equal(ch.appeared, in_box(pb, BOX_Z))
    assert np.array_equal(ch.changed, in_box(pb, BOX_Y)) and np.array_equal(ch.changed_a, in_box(pa, BOX_Y))
    assert not ch.unseen.any() and not ch.unseen_b.any()
    s = ch.summary()
    assert (s["vanished"], s["appeared"], s["changed"], s["voxels_a"], s["voxels_b"]) == (27, 36, 18, 145, 154)
    assert s["changed_volume_m3"] == (27 + 36 + 18) * CS ** 3
    found = ch.objects(min_voxels=4)
    assert [(c.kind, c.count, c.bbox) for c in found] == [("vanished", 27, BOX_X), ("appeared", 36, BOX_Z), ("changed", 18, BOX_Y)]
    assert [c.name for c in found] == ["chair", "plant", "plant"]                      # X was a chair; Z and the new Y are plants: no move
    assert found[0].center == (9.0, 9.0, 3.0) and found[1].center == (16.0, 16.0, 4.5) and found[2].center == (16.0, 6.0, 1.5)
    assert np.isnan(found[0].mean_cosine) and np.isnan(found[1].mean_cosine)
    assert found[2].mean_cosine == np.bincount(np.ones(18, np.int64), weights=ch.cosine_b[ch.changed])[1] / 18.0 and found[2].mean_cosine < 0
    assert [(c.kind, c.bbox) for c in ch.objects(min_voxels=19)] == [("vanished", BOX_X), ("appeared", BOX_Z)]
    assert ch.objects(min_voxels=37) == []
    # at radius 0 the jittered half of the wall vanishes from row 2 and appears in row 3: one category, one size -- a fourth change, moved
    at0 = a.compare(b, radius=0)
    assert at0.summary()["vanished"] == 27 + 50 and at0.summary()["appeared"] == 36 + 50
    kinds = [(c.kind, c.count, c.bbox, c.from_bbox, c.name) for c in at0.objects(min_voxels=4)]
    assert kinds == [("moved", 50, (3, 3, 2, 11, 1, 5), (2, 2, 2, 11, 1, 5), "wall"), ("vanished", 27, BOX_X, None, "chair"),
                     ("appeared", 36, BOX_Z, None, "plant"), ("changed", 18, BOX_Y, None, "plant")]
    # an audit of A under B's frames that never looked at the block tells vanished from unseen
    from avlmaps_amd.map.map import VisibilityAudit
    through = np.full(len(pa), 5, np.uint32)
    through[in_box(pa, BOX_X) & (pa[:, 2] == 4)] = 2
    audit = VisibilityAudit(np.full(len(pa), -1, np.int32), through, dict(gs=GS, cs=CS, vh=VH), [1])
    ch = a.compare(b, radius=1, audit=audit)
    assert np.array_equal(ch.unseen, in_box(pa, BOX_X) & (pa[:, 2] == 4)) and np.array_equal(ch.vanished, in_box(pa, BOX_X) & (pa[:, 2] < 4))
    with pytest.raises(ValueError):
        b.compare(a, audit=audit)                                                      # an audit of another map's voxels


def test_compare_pairs_a_block_of_one_category_into_one_move(ops):
    a, c = make_avlmap("a").vlmap, make_avlmap("c").vlmap
    found = a.compare(c, radius=1).objects(min_voxels=4)
    assert len(found) == 1
    m = found[0]
    assert (m.kind, m.count, m.bbox, m.from_count, m.from_bbox, m.name) == ("moved", 27, BOX_M, 27, BOX_X, "chair")
    assert m.center == (20.0, 11.0, 3.0) and m.from_center == (9.0, 9.0, 3.0)
    c.scores_mat = None                                                                # without scores on both maps nothing is paired
    kinds = [(x.kind, x.bbox, x.category, x.name) for x in a.compare(c, radius=1).objects(min_voxels=4)]
    assert kinds == [("vanished", BOX_X, -1, ""), ("appeared", BOX_M, -1, "")]


def test_index_changes_is_heatmap_from_mask_on_the_same_mask(ops):
    av_a, av_b = make_avlmap("a"), make_avlmap("b")
    ch = av_a.vlmap.compare(av_b.vlmap, radius=1)
    pa, pb = scene()["a"][0], scene()["b"][0]
    heat = av_b.index_changes(ch, decay_rate=0.05)
    want = ops.heatmap_from_mask(pb, in_box(pb, BOX_Z) | in_box(pb, BOX_Y), CS, 0.05)
    assert heat.dtype == np.float32 and same_bytes(heat, want) and (heat[ch.appeared | ch.changed] == 1).all() and (heat < 1).any()
    assert same_bytes(av_a.index_changes(ch, kinds="vanished"), ops.heatmap_from_mask(pa, in_box(pa, BOX_X), CS, 0.1))
    goal = av_b.index_goal(extra=[heat])                                               # "go and look at what changed"
    assert goal.value == 1.0 and goal.voxel == int(np.flatnonzero(ch.appeared | ch.changed)[0])
    for kinds in (("vanished",), ("vanished", "appeared"), ("unseen_b",), ("nothing",)):
        with pytest.raises(ValueError):
            av_b.index_changes(ch, kinds=kinds)
