"""CPU tests of the cell-to-cell line of sight (csrc/avl_sight.hip, ops/sight.py, Map.get_viewpoints / get_viewpoint_pos,
Navigator.plan_to_viewpoint, apps.plan_path --view): the scalar restatement's own properties, the C ABI's and the Python layer's
argument checks, and the host-side map layer on the restatement.  No GPU is needed."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import _audit_ref as A  # noqa: E402
import _sight_ref as S  # noqa: E402

SYMBOLS = ("avl_los_pairs", "avl_los_count")


# ------------------------------------------------------------------ the restatement
def test_the_walk_runs_from_the_eye_to_the_target_and_is_not_symmetric():
    assert A.walk3((0, 0, 0), (2, 1, 0)) == [(0, 0, 0), (1, 0, 0), (2, 1, 0)]
    assert A.walk3((2, 1, 0), (0, 0, 0)) == [(2, 1, 0), (1, 1, 0), (0, 0, 0)]
    one = np.array([[1, 0, 0]], np.int32)                                   # a voxel in the cell only the forward walk passes
    assert S.los_ref(one, 4, 2, [[0, 0, 0]], [[2, 1, 0]]).tolist() == [0]
    assert S.los_ref(one, 4, 2, [[2, 1, 0]], [[0, 0, 0]]).tolist() == [S.VISIBLE]


def test_a_walk_between_two_cells_of_the_grid_stays_in_the_grid():
    rng = np.random.default_rng(0)
    gs, vh = 9, 4
    corners = [(r, c, h) for r in (0, gs - 1) for c in (0, gs - 1) for h in (0, vh - 1)]
    pairs = [(a, b) for a in corners for b in corners]
    pairs += [(tuple(a), tuple(b)) for a, b in zip(rng.integers(0, (gs, gs, vh), (400, 3)).tolist(), rng.integers(0, (gs, gs, vh), (400, 3)).tolist())]
    for a, b in pairs:
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        cells = np.array(A.walk3(a, b))
        assert (cells >= lo).all() and (cells <= hi).all() and all(S.inside(x, gs, vh) for x in cells.tolist()), (a, b)


def test_blockers_of_the_restatement():
    gs, vh = 12, 3
    line = np.array([[0, 0, 0], [3, 0, 0], [5, 0, 0], [5, 0, 0], [9, 0, 0], [20, 0, 0]], np.int32)      # rows 2 and 3 share a cell
    index = A.cell_dict(line, gs, vh)
    assert index[(5, 0, 0)] == 3 and (20, 0, 0) not in index

    def see(e, t, **kw):
        return S.first_blocker(index, gs, vh, e, t, **kw)
    assert see((0, 0, 0), (9, 0, 0)) == 1                                   # the eye's own (occupied) cell does not block; the first blocker
    assert see((9, 0, 0), (0, 0, 0)) == 3                                   # from the other side the shared cell comes first: its largest row
    assert see((0, 0, 0), (3, 0, 0)) == S.VISIBLE                           # the target cell is never tested
    assert see((4, 0, 0), (4, 0, 0)) == see((4, 0, 0), (5, 0, 0)) == S.VISIBLE          # n = 0, n = 1
    assert see((0, 0, 0), (4, 0, 0), end_margin=0) == 1 and see((0, 0, 0), (4, 0, 0), end_margin=1) == S.VISIBLE
    assert see((0, 0, 0), (9, 0, 0), end_margin=3) == 1 and see((0, 0, 0), (9, 0, 0), end_margin=6) == S.VISIBLE
    assert see((0, 0, 0), (9, 0, 0), end_margin=100) == S.VISIBLE
    tr = np.zeros(6, np.uint8)
    tr[1] = 1
    assert see((0, 0, 0), (9, 0, 0), transparent=tr) == 3                   # the next blocker shows
    tr[3] = 1                                                               # the OWNER of the shared cell decides, not row 2
    assert see((0, 0, 0), (9, 0, 0), transparent=tr) == S.VISIBLE
    tr[3], tr[2] = 0, 1
    assert see((0, 0, 0), (9, 0, 0), transparent=tr) == 3
    for bad in ((-1, 0, 0), (0, 12, 0), (0, 0, 3), (0, 0, -1)):
        assert see(bad, (1, 1, 1)) == see((1, 1, 1), bad) == S.INVALID
    eyes = [[0, 0, 0], [9, 0, 0], [12, 0, 0], [4, 0, 0]]
    targets = [[9, 0, 0], [4, 0, 0], [0, 0, 0], [0, 0, 3], [8, 0, 0]]
    stats = {}
    visible, first = S.counts_ref(line, gs, vh, eyes, targets, stats=stats)
    assert visible.tolist() == [1, 2, 0, 1] and first.tolist() == [2, 0, -1, 1] and stats["eye_outside"] == 1 and stats["target_outside"] == 3
    assert visible.dtype == np.uint32 and first.dtype == np.int32
    # the range: squared distances 0, 4, 9 and 16 in a free layer; equality counts, a negative bound is no bound
    eyes, targets = [[6, 0, 1]], [[6, 4, 1], [8, 0, 1], [6, 3, 1], [6, 0, 1]]
    for r2, want, want_first in ((-1, 4, 0), (16, 4, 0), (15, 3, 1), (9, 3, 1), (8, 2, 1), (3, 1, 3), (0, 1, 3)):
        stats = {}
        visible, first = S.counts_ref(line, gs, vh, eyes, targets, max_range2=r2, stats=stats)
        assert visible.tolist() == [want] and first.tolist() == [want_first], r2
        assert ("at_range" in stats) == (r2 in (16, 9, 0)) and ("beyond_range" in stats) == (0 <= r2 < 16)


# ------------------------------------------------------------------ the library
def test_symbols_are_exported_and_the_source_is_built():
    from avlmaps_amd import _lib, build
    assert build.SOURCES.get("avl_sight.hip") == build.SOURCES["avl_audit.hip"] == ["-ffp-contract=off"]
    assert (build.CSRC / "avl_cellindex.h").exists()
    for src in ("avl_audit.hip", "avl_sight.hip"):
        assert '#include "avl_cellindex.h"' in (build.CSRC / src).read_text()
    assert "struct CellIndexView" not in (build.CSRC / "avl_audit.hip").read_text()          # one definition, in the header
    build.build()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def _c_pairs(lib, **over):
    """avl_los_pairs on made-up (never dereferenced) pointers: every check comes before any device work"""
    a = dict(index=0x1000, index_bytes=1 << 30, N=10, gs=64, vh=8, eyes=0x1000, targets=0x1000, M=5, transparent=None, end_margin=0,
             blocker=0x1000)
    a.update(over)
    return lib.avl_los_pairs(a["index"], a["index_bytes"], a["N"], a["gs"], a["vh"], a["eyes"], a["targets"], a["M"], a["transparent"],
                             a["end_margin"], a["blocker"], None)


def _c_count(lib, **over):
    a = dict(index=0x1000, index_bytes=1 << 30, N=10, gs=64, vh=8, eyes=0x1000, E=5, targets=0x1000, T=7, transparent=None, end_margin=0,
             max_range2=-1, visible=0x1000, first=0x1000)
    a.update(over)
    return lib.avl_los_count(a["index"], a["index_bytes"], a["N"], a["gs"], a["vh"], a["eyes"], a["E"], a["targets"], a["T"], a["transparent"],
                             a["end_margin"], a["max_range2"], a["visible"], a["first"], None)


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    lib = _lib.load()
    grids = [dict(N=-1), dict(gs=0), dict(vh=0), dict(gs=16385, vh=1), dict(gs=16384), dict(gs=8192, vh=32), dict(N=2 ** 31 - 1)]
    common = grids + [dict(index=None), dict(index_bytes=16), dict(end_margin=-1), dict(eyes=None)]
    for call, name, more in ((_c_pairs, b"avl_los_pairs", [dict(M=-1), dict(M=2 ** 31 - 1), dict(targets=None), dict(blocker=None)]),
                             (_c_count, b"avl_los_count", [dict(E=-1), dict(E=2 ** 31), dict(T=-1), dict(T=65537), dict(targets=None),
                                                           dict(visible=None)])):
        for over in common + more:
            assert call(lib, **over) != 0, (name, over)
            assert lib.avl_last_error().startswith(name), (name, over, lib.avl_last_error())
        assert call(lib, end_margin=-1) != 0 and b"end_margin" in lib.avl_last_error()
        assert call(lib, index=None) != 0 and b"null" in lib.avl_last_error()
        assert call(lib, index_bytes=16) != 0 and b"bytes" in lib.avl_last_error()
    assert _c_count(lib, T=65537) != 0 and b"65536" in lib.avl_last_error()
    # nothing to do is not an error and touches no pointer
    assert _c_pairs(lib, M=0, eyes=None, targets=None, blocker=None) == 0
    assert _c_count(lib, E=0, eyes=None, targets=None, visible=None, first=None) == 0
    # bad arguments are refused even when there is nothing to do
    assert _c_pairs(lib, M=0, end_margin=-1) != 0 and _c_count(lib, E=0, T=65537) != 0 and _c_count(lib, E=0, index_bytes=16) != 0


def test_python_layer_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import ops
    index = ops.CellIndex(None, 0, 10, 64, 8)                 # never built: every check below comes before it is read
    cells = np.zeros((4, 3), np.int32)
    for fn in (ops.line_of_sight, ops.visible_counts):
        kind = [dict(index=None), dict(index="index"), dict(eyes=cells.astype(np.float32)), dict(targets=cells.astype(np.float64)),
                dict(eyes=np.full((4, 3), 2 ** 31, np.int64)), dict(transparent=np.zeros(10, np.float32)), dict(transparent=np.zeros(10, np.int32)),
                dict(transparent=[0] * 10)]
        value = [dict(eyes=np.zeros((4, 2), np.int32)), dict(targets=np.zeros((4,), np.int32)), dict(eyes=np.zeros((1, 4, 3), np.int32)),
                 dict(end_margin=-1), dict(transparent=np.zeros(9, np.uint8)), dict(transparent=np.zeros((10, 1), bool))]
        if fn is ops.line_of_sight:
            value += [dict(targets=np.zeros((5, 3), np.int32)), dict(eyes=np.zeros((0, 3), np.int32))]         # mismatched M
        else:
            value += [dict(targets=np.zeros((ops.LOS_MAX_TARGETS + 1, 3), np.int32)), dict(max_range=-1.0), dict(max_range=float("nan")),
                      dict(max_range=float("inf"))]
        ok = dict(index=index, eyes=cells, targets=cells)
        for over in kind:
            with pytest.raises(TypeError):
                fn(**{**ok, **over})
        for over in value:
            with pytest.raises(ValueError):
                fn(**{**ok, **over})
    assert (ops.LOS_VISIBLE, ops.LOS_INVALID, ops.LOS_MAX_TARGETS) == (-1, -2, 65536) == (S.VISIBLE, S.INVALID, 65536)
    assert ops.line_of_sight.__module__ == ops.visible_counts.__module__ == "avlmaps_amd.ops.sight"


# ------------------------------------------------------------------ the map layer, on the restatement
GS, VH, CS = 24, 6, 0.1


def _config():
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": GS, "map_config.cell_size": CS}).map_config


def _room():
    """a VLMap whose voxels are a full-height wall along row 12 (columns 4 .. 19) and a three-voxel object behind it at rows 15 .. 16;
    the obstacle crop is rows 4 .. 21, columns 2 .. 21 with the wall's cells blocked"""
    from avlmaps_amd.map import VLMap
    vm = VLMap(_config())
    wall = [(12, c, h) for c in range(4, 20) for h in range(VH)]
    obj = [(15, 10, 1), (15, 11, 1), (16, 10, 2)]
    vm.grid_pos = np.array(wall + obj, np.int32)
    vm.occupied_ids = -np.ones((GS, GS, VH), np.int32)
    vm.occupied_ids[tuple(vm.grid_pos.T)] = np.arange(len(vm.grid_pos))
    vm.rmin, vm.rmax, vm.cmin, vm.cmax = 4, 21, 2, 21
    free = np.ones((18, 20), bool)
    free[12 - 4, 4 - 2:20 - 2] = False
    vm.obstacles_cropped = free
    mask = np.zeros(len(vm.grid_pos), bool)
    mask[len(wall):] = True
    return vm, mask


class _FakeIndex:
    def __init__(self, grid_pos, gs, vh):
        self.grid_pos, self.gs, self.vh = np.array(grid_pos), gs, vh

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


@pytest.fixture
def calls(monkeypatch):
    """ops.cell_index and ops.visible_counts replaced by the restatement; every call's arguments are recorded"""
    from avlmaps_amd import ops
    seen = []

    def fake_index(grid_pos, gs, vh, stream=None):
        seen.append(("cell_index", gs, vh))
        return _FakeIndex(grid_pos, gs, vh)

    def fake_counts(index, eyes, targets, transparent=None, end_margin=0, max_range=None, want_first=True, device=False, stream=None):
        seen.append(("visible_counts", np.array(eyes), np.array(targets), None if transparent is None else np.array(transparent), end_margin,
                     max_range))
        r2 = -1 if max_range is None else int(np.floor(float(max_range) ** 2))
        return S.counts_ref(index.grid_pos, index.gs, index.vh, eyes, targets, transparent, end_margin, r2)
    monkeypatch.setattr(ops, "cell_index", fake_index)
    monkeypatch.setattr(ops, "visible_counts", fake_counts)
    return seen


def test_get_viewpoints_window_eyes_and_result(calls):
    vm, mask = _room()
    vp = vm.get_viewpoints(mask, eye_height=0.35, max_range=0.5)
    assert [c[0] for c in calls] == ["cell_index", "visible_counts"] and calls[0][1:] == (GS, VH)           # one of each
    _, eyes, targets, transparent, end_margin, max_range = calls[1]
    assert np.array_equal(targets, vm.grid_pos[mask]) and targets.dtype == np.int32 and np.array_equal(transparent != 0, mask)
    assert end_margin == 0 and max_range == 0.5 / CS
    # the window: the targets' box rows 15 .. 16, columns 10 .. 11 grown by ceil(0.5 / 0.1) = 5 cells: rows 10 .. 21, columns 5 .. 16;
    # its free cells in raster order, all at height cell int(0.35 / 0.1) = 3
    want = [(r, c) for r in range(10, 22) for c in range(5, 17) if r != 12]
    assert eyes.dtype == np.int32 and eyes[:, :2].tolist() == [list(x) for x in want] and (eyes[:, 2] == 3).all()
    assert vp.cells.tolist() == [list(x) for x in want] and vp.n_targets == 3 and vp.eye_h == 3 and len(vp) == len(want)
    assert vp.window == (4, 2, 18, 20)
    ref_v, ref_f = S.counts_ref(vm.grid_pos, GS, VH, eyes, targets, mask, 0, 25)
    assert np.array_equal(vp.visible, ref_v) and np.array_equal(vp.first, ref_f) and vp.visible.dtype == np.uint32 and vp.first.dtype == np.int32
    behind = vp.cells[:, 0] < 12
    assert behind.any() and (vp.visible[behind] == 0).all() and (vp.visible[~behind] > 0).any()             # the wall hides the object
    m = vp.mask()
    assert m.shape == (18, 20) and m.dtype == bool and m.sum() == (vp.visible > 0).sum() and not m[:9].any()
    assert m[tuple((vp.cells[vp.visible > 0] - (4, 2)).T)].all()
    # a window that reaches beyond the crop is clipped to it
    vp = vm.get_viewpoints(mask, eye_height=0.35, max_range=2.0)
    assert vp.cells[:, 0].min() == 4 and vp.cells[:, 0].max() == 21 and vp.cells[:, 1].min() == 2 and vp.cells[:, 1].max() == 21
    assert len(vp) == 18 * 20 - 16 and calls[-1][5] == 2.0 / CS
    # free: any bool array over the crop; the customized crop; a category name
    only = np.zeros((18, 20), bool)
    only[14 - 4, 7 - 2] = only[0, 0] = True
    vp = vm.get_viewpoints(mask, eye_height=0.35, max_range=0.5, free=only, end_margin=2)
    assert vp.cells.tolist() == [[14, 7]] and calls[-1][4] == 2
    vm.obstacles_new_cropped = only.astype(np.float64)
    assert vm.get_viewpoints(mask, eye_height=0.35, max_range=0.5, customized=True).cells.tolist() == [[14, 7]]
    vm.index_map = lambda name: {"sofa": mask}[name]
    assert np.array_equal(vm.get_viewpoints("sofa", eye_height=0.35, max_range=0.5, free=only).visible, vp.visible)
    assert np.array_equal(vm.get_viewpoints(mask.astype(np.uint8), eye_height=0.35, max_range=0.5, free=only).visible, vp.visible)


def test_get_viewpoints_eye_height_clamp_and_default(calls):
    vm, mask = _room()
    for height, h in ((None, VH - 1), (0.35, 3), (0.0, 0), (-2.0, 0), (0.59, 5), (0.61, VH - 1), (100.0, VH - 1)):      # the config's camera is at 1.5 m
        vp = vm.get_viewpoints(mask, eye_height=height, max_range=0.3)
        assert vp.eye_h == h and (calls[-1][1][:, 2] == h).all(), height


def test_get_viewpoints_subsamples_the_targets(calls):
    vm, mask = _room()
    everything = np.ones(len(vm.grid_pos), bool)                            # 99 voxels
    for max_targets, step in ((1024, 1), (99, 1), (98, 2), (50, 2), (49, 3), (10, 10), (1, 99)):
        vp = vm.get_viewpoints(everything, eye_height=0.35, max_range=0.3, max_targets=max_targets)
        assert np.array_equal(calls[-1][2], vm.grid_pos[::step]) and vp.n_targets == len(vm.grid_pos[::step]) <= max_targets
        assert np.array_equal(calls[-1][3] != 0, everything)               # transparent stays the whole mask


def test_get_viewpoints_errors_and_empty_cases(calls):
    from avlmaps_amd import ops
    from avlmaps_amd.map import VLMap
    vm, mask = _room()
    with pytest.raises(ValueError):
        VLMap(_config()).get_viewpoints(mask)                               # no map loaded
    for bad in (dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=float("inf")), dict(max_range=float("nan")), dict(max_targets=0),
                dict(max_targets=ops.LOS_MAX_TARGETS + 1), dict(end_margin=-1), dict(free=np.ones((3, 3), bool)),
                dict(free=np.ones((18, 20), np.uint8))):
        with pytest.raises(ValueError):
            vm.get_viewpoints(mask, **bad)
    for bad in (mask[:-1], mask.astype(np.int32), mask.reshape(-1, 1)):
        with pytest.raises(ValueError):
            vm.get_viewpoints(bad)
    assert calls == []
    vp = vm.get_viewpoints(np.zeros_like(mask))                             # an empty target set
    assert len(vp) == 0 and vp.cells.shape == (0, 2) and vp.visible.shape == vp.first.shape == (0,) and vp.n_targets == 0
    assert vp.best(3).shape == (0,) and vp.select().shape == (0,) and not vp.mask().any() and vp.mask().shape == (18, 20)
    vp = vm.get_viewpoints(mask, free=np.zeros((18, 20), bool))             # no candidate cell
    assert len(vp) == 0 and vp.n_targets == 3 and calls == []
    assert vm.get_viewpoint_pos([5.0, 5.0], np.zeros_like(mask)) == ([5.0, 5.0], [[5.0, 5.0]])


def test_viewpoints_best_select_and_the_goal_cell():
    from avlmaps_amd.map.map import Viewpoints
    from avlmaps_amd.navigator import Navigator
    cells = [[5, 5], [5, 6], [6, 5], [6, 6], [7, 5], [7, 9]]
    vp = Viewpoints(cells, [0, 4, 9, 4, 9, 5], [-1, 0, 0, 1, 0, 2], 9, 3, (4, 2, 18, 20))
    assert vp.best().tolist() == [2] and vp.best(3).tolist() == [2, 4, 5] and vp.best(99).tolist() == [2, 4, 5, 1, 3] and vp.best(0).tolist() == []
    assert vp.select(0.5).tolist() == [2, 4, 5] and vp.select(0.0).tolist() == [1, 2, 3, 4, 5] and vp.select(1.0).tolist() == [2, 4]
    assert vp.select(4.0 / 9.0).tolist() == [1, 2, 3, 4, 5] and vp.select(0.45).tolist() == [2, 4, 5]       # ceil(0.45 * 9) = 5
    with pytest.raises(ValueError):
        vp.select(1.5)
    with pytest.raises(ValueError):
        Viewpoints(cells, [0, 1], [0, 1], 1, 0, (0, 0, 1, 1))

    class Stub:
        """a map that only has get_viewpoints"""
        from avlmaps_amd.map.map import Map
        get_viewpoint_pos = Map.get_viewpoint_pos

        def get_viewpoints(self, target, **kw):
            self.kw = (target, kw)
            return vp
    m = Stub()
    # without a navigator: the nearest of the selected cells in the plane, the first in raster order among equals
    assert m.get_viewpoint_pos([6.5, 5.0], "sofa", max_range=2.0) == ([6, 5], [[6.5, 5.0], [6, 5]]) and m.kw == ("sofa", dict(max_range=2.0))
    assert m.get_viewpoint_pos([5.0, 6.0], "sofa") == ([6, 5], [[5.0, 6.0], [6, 5]])                         # (5, 6) sees too little
    assert m.get_viewpoint_pos([5.0, 6.0], "sofa", min_fraction=0.0)[0] == [5, 6]
    assert m.get_viewpoint_pos([7.0, 8.0], vp, min_fraction=1.0)[0] == [7, 5]                               # a Viewpoints as the target
    nothing = Viewpoints(cells, [0] * 6, [-1] * 6, 9, 3, (4, 2, 18, 20))
    assert m.get_viewpoint_pos([1.0, 2.0], nothing) == ([1.0, 2.0], [[1.0, 2.0]])

    class Nav(Navigator):
        """plan_to_nearest on a stub: the goal with the largest column wins"""
        def plan_to_nearest(self, start, goals):
            self.goals = np.asarray(goals).tolist()
            k = int(np.argmax(np.asarray(goals)[:, 1]))
            return k, [list(start), self.goals[k]]
    nav = Nav()
    assert nav.plan_to_viewpoint([1.0, 1.0], vp) == (5, [[1.0, 1.0], [7.0, 9.0]]) and nav.goals == [[6.0, 5.0], [7.0, 5.0], [7.0, 9.0]]
    assert nav.plan_to_viewpoint([1.0, 1.0], vp, min_fraction=1.0)[0] == 2 and nav.goals == [[6.0, 5.0], [7.0, 5.0]]
    with pytest.raises(ValueError):
        nav.plan_to_viewpoint([1.0, 1.0], nothing)
    assert m.get_viewpoint_pos([1.0, 1.0], "sofa", navigator=nav) == ([7, 9], [[1.0, 1.0], [7.0, 9.0]])


# ------------------------------------------------------------------ apps.plan_path
def test_plan_path_view_flags():
    from avlmaps_amd.apps import plan_path
    base = ["--data-dir", "x", "--query", "sofa", "--start", "1", "2"]
    a = plan_path.parse_args(base)
    assert a.view is False and a.view_range is None and a.view_fraction is None and a.nearest == "euclid"      # the old branch
    a = plan_path.parse_args(base + ["--view"])
    assert a.view is True and a.view_range == 3.0 and a.view_fraction == 0.5
    a = plan_path.parse_args(base + ["--view", "--view-range", "6", "--view-fraction", "0.25", "--nearest", "path", "--known-free",
                                     "--customize-obstacles", "--render", "p.png"])
    assert (a.view_range, a.view_fraction, a.nearest, a.known_free, a.customize_obstacles, a.render) == (6.0, 0.25, "path", True, True, "p.png")
    for bad in (["--view-range", "2"], ["--view-fraction", "0.5"], ["--view", "--view-range", "0"], ["--view", "--view-range", "inf"],
                ["--view", "--view-range", "nan"], ["--view", "--view-fraction", "1.5"], ["--view", "--view-fraction", "-0.1"],
                ["--view", "--relation", "left", "--heading", "0"], ["--view", "--area", "kitchen"], ["--view", "--sound", "dog"],
                ["--view", "--image", "q.png"], ["--view", "--goal-2d"]):
        with pytest.raises(SystemExit):
            plan_path.parse_args(base + bad)
    with pytest.raises(SystemExit):
        plan_path.parse_args(["--data-dir", "x", "--start", "1", "2", "--goal", "frontier", "--view"])
