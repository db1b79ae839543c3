"""CPU tests of the visibility audit (csrc/avl_audit.hip, ops/audit.py, Map.audit_visibility, VLMap.prune_voxels): the walk of the
scalar restatement, the C ABI's and the Python layer's argument checks, and the host-side map layer.  No GPU is needed."""
import ctypes as C
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import _audit_ref as A  # noqa: E402
import _explore_ref as R  # noqa: E402

SYMBOLS = ("avl_cell_index_work_bytes", "avl_cell_index_build", "avl_cell_index_lookup", "avl_audit_rays")


# ------------------------------------------------------------------ the walk
def test_walk_lands_on_b_after_max_d_steps_one_cell_per_axis_per_step():
    a = (3, -2, 5)
    drives = set()
    for d in itertools.product(range(-9, 10), repeat=3):
        b = (a[0] + d[0], a[1] + d[1], a[2] + d[2])
        cells = A.walk3(a, b)
        n = max(abs(x) for x in d)
        assert len(cells) == n + 1 and cells[0] == a and cells[-1] == b, d
        steps = np.diff(np.array(cells), axis=0)
        assert np.abs(steps).max(initial=0) <= 1, d
        for k in range(3):                                                    # an axis only ever moves towards b
            assert set(np.sign(steps[:, k]).tolist()) <= {0, int(np.sign(d[k]))}, d
        if min(abs(x) for x in d) > 0:
            drives.add(([abs(x) for x in d].index(n), d[0] > 0, d[1] > 0, d[2] > 0))
    assert len(drives) == 24                                                  # all 8 octants under each of the three driving axes


def test_walk_without_height_is_the_carvers_walk():
    gs, a = 100, (45, 52)
    for dr in range(-33, 34):
        for dc in range(-33, 34):
            b = (a[0] + dr, a[1] + dc)
            flat = [(r, c) for r, c, h in A.walk3((a[0], a[1], 4), (b[0], b[1], 4))]
            assert flat == R.walk(a, b, gs, True), (dr, dc)


# ------------------------------------------------------------------ the library
def test_symbols_are_exported_and_the_source_is_built():
    from avlmaps_amd import _lib, build
    assert "avl_audit.hip" in build.SOURCES and build.SOURCES["avl_audit.hip"] == build.SOURCES["avl_explore.hip"] == ["-ffp-contract=off"]
    build.build()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def _c_audit(lib, **over):
    """avl_audit_rays on made-up (never dereferenced) pointers: every check comes before any device work"""
    K = np.eye(3)
    T = np.eye(4)[None].copy()
    ids = np.array([over.pop("frame_id", 0)], np.int32)
    a = dict(index=0x1000, index_bytes=1 << 30, N=10, gs=64, vh=8, depth=0x1000, u16=0, depth_div=1000.0, F=1, H=24, W=32, cs=0.1, stride=4,
             h_min=-0.1, h_max=0.8, min_depth=0.1, max_depth=3.0, end_margin=2, last_hit=0x1000, through=0x1000, after=None)
    a.update(over)
    return lib.avl_audit_rays(a["index"], a["index_bytes"], a["N"], a["gs"], a["vh"], a["depth"], a["u16"], a["depth_div"], a["F"], a["H"], a["W"],
                              K.ctypes.data, T.ctypes.data, ids.ctypes.data, a["cs"], a["stride"], a["h_min"], a["h_max"], a["min_depth"],
                              a["max_depth"], a["end_margin"], a["last_hit"], a["through"], a["after"], None)


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    lib = _lib.load()
    n = C.c_size_t(0)
    assert lib.avl_cell_index_work_bytes(2_000_000, 1000, 30, C.byref(n)) == 0
    # the bitmap and its prefix (4 bytes per 32 cells each), the permutation (4 bytes per voxel), the counts: 15.5 MB
    assert 2 * 4 * (30_000_000 // 32) + 4 * 2_000_000 <= n.value <= 2 * 4 * (30_000_000 // 32) + 4 * 2_000_000 + 8192
    assert lib.avl_cell_index_work_bytes(0, 1, 1, C.byref(n)) == 0 and n.value > 0
    assert lib.avl_cell_index_work_bytes(10, 64, 8, None) != 0 and b"null" in lib.avl_last_error()
    for N, gs, vh in ((-1, 64, 8), (10, 0, 8), (10, 64, 0), (10, 16385, 1), (10, 16384, 8), (10, 8192, 32), (2 ** 31 - 1, 64, 8)):
        assert lib.avl_cell_index_work_bytes(N, gs, vh, C.byref(n)) != 0, (N, gs, vh)
        assert lib.avl_cell_index_build(0x1000, N, gs, vh, 0x1000, 1 << 40, None) != 0, (N, gs, vh)
        assert lib.avl_cell_index_lookup(0x1000, 1 << 40, N, gs, vh, 0x1000, 1, 0x1000, None) != 0, (N, gs, vh)
        assert _c_audit(lib, N=N, gs=gs, vh=vh) != 0, (N, gs, vh)
    assert lib.avl_cell_index_build(0x1000, 10, 64, 8, None, 1 << 30, None) != 0 and b"null" in lib.avl_last_error()
    assert lib.avl_cell_index_build(None, 10, 64, 8, 0x1000, 1 << 30, None) != 0 and b"null" in lib.avl_last_error()
    assert lib.avl_cell_index_build(0x1000, 10, 64, 8, 0x1000, 16, None) != 0 and b"bytes" in lib.avl_last_error()
    assert lib.avl_cell_index_lookup(None, 1 << 30, 10, 64, 8, 0x1000, 1, 0x1000, None) != 0 and b"null" in lib.avl_last_error()
    assert lib.avl_cell_index_lookup(0x1000, 16, 10, 64, 8, 0x1000, 1, 0x1000, None) != 0 and b"bytes" in lib.avl_last_error()
    assert lib.avl_cell_index_lookup(0x1000, 1 << 30, 10, 64, 8, None, 1, 0x1000, None) != 0 and b"null" in lib.avl_last_error()
    assert lib.avl_cell_index_lookup(0x1000, 1 << 30, 10, 64, 8, 0x1000, -1, 0x1000, None) != 0
    bad = [dict(end_margin=-1), dict(stride=0), dict(cs=0.0), dict(cs=float("nan")), dict(h_min=1.0, h_max=0.5), dict(h_max=float("inf")),
           dict(min_depth=-0.1), dict(min_depth=3.0), dict(max_depth=float("nan")), dict(u16=1, depth_div=0.0), dict(F=-1), dict(H=0),
           dict(W=0), dict(H=65536, W=65536), dict(index=None), dict(index_bytes=16), dict(depth=None), dict(frame_id=-1)]
    for over in bad:
        assert _c_audit(lib, **over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_audit_rays"), over
    assert _c_audit(lib, end_margin=-1) != 0 and b"end_margin" in lib.avl_last_error()
    assert _c_audit(lib, frame_id=-1) != 0 and b"negative" in lib.avl_last_error()
    # nothing to do is not an error and touches no pointer: no frame, or no output
    assert _c_audit(lib, F=0, depth=None) == 0 and _c_audit(lib, last_hit=None, through=None) == 0


def test_python_layer_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import ops
    for gs, vh in ((0, 8), (64, 0), (16385, 1), (16384, 8)):
        with pytest.raises(ValueError):
            ops.cell_index(np.zeros((3, 3), np.int32), gs, vh)
    with pytest.raises(ValueError):
        ops.cell_index(np.zeros((3, 2), np.int32), 64, 8)
    with pytest.raises(TypeError):
        ops.cell_index(np.zeros((3, 3), np.float32), 64, 8)
    with pytest.raises(TypeError):
        ops.lookup_cells("index", np.zeros((1, 3), np.int32))
    index = ops.CellIndex(None, 0, 10, 64, 8)                 # never built: every check below comes before it is read
    with pytest.raises(ValueError):
        ops.lookup_cells(index, np.zeros((3,), np.int32))
    depth, K, T = np.ones((1, 24, 32), np.float32), R.calib(20.0, 16.0, 12.0), np.eye(4)[None]
    ok = dict(index=index, depth=depth, calib=K, transforms=T, frame_ids=[0], cs=0.1, last_hit=np.full(10, -1, np.int32))
    value = [dict(stride=0), dict(end_margin=-1), dict(cs=0.0), dict(cs=float("nan")), dict(h_min=1.0, h_max=0.0), dict(h_max=float("inf")),
             dict(min_depth=-1.0), dict(min_depth=6.0), dict(depth=np.ones((24,), np.float32)), dict(depth=np.ones((1, 1, 24, 32), np.float32)),
             dict(calib=np.eye(4)), dict(transforms=np.eye(4)[None].repeat(2, 0)), dict(frame_ids=[0, 1]), dict(frame_ids=[-1]),
             dict(frame_ids=[2 ** 31 - 1]), dict(frame_ids=[0.5]), dict(last_hit=np.full(9, -1, np.int32)), dict(through=np.zeros((10, 1), np.uint32)),
             dict(after=np.zeros(11, np.int32)), dict(depth=np.ones((1, 24, 32), np.uint16), depth_div=0.0)]
    for over in value:
        with pytest.raises(ValueError):
            ops.audit_rays(**{**ok, **over})
    kind = [dict(index=None), dict(depth=depth.astype(np.float64)), dict(last_hit=np.full(10, -1, np.int64)), dict(through=np.zeros(10, np.int32)),
            dict(after=np.zeros(10, np.uint32)), dict(last_hit=[-1] * 10)]
    for over in kind:
        with pytest.raises(TypeError):
            ops.audit_rays(**{**ok, **over})
    names = ("AUDIT_MAX_SIDE", "audit_rays", "cell_index", "CellIndex", "lookup_cells", "NEVER_HIT")
    assert all(hasattr(ops, n) for n in names) and ops.NEVER_HIT == -1 and ops.audit_rays.__module__ == "avlmaps_amd.ops.audit"


# ------------------------------------------------------------------ the map layer
def _config(gs=16):
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": gs, "map_config.cell_size": 0.1}).map_config


def _toy_map(n=7, gs=16, vh=4, D=8, Q=3):
    from avlmaps_amd.map import VLMap
    rng = np.random.default_rng(0)
    vm = VLMap(_config(gs))
    cells = rng.permutation(gs * gs * vh)[:n]
    vm.grid_pos = np.stack(np.unravel_index(cells, (gs, gs, vh)), axis=1).astype(np.int32)
    vm.grid_feat = rng.standard_normal((n, D)).astype(np.float32)
    vm.weight = rng.random(n).astype(np.float32)
    vm.grid_rgb = rng.integers(0, 255, (n, 3)).astype(np.uint8)
    vm.occupied_ids = -np.ones((gs, gs, vh), np.int32)
    vm.occupied_ids[tuple(vm.grid_pos.T)] = np.arange(n)
    vm.scores_mat = rng.standard_normal((n, Q)).astype(np.float32)
    vm.categories = ["a", "b", "c"]
    vm.mapped_iter_list = [0, 1]
    return vm


def test_prune_voxels_drops_rows_renumbers_cells_and_forgets_the_device_copies():
    from avlmaps_amd.map.map import VisibilityAudit
    vm = _toy_map()
    old = {k: getattr(vm, k).copy() for k in ("grid_pos", "grid_feat", "weight", "grid_rgb", "scores_mat")}
    sentinel = object()

    class Plan:
        closed = False

        def close(self):
            self.closed = True
    plan, inst = Plan(), Plan()
    vm._dev_feat, vm._dev_feat_src = sentinel, vm.grid_feat
    vm._dev_pos, vm._dev_pos_src = sentinel, vm.grid_pos
    vm._dev_rgb, vm._dev_rgb_src = sentinel, vm.grid_rgb
    vm._heat_plan_obj, vm._heat_plan_src = plan, sentinel
    vm._dev_scores, vm._dev_scores_src, vm._quantile_cache = sentinel, vm.scores_mat, {95.0: sentinel}
    vm._argmax, vm._argmax_src = np.argmax(vm.scores_mat, axis=1), vm.scores_mat
    vm._dev_argmax, vm._dev_argmax_src = sentinel, vm._argmax
    vm._instances_cache = (("key",), inst)
    vm.visibility = VisibilityAudit(np.full(7, -1, np.int32), np.zeros(7, np.uint32), {}, [1])
    mask = np.array([0, 1, 0, 0, 1, 0, 1], bool)
    with pytest.raises(ValueError):
        vm.prune_voxels(mask[:-1])
    with pytest.raises(ValueError):
        vm.prune_voxels(mask.astype(np.uint8))
    assert vm.prune_voxels(np.zeros(7, bool)) == 0 and vm._dev_feat is sentinel and vm.visibility is not None
    assert vm.prune_voxels(mask) == 3
    keep = ~mask
    for k, v in old.items():
        assert np.array_equal(getattr(vm, k), v[keep]) and getattr(vm, k).flags["C_CONTIGUOUS"] and getattr(vm, k).dtype == v.dtype, k
    want = -np.ones((16, 16, 4), np.int32)
    want[tuple(old["grid_pos"][keep].T)] = np.arange(4)
    assert np.array_equal(vm.occupied_ids, want) and vm.occupied_ids.dtype == np.int32
    assert (vm.occupied_ids[tuple(old["grid_pos"][mask].T)] == -1).all()
    for name in ("_dev_feat", "_dev_pos", "_dev_rgb", "_heat_plan_obj", "_dev_scores", "_dev_argmax", "_instances_cache", "visibility"):
        assert getattr(vm, name) is None, name
    assert plan.closed and inst.closed and vm._quantile_cache == {}
    # the closed-set query of the pruned map is the pruned rows' argmax
    assert np.array_equal(vm.index_map("b"), np.argmax(old["scores_mat"][keep], axis=1) == 1)
    # a map without scores or colours prunes too
    vm = _toy_map()
    vm.scores_mat = vm.grid_rgb = None
    assert vm.prune_voxels(np.ones(7, bool)) == 7 and vm.grid_pos.shape == (0, 3) and (vm.occupied_ids == -1).all()


def test_stale_thresholds():
    from avlmaps_amd.map.map import VisibilityAudit
    audit = VisibilityAudit(np.array([-1, 3, 0, 7, 2], np.int32), np.array([0, 2, 3, 4, 2 ** 32 - 1], np.uint32), dict(stride=4), [3, 5])
    assert audit.N == 5 and audit.frame_counts == [3, 5]
    assert audit.stale().tolist() == [False, False, True, True, True] and audit.stale().dtype == bool
    assert audit.stale(min_rays=1).tolist() == [False, True, True, True, True]
    assert audit.stale(min_rays=4).tolist() == [False, False, False, True, True]
    assert audit.stale(min_rays=2 ** 40).tolist() == [False, False, False, False, True]      # clamped to what a counter can hold
    with pytest.raises(ValueError):
        audit.stale(0)
    with pytest.raises(ValueError):
        VisibilityAudit(np.zeros(3, np.int32), np.zeros(4, np.uint32), {}, [])


def test_visibility_file_round_trips_and_a_file_of_another_map_is_left_alone(tmp_path):
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.map.map import VisibilityAudit
    from avlmaps_amd.utils.mapping_utils import save_3d_map
    vm = _toy_map()
    sc = tmp_path / "scene"
    (sc / "vlmap").mkdir(parents=True)
    save_3d_map(sc / "vlmap" / "vlmaps.h5df", vm.grid_feat, vm.grid_pos, vm.weight, vm.occupied_ids, vm.mapped_iter_list, vm.grid_rgb)
    plain = VLMap(_config())
    plain.prefetch_device = False
    assert plain.load_map(str(sc)) and plain.visibility is None             # a map without the file behaves as before
    params = dict(gs=16, cs=0.1, vh=4, stride=4, end_margin=2, n_frames=8)
    audit = VisibilityAudit(np.array([-1, 3, 0, 7, 2, 2, 5], np.int32), np.array([0, 2, 3, 4, 0, 9, 2 ** 32 - 1], np.uint32), params, [3, 5])
    audit.save(sc / "vlmap" / VLMap.VISIBILITY_FILE)
    other = VLMap(_config())
    other.prefetch_device = False
    assert other.load_map(str(sc))
    got = other.visibility
    assert got is not None and np.array_equal(got.last_hit, audit.last_hit) and np.array_equal(got.through, audit.through)
    assert got.last_hit.dtype == np.int32 and got.through.dtype == np.uint32 and got.params == params and got.frame_counts == [3, 5]
    # pruned and saved in place: the old file no longer matches the voxel count and is not picked up
    assert other.prune_voxels(got.stale()) == 4 and other.visibility is None
    save_3d_map(sc / "vlmap" / "vlmaps.h5df", other.grid_feat, other.grid_pos, other.weight, other.occupied_ids, other.mapped_iter_list,
                other.grid_rgb)
    again = VLMap(_config())
    again.prefetch_device = False
    assert again.load_map(str(sc)) and len(again.grid_pos) == 3 and again.visibility is None
    assert np.array_equal(again.grid_pos, vm.grid_pos[~audit.stale()]) and np.array_equal(again.occupied_ids, other.occupied_ids)
