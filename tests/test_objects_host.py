"""The scene inventory without a GPU (csrc/avl_objects.hip, ops/objects.py, map/scene_objects.py, apps/index_map.py): the symbols,
argument checks that happen before any device work, the workspace sizes as the header's formulas, the host arithmetic of Object3D,
the vote and the margin, vote_labels, the app's flags, and that there is no CPU fallback."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("avl_label_classes_work_bytes", "avl_label_classes", "avl_pick_columns", "avl_pool_rows_work_bytes", "avl_pool_rows")


@pytest.fixture(scope="module")
def lib():
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    build()
    return _lib.load()


def _fails(lib, rc, *words):
    msg = lib.avl_last_error().decode()
    assert rc == 1, (rc, msg)                                    # AVL_ERR_INVALID
    for w in words:
        assert w in msg, (w, msg)


def test_symbols_header_source_and_signatures(lib):
    from avlmaps_amd import _lib, build
    header = (ROOT / "include" / "avlmaps_hip.h").read_text()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and f"AVL_API int {name}(" in header
        comment = header[:header.index(f"AVL_API int {name}(")].rsplit("/*", 1)[1]
        assert "Upstream has no counterpart" in comment and re.search(r"nearest: map/\w+\.py:\d+", comment), name
        assert not name.startswith(("avl_render_", "avl_nav_", "avl_navmany_"))
    assert build.SOURCES["avl_objects.hip"] == ["-ffp-contract=off"] and (build.CSRC / "avl_objects.hip").exists()


def test_label_classes_rejects_bad_arguments_before_any_device_work(lib):
    one = C.c_void_p(256)                                        # never dereferenced: every call below fails in its checks
    n = C.c_size_t(0)
    _fails(lib, lib.avl_label_classes_work_bytes(4, None), "avl_label_classes_work_bytes", "null")
    _fails(lib, lib.avl_label_classes_work_bytes(-1, C.byref(n)), "avl_label_classes_work_bytes", "N = -1")
    _fails(lib, lib.avl_label_classes_work_bytes(1 << 31, C.byref(n)), "N = 2147483648")
    _fails(lib, lib.avl_label_classes(one, one, -1, 26, one, one, one, 1 << 20, None), "avl_label_classes", "N = -1")
    _fails(lib, lib.avl_label_classes(one, one, 1 << 31, 26, one, one, one, 1 << 20, None), "avl_label_classes", "N = 2147483648")
    for connectivity in (7, 0, 27, -6):
        _fails(lib, lib.avl_label_classes(one, one, 4, connectivity, one, one, one, 1 << 20, None), "avl_label_classes", f"connectivity {connectivity}")
    for k in (0, 1, 4, 5):
        args = [one, one, 4, 26, one, one, one, 1 << 20, None]
        args[k] = None
        _fails(lib, lib.avl_label_classes(*args), "avl_label_classes", "null", ("d_grid_pos", "d_classes", "", "", "d_labels", "d_n")[k])
    _fails(lib, lib.avl_label_classes(one, one, 4, 26, one, one, None, 1 << 20, None), "avl_label_classes", "workspace (ws)")
    _fails(lib, lib.avl_label_classes(one, one, 4, 26, one, one, one, 16, None), "workspace (ws) of 16 bytes")


def test_pick_columns_rejects_bad_arguments_before_any_device_work(lib):
    one = C.c_void_p(256)
    _fails(lib, lib.avl_pick_columns(one, -1, 3, 3, one, one, None), "avl_pick_columns", "N = -1")
    _fails(lib, lib.avl_pick_columns(one, 1 << 31, 3, 3, one, one, None), "avl_pick_columns", "N = 2147483648")
    _fails(lib, lib.avl_pick_columns(one, 4, 0, 3, one, one, None), "avl_pick_columns", "C = 0")
    _fails(lib, lib.avl_pick_columns(one, 4, 3, 2, one, one, None), "avl_pick_columns", "ld = 2", "C = 3")
    for k in (0, 4, 5):
        args = [one, 4, 3, 3, one, one, None]
        args[k] = None
        _fails(lib, lib.avl_pick_columns(*args), "avl_pick_columns", "null", ("d_rows", "", "", "", "d_cols", "d_out")[k])
    assert lib.avl_pick_columns(None, 0, 3, 3, None, None, None) == 0          # no row: nothing to do


def test_pool_rows_rejects_bad_arguments_before_any_device_work(lib):
    one = C.c_void_p(256)
    n = C.c_size_t(0)
    _fails(lib, lib.avl_pool_rows_work_bytes(4, 3, 2, None), "avl_pool_rows_work_bytes", "null")
    _fails(lib, lib.avl_pool_rows_work_bytes(-1, 3, 2, C.byref(n)), "avl_pool_rows_work_bytes", "N = -1")
    _fails(lib, lib.avl_pool_rows_work_bytes(1 << 31, 3, 2, C.byref(n)), "N = 2147483648")
    _fails(lib, lib.avl_pool_rows_work_bytes(4, 3, -1, C.byref(n)), "avl_pool_rows_work_bytes", "n = -1")
    _fails(lib, lib.avl_pool_rows_work_bytes(4, 0, 2, C.byref(n)), "avl_pool_rows_work_bytes", "C = 0")
    big = 1 << 20
    _fails(lib, lib.avl_pool_rows(one, -1, 3, 3, one, 2, one, one, big, None), "avl_pool_rows", "N = -1")
    _fails(lib, lib.avl_pool_rows(one, 1 << 31, 3, 3, one, 2, one, one, big, None), "avl_pool_rows", "N = 2147483648")
    _fails(lib, lib.avl_pool_rows(one, 4, 3, 3, one, -1, one, one, big, None), "avl_pool_rows", "n = -1")
    _fails(lib, lib.avl_pool_rows(one, 4, 0, 3, one, 2, one, one, big, None), "avl_pool_rows", "C = 0")
    _fails(lib, lib.avl_pool_rows(one, 4, 3, 2, one, 2, one, one, big, None), "avl_pool_rows", "ld = 2", "C = 3")
    for k in (0, 4, 6):
        args = [one, 4, 3, 3, one, 2, one, one, big, None]
        args[k] = None
        _fails(lib, lib.avl_pool_rows(*args), "avl_pool_rows", "null", ("d_rows", "", "", "", "d_labels", "", "d_sums")[k])
    _fails(lib, lib.avl_pool_rows(one, 4, 3, 3, one, 2, one, None, big, None), "avl_pool_rows", "workspace (ws)")
    _fails(lib, lib.avl_pool_rows(one, 4, 3, 3, one, 2, one, one, 16, None), "workspace (ws) of 16 bytes")
    assert lib.avl_pool_rows(None, 4, 3, 3, None, 0, None, None, 0, None) == 0  # no object: nothing to do


def align256(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("N", [0, 1, 65, 1025])
def test_work_bytes_are_the_headers_formulas(lib, N):
    from avlmaps_amd import ops
    n = C.c_size_t(0)
    assert lib.avl_label_classes_work_bytes(N, C.byref(n)) == 0, lib.avl_last_error()
    assert n.value == 256 + 2 * align256(8 * N) + 3 * align256(4 * N) + align256(4 * ((N + 1023) // 1024))
    same = C.c_size_t(0)
    assert lib.avl_label_voxels_work_bytes(N, C.byref(same)) == 0 and same.value == n.value      # 28 bytes per voxel, as for one mask
    assert ops.POOL_CHUNK == 256
    for Cc, k in ((1, 0), (1, 1), (63, 3), (64, 1000), (130, 7)):
        assert lib.avl_pool_rows_work_bytes(N, Cc, k, C.byref(n)) == 0, lib.avl_last_error()
        assert n.value == 4 * align256(4 * N) + 2 * align256(4 * (k + 1)) + align256(8 * Cc * (N // ops.POOL_CHUNK + k)), (N, Cc, k)


def test_object3d_arithmetic():
    from avlmaps_amd import ops
    row = np.array([4, 10, 12, 20, 21, 0, 3, 42, 82, 6, 17, 5], np.int64)
    names = ["chair", "table", "other"]
    it = ops.Object3D.from_row(3, row, np.float32(0.75), 0, np.array([0.5, 0.625, 0.25]), names)
    assert it == ops.Object3D(3, 4, (10, 12, 20, 21, 0, 3), (10.5, 20.5, 1.5), 5, 0.75, (10, 20), 0, "chair", 1, "table", 0.5, 0.125)
    assert it[:7] == ops.Instance3D.from_row(3, row, np.float32(0.75))            # Instance3D's fields come first, unchanged
    assert ops.Object3D._fields == ops.Instance3D._fields + ("category", "name", "voted", "voted_name", "mean_score", "margin")
    assert all(isinstance(v, float) for v in it.center + (it.mean_score, it.margin, it.best_score))
    assert all(isinstance(v, int) for v in it.cell + it.bbox + (it.label, it.count, it.category, it.voted))
    it = ops.Object3D.from_row(1, row, 0.0, 0, np.array([2.0]), ["chair"])
    assert it.voted == 0 and it.margin == np.inf and it.mean_score == 2.0


def test_vote_and_margin():
    from avlmaps_amd import ops
    mean = np.array([[0.1, 0.7, 0.3], [0.5, 0.5, 0.2], [0.2, 0.9, 0.9], [-3.0, -1.0, -2.0], [0.25, 0.25, 0.25]])
    voted, margin = ops.vote_rows(mean)
    assert voted.dtype == np.int32 and voted.tolist() == [1, 0, 1, 1, 0]           # the first maximum wins
    assert margin.dtype == np.float64 and margin.tolist() == [0.7 - 0.3, 0.0, 0.0, 1.0, 0.0]
    voted, margin = ops.vote_rows(np.array([[0.3], [-1.0]]))
    assert voted.tolist() == [0, 0] and margin.tolist() == [np.inf, np.inf]
    voted, margin = ops.vote_rows(np.zeros((0, 4)))
    assert voted.shape == (0,) and margin.shape == (0,)
    with pytest.raises(ValueError):
        ops.vote_rows(np.zeros((3, 0)))


def hand_made_scene(min_voxels):
    """three objects among eight voxels: 1 = three 'chair' voxels that vote 'table', 2 = one 'table' voxel, 3 = two 'table' voxels;
    voxels 6 and 7 belong to no object"""
    from avlmaps_amd.map.scene_objects import SceneObjects
    labels = np.array([1, 2, 1, 3, 3, 1, 0, 0], np.int32)
    argmax = np.array([0, 1, 0, 1, 1, 0, 2, 0], np.int32)
    table = np.zeros((3, 12), np.int64)
    table[:, 0] = [3, 1, 2]
    table[:, 10] = [0, 1, 3]
    table[:, 11] = [2, 1, 4]
    vo = SimpleNamespace(n=3, table=table, best_score=np.array([0.5, 0.25, 1.0], np.float32), classes_of=argmax[table[:, 10]],
                         labels=labels, stream=None)
    mean = np.array([[0.25, 0.75, 0.0], [0.0, 1.0, 0.5], [0.5, 0.5, 0.125]])
    return SceneObjects(vo, mean, argmax, ["chair", "table", "other"], min_voxels=min_voxels), labels, argmax


def test_scene_objects_and_vote_labels_on_hand_made_labels():
    scene, labels, argmax = hand_made_scene(2)
    assert scene.n == 3 and [it.label for it in scene.objects] == [1, 3]            # listed objects keep their labels
    assert scene.voted.tolist() == [1, 1, 0] and scene.margin.tolist() == [0.5, 0.5, 0.0]
    first, third = scene.objects
    assert (first.category, first.name, first.voted, first.voted_name, first.mean_score, first.margin) == (0, "chair", 1, "table", 0.25, 0.5)
    assert (third.category, third.voted, third.voted_name, third.mean_score, third.best_voxel, third.best_score) == (1, 0, "chair", 0.5, 4, 1.0)
    votes = scene.vote_labels()
    assert votes.dtype == np.int32 and votes.tolist() == [1, 1, 1, 0, 0, 1, 2, 0]   # object 2 is not listed: its voxel keeps its argmax
    assert argmax.tolist() == [0, 1, 0, 1, 1, 0, 2, 0]                              # the argmax itself is left alone
    everything, _, _ = hand_made_scene(0)
    assert [it.label for it in everything.objects] == [1, 2, 3] and everything.vote_labels().tolist() == [1, 1, 1, 0, 0, 1, 2, 0]
    nothing, _, _ = hand_made_scene(4)
    assert nothing.objects == [] and np.array_equal(nothing.vote_labels(), argmax)


def test_json_round_trip_of_hand_made_objects(tmp_path):
    import json
    from avlmaps_amd.map.scene_objects import SceneObjects, objects_from_json
    scene, _, _ = hand_made_scene(0)
    text = scene.to_json()
    doc = json.loads(text)
    assert doc["categories"] == ["chair", "table", "other"] and doc["n_objects"] == 3 and doc["min_voxels"] == 0
    assert objects_from_json(text) == scene.objects
    scene.save(tmp_path / "objects.json")
    assert objects_from_json((tmp_path / "objects.json").read_text()) == scene.objects
    vo = SimpleNamespace(**dict(vars(scene.voxel_objects), classes_of=np.zeros(3, np.int32)))       # one column: every class is 0
    one = SceneObjects(vo, np.array([[1.0], [2.0], [3.0]]), np.zeros(8, np.int32), ["chair"], min_voxels=0)
    assert "Infinity" not in one.to_json() and objects_from_json(one.to_json()) == one.objects and one.objects[0].margin == np.inf


def test_index_map_lists_the_inventory_flags(capsys):
    from avlmaps_amd.apps import index_map
    with pytest.raises(SystemExit) as e:
        index_map.parse_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--inventory", "--inventory-json PATH", "--min-voxels", "--connectivity"):
        assert flag in text, flag
    base = ["--data-dir", "x", "--query", "chair"]
    args = index_map.parse_args(base + ["--categories", "chair,table", "--inventory", "--inventory-json", "o.json", "--connectivity", "18"])
    assert args.inventory and args.inventory_json == "o.json" and args.min_voxels == 50 and args.connectivity == 18
    assert index_map.parse_args(base).inventory is False and index_map.parse_args(base).inventory_json is None
    for bad in (["--inventory"], ["--inventory-json", "o.json"], ["--modality", "area", "--categories", "chair", "--inventory"]):
        with pytest.raises(SystemExit):
            index_map.parse_args(base + bad)                     # both need --modality object and --categories


def test_python_checks_come_before_the_device():
    from avlmaps_amd import ops
    pos, classes = np.zeros((4, 3), np.int32), np.zeros(4, np.int32)
    with pytest.raises(ValueError):
        ops.label_voxel_classes(pos, classes, connectivity=7)
    with pytest.raises(ValueError):
        ops.label_voxel_classes(pos[:, :2], classes)
    with pytest.raises(ValueError):
        ops.label_voxel_classes(pos, classes[:-1])
    with pytest.raises(ValueError):
        ops.label_voxel_classes(pos, classes, scores=np.zeros(3, np.float32))
    with pytest.raises(TypeError):
        ops.label_voxel_classes(pos, classes.astype(np.float32))
    with pytest.raises(ValueError):
        ops.pick_columns(np.zeros((4, 3), np.float32), np.zeros(5, np.int32))
    with pytest.raises(ValueError):
        ops.pick_columns(np.zeros(4, np.float32), np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        ops.pool_rows(np.zeros((4, 3), np.float32), np.zeros(4, np.int32), -1)
    with pytest.raises(ValueError):
        ops.pool_rows(np.zeros((4, 3), np.float32), np.zeros(3, np.int32), 2)
    assert ops.pool_rows(np.zeros((4, 3), np.float32), np.zeros(4, np.int32), 0).shape == (0, 3)


def test_no_cpu_fallback_without_gpu(lib):
    from avlmaps_amd import _lib, ops
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.AvlError):
        ops.label_voxel_classes(np.zeros((4, 3), np.int32), np.zeros(4, np.int32))
    with pytest.raises(_lib.AvlError):
        ops.pick_columns(np.zeros((4, 3), np.float32), np.zeros(4, np.int32))
    with pytest.raises(_lib.AvlError):
        ops.pool_rows(np.zeros((4, 3), np.float32), np.ones(4, np.int32), 1)


def test_get_objects_needs_categories_and_unsharded_rows(monkeypatch):
    from avlmaps_amd import parallel
    from avlmaps_amd.map.vlmap import VLMap
    vm = VLMap.__new__(VLMap)
    vm.scores_mat = vm.categories = None
    vm.shard_index_rows = True
    with pytest.raises(Exception, match="init_categories"):
        vm.get_objects()
    vm.scores_mat, vm.categories = np.zeros((4, 2), np.float32), ["chair", "table"]
    monkeypatch.setattr(parallel, "rank_world", lambda group=None: (0, 2))
    with pytest.raises(NotImplementedError, match="sharded"):
        vm.get_objects()
