"""Object relations without a GPU (csrc/avl_relations.hip, ops/relations.py, map/scene_graph.py, apps/index_map.py): the symbols,
the argument checks that happen before any device work, the workspace size as the header's formula, the Python checks that come
before the library, every SceneGraph method on a hand-made table, the reference of the GPU tests on a case worked out by hand, and
the app's flags."""
import ctypes as C
import json
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
SYMBOLS = ("avl_object_relations_work_bytes", "avl_object_relations")


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
    from avlmaps_amd import _lib, build, ops
    header = (ROOT / "include" / "avlmaps_hip.h").read_text()
    assert "(24) object relations" in header
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and f"AVL_API int {name}(" in header
        comment = header[:header.index(f"AVL_API int {name}(")].rsplit("/*", 1)[1]
        assert "Upstream has no counterpart" in comment and re.search(r"nearest: map/\w+\.py:\d+", comment), name
    section = header[header.index("(24) object relations"):]
    for words in ("checked before any device work", "order in which atomics land", "ASYMMETRIC", "scans but is never seen"):
        assert words in section, words
    assert build.SOURCES["avl_relations.hip"] == ["-ffp-contract=off"] and (build.CSRC / "avl_relations.hip").exists()
    assert (ops.RELATIONS_MAX_RADIUS, ops.RELATION_TABLE_COLS) == (15, 8)


def index_bytes(lib, N, gs, vh):
    n = C.c_size_t(0)
    assert lib.avl_cell_index_work_bytes(N, gs, vh, C.byref(n)) == 0, lib.avl_last_error()
    return n.value


def test_object_relations_rejects_bad_arguments_before_any_device_work(lib):
    one = C.c_void_p(256)                                        # never dereferenced: every call below fails in its checks
    n = C.c_size_t(0)
    who = "avl_object_relations"
    _fails(lib, lib.avl_object_relations_work_bytes(4, None), "avl_object_relations_work_bytes", "null")
    for bad in (0, -1, (1 << 28) + 1):
        _fails(lib, lib.avl_object_relations_work_bytes(bad, C.byref(n)), "avl_object_relations_work_bytes", f"max_pairs = {bad}")
    ib, big = index_bytes(lib, 4, 8, 4), 1 << 30
    good = [one, ib, 4, 8, 4, one, one, 3, 2, 16, one, one, one, big, None]
    for k, name in ((0, "d_index"), (5, "d_grid_pos"), (6, "d_labels"), (10, "d_table"), (11, "d_count")):
        args = list(good)
        args[k] = None
        _fails(lib, lib.avl_object_relations(*args), who, "null", name)
    for N, word in ((-1, "-1 voxels"), ((1 << 31) - 1, "2147483647 voxels")):
        args = list(good)
        args[2] = N
        _fails(lib, lib.avl_object_relations(*args), who, word)
    for gs, vh in ((0, 4), (16385, 1), (8, 0), (16384, 8)):
        args = list(good)
        args[3], args[4] = gs, vh
        _fails(lib, lib.avl_object_relations(*args), who, f"grid {gs} x {gs} x {vh}")
    args = list(good)
    args[1] = ib - 1
    _fails(lib, lib.avl_object_relations(*args), who, "index buffer", f"{ib - 1} bytes")
    args = list(good)
    args[7] = -1
    _fails(lib, lib.avl_object_relations(*args), who, "n = -1")
    for bad in (0, -3, (1 << 28) + 1):
        args = list(good)
        args[9] = bad
        _fails(lib, lib.avl_object_relations(*args), who, f"max_pairs = {bad}")
    for bad in (0, -1, 16, 100):
        args = list(good)
        args[8] = bad
        _fails(lib, lib.avl_object_relations(*args), who, f"radius {bad}")
    args = list(good)
    args[12] = None
    _fails(lib, lib.avl_object_relations(*args), who, "workspace (ws)")
    args = list(good)
    args[13] = 16
    _fails(lib, lib.avl_object_relations(*args), who, "workspace (ws) of 16 bytes")


def align256(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("max_pairs", [1, 2, 3, 1000, 1024, 1025, 1 << 20, 1 << 28])
def test_work_bytes_are_the_headers_formula(lib, max_pairs):
    n = C.c_size_t(0)
    assert lib.avl_object_relations_work_bytes(max_pairs, C.byref(n)) == 0, lib.avl_last_error()
    H = 2
    while H < 2 * max_pairs:
        H *= 2
    assert n.value == (256 + 2 * align256(8 * H) + align256(24 * H) + align256(4 * ((H + 1023) // 1024)) + 2 * align256(8 * max_pairs)
                       + 2 * align256(4 * max_pairs))


def test_python_checks_come_before_the_library(monkeypatch):
    from avlmaps_amd import _lib, ops

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    index = ops.CellIndex(None, 0, 4, 8, 4)
    pos, labels = np.zeros((4, 3), np.int32), np.ones(4, np.int32)
    with pytest.raises(TypeError, match="CellIndex"):
        ops.object_relations(object(), pos, labels, 2, 2)
    with pytest.raises(ValueError, match="cells"):
        ops.object_relations(index, pos[:, :2], labels, 2, 2)
    with pytest.raises(ValueError, match="built over 4"):
        ops.object_relations(index, pos[:3], labels[:3], 2, 2)
    with pytest.raises(ValueError, match="labels has shape"):
        ops.object_relations(index, pos, labels[:3], 2, 2)
    with pytest.raises(TypeError, match="int32"):
        ops.object_relations(index, pos, labels.astype(np.float32), 2, 2)
    with pytest.raises(TypeError, match="int32"):
        ops.object_relations(index, pos.astype(np.float64), labels, 2, 2)
    with pytest.raises(ValueError, match="n = -1"):
        ops.object_relations(index, pos, labels, -1, 2)
    for radius in (0, 16, -2):
        with pytest.raises(ValueError, match=f"radius {radius}"):
            ops.object_relations(index, pos, labels, 2, radius)
    for max_pairs in (0, (1 << 28) + 1):
        with pytest.raises(ValueError, match="max_pairs"):
            ops.object_relations(index, pos, labels, 2, 2, max_pairs=max_pairs)


def test_no_cpu_fallback_without_gpu(lib):
    from avlmaps_amd import _lib, ops
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.AvlError):
        ops.object_relations(ops.CellIndex(None, 0, 4, 8, 4), np.zeros((4, 3), np.int32), np.ones(4, np.int32), 2, 2)


def test_the_reference_on_a_case_worked_out_by_hand():
    """a 2 x 2 plate of object 1 at height 0, one voxel of object 2 on it and one of object 3 two cells to the side"""
    from _scene_graph_ref import offset_code, reference_relations
    pos = np.array([[1, 1, 0], [1, 2, 0], [2, 1, 0], [2, 2, 0], [1, 1, 1], [1, 4, 0], [9, 9, 9]], np.int32)
    labels = np.array([1, 1, 1, 1, 2, 3, 3], np.int32)                           # the last row lies outside the 6 x 6 x 3 grid
    table, P = reference_relations(pos, labels, 3, 2, 6, 3)
    # (1, 2): row 0 sees row 4 straight above (d2 1); 2 rests on 1 with one voxel; row 4 touches all four plate voxels, each touches it
    # (1, 3): rows 1 and 3 are 2 and sqrt(5) from row 5: d2 4, scanned by row 1 at (0, 2, 0); (2, 3): 3^2 + 1 > 4, no pair
    assert P == 2 and table.tolist() == [[1, 2, 1, 0, 4, 0, 1, 8], [1, 3, 4, 1, 5, 0, 0, 0]]
    assert reference_relations(pos, labels, 3, 1, 6, 3)[0].tolist() == [[1, 2, 1, 0, 4, 0, 1, 2]]
    assert reference_relations(pos, labels, 1, 2, 6, 3)[1] == 0 and reference_relations(pos[:0], labels[:0], 3, 2, 6, 3)[1] == 0
    assert offset_code(-2, -2, -2, 2) == 0 and offset_code(0, 0, 0, 2) == 62 and offset_code(15, 0, 0, 15) == 29310 < 2 ** 15


# ------------------------------------------------------------------ the scene graph on a hand-made table
def hand_made_graph():
    """five objects, four of them listed: a table (1), a mug (2) and a book (3) on it, a chair (4) that leans on the table with
    contacts in both directions, and an unlisted crumb (5)"""
    from avlmaps_amd import ops
    from avlmaps_amd.map.scene_graph import SceneGraph
    names = {1: "table", 2: "mug", 3: "book", 4: "chair"}
    objects = SimpleNamespace(objects=[SimpleNamespace(label=k, voted_name=v) for k, v in names.items()], n=5, min_voxels=2)
    labels = np.array([1, 2, 3, 4, 5, 1, 2, 4], np.int32)
    table = np.array([[1, 2, 1, 0, 1, 0, 16, 40],                                # the mug on the table: row 0 (table) scans row 1 (mug)
                      [1, 3, 1, 2, 5, 0, 30, 90],                                # the book on the table, scanned from the book's row 2
                      [1, 4, 1, 3, 0, 2, 5, 12],                                 # contacts both ways: the chair has more on the table
                      [1, 5, 1, 4, 0, 0, 1, 4],                                  # the crumb is not listed
                      [2, 3, 9, 6, 2, 0, 0, 0],                                  # mug and book: near, not touching
                      [3, 4, 4, 2, 7, 3, 3, 6]], np.int64)                       # as many on each other: nobody rests
    rel = ops.ObjectRelations(len(table), table, 3, 5)
    return SceneGraph(objects, rel, 0.05, 3, labels=labels), rel


def test_scene_graph_methods_on_a_hand_made_table():
    from avlmaps_amd.map.scene_graph import Relation
    g, rel = hand_made_graph()
    assert [(e.a, e.b) for e in g.edges] == [(1, 2), (1, 3), (1, 4), (2, 3), (3, 4)]        # the crumb's row is no edge
    assert g.edges[0] == Relation(1, 2, 1, 0.05, 0, 1, 0, 16, 40)
    assert g.edges[1] == Relation(1, 3, 1, 0.05, 5, 2, 0, 30, 90)               # the witness scanned from the book: its sides are exchanged
    assert g.relation(2, 1) == Relation(2, 1, 1, 0.05, 1, 0, 16, 0, 40) == g.edges[0].mirrored()
    assert g.relation(1, 5).contacts == 4 and g.relation(2, 4) is None and g.relation(2, 2) is None
    assert rel.pair(3, 2).tolist() == rel.pair(2, 3).tolist() == [2, 3, 9, 6, 2, 0, 0, 0] and rel.pair(4, 5) is None
    assert g.edges[3].distance == 3 * 0.05
    assert [(e.b, e.d2) for e in g.neighbors(3)] == [(1, 1), (4, 4), (2, 9)]     # by (d2, label)
    assert [e.b for e in g.neighbors(1)] == [2, 3, 4] and g.neighbors(5) == [] and g.neighbors(7) == []
    assert [e.b for e in g.rests_on(2)] == [1] and [e.b for e in g.rests_on(3)] == [1] and g.rests_on(1) == []
    assert [e.b for e in g.rests_on(4)] == [1]                                   # 5 of the chair on the table, 2 of the table on the chair
    assert [(e.b, e.b_on_a) for e in g.supports(1)] == [(3, 30), (2, 16), (4, 5)]  # most support first
    assert g.supports(3) == [] and g.supports(4) == [] and g.rests_on(3)[0].a_on_b == 30     # 3 on 4 and 4 on 3 alike: nobody rests
    assert [(e.b, e.contacts) for e in g.touching(3)] == [(1, 90), (4, 6)] and [e.b for e in g.touching(2)] == [1]


def test_find_orders_and_matches_voted_names():
    g, _ = hand_made_graph()
    hit = g.find("mug", "on", "table")
    assert len(hit) == 1 and (hit[0][0].label, hit[0][1].label) == (2, 1) and hit[0][2] == g.relation(2, 1)
    assert [(s.label, t.label) for s, t, _ in g.find("table", "under", "mug")] == [(1, 2)]
    assert g.find("table", "under", "mug")[0][2] == g.relation(1, 2)
    assert g.find("table", "on", "mug") == [] and g.find("mug", "under", "table") == [] and g.find("book", "on", "chair") == []
    assert [(s.label, t.label) for s, t, _ in g.find("Chair ", "on", "TABLE")] == [(4, 1)]
    assert [(s.label, t.label, e.d2) for s, t, e in g.find("book", "near", "mug")] == [(3, 2, 9)]
    assert g.find("book", "touching", "mug") == [] and len(g.find("book", "touching", "chair")) == 1
    assert g.find("sofa", "near", "table") == [] and g.find("table", "near", "table") == []
    with pytest.raises(ValueError, match="relation"):
        g.find("mug", "beside", "table")
    # two subjects of one name: most support first, then by label
    g.objects.objects[2].voted_name = "mug"
    g2 = type(g)(g.objects, g.relations, g.cs, g.R, labels=g._host_labels())
    assert [(s.label, e.a_on_b) for s, _, e in g2.find("mug", "on", "table")] == [(3, 30), (2, 16)]
    assert [(s.label, t.label) for s, t, _ in g2.find("mug", "near", "mug")] == [(2, 3), (3, 2)]


def test_json_round_trip(tmp_path):
    from avlmaps_amd.map.scene_graph import relations_from_json
    g, _ = hand_made_graph()
    doc = json.loads(g.to_json())
    assert doc["radius_cells"] == 3 and doc["cell_size"] == 0.05 and doc["n_objects"] == 5 and doc["n_pairs"] == 6
    assert doc["labels"] == [1, 2, 3, 4] and doc["names"]["2"] == "mug" and len(doc["edges"]) == 5
    assert set(doc["edges"][0]) == {"a", "b", "d2", "distance", "voxel_a", "voxel_b", "a_on_b", "b_on_a", "contacts"}
    assert relations_from_json(g.to_json()) == g.edges
    g.save(tmp_path / "relations.json")
    assert relations_from_json((tmp_path / "relations.json").read_text()) == g.edges


# ------------------------------------------------------------------ the app
def test_index_map_lists_and_checks_the_relation_flags(capsys):
    from avlmaps_amd.apps import index_map
    with pytest.raises(SystemExit) as e:
        index_map.parse_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--relations", "--relation-radius M", "--relations-json PATH", "--related"):
        assert flag in text, flag
    base = ["--data-dir", "x", "--query", "chair"]
    cats = ["--categories", "chair,table"]
    plain = index_map.parse_args(base)
    assert plain.relations is False and plain.relations_json is None and plain.related is None and plain.relation_radius == 0.25
    args = index_map.parse_args(base + cats + ["--inventory", "--relations", "--relation-radius", "0.4", "--relations-json", "r.json"])
    assert args.relations and args.relation_radius == 0.4 and args.relations_json == "r.json"
    assert index_map.parse_args(base + cats + ["--related", "mug on table"]).related == ("mug", "on", "table")
    assert index_map.parse_args(base + cats + ["--relations-json", "r.json"]).relations_json == "r.json"
    for bad in (cats + ["--relations"],                          # without --inventory
                ["--relations-json", "r.json"], ["--related", "mug on table"],           # without --categories
                cats + ["--related", "mug on"], cats + ["--related", "mug beside table"], cats + ["--related", "mug on the table"],
                cats + ["--related", "mug on table", "--instance", "1"],
                cats + ["--inventory", "--relations", "--relation-radius", "0"],
                ["--modality", "area"] + cats + ["--related", "mug on table"]):
        with pytest.raises(SystemExit):
            index_map.parse_args(base + bad)


def test_get_scene_graph_goes_through_get_objects(monkeypatch):
    from avlmaps_amd import parallel
    from avlmaps_amd.map.vlmap import VLMap
    vm = VLMap.__new__(VLMap)
    vm.scores_mat = vm.categories = None
    vm.shard_index_rows = True
    with pytest.raises(Exception, match="init_categories"):
        vm.get_scene_graph()
    vm.scores_mat, vm.categories = np.zeros((4, 2), np.float32), ["chair", "table"]
    monkeypatch.setattr(parallel, "rank_world", lambda group=None: (0, 2))
    with pytest.raises(NotImplementedError, match="sharded"):
        vm.get_scene_graph()
