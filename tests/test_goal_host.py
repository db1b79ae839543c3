"""Cross-modal goals without a GPU: the C ABI of avl_goal_fuse (declared, exported, bound, arguments validated before any device
work), the term list AVLMap.index_goal builds (parsing of names, pairs and lists, the fixed term order) and the apps' new flags."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    from avlmaps_amd.build import build
    build()
    from avlmaps_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ ABI
def test_symbol_is_declared_exported_and_bound(lib):
    from avlmaps_amd import _lib
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    assert re.search(r"AVL_API\s+int\s+avl_goal_fuse\s*\(const avl_goal_term\* h_terms, int K,", text)
    assert "typedef struct avl_goal_term" in text
    assert hasattr(C.CDLL(str(_lib.LIB_PATH)), "avl_goal_fuse")
    assert "avl_goal_fuse" in _lib.EXPORTED_SYMBOLS
    assert "avl_goal.hip" in __import__("avlmaps_amd.build", fromlist=["SOURCES"]).SOURCES


def test_term_struct_matches_the_header():
    """the ctypes mirror has the header's layout: 4 x int32, two pointers, int64, double = 48 bytes"""
    from avlmaps_amd import ops
    assert C.sizeof(ops._GoalTermC) == 48
    assert [f[0] for f in ops._GoalTermC._fields_] == ["kind", "gs", "vh", "reserved", "d_data", "d_aux", "n_points", "decay"]
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    body = text[text.index("typedef struct avl_goal_term {"):text.index("} avl_goal_term;")]
    names = re.findall(r"^\s+[\w \*]+?\b(\w+);", body, flags=re.M)
    assert names == ["kind", "gs", "vh", "reserved", "d_data", "d_aux", "n_points", "decay"]
    for name, val in (("DENSE_F32", 0), ("DENSE_F64", 1), ("FIELD_F32", 2), ("FIELD_F64", 3), ("CONES", 4)):
        assert re.search(rf"AVL_GOAL_{name} = {val}\b", text) and getattr(ops, f"GOAL_{name}") == val
    assert re.search(r"#define AVL_GOAL_MAX_TERMS 8\b", text) and ops.GOAL_MAX_TERMS == 8


def _call(lib, terms, K, pos=0x1000, N=10, out=None, want_host=True):
    idx, val = C.c_int64(-7), C.c_double(-7.0)
    p3 = (C.c_int32 * 3)(-7, -7, -7)
    rc = lib.avl_goal_fuse(terms, K, pos, N, out, C.byref(idx) if want_host else None, C.byref(val) if want_host else None,
                           C.cast(p3, C.c_void_p) if want_host else None, None)
    return rc, lib.avl_last_error().decode(), (idx.value, val.value, list(p3))


def _terms(*specs):
    from avlmaps_amd import ops
    arr = (ops._GoalTermC * max(len(specs), 1))()
    for k, s in enumerate(specs):
        for name, v in s.items():
            setattr(arr[k], name, v)
    return arr


def test_arguments_are_validated_before_any_device_work(lib):
    """every call below carries pointers that must never be dereferenced: a non-zero status with a message, outputs untouched"""
    dense = dict(kind=0, d_data=0x2000)
    untouched = (-7, -7.0, [-7, -7, -7])
    rc, msg, out = _call(lib, None, 1)
    assert rc != 0 and "null terms" in msg and out == untouched
    for K in (0, 9, -1):
        rc, msg, out = _call(lib, _terms(*[dense] * 9), K)
        assert rc != 0 and f"K = {K}" in msg and out == untouched
    rc, msg, out = _call(lib, _terms(dict(kind=5, d_data=0x2000)), 1)
    assert rc != 0 and "unknown kind 5" in msg and out == untouched
    rc, msg, out = _call(lib, _terms(dense, dict(kind=-1)), 2)
    assert rc != 0 and "term 1" in msg and "unknown kind" in msg
    rc, msg, out = _call(lib, _terms(dict(kind=4, d_data=0x2000, d_aux=0x3000, n_points=0, decay=0.1)), 1)
    assert rc != 0 and "P = 0" in msg and out == untouched
    rc, msg, _ = _call(lib, _terms(dict(kind=4, d_data=0x2000, d_aux=0x3000, n_points=3, decay=-0.5)), 1)
    assert rc != 0 and "decay" in msg
    rc, msg, _ = _call(lib, _terms(dict(kind=4, d_data=0x2000, d_aux=0, n_points=3, decay=0.5)), 1)
    assert rc != 0 and "null" in msg
    rc, msg, _ = _call(lib, _terms(dict(kind=2, d_data=0x2000, d_aux=0x3000, gs=0, vh=4)), 1)
    assert rc != 0 and "gs 0" in msg
    rc, msg, _ = _call(lib, _terms(dict(kind=3, d_data=0x2000, d_aux=0, gs=10, vh=4)), 1)
    assert rc != 0 and "null" in msg
    rc, msg, _ = _call(lib, _terms(dict(kind=1, d_data=0)), 1)
    assert rc != 0 and "null data" in msg
    rc, msg, _ = _call(lib, _terms(dense), 1, N=-1)
    assert rc != 0 and "N -1" in msg
    rc, msg, _ = _call(lib, _terms(dense), 1, pos=None)
    assert rc != 0 and "null grid_pos" in msg


def test_an_empty_map_has_no_goal(lib):
    dense = dict(kind=0, d_data=0x2000)
    rc, msg, out = _call(lib, _terms(dense), 1, N=0)
    assert rc != 0 and "empty map" in msg and out == (-7, -7.0, [-7, -7, -7])
    rc, _, _ = _call(lib, _terms(dense), 1, N=0, want_host=False)            # nothing to compute, nothing asked back: fine
    assert rc == 0


def test_ops_term_constructors_check_their_arguments():
    from avlmaps_amd import ops
    with pytest.raises(ValueError):
        ops.goal_terms_array([])
    with pytest.raises(ValueError):
        ops.goal_terms_array([ops.GoalTerm(ops.GOAL_DENSE_F32, data=1, n=1)] * 9)
    arr = ops.goal_terms_array([ops.GoalTerm(ops.GOAL_CONES, data=16, aux=32, n_points=5, decay=0.25),
                                ops.GoalTerm(ops.GOAL_FIELD_F64, data=48, aux=64, gs=100, vh=7)])
    assert (arr[0].kind, arr[0].d_data, arr[0].d_aux, arr[0].n_points, arr[0].decay) == (4, 16, 32, 5, 0.25)
    assert (arr[1].kind, arr[1].gs, arr[1].vh) == (3, 100, 7)
    with pytest.raises(ValueError):
        ops.GoalTerm.cones(np.zeros((0, 2), np.int32), np.zeros(0), 0.1)     # P = 0
    with pytest.raises(ValueError):
        ops.GoalTerm.cones([[1, 2]], [np.nan], 0.1)
    with pytest.raises(ValueError):
        ops.GoalTerm.cones([[1, 2]], [1.0], -1.0)
    with pytest.raises(ValueError):
        ops.GoalTerm.cones([[1, 2], [3, 4]], [1.0], 0.1)


# ------------------------------------------------------------------ AVLMap: the term list
def test_index_goal_without_a_term_is_a_value_error():
    from avlmaps_amd.map import AVLMap, Goal
    av = AVLMap.__new__(AVLMap)                         # no map, no GPU: the check comes first
    with pytest.raises(ValueError, match="at least one"):
        av.index_goal()
    with pytest.raises(ValueError, match="at least one"):
        av.index_goal(obj=[], extra=())
    g = Goal(None, 3, 0.5, [4, 5, 6])
    assert g.heat is None and g.voxel == 3 and g.value == 0.5 and g.pos.tolist() == [4, 5, 6] and g.cell.tolist() == [4, 5]


def test_goal_specs_parse_names_pairs_and_lists_in_the_fixed_order():
    from avlmaps_amd.map import AVLMap
    S = AVLMap._goal_specs
    assert S(obj="sofa") == [("obj", "sofa", 0.1)]
    assert S(obj=("sofa", 0.3)) == [("obj", "sofa", 0.3)]
    assert S(obj=["sofa", ("chair", 0.5)]) == [("obj", "sofa", 0.1), ("obj", "chair", 0.5)]
    assert S(obj=("sofa", "chair")) == [("obj", "sofa", 0.1), ("obj", "chair", 0.1)]        # a tuple of two names is a list
    assert S(area="kitchen", sound="dog") == [("area", "kitchen", 0.1), ("sound", "dog", 0.01)]
    img, e0, e1 = np.zeros((2, 2, 3), np.uint8), np.ones(4), np.zeros(4)
    # whatever order the keywords come in, the factors are objects, areas, sounds, image, extras
    got = S(extra=(e0, e1), img=img, sound=["dog", ("glass breaking", 0.02)], area=("kitchen", 0.2), obj=["sofa", "table"])
    assert [(k, r) for k, _, r in got] == [("obj", 0.1), ("obj", 0.1), ("area", 0.2), ("sound", 0.01), ("sound", 0.02), ("img", 0.01),
                                           ("extra", None), ("extra", None)]
    assert [w for _, w, _ in got[:5]] == ["sofa", "table", "kitchen", "dog", "glass breaking"]
    assert got[5][1] is img and got[6][1] is e0 and got[7][1] is e1
    # decay_rates overrides the default of a modality, an explicit pair still wins
    got = S(obj=["sofa", ("chair", 0.5)], sound="dog", img=img, decay_rates={"obj": 0.25, "img": 0.04})
    assert got == [("obj", "sofa", 0.25), ("obj", "chair", 0.5), ("sound", "dog", 0.01), ("img", img, 0.04)]
    with pytest.raises(ValueError):
        S(obj="sofa", decay_rates={"object": 0.1})
    with pytest.raises(TypeError):
        S(obj=[3])
    with pytest.raises(TypeError):
        S(area=[("kitchen", "x", 1)])


def test_goal_terms_are_built_from_the_stand_alone_queries(monkeypatch):
    """_goal_terms with the queries stubbed: one call per factor, in order, with the factor's own decay rate; area and sound
    fields are checked for a degenerate normalisation; the image is a one-point cone of peak 1 at the localised cell"""
    from avlmaps_amd import ops
    from avlmaps_amd.map import AVLMap
    calls = []

    class FakeTerm:
        @staticmethod
        def dense(heat):
            return ("dense", heat)

        @staticmethod
        def field(gf, vh):
            return ("field", gf, vh)

        @staticmethod
        def cones(cells, peaks, decay):
            return ("cones", np.asarray(cells).tolist(), np.asarray(peaks).tolist(), decay)

    monkeypatch.setattr(ops, "GoalTerm", FakeTerm)
    av = AVLMap.__new__(AVLMap)
    av._object_heat = lambda name, rate: calls.append(("obj", name, rate)) or f"heat:{name}"
    av._area_field = lambda name, rate: calls.append(("area", name, rate)) or f"field:{name}"
    av._sound_field = lambda name, rate: calls.append(("sound", name, rate)) or f"field:{name}"
    av._image_cell = lambda img, intr: calls.append(("img", img, intr)) or (12, 34)
    av._check_bounds = lambda gf, what: calls.append(("bounds", gf, what))
    av._vh = lambda: 30
    extra = np.arange(3.0)
    specs = AVLMap._goal_specs(obj=["sofa", ("chair", 0.5)], area="kitchen", sound=("dog", 0.02), img="IMG", extra=[extra])
    terms = av._goal_terms(specs, intr_mat="K")
    assert terms == [("dense", "heat:sofa"), ("dense", "heat:chair"), ("field", "field:kitchen", 30), ("field", "field:dog", 30),
                     ("cones", [[12, 34]], [1.0], 0.01), ("dense", extra)]
    assert calls == [("obj", "sofa", 0.1), ("obj", "chair", 0.5), ("area", "kitchen", 0.1), ("bounds", "field:kitchen", "area 'kitchen'"),
                     ("sound", "dog", 0.02), ("bounds", "field:dog", "sound 'dog'"), ("img", "IMG", "K")]


def test_index_goal_raises_what_the_queries_raise_before_any_gpu_work():
    from avlmaps_amd.map.avlmap import AVLMap, MissingSubMap
    av = AVLMap.__new__(AVLMap)
    av._area_loaded = False
    av.sound_map = None

    class VM:
        grid_pos = np.zeros((5, 3), np.int32)
    av.vlmap = VM()
    with pytest.raises(MissingSubMap):
        av.index_goal(area="kitchen")
    with pytest.raises(MissingSubMap):
        av.index_goal(sound="dog")
    VM.grid_pos = np.zeros((0, 3), np.int32)
    with pytest.raises(ValueError, match="empty map"):
        av.index_goal(area="kitchen")


# ------------------------------------------------------------------ apps
def test_index_map_fused_flags(capsys):
    from avlmaps_amd.apps import index_map
    with pytest.raises(SystemExit) as e:
        index_map.parse_args(["--data-dir", "x", "--modality", "fused"])
    assert e.value.code == 2 and "at least one of --object, --area, --sound, --image" in capsys.readouterr().err
    a = index_map.parse_args(["--data-dir", "x", "--modality", "fused", "--object", "sofa", "--object", "chair", "--sound", "dog",
                              "--area", "kitchen", "--sound-decay", "0.05", "--object-decay", "0.2"])
    assert a.object == ["sofa", "chair"] and a.area == ["kitchen"] and a.sound == ["dog"] and a.image is None
    assert index_map.fused_decay_rates(a) == {"obj": 0.2, "sound": 0.05}
    a = index_map.parse_args(["--data-dir", "x", "--modality", "fused", "--image", "q.png"])
    assert a.image == "q.png" and index_map.fused_decay_rates(a) == {}
    # the four existing modalities parse as before
    a = index_map.parse_args(["--data-dir", "x", "--query", "sofa"])
    assert a.modality == "object" and a.query == "sofa" and a.decay_rate is None
    with pytest.raises(SystemExit):
        index_map.parse_args(["--data-dir", "x", "--modality", "area"])
    with pytest.raises(SystemExit):
        index_map.parse_args(["--data-dir", "x", "--modality", "image"])
    with pytest.raises(SystemExit):
        index_map.parse_args(["--data-dir", "x", "--query", "sofa", "--sound", "dog"])     # a fused flag without --modality fused


def test_plan_path_takes_the_old_branch_without_the_new_flags():
    from avlmaps_amd.apps import plan_path
    base = ["--data-dir", "x", "--query", "sofa", "--start", "3", "4"]
    a = plan_path.parse_args(base)
    assert not plan_path.is_cross_modal(a) and a.area == [] and a.sound == [] and a.image is None and a.start == [3.0, 4.0]
    for more in (["--sound", "dog"], ["--area", "kitchen", "--area", "hall"], ["--image", "q.png"]):
        assert plan_path.is_cross_modal(plan_path.parse_args(base + more))


def test_goal_cell_is_clamped_into_the_crop():
    from avlmaps_amd.apps.plan_path import clamp_cell
    assert clamp_cell([50, 60], 40, 45, (30, 35)) == [50, 60]                  # inside: unchanged
    assert clamp_cell([39, 60], 40, 45, (30, 35)) == [40, 60]
    assert clamp_cell([70, 44], 40, 45, (30, 35)) == [69, 45]
    assert clamp_cell([500, 500], 40, 45, (30, 35)) == [69, 79]
    assert clamp_cell(np.array([-3, 79], np.int32), 40, 45, (30, 35)) == [40, 79]
