"""The 2-D distance transform and the 2-D goal maps without a GPU: the C ABI of csrc/avl_edt2d.hip and its companions (declared,
exported, bound, arguments validated before any device work), the Python surface with the signatures the callers rely on, and the
absence of a CPU fallback."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("avl_edt2d_work_bytes", "avl_edt2d", "avl_mask_decay_2d", "avl_gauss2d_f32", "avl_product_argmax_2d")


@pytest.fixture(scope="module")
def lib():
    from avlmaps_amd.build import build
    build()
    from avlmaps_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.avl_last_error().decode()


# ------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_bound(lib):
    from avlmaps_amd import _lib
    from avlmaps_amd.build import SOURCES
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name in NEW_SYMBOLS:
        assert re.search(rf"AVL_API\s+int\s+{name}\s*\(", text), name
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS, name
    assert SOURCES["avl_edt2d.hip"] == ["-ffp-contract=off"]
    assert "typedef struct avl_window_term" in text


def test_window_term_struct_matches_the_header():
    from avlmaps_amd import ops
    assert C.sizeof(ops._WindowTermC) == 24
    text = (ROOT / "include" / "avlmaps_hip.h").read_text()
    body = text[text.index("typedef struct avl_window_term {"):text.index("} avl_window_term;")]
    names = re.findall(r"^\s+[\w \*]+?\b(\w+);", body, flags=re.M)
    assert names == [f[0] for f in ops._WindowTermC._fields_] == ["d_data", "ld", "is_f64", "reserved"]


def test_edt_arguments_are_validated_before_any_device_work(lib):
    """every pointer below is fake and must never be dereferenced: a non-zero status and a message in avl_last_error()"""
    n = C.c_size_t(77)
    assert lib.avl_edt2d_work_bytes(10, 10, None) != 0 and "null" in _err(lib)
    for H, W in ((16385, 4), (4, 16385), (0, 4), (4, -1)):
        assert lib.avl_edt2d_work_bytes(H, W, C.byref(n)) != 0 and "bad shape" in _err(lib) and n.value == 77
        assert lib.avl_edt2d(0x1000, W, H, W, 0, 0x2000, 0x3000, 0x4000, 1 << 40, None) != 0 and "bad shape" in _err(lib)
        assert lib.avl_mask_decay_2d(0x1000, W, H, W, 1.0, 0.1, 1, 0x2000, 0x3000, 0x4000, 0x5000, 1 << 40, None) != 0
        assert "bad shape" in _err(lib)
    assert lib.avl_edt2d_work_bytes(16384, 16384, C.byref(n)) == 0 and n.value >= 4 * 16384 * 16384
    assert lib.avl_edt2d_work_bytes(100, 30, C.byref(n)) == 0 and n.value >= 4 * 100 * 30
    need = n.value
    for img, out, flag, ws in ((None, 0x2000, 0x3000, 0x4000), (0x1000, None, 0x3000, 0x4000), (0x1000, 0x2000, None, 0x4000)):
        assert lib.avl_edt2d(img, 30, 100, 30, 0, out, flag, ws, need, None) != 0 and "null" in _err(lib)
    assert lib.avl_edt2d(0x1000, 30, 100, 30, 0, 0x2000, 0x3000, None, need, None) != 0 and "workspace" in _err(lib)
    assert lib.avl_edt2d(0x1000, 30, 100, 30, 0, 0x2000, 0x3000, 0x4000, need - 1, None) != 0 and "workspace" in _err(lib)
    assert lib.avl_edt2d(0x1000, 29, 100, 30, 0, 0x2000, 0x3000, 0x4000, need, None) != 0 and "rows of 29" in _err(lib)


def test_decay_arguments_are_validated_before_any_device_work(lib):
    ok = dict(mask=0x1000, ld=30, H=100, W=30, cs=1.0, rate=0.1, norm=1, out=0x2000, mm=0x3000, flag=0x4000, ws=0x5000, n=1 << 30)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.avl_mask_decay_2d(a["mask"], a["ld"], a["H"], a["W"], a["cs"], a["rate"], a["norm"], a["out"], a["mm"], a["flag"], a["ws"],
                                   a["n"], None)
        return rc, _err(lib)
    for kw, word in ((dict(mask=None), "null"), (dict(out=None), "null"), (dict(flag=None), "null"), (dict(mm=None), "d_minmax"),
                     (dict(rate=-0.1), "decay_rate"), (dict(rate=float("nan")), "decay_rate"), (dict(cs=0.0), "cell_size"),
                     (dict(cs=float("inf")), "cell_size"), (dict(ws=None), "workspace"), (dict(n=16), "workspace"), (dict(ld=7), "rows of 7")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)


def test_gauss_f32_and_product_arguments_are_validated_before_any_device_work(lib):
    from avlmaps_amd import ops
    w = np.array([0.25, 0.5, 0.25])
    assert lib.avl_gauss2d_f32(None, 1, 30, 10, 30, w.ctypes.data, 1, 0x2000, None, 0.5, 0x3000, None) != 0 and "bad image" in _err(lib)
    assert lib.avl_gauss2d_f32(0x1000, 1, 29, 10, 30, w.ctypes.data, 1, 0x2000, None, 0.5, 0x3000, None) != 0 and "bad image" in _err(lib)
    assert lib.avl_gauss2d_f32(0x1000, 1, 30, 10, 30, w.ctypes.data, 1, None, None, 0.5, 0x3000, None) != 0 and "no output" in _err(lib)
    assert lib.avl_gauss2d_f32(0x1000, 1, 30, 10, 30, None, 1, 0x2000, None, 0.5, 0x3000, None) != 0 and "null weights" in _err(lib)
    assert lib.avl_gauss2d_f32(0x1000, 1, 30, 10, 30, w.ctypes.data, 33, 0x2000, None, 0.5, 0x3000, None) != 0 and "radius 33" in _err(lib)
    idx, val = C.c_int64(-7), C.c_double(-7.0)
    terms = (ops._WindowTermC * 9)(*[ops._WindowTermC(0x1000, 30, 1, 0)] * 9)

    def call(t, K, h=10, w=30, out=0x2000):
        rc = lib.avl_product_argmax_2d(t, K, h, w, out, C.byref(idx), C.byref(val), None)
        return rc, _err(lib)
    assert call(None, 1)[0] != 0 and "null terms" in _err(lib)
    for K in (0, 9, -1):
        rc, msg = call(terms, K)
        assert rc != 0 and f"K = {K}" in msg
    rc, msg = call(terms, 2, h=0)
    assert rc != 0 and "bad window" in msg
    rc, msg = call(terms, 2, w=31)
    assert rc != 0 and "rows of 30" in msg
    terms[1].d_data = None
    rc, msg = call(terms, 2)
    assert rc != 0 and "term 1" in msg and "null data" in msg
    assert (idx.value, val.value) == (-7, -7.0)
    assert lib.avl_product_argmax_2d(terms, 1, 10, 30, None, None, None, None) != 0 and "no output" in _err(lib)


# ------------------------------------------------------------------ the Python surface
def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_new_names_exist_with_their_signatures():
    E = inspect.Parameter.empty
    from avlmaps_amd import ops
    from avlmaps_amd.map import AVLMap, Goal2D, Map, VLMap
    from avlmaps_amd.utils import visualize_utils
    assert _params(ops.distance_transform_edt) == [("image", E), ("device", False), ("stream", None)]
    assert _params(ops.mask_decay_2d)[:7] == [("mask", E), ("decay_rate", E), ("cell_size", 1.0), ("normalize", False), ("smooth_sigma", None),
                                              ("device", False), ("stream", None)]
    assert _params(ops.product_argmax_2d)[:2] == [("terms", E), ("want_heat", True)]
    assert _params(visualize_utils.get_heatmap_from_mask_2d) == [("mask", E), ("cell_size", 0.05), ("decay_rate", 0.01)]
    assert _params(VLMap.get_predict_mask) == [("self", E), ("name", E)]
    assert _params(VLMap.get_distribution_map) == [("self", E), ("name", E), ("decay_rate", 0.1)]
    assert _params(Map.get_max_pos) == [("self", E), ("map_2d", E)]
    assert _params(AVLMap.index_goal_2d) == [("self", E), ("obj", None), ("area", None), ("sound", None), ("decay_rates", None),
                                             ("want_heat", True)]
    assert VLMap.get_predict_mask is not Map.get_predict_mask and VLMap.get_distribution_map is not Map.get_distribution_map
    g = Goal2D(None, 0.5, (40, 50))
    assert g.heat is None and g.value == 0.5 and g.cell.tolist() == [40, 50]
    assert ops.EDT_MAX_SIDE == 16384


def test_the_abstract_methods_of_map_raise():
    from avlmaps_amd.map import Map
    m = Map.__new__(Map)
    with pytest.raises(NotImplementedError):
        m.get_predict_mask("sofa")
    with pytest.raises(NotImplementedError):
        m.get_distribution_map("sofa")


def test_python_checks_come_before_the_device(lib):
    from avlmaps_amd import _lib, ops
    from avlmaps_amd.map import AVLMap
    with pytest.raises(ValueError):
        ops.distance_transform_edt(np.zeros((3, 4, 5), bool))
    with pytest.raises(ValueError):
        ops.distance_transform_edt(np.zeros((0, 4), bool))
    with pytest.raises(_lib.AvlError, match="bad shape"):                    # the library's argument error, no device involved
        ops.distance_transform_edt(np.zeros((1, 16385), bool))
    with pytest.raises(_lib.AvlError, match="bad shape"):
        ops.mask_decay_2d(np.ones((16385, 1), bool), 0.1)
    with pytest.raises(ValueError):
        ops.mask_decay_2d(np.ones((4, 4), bool), -1.0)
    with pytest.raises(ValueError):
        ops.mask_decay_2d(np.ones((4, 4), bool), 0.1, cell_size=0.0)
    with pytest.raises(ValueError):
        ops.mask_decay_2d(np.ones((4, 4), bool), 0.1, window=(0, 5, 0, 4))
    with pytest.raises(ValueError):
        ops.product_argmax_2d([])
    with pytest.raises(ValueError):
        ops.product_argmax_2d([np.ones((2, 2))] * 9)
    with pytest.raises(ValueError):
        ops.product_argmax_2d([np.ones((2, 2)), np.ones((2, 3))])
    with pytest.raises(ValueError):
        ops.Window(np.ones((4, 4)), 0, 5, 0, 4)
    av = AVLMap.__new__(AVLMap)
    with pytest.raises(ValueError, match="at least one"):
        av.index_goal_2d()


def test_no_cpu_fallback_without_gpu(lib):
    from avlmaps_amd import _lib, ops
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    img = np.ones((8, 9), bool)
    img[3, 4] = False
    with pytest.raises(_lib.AvlError):
        ops.distance_transform_edt(img)
    with pytest.raises(_lib.AvlError):
        ops.mask_decay_2d(~img, 0.1)
    with pytest.raises(_lib.AvlError):
        ops.product_argmax_2d([np.ones((2, 2))])


def test_plan_path_goal_2d_flag(capsys):
    from avlmaps_amd.apps import plan_path
    base = ["--data-dir", "x", "--query", "sofa", "--start", "3", "4"]
    assert not plan_path.parse_args(base).goal_2d and not plan_path.is_cross_modal(plan_path.parse_args(base))
    a = plan_path.parse_args(base + ["--goal-2d", "--sound", "dog"])
    assert a.goal_2d and plan_path.is_cross_modal(a)
    assert plan_path.is_cross_modal(plan_path.parse_args(base + ["--goal-2d"]))
    with pytest.raises(SystemExit):
        plan_path.parse_args(base + ["--goal-2d", "--image", "q.png"])
    assert "no 2-D map" in capsys.readouterr().err
