"""The open-set quantile queries without a GPU (csrc/avl_colselect.hip, ops/select.py, apps/index_map.py): the host interpolation
against NumPy, the exported symbols and the source list, argument checks that happen before any device work, the bare import of
the family module, the app's flag, and that there is no CPU fallback."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SIZES = [1, 2, 3, 64, 257, 4099]
PERCENTILES = [0, 1, 33.3, 50, 95, 99.9, 100]


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


def _column(N, kind, seed=0):
    rng = np.random.default_rng(seed + N)
    if kind == "ties":                                           # a third of the values tied, and more
        return rng.choice(np.array([-1.5, 0.25, 0.3, 7.0], np.float32), N)
    x = rng.standard_normal(N).astype(np.float32)
    x[rng.random(N) < 1 / 3] = np.float32(0.125)
    return x


@pytest.mark.parametrize("kind", ["ties", "mixed"])
@pytest.mark.parametrize("N", SIZES)
def test_the_host_lerp_is_numpys_float64_percentile(N, kind):
    """quantile_index and quantile_lerp on the two order statistics of the sorted column give np.percentile of the float64 column,
    bit for bit"""
    from avlmaps_amd import ops
    col = _column(N, kind)
    srt = np.sort(col)
    for q in PERCENTILES:
        k, t = ops.quantile_index(q, N)
        assert 0 <= k < N and 0 <= t < 1 and isinstance(k, int)
        got = ops.quantile_lerp(srt[k], srt[min(k + 1, N - 1)], t)
        want = np.percentile(col.astype(np.float64), q)
        assert got.dtype == np.float64 and got.tobytes() == np.float64(want).tobytes(), (N, q, float(got), float(want))
    k, t = ops.quantile_index(100, N)
    assert (k, t) == (N - 1, 0.0)


def test_the_lerp_of_arrays_and_bad_percentiles():
    from avlmaps_amd import ops
    a, b = np.array([1, 1, -2], np.float32), np.array([3, 1, 6], np.float32)
    assert ops.quantile_lerp(a, b, 0.25).tolist() == [1.5, 1.0, 0.0] and ops.quantile_lerp(a, b, 0.75).tolist() == [2.5, 1.0, 4.0]
    assert np.isnan(ops.quantile_lerp(np.float32(-np.inf), np.float32(1), 0.0))          # inf * 0, as NumPy's _lerp has it
    for q in (-0.1, 100.5, float("nan")):
        with pytest.raises(ValueError):
            ops.quantile_index(q, 10)
    assert ops.COLSELECT_SLOTS == 64
    assert ops.ColumnOrderStats._fields == ("v_k", "v_next", "count_lt", "count_le", "nan_count")


def test_symbols_and_source(lib):
    from avlmaps_amd import _lib, build
    for name in ("avl_colselect_workspace_bytes", "avl_colselect_f32", "avl_cols_above_f32"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "avl_colselect.hip" in build.SOURCES and (build.CSRC / "avl_colselect.hip").exists()
    header = (ROOT / "include" / "avlmaps_hip.h").read_text()
    for name in ("avl_colselect_workspace_bytes", "avl_colselect_f32", "avl_cols_above_f32"):
        at = header.index(f"AVL_API int {name}(")
        assert "map/clip_map.py:62-75" in header[header.rindex("/*", 0, at):at], name      # what the declaration replaces


def _select(lib, N, Q, ld, columns, ks, ws_bytes=1 << 20, **null):
    one = C.c_void_p(256)                                        # never dereferenced: every call fails in its checks
    cols, kk = (C.c_int32 * len(columns))(*columns), (C.c_int64 * len(ks))(*ks)
    args = dict(scores=one, cols=cols, kk=kk, v_k=one, v_next=one, lt=one, le=one, nan=one, ws=one)
    args.update(null)
    return lib.avl_colselect_f32(args["scores"], N, Q, ld, args["cols"], args["kk"], len(columns), args["v_k"], args["v_next"], args["lt"],
                                 args["le"], args["nan"], args["ws"], ws_bytes, None)


def test_colselect_rejects_bad_arguments_before_any_device_work(lib):
    _fails(lib, _select(lib, 10, 4, 3, [0], [0]), "avl_colselect_f32", "ld = 3 < Q = 4")
    _fails(lib, _select(lib, 10, 4, 4, [0, 1], [0, 10]), "avl_colselect_f32", "slot 1", "k = 10 of N = 10")
    _fails(lib, _select(lib, 10, 4, 4, [0], [-1]), "slot 0", "k = -1")
    _fails(lib, _select(lib, 10, 4, 4, [0, 4], [0, 0]), "avl_colselect_f32", "slot 1", "column 4 of 4")
    _fails(lib, _select(lib, 10, 4, 4, [-1], [0]), "column -1 of 4")
    _fails(lib, _select(lib, 0, 4, 4, [0], [0]), "avl_colselect_f32", "N = 0")
    _fails(lib, _select(lib, 1 << 31, 4, 4, [0], [0]), "N = 2147483648")
    _fails(lib, _select(lib, 10, 0, 4, [0], [0]), "Q = 0")
    for name in ("scores", "v_k", "v_next", "lt", "le", "nan", "ws", "cols", "kk"):
        _fails(lib, _select(lib, 10, 4, 4, [0], [0], **{name: None}), "avl_colselect_f32", "null")
    _fails(lib, _select(lib, 10, 4, 4, [0], [0], ws_bytes=16), "workspace (ws) of 16 bytes")
    n = C.c_size_t(0)
    _fails(lib, lib.avl_colselect_workspace_bytes(1, None), "avl_colselect_workspace_bytes", "null")
    _fails(lib, lib.avl_colselect_workspace_bytes(-1, C.byref(n)), "-1 slots")
    assert lib.avl_colselect_workspace_bytes(1, C.byref(n)) == 0 and n.value >= 64 * 256 * 8
    one_slot = n.value
    assert lib.avl_colselect_workspace_bytes(1000, C.byref(n)) == 0 and n.value == one_slot       # the groups share one workspace


def test_cols_above_rejects_bad_arguments_before_any_device_work(lib):
    one = C.c_void_p(256)
    _fails(lib, lib.avl_cols_above_f32(one, 10, 4, 3, one, -1, one, one, None, None), "avl_cols_above_f32", "ld = 3 < Q = 4")
    _fails(lib, lib.avl_cols_above_f32(one, -1, 4, 4, one, -1, one, one, None, None), "avl_cols_above_f32", "N = -1")
    _fails(lib, lib.avl_cols_above_f32(one, 10, 0, 4, one, -1, one, one, None, None), "Q = 0")
    _fails(lib, lib.avl_cols_above_f32(one, 10, 4, 4, one, 4, one, one, one, None), "mask column 4 of 4")
    _fails(lib, lib.avl_cols_above_f32(one, 10, 4, 4, one, 2, one, one, None, None), "mask column 2")        # a column without a mask
    _fails(lib, lib.avl_cols_above_f32(one, 10, 4, 4, one, -1, one, one, one, None), "mask column -1")       # a mask without a column
    _fails(lib, lib.avl_cols_above_f32(None, 10, 4, 4, one, -1, one, one, None, None), "null")
    _fails(lib, lib.avl_cols_above_f32(one, 10, 4, 4, None, -1, one, one, None, None), "null")
    _fails(lib, lib.avl_cols_above_f32(one, 10, 4, 4, one, -1, one, None, None, None), "null")
    _fails(lib, lib.avl_cols_above_f32(one, 10, 4, 4, one, -1, None, one, None, None), "null")


def test_python_checks_come_before_the_device():
    from avlmaps_amd import ops
    scores = np.zeros((5, 3), np.float32)
    with pytest.raises(IndexError):
        ops.column_order_stats(scores, [3], [0])
    with pytest.raises(IndexError):
        ops.column_order_stats(scores, [0], [5])
    with pytest.raises(ValueError):
        ops.column_order_stats(scores, [0, 1], [0])
    with pytest.raises(ValueError):
        ops.column_order_stats(np.zeros((0, 3), np.float32), [0], [0])
    with pytest.raises(ValueError):
        ops.column_quantiles(scores, 101)
    with pytest.raises(ValueError):
        ops.column_quantiles(np.zeros(5, np.float32), 50)
    with pytest.raises(IndexError):
        ops.cols_above(scores, np.zeros(3), column=3)
    with pytest.raises(ValueError):
        ops.cols_above(scores, np.zeros(4))


def test_ops_select_imports_without_torch_and_without_the_library():
    code = ("import sys; import avlmaps_amd.ops.select as s; from avlmaps_amd import _lib, ops; "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert _lib._lib is None, 'the library was loaded'; "
            "assert ops.column_quantiles is s.column_quantiles and ops.cols_above is s.cols_above "
            "and ops.column_order_stats is s.column_order_stats and ops.ColumnOrderStats is s.ColumnOrderStats")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_vlmap_needs_categories_and_unsharded_rows(monkeypatch):
    from avlmaps_amd import parallel
    from avlmaps_amd.map.vlmap import VLMap
    vm = VLMap.__new__(VLMap)
    vm.scores_mat = vm.categories = None
    vm.shard_index_rows = True
    for call in (vm.quantile_thresholds, vm.quantile_labels, lambda: vm.index_map_quantile("chair"), lambda: vm.get_quantile_predict_mask("chair")):
        with pytest.raises(Exception, match="init_categories"):
            call()
    vm.scores_mat, vm.categories = np.zeros((4, 2), np.float32), ["chair", "table"]
    monkeypatch.setattr(parallel, "rank_world", lambda group=None: (0, 2))
    for call in (vm.quantile_thresholds, vm.quantile_labels, lambda: vm.index_map_quantile("chair")):
        with pytest.raises(NotImplementedError, match="sharded"):
            call()
    doc = VLMap.index_map_quantile.__doc__
    for words in ("map/clip_map.py:45-75", "maximum in float32", "dense 2-D CLIP grid", "float64(score) > threshold", "cannot be imported"):
        assert words in doc, words


def test_index_map_lists_the_quantile_flag(capsys):
    from avlmaps_amd.apps import index_map
    with pytest.raises(SystemExit) as e:
        index_map.parse_args(["--help"])
    assert e.value.code == 0
    assert "--quantile P" in capsys.readouterr().out
    base = ["--data-dir", "x", "--query", "chair"]
    args = index_map.parse_args(base + ["--categories", "chair,table", "--quantile", "95", "--instances"])
    assert args.quantile == 95.0 and args.instances
    assert index_map.parse_args(base).quantile is None
    for bad in (["--quantile", "95"], ["--categories", "chair", "--quantile", "101"], ["--categories", "chair", "--quantile", "95", "--instance", "1"],
                ["--categories", "chair", "--quantile", "95", "--modality", "sound"]):
        with pytest.raises(SystemExit):
            index_map.parse_args(base + bad)


def test_no_cpu_fallback_without_gpu(lib):
    from avlmaps_amd import _lib, ops
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    scores = np.zeros((4, 2), np.float32)
    with pytest.raises(_lib.AvlError):
        ops.column_order_stats(scores, [0], [1])
    with pytest.raises(_lib.AvlError):
        ops.column_quantiles(scores, 95)
    with pytest.raises(_lib.AvlError):
        ops.cols_above(scores, np.zeros(2))
