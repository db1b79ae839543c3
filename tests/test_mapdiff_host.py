"""CPU tests of the map comparison (csrc/avl_mapdiff.hip, ops/mapdiff.py, map/changes.py, apps/audit_map.py --compare): the
declarations and bindings, the argument checks of the C ABI and of the Python layer, the restatements against plain NumPy, the
MapChanges file, the pairing of moved objects and the command line.  No GPU is needed."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

import _mapdiff_ref as R  # noqa: E402

SYMBOLS = {"avl_map_match_cells": 12, "avl_row_dots_f32": 8, "avl_map_diff_status": 9}
SIZE_QUERY = re.compile(r"_(work_bytes|workspace_bytes|ws_bytes)(_n)?$")


# ------------------------------------------------------------------ the library
def test_symbols_are_declared_exported_and_bound_and_none_is_a_size_query():
    from avlmaps_amd import _lib, build
    assert build.SOURCES["avl_mapdiff.hip"] == ["-ffp-contract=off"] and (build.CSRC / "avl_mapdiff.hip").exists()
    header = (ROOT / "include" / "avlmaps_hip.h").read_text()
    lib = _lib.load()
    for name, arity in SYMBOLS.items():
        m = re.search(r"AVL_API int " + name + r"\(([^;]*)\);", header)
        assert m is not None, name
        assert len(m.group(1).split(",")) == arity, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        res, args = _lib._SIGS[name]
        assert res is C.c_int and len(args) == arity, name
        assert not SIZE_QUERY.search(name)
    assert "(30) comparing two voxel maps" in header and "DESIGN.md 4.32" in header
    source = (build.CSRC / "avl_mapdiff.hip").read_text()
    assert not [n for n in re.findall(r"\bavl_\w+(?=\()", source) if SIZE_QUERY.search(n)]
    assert "-ffp-contract=off" in source                                        # the source says how fusing is kept out


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    lib = _lib.load()
    p, big = 0x1000, 1 << 40
    shift = (C.c_int32 * 3)(0, 0, 0)

    def match(index=p, nbytes=big, N=10, gs=64, vh=8, cells=p, n=5, radius=1, out=p, d2=p):
        return lib.avl_map_match_cells(index, nbytes, N, gs, vh, cells, n, shift, radius, out, d2, None)
    for over in (dict(radius=3), dict(radius=-1), dict(index=None), dict(nbytes=16), dict(cells=None), dict(out=None), dict(d2=None), dict(n=-1),
                 dict(n=2 ** 31 - 1), dict(N=-1), dict(gs=0), dict(vh=0), dict(gs=16385, vh=1), dict(gs=16384, vh=8)):
        assert match(**over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_map_match_cells"), over
    assert match(radius=3) != 0 and b"radius" in lib.avl_last_error()
    assert match(n=0, cells=None, out=None, d2=None) == 0                      # nothing to do touches no pointer

    def dots(a=p, n=5, b=p, N=7, D=16, m=p, sums=p):
        return lib.avl_row_dots_f32(a, n, b, N, D, m, sums, None)
    for over in (dict(D=0), dict(D=8193), dict(D=-4), dict(a=None), dict(b=None), dict(m=None), dict(sums=None), dict(n=-1), dict(N=-1)):
        assert dots(**over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_row_dots_f32"), over
    assert dots(n=0, a=None, m=None, sums=None) == 0

    def status(m=p, sums=p, n=5, t2=0.64, through=None, min_rays=3, out=p, counts=p):
        return lib.avl_map_diff_status(m, sums, n, t2, through, min_rays, out, counts, None)
    for over in (dict(t2=0.0), dict(t2=-0.5), dict(t2=1.0000001), dict(t2=float("nan")), dict(n=-1), dict(counts=None)):
        assert status(**over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_map_diff_status"), over


def test_python_layer_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import ops
    index = ops.CellIndex(None, 0, 10, 64, 8)               # never built: every check below comes before it is read
    cells, feat = np.zeros((4, 3), np.int32), np.ones((4, 16), np.float32)
    for over in (dict(radius=3), dict(radius=-1), dict(radius=1.5), dict(cells=np.zeros((4, 2), np.int32)), dict(cells=np.zeros((12,), np.int32)),
                 dict(shift=(0, 0)), dict(shift=(0.5, 0, 0))):
        with pytest.raises(ValueError):
            ops.match_cells(**{**dict(index=index, cells=cells), **over})
    with pytest.raises(TypeError):
        ops.match_cells("index", cells)
    with pytest.raises(TypeError):
        ops.match_cells(index, cells.astype(np.float32))
    match = np.zeros(4, np.int32)
    for a, b, m in ((np.ones((4, 0), np.float32), np.ones((4, 0), np.float32), match), (feat, np.ones((4, 8), np.float32), match),
                    (feat, feat, np.zeros(3, np.int32)), (feat, feat, np.array([0, 1, 2, 4], np.int32)), (feat[0], feat, match),
                    (np.ones((4, 8193), np.float32), np.ones((4, 8193), np.float32), match)):
        with pytest.raises(ValueError):
            ops.row_dots(a, b, m)
    for a, b, m in ((feat.astype(np.float64), feat, match), (feat, feat.astype(np.float64), match), (feat, feat, match.astype(np.float32)),
                    (feat.astype(np.float16), feat, match)):
        with pytest.raises(TypeError):
            ops.row_dots(a, b, m)
    sums = np.ones((4, 3))
    for over in (dict(threshold=0.0), dict(threshold=1.5), dict(threshold=-0.2), dict(threshold=float("nan")), dict(sums=np.ones((4, 2))),
                 dict(sums=np.ones((3, 3))), dict(through=np.zeros(5, np.int32)), dict(match=np.zeros((4, 1), np.int32))):
        with pytest.raises(ValueError):
            ops.diff_status(**{**dict(match=match, sums=sums), **over})
    ok = dict(pos_a=cells, feat_a=feat, pos_b=cells[:3], feat_b=feat[:3], gs=64, vh=8)
    for over in (dict(radius=3), dict(threshold=0.0), dict(threshold=1.01), dict(feat_a=np.ones((4, 0), np.float32), feat_b=np.ones((3, 0), np.float32)),
                 dict(feat_b=np.ones((3, 8), np.float32)), dict(feat_a=feat[:3]), dict(pos_a=np.zeros((4, 2), np.int32)), dict(gs=0), dict(vh=0),
                 dict(gs=16384, vh=8), dict(shift=(1, 2)), dict(through_a=np.zeros(3, np.int32)),
                 dict(index_b=ops.CellIndex(None, 0, 3, 32, 8)),           # mismatched grids: an index of another grid
                 dict(index_a=ops.CellIndex(None, 0, 4, 64, 4)), dict(index_a=ops.CellIndex(None, 0, 5, 64, 8))):
        with pytest.raises(ValueError):
            ops.map_diff(**{**ok, **over})
    for over in (dict(feat_a=feat.astype(np.float64)), dict(feat_b=feat[:3].astype(np.float64)), dict(pos_b=cells[:3].astype(np.float32)),
                 dict(index_a="index")):
        with pytest.raises(TypeError):
            ops.map_diff(**{**ok, **over})
    names = ("match_cells", "row_dots", "diff_status", "map_diff", "MapDiff", "DIFF_SAME", "DIFF_CHANGED", "DIFF_NO_MATCH", "DIFF_UNSEEN")
    assert all(hasattr(ops, n) for n in names) and ops.map_diff.__module__ == "avlmaps_amd.ops.mapdiff"
    assert (ops.DIFF_SAME, ops.DIFF_CHANGED, ops.DIFF_NO_MATCH, ops.DIFF_UNSEEN) == (0, 1, 2, 3)


# ------------------------------------------------------------------ the restatements
def test_the_restated_sums_are_a_dot_product_and_padding_changes_nothing():
    rng = np.random.default_rng(3)
    for D in (1, 5, 256, 300, 1000):
        a, b = rng.standard_normal((6, D)).astype(np.float32), rng.standard_normal((4, D)).astype(np.float32)
        match = np.array([0, 3, -1, 2, 1, 1], np.int32)
        sums = R.ref_row_dots(a, b, match)
        assert (sums[2] == 0).all()
        ok = match >= 0
        exact = np.einsum("ij,ij->i", a[ok].astype(np.float64), b[match[ok]].astype(np.float64))
        assert np.allclose(sums[ok, 0], exact, rtol=1e-12, atol=1e-12)
        assert np.allclose(sums[ok, 1], (a[ok].astype(np.float64) ** 2).sum(1), rtol=1e-12)
        pad = np.zeros((6, 2048), np.float32), np.zeros((4, 2048), np.float32)           # explicit zero padding: the same bytes
        pad[0][:, :D], pad[1][:, :D] = a, b
        assert sums.tobytes() == R.ref_row_dots(pad[0], pad[1], match).tobytes()
    # ownership: element d belongs to lane (d // 4) % 64 -- a row that is non-zero in one lane's elements only keeps its plain sum
    x = np.zeros(600, np.float32)
    x[[12, 13, 14, 15, 268, 269, 524]] = [1, 2, 3, 4, 5, 6, 7]
    assert R._lane_sums(x, x) == float(1 + 4 + 9 + 16 + 25 + 36 + 49)


def test_the_restated_join_orders_by_distance_then_linear_cell():
    pos_b = [(4, 4, 2), (4, 4, 2), (3, 4, 2), (5, 4, 2), (4, 5, 3), (7, 7, 4)]
    match, d2 = R.ref_match_cells(pos_b, [(4, 4, 2), (4, 4, 3), (4, 4, 1), (6, 6, 4), (7, 7, 5), (0, 0, 0)], 8, 5, 1)
    assert match.tolist() == [1, 1, 1, 5, -1, -1] and d2.tolist() == [0, 1, 1, 2, -1, -1]
    match, d2 = R.ref_match_cells(pos_b[2:5], [(4, 4, 2)], 8, 5, 1)
    assert match.tolist() == [0] and d2.tolist() == [1]                     # (3, 4, 2) and (5, 4, 2) tie: the smaller linear cell
    match, d2 = R.ref_match_cells(pos_b, [(4, 4, 2), (6, 6, 3)], 8, 5, 0, shift=(1, 1, 1))
    assert match.tolist() == [-1, 5] and d2.tolist() == [-1, 0]


def test_the_restated_status():
    match = np.array([0, 0, 0, -1, -1, 0], np.int32)
    sums = np.array([[3, 3, 3], [2.9, 3, 3], [-3, 3, 3], [0, 0, 0], [0, 0, 0], [1, 0, 3]], np.float64)
    status, counts = R.ref_status(match, sums, 1.0, np.array([9, 9, 9, 2, 3, 0]), 3)
    assert status.tolist() == [0, 1, 1, 3, 2, 1] and counts.tolist() == [1, 3, 1, 1]
    assert R.ref_status(match, sums, 0.9)[0].tolist() == [0, 0, 1, 2, 2, 1]


# ------------------------------------------------------------------ the map layer
def _changes(n_a=6, n_b=5):
    from avlmaps_amd.map.changes import MapChanges
    rng = np.random.default_rng(1)
    pos_a, pos_b = rng.integers(0, 16, (n_a, 3)).astype(np.int32), rng.integers(0, 16, (n_b, 3)).astype(np.int32)
    masks = dict(vanished=np.array([1, 0, 0, 1, 0, 0], bool), unseen=np.array([0, 1, 0, 0, 0, 0], bool), changed_a=np.array([0, 0, 1, 0, 0, 0], bool),
                 appeared=np.array([0, 0, 1, 1, 1], bool), changed=np.array([1, 0, 0, 0, 0], bool), unseen_b=np.zeros(5, bool))
    cos_a, cos_b = np.array([np.nan, np.nan, 0.25, np.nan, 1.0, 0.9]), np.array([0.25, 1.0, np.nan, np.nan, np.nan])
    params = dict(gs=16, cs=0.1, vh=16, radius=1, threshold=0.8, shift=(1, 0, -2), min_rays=3)
    return MapChanges(pos_a, pos_b, masks, cos_a, cos_b, params)


def test_map_changes_summary_masks_and_file_round_trip(tmp_path):
    from avlmaps_amd.map.changes import MapChanges
    ch = _changes()
    s = ch.summary()
    assert (s["vanished"], s["appeared"], s["changed"], s["unseen"], s["unseen_b"], s["changed_a"], s["voxels_a"], s["voxels_b"]) == (2, 3, 1, 1, 0, 1, 6, 5)
    assert s["changed_volume_m3"] == 6 * 0.1 ** 3
    assert ch.mask(("appeared", "changed")).tolist() == [True, False, True, True, True] and ch.mask("vanished").tolist() == ch.vanished.tolist()
    for kinds in (("vanished", "appeared"), (), ("moved",), ("gone",)):
        with pytest.raises(ValueError):
            ch.mask(kinds)
    with pytest.raises(ValueError):
        ch.mask("vanished", side="b")
    ch.save(tmp_path / "changes.npz")
    got = MapChanges.load(tmp_path / "changes.npz")
    for name in ("pos_a", "pos_b", "cosine_a", "cosine_b", "vanished", "unseen", "changed_a", "appeared", "changed", "unseen_b"):
        a, b = getattr(ch, name), getattr(got, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert got.params == ch.params and got.summary() == s and got.scores_a is None and got.categories is None
    with pytest.raises(ValueError):
        MapChanges(ch.pos_a, ch.pos_b, {**{k: getattr(ch, k) for k in ("vanished", "unseen", "changed_a", "changed", "unseen_b")},
                                        "appeared": np.zeros(6, bool)}, ch.cosine_a, ch.cosine_b, ch.params)


def _change(kind, count, center, category, name="thing"):
    from avlmaps_amd.map.changes import Change
    r, c, h = (int(x) for x in center)
    return Change(kind, count, (r, r, c, c, h, h), tuple(float(x) for x in center), float("nan"), category, name if category >= 0 else "")


def test_moved_pairing_on_hand_made_tables():
    from avlmaps_amd.map.changes import pair_moved
    van = [_change("vanished", 40, (5, 5, 1), 2), _change("vanished", 30, (20, 20, 1), 2), _change("vanished", 10, (9, 9, 1), 1),
           _change("vanished", 50, (1, 1, 1), -1), _change("vanished", 100, (6, 6, 1), 3)]
    app = [_change("appeared", 35, (18, 18, 1), 2), _change("appeared", 60, (6, 5, 1), 2), _change("appeared", 21, (9, 10, 1), 1),
           _change("appeared", 50, (1, 1, 2), -1), _change("appeared", 49, (6, 7, 1), 3)]
    moved, left_v, left_a = pair_moved(van, app)
    # category 2: the nearest pair first (40 at (5, 5) with 60 at (6, 5), within a factor of 2), then 30 at (20, 20) with 35 at (18, 18);
    # category 1: 10 against 21 voxels is more than a factor of 2; no category: never paired; category 3: 100 against 49 is too
    assert [(m.kind, m.from_count, m.count, m.from_center, m.center, m.category) for m in moved] == [
        ("moved", 40, 60, (5.0, 5.0, 1.0), (6.0, 5.0, 1.0), 2), ("moved", 30, 35, (20.0, 20.0, 1.0), (18.0, 18.0, 1.0), 2)]
    assert [v.count for v in left_v] == [10, 50, 100] and [a.count for a in left_a] == [21, 50, 49]
    assert moved[0].bbox == (6, 6, 5, 5, 1, 1) and moved[0].from_bbox == (5, 5, 5, 5, 1, 1) and moved[0].name == "thing"
    # a vanished component is used once: of two appeared candidates the nearer one gets it
    moved, left_v, left_a = pair_moved(van[:1], [_change("appeared", 40, (9, 5, 1), 2), _change("appeared", 40, (7, 5, 1), 2)])
    assert len(moved) == 1 and moved[0].center == (7.0, 5.0, 1.0) and left_v == [] and [a.center for a in left_a] == [(9.0, 5.0, 1.0)]
    assert pair_moved([], app) == ([], [], app) and pair_moved(van, []) == ([], van, [])
    # exactly a factor of 2 still pairs
    moved, _, _ = pair_moved([_change("vanished", 20, (0, 0, 0), 0)], [_change("appeared", 40, (1, 0, 0), 0)])
    assert len(moved) == 1
    d = moved[0].to_json()
    assert d["kind"] == "moved" and d["from_bbox"] == [0, 0, 0, 0, 0, 0] and "mean_cosine" not in d


def _toy_map(gs=16, vh=4, D=8, cs=0.1):
    from avlmaps_amd.apps.common import load_config
    from avlmaps_amd.map import VLMap
    vm = VLMap(load_config(overrides={"map_config.grid_size": gs, "map_config.cell_size": cs}).map_config)
    vm.grid_pos = np.zeros((3, 3), np.int32)
    vm.grid_feat = np.ones((3, D), np.float32)
    vm.occupied_ids = -np.ones((gs, gs, vh), np.int32)
    return vm


def test_compare_raises_unless_the_maps_share_a_grid():
    from avlmaps_amd.map.map import VisibilityAudit
    a = _toy_map()
    for kw in (dict(gs=32), dict(vh=5), dict(D=16), dict(cs=0.05)):
        with pytest.raises(ValueError):
            a.compare(_toy_map(**kw))
    empty = _toy_map()
    empty.grid_feat = None
    with pytest.raises(ValueError):
        a.compare(empty)
    for kw in (dict(radius=3), dict(threshold=0.0), dict(threshold=1.5), dict(shift=(0.5, 0, 0)),
               dict(audit=VisibilityAudit(np.zeros(4, np.int32), np.zeros(4, np.uint32), {}, [1]))):
        with pytest.raises(ValueError):
            a.compare(_toy_map(), **kw)
    assert "rotation" in type(a).compare.__doc__ and "Whole-cell shifts only" in type(a).compare.__doc__


# ------------------------------------------------------------------ the command line
def test_cli_parsing(capsys):
    from avlmaps_amd.apps import audit_map
    args = audit_map.parse_args(["--data-dir", "scene"])
    assert args.compare is None and args.compare_radius == 1 and args.compare_threshold == 0.8 and args.compare_shift == [0, 0, 0]
    assert args.compare_json is None
    args = audit_map.parse_args(["--data-dir", "scene", "--compare", "later", "--compare-radius", "2", "--compare-threshold", "0.6",
                                 "--compare-shift", "1", "-2", "0", "--compare-json", "out.json"])
    assert (args.compare, args.compare_radius, args.compare_threshold, args.compare_shift, args.compare_json) == ("later", 2, 0.6, [1, -2, 0], "out.json")
    for bad in (["--compare-radius", "1"], ["--compare-threshold", "0.5"], ["--compare-shift", "0", "0", "1"], ["--compare-json", "x.json"],
                ["--compare", "later", "--compare-radius", "3"], ["--compare", "later", "--compare-threshold", "0"],
                ["--compare", "later", "--compare-threshold", "1.5"], ["--compare", "later", "--compare-shift", "1", "2"]):
        with pytest.raises(SystemExit):
            audit_map.parse_args(["--data-dir", "scene", *bad])
    capsys.readouterr()
    assert "--compare" in audit_map.__doc__ and "Whole-cell shifts only" in audit_map.__doc__
