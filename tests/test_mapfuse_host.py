"""CPU tests of the map fusion (csrc/avl_mapfuse.hip, ops/mapfuse.py, map/fuse.py, Map.transform_from, apps/audit_map.py --fuse): the
declarations and bindings, the argument checks of the C ABI and of the Python layer, the transform between two recordings' frames,
the masks taken from a MapChanges, the command line and the restatements' own invariants.  No GPU is needed."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

import _mapfuse_ref as R  # noqa: E402

SYMBOLS = {"avl_map_move_cells": 10, "avl_map_fuse_plan": 25, "avl_map_fuse_rows": 25}
SIZE_QUERY = re.compile(r"_(work_bytes|workspace_bytes|ws_bytes)(_n)?$")


# ------------------------------------------------------------------ the library
def test_symbols_are_declared_exported_and_bound_and_none_is_a_size_query():
    from avlmaps_amd import _lib, build
    assert build.SOURCES["avl_mapfuse.hip"] == ["-ffp-contract=off"] and (build.CSRC / "avl_mapfuse.hip").exists()
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
    assert "(31) fusing a revisit into the map" in header and "DESIGN.md 4.33" in header
    source = (build.CSRC / "avl_mapfuse.hip").read_text()
    assert "-ffp-contract=off" in source and "__shared__" not in source         # the source says how fusing is kept out; no LDS


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    lib = _lib.load()
    p, big = 0x1000, 1 << 40
    shift = (C.c_int32 * 3)(0, 0, 0)
    eye = (C.c_double * 16)(*np.eye(4).ravel())
    nan, skew = (C.c_double * 16)(*np.eye(4).ravel()), (C.c_double * 16)(*np.eye(4).ravel())
    nan[6], skew[13] = float("nan"), 0.25

    def move(cells=p, n=5, T=eye, gs=64, cs=0.05, vh=8, out=p, inside=p):
        return lib.avl_map_move_cells(cells, n, T, shift, gs, cs, vh, out, inside, None)
    for over in (dict(T=nan), dict(T=skew), dict(cs=0.0), dict(cs=-1.0), dict(cs=float("inf")), dict(cs=float("nan")), dict(n=-1), dict(gs=0),
                 dict(vh=0), dict(gs=16385, vh=1), dict(cells=None), dict(out=None), dict(inside=None)):
        assert move(**over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_map_move_cells"), over
    assert move(n=0, cells=None, out=None, inside=None) == 0                    # nothing to do touches no pointer

    def plan(ca=p, wa=p, n_a=5, cb=p, wb=p, n_b=7, gs=64, vh=8, index=p, ib=big, sort=p, sb=big, scratch=p, si=9 * 7 + 1024, head=p, a_row=p,
             b_start=p, b_rows=p, oa=p, ob=p, counts=p):
        return lib.avl_map_fuse_plan(ca, None, wa, n_a, cb, None, None, wb, n_b, gs, vh, index, ib, sort, sb, scratch, si, head, a_row, b_start, b_rows,
                                     oa, ob, counts, None)
    for over in (dict(n_a=-1), dict(n_b=-1), dict(n_a=2 ** 30, n_b=2 ** 30), dict(gs=0), dict(vh=0), dict(index=None), dict(ib=16), dict(sb=16),
                 dict(sort=None), dict(scratch=None), dict(scratch=p + 4), dict(si=9 * 7 + 1023), dict(head=None), dict(a_row=None), dict(b_start=None),
                 dict(b_rows=None), dict(oa=None), dict(ob=None), dict(counts=None), dict(ca=None), dict(wa=None), dict(cb=None), dict(wb=None)):
        assert plan(**over) != 0, over
        assert lib.avl_last_error().startswith((b"avl_map_fuse_plan", b"avl_argsort_bits")), over

    def rows(n_out=4, a_row=p, b_start=p, b_rows=p, fa=p, n_a=5, fb=p, n_b=7, D=16, g_a=1.0, g_b=1.0, gs=64, vh=8, out=p, w=p, rgb=p, pos=p):
        return lib.avl_map_fuse_rows(n_out, a_row, b_start, b_rows, fa, p, p, p, n_a, fb, p, p, p, n_b, D, g_a, g_b, gs, vh, out, w, rgb, pos, None, None)
    for over in (dict(D=0), dict(D=8193), dict(g_a=0.0), dict(g_b=-1.0), dict(g_b=float("nan")), dict(g_a=float("inf")), dict(n_out=-1),
                 dict(n_out=13), dict(n_a=-1), dict(gs=0), dict(a_row=None), dict(b_start=None), dict(b_rows=None), dict(fa=None), dict(fb=None),
                 dict(out=None), dict(w=None), dict(rgb=None), dict(pos=None)):
        assert rows(**over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_map_fuse_rows"), over
    assert rows(n_out=0, a_row=None, b_start=None, out=None, w=None, rgb=None, pos=None) == 0


def test_python_layer_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import ops
    cells = np.zeros((4, 3), np.int32)
    projective = np.eye(4)
    projective[3, 0] = 1.0
    bad_T = [np.eye(3), np.full((4, 4), np.nan), np.diag([1.0, 1.0, 1.0, 2.0]), projective]
    for over in [dict(transform=T) for T in bad_T] + [dict(shift=(0, 0)), dict(shift=(0.5, 0, 0)), dict(cs=0.0), dict(cs=float("nan")), dict(gs=0),
                                                      dict(vh=0), dict(cells=np.zeros((4, 2), np.int32))]:
        kw = dict(cells=cells, gs=16, cs=0.1, vh=4)
        kw.update(over)
        with pytest.raises(ValueError):
            ops.move_cells(**kw)
    with pytest.raises(TypeError):
        ops.move_cells(np.zeros((4, 3), np.float32), 16, 0.1, 4)

    def args(n_a=3, n_b=2, D=8):
        return dict(pos_a=np.zeros((n_a, 3), np.int32), feat_a=np.ones((n_a, D), np.float32), w_a=np.ones(n_a, np.float32),
                    rgb_a=np.zeros((n_a, 3), np.uint8), pos_b=np.zeros((n_b, 3), np.int32), feat_b=np.ones((n_b, D), np.float32),
                    w_b=np.ones(n_b, np.float32), rgb_b=np.zeros((n_b, 3), np.uint8), gs=16, cs=0.1, vh=4)
    base = args()
    value = [dict(feat_b=np.ones((2, 9), np.float32)), dict(feat_a=np.ones((4, 8), np.float32)), dict(feat_a=np.ones((3, 0), np.float32)),
             dict(feat_a=np.ones((3, 8193), np.float32), feat_b=np.ones((2, 8193), np.float32)), dict(w_a=np.ones(4, np.float32)),
             dict(rgb_b=np.zeros((2, 4), np.uint8)), dict(use_a=np.ones(4, bool)), dict(use_b=np.ones((2, 1), bool)), dict(gain_a=0.0), dict(gain_b=-1.0),
             dict(gain_b=float("nan")), dict(gain_a=float("inf")), dict(transform=np.full((4, 4), np.inf)), dict(transform=np.diag([1.0, 1.0, 1.0, 0.5])),
             dict(shift=(1, 2)), dict(cs=-0.1), dict(gs=0), dict(pos_b=np.zeros((2, 2), np.int32))]
    for over in value:
        with pytest.raises(ValueError):
            ops.fuse_maps(**{**base, **over})
    for over in (dict(feat_a=np.ones((3, 8), np.float64)), dict(w_b=np.ones(2, np.float64)), dict(rgb_a=np.zeros((3, 3), np.int32)),
                 dict(use_a=np.ones(3, np.float32)), dict(pos_a=np.zeros((3, 3), np.float32))):
        with pytest.raises(TypeError):
            ops.fuse_maps(**{**base, **over})
    with pytest.raises(TypeError):
        ops.fuse_rows(object(), *(base[k] for k in ("feat_a", "w_a", "rgb_a", "feat_b", "w_b", "rgb_b")))
    with pytest.raises(ValueError):
        ops.fuse_plan(base["pos_a"], base["w_a"], base["pos_b"], np.ones(3, np.float32), 16, 4)
    with pytest.raises(ValueError):
        ops.fuse_plan(base["pos_a"], base["w_a"], base["pos_b"], base["w_b"], 16, 4, inside_b=np.ones(3, np.uint8))
    assert ops.check_gain(0.25, "x") == 0.25 and ops.check_transform(None, "x") is None
    assert ops.FUSE_COUNTS == ("dropped_a", "unselected_b", "outside_b", "merged_b", "new_cells", "shared_b")


# ------------------------------------------------------------------ the map layer
def _config(gs=16):
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": gs, "map_config.cell_size": 0.1}).map_config


def _poses(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([rng.uniform(-2, 2, (n, 3)), q], axis=1)


def test_transform_from_carries_every_frame_of_the_other_recording_into_this_maps_frame(tmp_path):
    from avlmaps_amd.map import VLMap
    rng = np.random.default_rng(4)
    for name, n in (("a", 3), ("b", 6)):
        (tmp_path / name / "depth").mkdir(parents=True)
        np.savetxt(tmp_path / name / "poses.txt", _poses(rng, n))
        for k in range(n):
            (tmp_path / name / "depth" / f"{k:06d}.npy").touch()        # listed, never read: the transforms come from poses.txt
    vm = VLMap(_config(), data_dir=str(tmp_path / "a"))
    S = vm.transform_from(tmp_path / "b")
    own = vm._audit_frames(tmp_path / "b")[1]
    here = vm._audit_frames(tmp_path / "b", vm._own_first_pose())[1]
    assert S.shape == (4, 4) and S.dtype == np.float64 and S[3].tolist() == [0, 0, 0, 1] and len(own) == len(here) == 6
    for i in range(6):
        assert np.abs(S @ own[i] - here[i]).max() <= 1e-12, i
    assert np.abs(S - np.eye(4)).max() > 1e-3
    # a registration's correction is left-multiplied; a map without a scene of its own shares the directory's frame
    turn = np.eye(4)
    turn[:2, :2], turn[0, 3] = [[0, -1], [1, 0]], 0.3

    class Reg:
        correction = turn
    assert np.abs(vm.transform_from(tmp_path / "b", registration=Reg()) - turn @ S).max() <= 1e-12
    assert np.abs(VLMap(_config()).transform_from(tmp_path / "b") - np.eye(4)).max() <= 1e-12


def _changes(n_a=6, n_b=5, shift=(0, 0, 0)):
    from avlmaps_amd.map.changes import MapChanges
    masks = dict(vanished=[1, 0, 0, 0, 0, 0], unseen=[0, 1, 0, 0, 0, 0], changed_a=[0, 0, 1, 1, 0, 0], appeared=[1, 0, 0, 0, 0], changed=[0, 1, 1, 0, 0],
                 unseen_b=[0, 0, 0, 0, 1])
    return MapChanges(np.zeros((n_a, 3)), np.zeros((n_b, 3)), {k: np.array(v, bool) for k, v in masks.items()}, np.zeros(n_a), np.zeros(n_b),
                      dict(gs=16, cs=0.1, vh=4, radius=1, threshold=0.8, shift=shift, min_rays=3))


def test_masks_from_a_map_changes():
    from avlmaps_amd.map.fuse import fuse_masks
    ch = _changes()
    use_a, use_b = fuse_masks(ch)
    assert use_a.tolist() == [False, True, False, False, True, True] and use_b.tolist() == [True, True, True, True, False]
    assert fuse_masks(ch, drop_vanished=False)[0].tolist() == [True, True, False, False, True, True]
    assert fuse_masks(ch, replace_changed=False)[0].tolist() == [False, True, True, True, True, True]
    assert fuse_masks(ch, False, False)[0].all() and use_a.dtype == bool
    with pytest.raises(TypeError):
        fuse_masks(dict(vanished=[]))


def test_fuse_and_resample_check_their_maps_before_any_device_work():
    from avlmaps_amd.map import VLMap

    def toy(n, D=8, gs=16, vh=4):
        vm = VLMap(_config(gs))
        vm.grid_pos, vm.grid_feat = np.zeros((n, 3), np.int32), np.ones((n, D), np.float32)
        vm.weight, vm.grid_rgb, vm.occupied_ids = np.ones(n, np.float32), np.zeros((n, 3), np.uint8), -np.ones((gs, gs, vh), np.int32)
        return vm
    a, b = toy(6), toy(5)
    for other in (toy(5, D=9), toy(5, gs=18), toy(5, vh=5), VLMap(_config())):
        with pytest.raises(ValueError):
            a.fuse(other)
    for kw in (dict(gain=0.0), dict(gain=float("nan")), dict(transform=np.full((4, 4), np.nan)), dict(transform=np.diag([1.0, 1, 1, 2])),
               dict(shift=(0, 0)), dict(changes=_changes(), transform=np.eye(4)), dict(changes=_changes(), shift=(1, 0, 0)),
               dict(changes=_changes(shift=(1, 0, 0))), dict(gain=-2)):
        with pytest.raises(ValueError):
            a.fuse(b, **kw)
    with pytest.raises(ValueError):
        toy(7).fuse(b, changes=_changes())                          # the changes are of 6 and 5 voxels
    with pytest.raises(TypeError):
        a.fuse(b, changes=object())
    with pytest.raises(ValueError):
        a.resample(transform=np.full((4, 4), np.inf))
    with pytest.raises(ValueError):
        VLMap(_config()).resample()
    assert len(a.grid_pos) == 6 and a._drop_derived() is None


def test_cli_parsing(capsys, tmp_path):
    from avlmaps_amd.apps import audit_map
    args = audit_map.parse_args(["--data-dir", "scene"])
    assert args.fuse is None and args.fuse_out is None and args.fuse_gain == 1.0 and not args.fuse_keep_vanished and not args.fuse_keep_changed
    args = audit_map.parse_args(["--data-dir", "scene", "--fuse", "later", "--fuse-out", "both", "--register", "--fuse-keep-vanished",
                                 "--fuse-keep-changed", "--fuse-gain", "2.5", "--fuse-json", "f.json", "--compare-radius", "2"])
    assert (args.fuse, args.fuse_out, args.register, args.fuse_keep_vanished, args.fuse_keep_changed, args.fuse_gain, args.fuse_json) == \
        ("later", "both", True, True, True, 2.5, "f.json") and args.compare_radius == 2 and args.compare is None
    for bad in (["--fuse", "later"], ["--fuse-out", "both"], ["--fuse-gain", "2"], ["--fuse-keep-vanished"], ["--fuse-keep-changed"],
                ["--fuse-json", "f.json"], ["--fuse", "later", "--fuse-out", "later"], ["--fuse", "later", "--fuse-out", "scene"],
                ["--fuse", "later", "--fuse-out", "./scene/"], ["--fuse", "later", "--fuse-out", "both", "--fuse-gain", "0"],
                ["--fuse", "later", "--fuse-out", "both", "--fuse-gain", "nan"], ["--fuse", "later", "--fuse-out", "both", "--fuse-gain", "-1"]):
        with pytest.raises(SystemExit):
            audit_map.parse_args(["--data-dir", "scene", *bad])
    capsys.readouterr()
    assert "--fuse" in audit_map.__doc__ and "no input map is written over" in audit_map.__doc__


# ------------------------------------------------------------------ the restatements
def test_the_restatements_keep_their_own_invariants():
    rng = np.random.default_rng(9)
    gs, vh, D = 12, 6, 5
    every = np.stack(np.meshgrid(np.arange(gs), np.arange(gs), np.arange(vh), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    cells_a = every[rng.choice(len(every), 120, replace=False)]
    cells_b = np.concatenate([cells_a[rng.integers(0, 120, 60)], every[rng.integers(0, len(every), 90)], [[gs, 0, 0], [0, -1, 0]]]).astype(np.int32)
    w_a, w_b = rng.uniform(0.1, 9, 120).astype(np.float32), rng.uniform(0.1, 9, 152).astype(np.float32)
    w_a[::11], w_b[::13] = 0, np.nan
    use_a, use_b = rng.random(120) < 0.8, rng.random(152) < 0.8
    plan = R.ref_fuse_plan(cells_a, w_a, cells_b, w_b, gs, vh, None, use_a, use_b)
    sel_a = use_a & np.isfinite(w_a) & (w_a > 0)
    sel_b = use_b & np.isfinite(w_b) & (w_b > 0) & ((cells_b >= 0) & (cells_b < [gs, gs, vh])).all(1)
    wanted_b = use_b & np.isfinite(w_b) & (w_b > 0)
    assert plan["error"] == 0 and plan["counts"][0] == (~sel_a).sum() and plan["counts"][1:].sum() == 152
    assert plan["counts"][1] == (~wanted_b).sum() and plan["counts"][2] == (wanted_b & ~sel_b).sum() == wanted_b[-2:].sum()
    feat_a, feat_b = rng.standard_normal((120, D)).astype(np.float32), rng.standard_normal((152, D)).astype(np.float32)
    rgb_a, rgb_b = rng.integers(0, 256, (120, 3)).astype(np.uint8), rng.integers(0, 256, (152, 3)).astype(np.uint8)
    pos, feat, weight, rgb, occ = R.ref_fuse_rows(plan, cells_a, feat_a, w_a, rgb_a, cells_b, feat_b, w_b, rgb_b, gs, vh, 1.0, 0.5)
    # the output cells are the union of the selected cells, each once, and occupied_ids names them
    union = {tuple(c) for c in cells_a[sel_a].tolist()} | {tuple(c) for c in cells_b[sel_b].tolist()}
    assert len(pos) == plan["n_out"] == len(union) and {tuple(c) for c in pos.tolist()} == union
    assert np.array_equal(occ[tuple(pos.T)], np.arange(len(pos))) and (occ >= 0).sum() == len(pos)
    assert np.array_equal(pos[:sel_a.sum()], cells_a[sel_a]) and np.array_equal(plan["out_of_a"] >= 0, sel_a) and np.array_equal(plan["out_of_b"] >= 0, sel_b)
    # W is the sum of the member weights, a voxel's row lies within its members' range, a sole member comes back as it is
    for v in range(plan["n_out"]):
        members_b = plan["b_rows"][plan["b_start"][v]:plan["b_start"][v + 1]]
        ws = ([float(w_a[plan["a_row"][v]])] if plan["a_row"][v] >= 0 else []) + [0.5 * float(w) for w in w_b[members_b]]
        fs = ([feat_a[plan["a_row"][v]]] if plan["a_row"][v] >= 0 else []) + [feat_b[j] for j in members_b]
        assert abs(float(weight[v]) - sum(ws)) <= 1e-6 * sum(ws) and (plan["out_of_b"][members_b] == v).all() and list(members_b) == sorted(members_b)
        assert (feat[v] >= np.min(fs, axis=0) - 1e-6).all() and (feat[v] <= np.max(fs, axis=0) + 1e-6).all()
        if len(fs) == 1 and plan["a_row"][v] >= 0:
            assert feat[v].tobytes() == fs[0].tobytes() and weight[v] == w_a[plan["a_row"][v]] and rgb[v].tobytes() == rgb_a[plan["a_row"][v]].tobytes()
    # the move: identity and a pure shift
    moved, inside = R.ref_move_cells(every, gs, 0.05, vh, np.eye(4))
    assert np.array_equal(moved, every) and inside.all()
    moved, inside = R.ref_move_cells(every, gs, 0.05, vh, None, (1, 0, -1))
    ok = (every[:, 0] + 1 < gs) & (every[:, 2] - 1 >= 0)
    assert np.array_equal(inside.astype(bool), ok) and np.array_equal(moved[ok], every[ok] + [1, 0, -1]) and (moved[~ok] == -1).all()
