"""CPU tests of the backward resampling of a voxel map (csrc/avl_mappull.hip, ops/mappull.py, VLMap.resample's method, apps/audit_map.py
--fuse-resample): the declarations and bindings, the argument checks of the C ABI and of the Python layer, the command line and the
restatement's own invariants.  No GPU is needed."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

import _mappull_ref as R  # noqa: E402

SYMBOLS = {"avl_map_pull_plan": 17, "avl_map_pull_fill": 20, "avl_map_pull_rows": 12}
SIZE_QUERY = re.compile(r"_(work_bytes|workspace_bytes|ws_bytes)(_n)?$")


# ------------------------------------------------------------------ the library
def test_symbols_are_declared_exported_and_bound_and_none_is_a_size_query():
    from avlmaps_amd import _lib, build
    assert build.SOURCES["avl_mappull.hip"] == ["-ffp-contract=off"] and (build.CSRC / "avl_mappull.hip").exists()
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
    assert not [s for s in _lib.EXPORTED_SYMBOLS if s.startswith("avl_map_pull") and SIZE_QUERY.search(s)]
    assert "(32) resampling a finished voxel map backward" in header and "DESIGN.md 4.34" in header
    assert header.index("(31) fusing a revisit") < header.index("(32) resampling a finished")
    source = (build.CSRC / "avl_mappull.hip").read_text()
    assert "-ffp-contract=off" in source and '#include "avl_mapfuse.h"' in source
    rows = source[source.index("void pl_rows_kernel"):source.index("static int pl_check")]
    assert "__shared__" not in rows and "__shfl" not in rows                    # the hot kernel: no LDS, no cross-lane step
    # the forward source shares the helpers through the header and keeps none of its own
    forward = (build.CSRC / "avl_mapfuse.hip").read_text()
    assert '#include "avl_mapfuse.h"' in forward and "struct MfAcc" not in forward and "struct MfAcc" in (build.CSRC / "avl_mapfuse.h").read_text()


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    lib = _lib.load()
    p, big = 0x1000, 1 << 40
    shift = (C.c_int32 * 3)(0, 0, 0)
    eye = (C.c_double * 16)(*np.eye(4).ravel())
    nan, skew = (C.c_double * 16)(*np.eye(4).ravel()), (C.c_double * 16)(*np.eye(4).ravel())
    nan[6], skew[13] = float("nan"), 0.25
    need = 4 * 7 + 2 * 1024 + 1 + 512                                           # 64 x 64 x 8 cells are 1024 words

    def plan(cells=p, w=p, n_b=7, P=eye, gs=64, cs=0.05, vh=8, mode=1, support=0.5, index=p, ib=big, scratch=p, si=need, head=p):
        return lib.avl_map_pull_plan(cells, None, w, n_b, P, shift, gs, cs, vh, mode, support, index, ib, scratch, si, head, None)
    for over in (dict(P=nan), dict(P=skew), dict(cs=0.0), dict(cs=-1.0), dict(cs=float("inf")), dict(cs=float("nan")), dict(n_b=-1), dict(gs=0),
                 dict(vh=0), dict(gs=16385, vh=1), dict(mode=2), dict(mode=-1), dict(support=0.0), dict(support=1.5), dict(support=float("nan")),
                 dict(support=-0.5), dict(cells=None), dict(w=None), dict(index=None), dict(ib=16), dict(scratch=None), dict(si=need - 1), dict(head=None)):
        assert plan(**over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_map_pull_plan"), over

    def fill(n_b=7, P=eye, gs=64, cs=0.05, vh=8, mode=1, support=0.5, index=p, ib=big, scratch=p, si=need, head=p, n_out=5, cells=p, members=p, lam=p,
             counts=p):
        return lib.avl_map_pull_fill(n_b, P, shift, gs, cs, vh, mode, support, index, ib, scratch, si, head, n_out, cells, members, lam, None, counts, None)
    for over in (dict(P=nan), dict(P=skew), dict(cs=0.0), dict(n_b=-1), dict(gs=0), dict(vh=0), dict(mode=2), dict(support=0.0), dict(support=2.0),
                 dict(index=None), dict(ib=16), dict(scratch=None), dict(si=need - 1), dict(head=None), dict(n_out=-1), dict(n_out=64 * 64 * 8 + 1),
                 dict(cells=None), dict(members=None), dict(lam=None), dict(counts=None)):
        assert fill(**over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_map_pull_fill"), over

    def rows(n_out=4, members=p, lam=p, fb=p, w=p, rgb=p, n_b=7, D=16, out=p, wout=p, rgb_out=p):
        return lib.avl_map_pull_rows(n_out, members, lam, fb, w, rgb, n_b, D, out, wout, rgb_out, None)
    for over in (dict(D=0), dict(D=8193), dict(n_out=-1), dict(n_b=-1), dict(n_out=2 ** 31 - 1), dict(members=None), dict(lam=None), dict(lam=p + 4),
                 dict(fb=None), dict(w=None), dict(rgb=None), dict(out=None), dict(wout=None), dict(rgb_out=None)):
        assert rows(**over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_map_pull_rows"), over
    assert rows(n_out=0, members=None, lam=None, out=None, wout=None, rgb_out=None) == 0      # nothing to do touches no pointer


def test_python_layer_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import ops
    projective, singular, flat = np.eye(4), np.eye(4), np.eye(4)
    projective[3, 0], singular[1, 1], flat[:3, :3] = 1.0, 0.0, [[1, 2, 3], [2, 4, 6], [0, 0, 1]]

    def args(n_b=3, D=8):
        return dict(pos_b=np.zeros((n_b, 3), np.int32), feat_b=np.ones((n_b, D), np.float32), w_b=np.ones(n_b, np.float32),
                    rgb_b=np.zeros((n_b, 3), np.uint8), gs=16, cs=0.1, vh=4)
    base = args()
    value = [dict(transform=np.eye(3)), dict(transform=np.full((4, 4), np.nan)), dict(transform=np.diag([1.0, 1.0, 1.0, 2.0])), dict(transform=projective),
             dict(transform=singular), dict(transform=flat), dict(transform=np.zeros((4, 4)) + np.diag([0, 0, 0, 1.0])), dict(shift=(0, 0)),
             dict(shift=(0.5, 0, 0)), dict(cs=0.0), dict(cs=float("nan")), dict(gs=0), dict(vh=0), dict(interp="cubic"), dict(interp=None),
             dict(interp="forward"), dict(min_support=0.0), dict(min_support=1.01), dict(min_support=float("nan")), dict(min_support=-1),
             dict(pos_b=np.zeros((3, 2), np.int32)), dict(feat_b=np.ones((4, 8), np.float32)), dict(feat_b=np.ones((3, 0), np.float32)),
             dict(feat_b=np.ones((3, 8193), np.float32)), dict(w_b=np.ones(4, np.float32)), dict(rgb_b=np.zeros((3, 4), np.uint8)),
             dict(use_b=np.ones(4, bool)), dict(use_b=np.ones((3, 1), bool))]
    for over in value:
        with pytest.raises(ValueError):
            ops.pull_map(**{**base, **over})
    for over in (dict(feat_b=np.ones((3, 8), np.float64)), dict(w_b=np.ones(3, np.float64)), dict(rgb_b=np.zeros((3, 3), np.int32)),
                 dict(use_b=np.ones(3, np.float32)), dict(pos_b=np.zeros((3, 3), np.float32))):
        with pytest.raises(TypeError):
            ops.pull_map(**{**base, **over})
    plan_kw = dict(cells_b=base["pos_b"], w_b=base["w_b"], gs=16, cs=0.1, vh=4)
    for over in (dict(transform=singular), dict(interp="cubic"), dict(min_support=0), dict(w_b=np.ones(4, np.float32)), dict(use_b=np.ones(2, bool)),
                 dict(shift=(1, 2)), dict(cs=-0.1), dict(gs=0), dict(cells_b=np.zeros((3, 4), np.int32))):
        with pytest.raises(ValueError):
            ops.pull_plan(**{**plan_kw, **over})
    with pytest.raises(TypeError):
        ops.pull_rows(object(), base["feat_b"], base["w_b"], base["rgb_b"])
    assert ops.PULL_COUNTS == ("unselected_b", "outside_b", "below_support", "unused_b") and ops.PULL_INTERP == ("nearest", "linear")
    assert ops.check_min_support(1, "x") == 1.0 and ops.check_interp("linear", "x") == 1 and ops.inverse_transform(None, "x") is None
    # the inverse: float64, bottom row exact, P T = 1
    T = np.eye(4)
    a = np.radians(10.0)
    T[:2, :2], T[:3, 3] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], (0.3, -0.2, 0.1)
    P = ops.inverse_transform(T, "x")
    assert P.dtype == np.float64 and P.flags.c_contiguous and P[3].tolist() == [0, 0, 0, 1] and np.abs(P @ T - np.eye(4)).max() <= 1e-15


# ------------------------------------------------------------------ the map layer and the app
def _config(gs=16):
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": gs, "map_config.cell_size": 0.1}).map_config


def test_resample_checks_its_method_before_any_device_work():
    import inspect
    from avlmaps_amd.map import VLMap
    vm = VLMap(_config())
    gs, vh, n = 16, 4, 6
    vm.grid_pos, vm.grid_feat = np.zeros((n, 3), np.int32), np.ones((n, 8), np.float32)
    vm.weight, vm.grid_rgb, vm.occupied_ids = np.ones(n, np.float32), np.zeros((n, 3), np.uint8), -np.ones((gs, gs, vh), np.int32)
    singular = np.diag([1.0, 0.0, 1.0, 1.0])
    for kw in (dict(method="cubic"), dict(method=None), dict(method="linear", min_support=0.0), dict(method="nearest", min_support=2.0),
               dict(method="linear", transform=singular), dict(method="nearest", transform=np.full((4, 4), np.inf)), dict(method="linear", shift=(0, 0))):
        with pytest.raises(ValueError):
            vm.resample(**kw)
    with pytest.raises(ValueError):
        VLMap(_config()).resample(method="linear")                  # no map
    sig = inspect.signature(VLMap.resample)
    assert sig.parameters["method"].default == "forward" and sig.parameters["min_support"].default == 0.5
    assert list(sig.parameters)[:3] == ["self", "transform", "shift"]
    for doc in (VLMap.resample.__doc__, VLMap.fuse.__doc__, VLMap.compare.__doc__):
        assert 'method="linear"' in doc and "nearest" in doc and "object" in doc
    assert "order the voxels by linear cell" in " ".join(VLMap.resample.__doc__.split())


def test_cli_parsing(capsys):
    from avlmaps_amd.apps import audit_map
    fuse = ["--data-dir", "scene", "--fuse", "later", "--fuse-out", "both"]
    args = audit_map.parse_args(fuse)
    assert args.fuse_resample == "forward" and args.fuse_min_support == 0.5                      # today's outputs stay
    args = audit_map.parse_args(["--data-dir", "scene"])
    assert args.fuse is None and args.fuse_resample == "forward"
    args = audit_map.parse_args([*fuse, "--fuse-resample", "linear", "--fuse-min-support", "0.25"])
    assert args.fuse_resample == "linear" and args.fuse_min_support == 0.25
    assert audit_map.parse_args([*fuse, "--fuse-resample", "nearest"]).fuse_resample == "nearest"
    assert audit_map.parse_args([*fuse, "--fuse-resample", "linear"]).fuse_min_support == 0.5
    for bad in (["--data-dir", "scene", "--fuse-resample", "linear"], ["--data-dir", "scene", "--fuse-min-support", "0.5"],
                [*fuse, "--fuse-resample", "cubic"], [*fuse, "--fuse-min-support", "0.5"], [*fuse, "--fuse-resample", "nearest", "--fuse-min-support", "0.5"],
                [*fuse, "--fuse-resample", "linear", "--fuse-min-support", "0"], [*fuse, "--fuse-resample", "linear", "--fuse-min-support", "1.5"],
                [*fuse, "--fuse-resample", "linear", "--fuse-min-support", "nan"], [*fuse, "--fuse-resample"]):
        with pytest.raises(SystemExit):
            audit_map.parse_args(bad)
    capsys.readouterr()
    assert "--fuse-resample" in audit_map.__doc__ and "--fuse-min-support" in audit_map.__doc__ and "DESIGN.md 4.34" in audit_map.__doc__


# ------------------------------------------------------------------ the restatement
def test_the_lattice_rule_maps_every_centre_back_to_its_cell():
    """a few float64 roundings of s = x / cs near 10^4 stay far below 1e-9"""
    for cs in (0.025, 0.05, 0.1):
        for k in range(-10000, 10001):
            k0, t = R.bracket(R.centre(k, cs) / cs)
            assert (k0 == k and t <= 1e-9) or (k0 == k - 1 and 1.0 - t <= 1e-9), (cs, k, k0, t)
    for cs in (0.025, 0.05, 0.1):
        for h in range(0, 200):
            h0, t = R.bracket_h((h + 0.5) * cs / cs)
            assert (h0 == h and t <= 1e-9) or (h0 == h - 1 and 1.0 - t <= 1e-9), (cs, h, h0, t)
    # between two centres the fraction is the share of the way, also across the double-width cell
    assert R.bracket(0.75) == (0, 0.5) and R.bracket(-0.75) == (-1, 0.5) and R.bracket(2.0) == (1, 0.5) and R.bracket(-2.0) == (-2, 0.5)
    assert R.bracket(0.0) == (0, 0.0) and R.bracket(-0.0) == (0, 0.0) and R.bracket(-1.5) == (-1, 0.0) and R.bracket(1.5) == (1, 0.0)


def test_the_corner_weights_add_up_to_one_and_a_solid_block_has_full_support():
    rng = np.random.default_rng(2)
    for q in rng.uniform(-40, 40, (2000, 3)):
        cs_ = R.corners(q[0], q[1], q[2], 33)
        assert abs(sum(l for _, l in cs_) - 1.0) <= 1e-12 and all(0.0 <= l <= 1.0 for _, l in cs_) and len({c for c, _ in cs_}) == 8
    # corner order: dz is the lowest bit, then dy, then dx
    cells = [c for c, _ in R.corners(2.25, 3.25, 4.25, 33)]
    assert cells[0] == (16 - 1, 16 - 2, 3) and cells[1] == (16 - 1, 16 - 2, 4) and cells[2] == (16 - 1, 16 - 3, 3) and cells[4] == (16 - 2, 16 - 2, 3)
    # inside a solid block every corner is a member: the support is 1 whatever the transform
    gs, vh, cs = 33, 10, 0.05
    block = np.array([(r, c, h) for r in range(2, 31) for c in range(2, 31) for h in range(10)], np.int32)
    a = np.radians(30.0)
    T = np.eye(4)
    T[:2, :2], T[:3, 3] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], (0.013, -0.02, 0.0)
    P = np.linalg.inv(T)
    P[3] = [0, 0, 0, 1]
    plan = R.ref_pull_plan(block, np.ones(len(block), np.float32), gs, cs, vh, P, interp="linear", min_support=1.0 - 1e-12)
    inner = (np.abs(plan["cells"][:, :2] - 16).max(1) <= 8) & (plan["cells"][:, 2] >= 1) & (plan["cells"][:, 2] <= 8)
    assert inner.sum() == 17 * 17 * 8
    assert (np.abs(plan["lam"][inner].sum(1) - 1.0) <= 1e-12).all() and ((plan["members"][inner] >= 0) | (plan["lam"][inner] == 0)).all()


def test_the_restatement_keeps_its_own_invariants():
    rng = np.random.default_rng(9)
    gs, vh, D = 12, 6, 5
    every = np.stack(np.meshgrid(np.arange(gs), np.arange(gs), np.arange(vh), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    cells = np.concatenate([every[rng.choice(len(every), 150, replace=False)], [[gs, 0, 0], [0, -1, 0]]]).astype(np.int32)
    w = rng.uniform(0.1, 9, 152).astype(np.float32)
    w[::13] = np.nan
    use = rng.random(152) < 0.8
    sel = use & np.isfinite(w) & (w > 0)
    inside = ((cells >= 0) & (cells < [gs, gs, vh])).all(1)
    feat, rgb = rng.standard_normal((152, D)).astype(np.float32), rng.integers(0, 256, (152, 3)).astype(np.uint8)
    # without a transform: the selected rows, in linear cell order, bit for bit, in both modes
    for interp in ("nearest", "linear"):
        plan = R.ref_pull_plan(cells, w, gs, 0.05, vh, None, (0, 0, 0), use, interp)
        rows = plan["members"][:, 0]
        lin = (cells[:, 0] * gs + cells[:, 1]) * vh + cells[:, 2]
        want = np.flatnonzero(sel & inside)
        want = want[np.argsort(lin[want])]
        assert np.array_equal(rows, want) and (plan["members"][:, 1:] == -1).all() and np.array_equal(plan["cells"], cells[want])
        assert plan["counts"].tolist() == [(~sel).sum(), (sel & ~inside).sum(), 0, 0]
        assert np.array_equal(plan["occupied"][tuple(plan["cells"].T)], np.arange(plan["n_out"])) and (plan["occupied"] >= 0).sum() == plan["n_out"]
        f, wt, c = R.ref_pull_rows(plan, feat, w, rgb)
        assert f.tobytes() == feat[want].tobytes() and wt.tobytes() == w[want].tobytes() and c.tobytes() == rgb[want].tobytes()
    # a shift moves the cells and drops what leaves the grid; the identity as a matrix changes nothing in nearest mode
    plan = R.ref_pull_plan(cells, w, gs, 0.05, vh, None, (1, 0, -1), use)
    moved = cells[plan["members"][:, 0]] + [1, 0, -1]
    assert np.array_equal(plan["cells"], moved) and plan["counts"][3] == (sel & inside).sum() - plan["n_out"] > 0
    near = R.ref_pull_plan(cells, w, gs, 0.05, vh, np.eye(4), (0, 0, 0), use, "nearest")
    assert np.array_equal(near["members"], R.ref_pull_plan(cells, w, gs, 0.05, vh, None, (0, 0, 0), use)["members"])
    # linear under a rotation: a voxel lies within its members' range and its weight within theirs
    a = np.radians(10.0)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    P = np.linalg.inv(T)
    P[3] = [0, 0, 0, 1]
    plan = R.ref_pull_plan(cells, w, gs, 0.05, vh, P, (0, 0, 0), use, "linear", 0.25)
    f, wt, c = R.ref_pull_rows(plan, feat, w, rgb)
    assert plan["n_out"] > 0 and plan["counts"][2] > 0 and (np.diff((plan["cells"][:, 0] * gs + plan["cells"][:, 1]) * vh + plan["cells"][:, 2]) > 0).all()
    for v in range(plan["n_out"]):
        m = plan["members"][v][plan["members"][v] >= 0]
        assert len(m) and sel[m].all() and plan["lam"][v][plan["members"][v] >= 0].sum() >= 0.25
        assert (f[v] >= feat[m].min(0) - 1e-6).all() and (f[v] <= feat[m].max(0) + 1e-6).all() and w[m].min() * (1 - 1e-6) <= wt[v] <= w[m].max() * (1 + 1e-6)
    with pytest.raises(ValueError):
        R.ref_pull_plan(np.array([(1, 1, 1), (2, 2, 2), (1, 1, 1)]), np.ones(3, np.float32), gs, 0.05, vh)
    assert R.pinholes(np.array([(1, 0, 0), (0, 1, 0), (2, 1, 0), (1, 2, 0)]), 4, 1) == 1 and R.pinholes(np.array([(1, 0, 0), (0, 1, 0), (2, 1, 0)]), 4, 1) == 0
