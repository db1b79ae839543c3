"""CPU tests of the correlative pose search (csrc/avl_match.hip, ops/match.py, Map.register_frames, Map.audit_visibility's
corrections, apps.audit_map --register): the restatement's own properties, the C ABI's and the Python layer's argument checks, and
the host-side map layer on the restatement.  No GPU is needed."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from oracle import avl_oracle as O  # noqa: E402

import _audit_ref as A  # noqa: E402
import _match_ref as M  # noqa: E402

SYMBOLS = ("avl_match_ws_bytes", "avl_match_frames")


def _angles(max_deg, step_deg):
    from avlmaps_amd import ops
    return ops.match_angles(max_deg, step_deg)


# ------------------------------------------------------------------ the restatement
def test_the_zero_angle_at_shift_zero_gives_the_builders_cells():
    depth, Ts = M.scene(2)
    vh, stride = 8, 1
    Kinv = np.linalg.inv(M.K)
    for f in range(2):
        # the builder's own chain, point by point: depth2pc, transform_pc, base_pos2grid_id_3d, its range rule
        lat = M.lattice(M.H, M.W, stride)
        pcs, ok = O.depth2pc_pixels(depth[f], Kinv, [v * M.W + u for v, u in lat], **M.DEPTHS)
        built = [tuple(O.base_pos2grid_id_3d(M.GS, M.CS, *g)) for g in O.transform_points(Ts[f], pcs)[ok]]
        (points, (px, py)), = M.volumes(depth[f], M.K, Ts[f], M.CS, vh, stride, h_band=(0, None), **M.DEPTHS)
        assert (px, py) == (Ts[f, 0, 3], Ts[f, 1, 3])
        cells = M.cells_of(points, 1.0, 0.0, px, py, M.GS, M.CS, 64)
        assert sorted(map(tuple, cells.tolist())) == sorted(c for c in built if 0 <= c[2] < vh and -64 <= c[0] < M.GS + 64 and -64 <= c[1] < M.GS + 64)
        # and a map of the builder's voxels scores every point that the builder fused, at the zero angle and shift
        pos = np.array([c for c in built if 0 <= c[0] < M.GS and 0 <= c[1] < M.GS and 0 <= c[2] < vh], np.int32)
        scores, best, valid = M.match_ref(pos, M.GS, vh, depth[f], M.K, Ts[f], M.CS, _angles(4, 2), 2, stride=stride, h_band=(0, None), **M.DEPTHS)
        assert 0 < len(pos) == scores[0, 2, 2, 2] <= valid[0] and best[0, 3] >= len(pos)
    assert M.rotate(0.3, -0.7, 1.0, 0.0, 5.0, 6.0) == (0.3, -0.7)          # the point itself, not px + (dx) with its two roundings
    assert M.rotate(0.3, -0.7, 0.0, 1.0, 0.0, 0.0) == (0.7, 0.3)


def test_a_point_outside_the_grid_scores_once_it_is_shifted_in_and_points_count_once_each():
    gs, vh, R = 8, 4, 4
    occ = M.dense(np.array([[0, 5, 3], [7, 7, 0]], np.int32), gs, vh)
    got = M.score_cells(occ, np.array([[-3, 5, 3]]), R)
    want = np.zeros((9, 9), np.uint32)
    want[3 + R, 0 + R] = 1
    assert np.array_equal(got, want) and got.dtype == np.uint32
    got = M.score_cells(occ, np.array([[9, 10, 0], [9, 10, 0], [7, 7, 0]]), R)      # two points of one cell count twice
    want = np.zeros((9, 9), np.uint32)
    want[-2 + R, -3 + R], want[R, R] = 2, 1
    assert np.array_equal(got, want)
    assert not M.score_cells(occ, np.array([[0, 5, 2]]), R).any()                    # the layer is part of the cell
    # a point that no shift can bring in is left out of the list; one at the very reach of the window is kept
    pts = [(-(gs / 2 + R) * 0.5 + 0.01, 0.0, 1), (-(gs / 2 + R + 1) * 0.5 + 0.01, 0.0, 1), ((gs / 2 + R) * 0.5 + 0.01, 0.0, 1),
           ((gs / 2 + R + 1) * 0.5 + 0.01, 0.0, 1)]
    assert M.cells_of(pts, 1.0, 0.0, 0.0, 0.0, gs, 0.5, R)[:, 0].tolist() == [gs - 1 + R, -R]


def test_height_band_edges_and_depth_limits():
    depth, Ts = M.scene(1)
    vh = 30
    every = M.volumes(depth, M.K, Ts, M.CS, vh, 1, h_band=(0, None), **M.DEPTHS)[0][0]
    hs = sorted({h for _, _, h in every})
    assert hs[0] <= 3 and hs[-1] >= 12                                               # the walls span the band of the next lines
    for band in ((4, 11), (5, 5), (0, 3), (12, None)):
        got = M.volumes(depth, M.K, Ts, M.CS, vh, 1, h_band=band, **M.DEPTHS)[0][0]
        lo, hi = band[0], vh - 1 if band[1] is None else band[1]
        assert got == [p for p in every if lo <= p[2] <= hi] and {lo, hi} & {h for _, _, h in got} == ({lo, hi} & set(hs))
    # the eight special pixels of frame 0: zero, NaN, inf, both limits themselves, beyond them and a negative depth all drop
    Kinv = np.linalg.inv(M.K)
    _, ok = O.depth2pc_pixels(depth[0], Kinv, list(range(10)), **M.DEPTHS)
    assert ok.tolist() == [False] * 8 + [True] * 2
    assert depth[0, 0, 3] == M.DEPTHS["max_depth"] and depth[0, 0, 5] == M.DEPTHS["min_depth"]


def test_every_level_of_the_tie_rule_and_the_empty_volume():
    K, R = 5, 2
    S = 2 * R + 1

    def win(entries, k0=2):
        sc = np.zeros((K, S, S), np.uint32)
        for (k, di, dj), v in entries.items():
            sc[k, di + R, dj + R] = v
        return M.winner(sc, k0)
    assert win({}) == (2, 0, 0, 0) and win({}, k0=4) == (4, 0, 0, 0)                  # the empty volume: the prior
    assert win({(0, 2, 2): 7, (2, 0, 0): 6}) == (0, 2, 2, 7)                         # 1 the larger score
    assert win({(0, 1, 0): 7, (2, 1, 1): 7}) == (0, 1, 0, 7)                         # 2 the smaller di^2 + dj^2
    assert win({(0, 1, 0): 7, (3, 0, -1): 7}) == (3, 0, -1, 7)                       # 3 the smaller |k - k0| ...
    assert win({(0, 1, 0): 7, (3, 0, -1): 7}, k0=0) == (0, 1, 0, 7)                  #   ... about the caller's k0
    assert win({(3, 1, 0): 7, (1, 0, 1): 7}) == (1, 0, 1, 7)                         # 4 the smaller k
    assert win({(1, 1, 0): 7, (1, 0, 1): 7, (1, -1, 0): 7}) == (1, -1, 0, 7)         # 5 the smaller di
    assert win({(1, 0, 1): 7, (1, 0, -1): 7}) == (1, 0, -1, 7)                       # 6 the smaller dj
    assert win({(4, 0, 0): 1, (0, 0, 0): 1}, k0=4) == (4, 0, 0, 1) and win({(4, 0, 0): 1, (0, 0, 0): 1}, k0=1) == (0, 0, 0, 1)
    # an all-invalid frame and a map without voxels
    depth, Ts = np.zeros((2, M.H, M.W), np.float32), np.stack([M.camera((0, 0, 0.4))] * 2)
    for joint in (False, True):
        scores, best, valid = M.match_ref(M.voxels(8), M.GS, 8, depth, M.K, Ts, M.CS, _angles(2, 1), 1, joint=joint, k0=1, **M.DEPTHS)
        assert not scores.any() and not valid.any() and best.tolist() == [[1, 0, 0, 0]] * (1 if joint else 2)
    depth, Ts = M.scene(1)
    scores, best, valid = M.match_ref(np.zeros((0, 3), np.int32), M.GS, 8, depth, M.K, Ts, M.CS, _angles(2, 1), 1, stride=1, **M.DEPTHS)
    assert not scores.any() and valid[0] > 100 and best.tolist() == [[2, 0, 0, 0]]


PLANTS = [(8, 5, 3, -2), (30, 1, -4, 5), (7, 3, 0, 0), (30, 6, 5, 5)]


@pytest.mark.parametrize("vh,k_star,di_star,dj_star", PLANTS)
def test_a_planted_pose_is_the_unique_maximum_of_the_restatement(vh, k_star, di_star, dj_star):
    angles, R = _angles(6, 2), 5
    depth, T, pos = M.planted(angles, k_star, di_star, dj_star, vh, R)
    scores, best, valid = M.match_ref(pos, M.GS, vh, depth, M.K, T, M.CS, angles, R, stride=1, **M.DEPTHS)
    assert valid[0] > 200 and best[0].tolist() == [k_star, di_star, dj_star, int(valid[0])]
    assert int((scores == scores.max()).sum()) == 1 and scores[0, k_star, di_star + R, dj_star + R] == valid[0]


# ------------------------------------------------------------------ the library
def test_symbols_are_exported_and_the_source_is_built():
    from avlmaps_amd import _lib, build
    assert build.SOURCES["avl_match.hip"] == ["-ffp-contract=off"]
    text = (build.CSRC / "avl_match.hip").read_text()
    assert '#include "avl_sightray.h"' in text and '#include "avl_cellindex.h"' in text
    for shared in ("RayParams", "RayBatch", "ray_launches(", "ray_pixel(", "ray_cell_rc(", "ci_check_grid(", "ci_layout("):
        assert shared in text, shared
    header = (build.PKG.parent / "include" / "avlmaps_hip.h").read_text()
    build.build()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and f"AVL_API int {name}(" in header


def _c_match(lib, **over):
    """avl_match_frames on made-up (never dereferenced) pointers: every check comes before any device work"""
    table = np.ascontiguousarray(over.pop("table", _angles(2, 1)))
    Kinv, T = np.ascontiguousarray(np.linalg.inv(M.K)), np.ascontiguousarray(over.pop("T", np.stack([np.eye(4)] * 3)))
    a = dict(index=0x1000, index_bytes=1 << 30, N=10, gs=64, vh=8, depth=0x1000, u16=0, depth_div=1000.0, F=3, H=24, W=32,
             calib_inv=Kinv.ctypes.data, transforms=T.ctypes.data, cs=0.05, stride=1, min_depth=0.1, max_depth=6.0, angles=table.ctypes.data,
             K=len(table), R=2, h_lo=2, h_hi=7, joint=0, px=0.0, py=0.0, k0=len(table) // 2, split=0, scores=0x1000, best=0x1000, valid=0x1000,
             ws=0x1000, ws_bytes=1 << 40)
    a.update(over)
    return lib.avl_match_frames(a["index"], a["index_bytes"], a["N"], a["gs"], a["vh"], a["depth"], a["u16"], a["depth_div"], a["F"], a["H"],
                                a["W"], a["calib_inv"], a["transforms"], a["cs"], a["stride"], a["min_depth"], a["max_depth"], a["angles"],
                                a["K"], a["R"], a["h_lo"], a["h_hi"], a["joint"], a["px"], a["py"], a["k0"], a["split"], a["scores"], a["best"], a["valid"],
                                a["ws"], a["ws_bytes"], None)


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    import ctypes
    from avlmaps_amd import _lib
    lib = _lib.load()
    bad_table, bad_T = _angles(2, 1), np.stack([np.eye(4)] * 3)
    bad_table[3, 1] = np.nan
    bad_T[1, 0, 3] = np.inf
    cases = [dict(N=-1), dict(gs=0), dict(vh=0), dict(gs=16385, vh=1), dict(gs=16384), dict(N=2 ** 31 - 1),                   # ci_check_grid's
             dict(K=0), dict(K=1025), dict(R=-1), dict(R=65), dict(F=-1), dict(H=0), dict(W=0), dict(stride=0), dict(cs=0.0),
             dict(cs=float("nan")), dict(min_depth=-1.0), dict(max_depth=0.05), dict(u16=1, depth_div=0.0),
             dict(F=1 << 20, K=1024, R=64), dict(F=1 << 21, K=1024, R=0),            # V * K * S^2 >= 2^31, and 2^31 itself
             dict(h_lo=-1), dict(h_lo=5, h_hi=4), dict(h_hi=8), dict(k0=-1), dict(k0=5), dict(split=-1), dict(split=65537),
             dict(joint=1, px=float("nan")), dict(joint=1, py=float("inf")), dict(table=bad_table), dict(T=bad_T),
             dict(index=None), dict(depth=None), dict(calib_inv=None), dict(transforms=None), dict(angles=None), dict(scores=None),
             dict(best=None), dict(valid=None), dict(ws=None), dict(index_bytes=16), dict(ws_bytes=16),
             dict(gs=4, vh=2 ** 26, h_hi=7, R=64)]                                   # (gs + 2R)^2 * vh >= 2^32
    for over in cases:
        assert _c_match(lib, **over) != 0, over
        assert lib.avl_last_error().startswith(b"avl_match_frames"), (over, lib.avl_last_error())
    assert _c_match(lib, index=None) != 0 and b"null" in lib.avl_last_error()
    assert _c_match(lib, ws_bytes=16) != 0 and b"workspace" in lib.avl_last_error()
    assert _c_match(lib, K=1025) != 0 and b"1024" in lib.avl_last_error()
    assert _c_match(lib, R=65) != 0 and b"64" in lib.avl_last_error()
    assert _c_match(lib, table=bad_table) != 0 and b"angle 3" in lib.avl_last_error()
    assert _c_match(lib, T=bad_T) != 0 and b"frame 1" in lib.avl_last_error()
    # a joint call does not read the frames' origins: with them bad it gets as far as the last check, the workspace's size -- and a
    # call on made-up pointers must never get past the checks
    assert _c_match(lib, T=bad_T, joint=1, ws_bytes=16) != 0 and b"workspace" in lib.avl_last_error()
    assert _c_match(lib, split=65537) != 0 and b"split" in lib.avl_last_error()
    # nothing to do is not an error and touches no pointer; bad arguments are refused even then
    none = dict(index=None, depth=None, calib_inv=None, transforms=None, angles=None, scores=None, best=None, valid=None, ws=None, ws_bytes=0)
    assert _c_match(lib, F=0, **none) == 0 and _c_match(lib, F=0, joint=1, **none) == 0
    assert _c_match(lib, F=0, R=65, **none) != 0 and _c_match(lib, F=0, h_hi=8, **none) != 0
    # the size query: the same limits, and 4 bytes per lattice pixel, frame and angle
    n = ctypes.c_size_t(0)
    for args in ((3, 24, 32, 1, 0, 2, 0), (3, 24, 32, 1, 1025, 2, 0), (3, 24, 32, 1, 5, 65, 0), (3, 24, 32, 0, 5, 2, 0), (-1, 24, 32, 1, 5, 2, 0),
                 (3, 0, 32, 1, 5, 2, 0), (1 << 20, 24, 32, 1, 1024, 64, 0)):
        assert lib.avl_match_ws_bytes(*args, ctypes.byref(n)) != 0 and lib.avl_last_error().startswith(b"avl_match_ws_bytes"), args
    assert lib.avl_match_ws_bytes(3, 24, 32, 1, 5, 2, 0, None) != 0 and b"null" in lib.avl_last_error()
    for joint in (0, 1):
        assert lib.avl_match_ws_bytes(3, 24, 32, 1, 5, 2, joint, ctypes.byref(n)) == 0
        assert 3 * 24 * 32 * 5 * 4 <= n.value <= 3 * 24 * 32 * 5 * 4 + 4096
    assert lib.avl_match_ws_bytes(3, 24, 32, 3, 5, 2, 0, ctypes.byref(n)) == 0 and 3 * 8 * 11 * 5 * 4 <= n.value <= 3 * 8 * 11 * 5 * 4 + 4096
    assert lib.avl_match_ws_bytes(0, 24, 32, 1, 5, 2, 1, ctypes.byref(n)) == 0 and n.value <= 4096
    # V * K * S^2 < 2^31 exactly: 2^31 - 1 scores are taken, 2^31 are not
    assert lib.avl_match_ws_bytes(2 ** 31 - 1, 1, 1, 1, 1, 0, 0, ctypes.byref(n)) == 0 and n.value >= 8 * (2 ** 31 - 1)
    assert lib.avl_match_ws_bytes(2 ** 21 - 1, 1, 1, 1, 1024, 0, 0, ctypes.byref(n)) == 0
    assert lib.avl_match_ws_bytes(2 ** 21, 1, 1, 1, 1024, 0, 0, ctypes.byref(n)) != 0 and b"2^31 scores" in lib.avl_last_error()


def test_python_layer_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import ops
    index = ops.CellIndex(None, 0, 10, 64, 8)                 # never built: every check below comes before it is read
    depth, T = np.ones((2, 24, 32), np.float32), np.stack([np.eye(4)] * 2)
    ok = dict(index=index, depth=depth, calib=M.K, transforms=T, cs=0.05, angles=_angles(2, 1), radius=2)
    nan_T, nan_table = T.copy(), _angles(2, 1)
    nan_T[1, 1, 3] = np.nan
    nan_table[0, 0] = np.inf
    value = [dict(radius=-1), dict(radius=65), dict(angles=np.zeros((0, 2))), dict(angles=np.zeros((5, 3))), dict(angles=np.zeros((1025, 2))),
             dict(angles=nan_table), dict(angles=np.array([[0.0, 1.0]])), dict(k0=-1), dict(k0=5), dict(h_band=(-1, None)), dict(h_band=(5, 4)),
             dict(h_band=(2, 8)), dict(stride=0), dict(cs=0.0), dict(cs=float("nan")), dict(min_depth=-1.0), dict(min_depth=6.0),
             dict(depth=np.ones((24,), np.float32)), dict(calib=np.eye(4)), dict(transforms=np.stack([np.eye(4)] * 3)), dict(transforms=nan_T),
             dict(joint=True, pivot=(np.nan, 0.0)), dict(joint=True, pivot=(0.0, 1.0, 2.0)),
             dict(depth=np.ones((2 ** 17, 1, 1), np.float32), transforms=np.stack([np.eye(4)] * 2 ** 17), angles=np.tile([[1.0, 0.0]], (1024, 1)),
                  radius=64, k0=0),
             dict(depth=np.ones((2, 24, 32), np.uint16), depth_div=0.0), dict(split=0), dict(split=-1), dict(split=65537)]
    for over in value:
        with pytest.raises(ValueError):
            ops.match_frames(**{**ok, **over})
    for over in (dict(index=None), dict(index="index"), dict(depth=depth.astype(np.float64)), dict(depth=depth.astype(np.int32))):
        with pytest.raises(TypeError):
            ops.match_frames(**{**ok, **over})
    with pytest.raises(ValueError):
        ops.match_frames(ops.CellIndex(None, 0, 10, 4, 2 ** 26), depth, M.K, T, 0.05, _angles(2, 1), 64)           # (gs + 2R)^2 * vh >= 2^32
    assert ops.match_frames.__module__ == ops.match_angles.__module__ == ops.MatchResult.__module__ == "avlmaps_amd.ops.match"
    assert (ops.MATCH_MAX_ANGLES, ops.MATCH_MAX_RADIUS, ops.MATCH_MAX_SPLIT) == (1024, 64, 65536) and not hasattr(ops, "_angle_table")
    import inspect
    sig = inspect.signature(ops.match_frames)
    assert list(sig.parameters)[:7] == ["index", "depth", "calib", "transforms", "cs", "angles", "radius"]
    want = dict(stride=4, min_depth=0.1, max_depth=6.0, h_band=(2, None), joint=False, pivot=None, k0=None, device=False, stream=None, split=None)
    assert {k: sig.parameters[k].default for k in want} == want


def test_match_angles_is_symmetric_about_an_exact_zero():
    from avlmaps_amd import ops
    for max_deg, step, K in ((10.0, 0.5, 41), (6, 2, 7), (0, 1, 1), (1.0, 0.3, 7), (90, 90, 3)):
        a = ops.match_angles(max_deg, step)
        assert a.shape == (K, 2) and a.dtype == np.float64 and a[K // 2].tolist() == [1.0, 0.0]
        assert np.array_equal(a[::-1, 0], a[:, 0]) and np.array_equal(a[::-1, 1], -a[:, 1])
        assert np.all(np.diff(np.arctan2(a[:, 1], a[:, 0])) > 0)
        assert np.allclose(np.degrees(np.arctan2(a[:, 1], a[:, 0])), (np.arange(K) - K // 2) * step, atol=1e-12)
    for bad in ((-1, 1), (1, 0), (1, -1), (float("nan"), 1), (600, 1)):
        with pytest.raises(ValueError):
            ops.match_angles(*bad)


def test_corrections_against_a_hand_built_matrix():
    from avlmaps_amd import ops
    angles = _angles(10, 5)                                    # -10, -5, 0, 5, 10 degrees
    best = np.array([[4, 3, -2, 9], [2, 0, 0, 0], [0, -1, 5, 1]], np.int32)
    res = ops.MatchResult(None, best, np.array([9, 0, 4], np.uint32), 5)
    assert res.fraction.tolist() == [1.0, 0.0, 0.25]
    pivots = np.array([[0.5, -1.0], [7.0, 7.0], [0.0, 0.0]])
    C = res.corrections(0.05, angles, pivots)
    c, s = np.cos(np.deg2rad(10.0)), np.sin(np.deg2rad(10.0))
    want0 = np.array([[c, -s, 0, 0.5 - (c * 0.5 - s * -1.0) - 3 * 0.05], [s, c, 0, -1.0 - (s * 0.5 + c * -1.0) + 2 * 0.05], [0, 0, 1, 0],
                      [0, 0, 0, 1]])
    assert C.shape == (3, 4, 4) and C.dtype == np.float64 and np.allclose(C[0], want0, atol=1e-15, rtol=0)
    assert np.array_equal(C[1], np.eye(4))                                   # the prior itself: exactly the identity
    assert np.allclose(C[2], M.correction_ref(0, -1, 5, 0.05, angles, (0.0, 0.0)), atol=1e-15, rtol=0) and C[2][0, 3] == 0.05
    assert np.allclose(C[0] @ [0.5, -1.0, 3.0, 1.0], [0.5 - 0.15, -1.0 + 0.1, 3.0, 1.0], atol=1e-15)      # the pivot only shifts
    one = ops.MatchResult(None, best, None, 5).corrections(0.05, angles, (0.5, -1.0))                     # one pivot for all volumes
    assert np.array_equal(one[0], C[0])
    res.free()                                                               # a host result holds nothing on the device
    assert res.best is best and res.fraction.tolist() == [1.0, 0.0, 0.25]


# ------------------------------------------------------------------ the map layer and the app, on the restatement
VH = 16
N_FRAMES = 5
ANGLE, STEP, RADIUS_M = 4.0, 2.0, 0.15                  # the search of the end-to-end test: 5 angles, R = 3 cells
PLANT = (3, 2, -1)                                       # (k, di, dj): +2 degrees, two rows, one col


def _config():
    return M.recording_config()


class _FakeIndex:
    def __init__(self, grid_pos, gs, vh):
        self.grid_pos, self.gs, self.vh = np.array(grid_pos), gs, vh

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


class _HostArray:
    """a DeviceArray that lives on the host, for the map layer's own bookkeeping"""

    def __init__(self, shape, dtype):
        self.a = np.empty(shape, dtype)

    @classmethod
    def from_numpy(cls, a, stream=None):
        out = cls(np.shape(a), np.asarray(a).dtype)
        out.a[...] = a
        return out

    def zero_(self, stream=None):
        self.a[...] = 0
        return self

    def numpy(self, stream=None):
        return self.a.copy()

    def free(self):
        pass


@pytest.fixture(scope="module")
def revisit(tmp_path_factory):
    """a recording of N_FRAMES frames in the asymmetric room, and a map whose voxels are the restatement's cells of frames 0, 2 and 4
    of that recording under the planted correction"""
    from avlmaps_amd import ops
    from avlmaps_amd.map import VLMap
    sc = tmp_path_factory.mktemp("match") / "b"
    cfg = _config()
    vm = VLMap(cfg)
    angles = ops.match_angles(ANGLE, STEP)
    depth, Ts, pos, n_points, (mn, mx) = M.recording(sc, cfg, N_FRAMES, angles, PLANT, VH, [0, 2, 4])
    vm.grid_pos = pos
    vm.occupied_ids = -np.ones((M.GS, M.GS, VH), np.int32)
    vm.occupied_ids[tuple(pos.T)] = np.arange(len(pos))
    return vm, sc, depth, Ts, angles, n_points, (mn, mx)


@pytest.fixture
def calls(monkeypatch):
    """ops.cell_index, ops.match_frames and ops.audit_rays replaced by the restatements, DeviceArray by a host array; every call's
    arguments are recorded"""
    from avlmaps_amd import ops
    seen = []

    def cell_index(grid_pos, gs, vh, stream=None):
        return _FakeIndex(grid_pos, gs, vh)

    def match_frames(index, depth, calib, transforms, cs, angles, radius, stride=4, min_depth=0.1, max_depth=6.0, h_band=(2, None), joint=False,
                     pivot=None, k0=None, device=False, stream=None):
        seen.append(("match", dict(depth=np.array(depth), transforms=np.array(transforms), angles=np.array(angles), radius=radius, stride=stride,
                                   h_band=h_band, joint=joint, pivot=None if pivot is None else tuple(pivot), k0=k0, depths=(min_depth, max_depth))))
        got = M.match_ref(index.grid_pos, index.gs, index.vh, depth, calib, transforms, cs, angles, radius, stride, min_depth, max_depth, h_band,
                          joint, pivot, k0)
        return ops.MatchResult(*got, radius)

    def audit_rays(index, depth, calib, transforms, frame_ids, cs, stride=4, min_depth=0.1, max_depth=6.0, end_margin=2, last_hit=None,
                   through=None, after=None, **kw):
        seen.append(("audit", dict(transforms=np.array(transforms), ids=np.array(frame_ids))))
        lh, th = A.audit_ref(index.grid_pos, index.gs, index.vh, depth.a, calib, transforms, frame_ids, cs, stride, None, None, min_depth, max_depth,
                             end_margin, None if last_hit is None else last_hit.a, None if through is None else through.a,
                             None if after is None else after.a)
        for dev, new in ((last_hit, lh), (through, th)):
            if dev is not None:
                dev.a[...] = new
        return last_hit, through
    monkeypatch.setattr(ops, "cell_index", cell_index)
    monkeypatch.setattr(ops, "match_frames", match_frames)
    monkeypatch.setattr(ops, "audit_rays", audit_rays)
    monkeypatch.setattr("avlmaps_amd.device.DeviceArray", _HostArray)
    return seen


def test_register_frames_finds_the_planted_correction_and_the_audit_applies_it(revisit, calls, tmp_path):
    vm, sc, depth, Ts, angles, n_points, (mn, mx) = revisit
    reg = vm.register_frames(sc, max_angle_deg=ANGLE, angle_step_deg=STEP, radius_m=RADIUS_M, max_frames=3, stride=1)
    (kind, call), = calls
    # frame selection: three evenly spaced frames of five; the pivot: the first frame's origin; the prior: the table's middle
    assert kind == "match" and call["joint"] and np.array_equal(call["depth"], depth[[0, 2, 4]]) and np.array_equal(call["transforms"], Ts[[0, 2, 4]])
    assert call["pivot"] == (Ts[0, 0, 3], Ts[0, 1, 3]) and call["k0"] == 2 and call["radius"] == 3 and call["stride"] == 1
    assert call["h_band"] == (2, VH - 1) and call["depths"] == (mn, mx) and np.array_equal(call["angles"], angles)
    assert reg.frames.tolist() == [0, 2, 4] and reg.joint and reg.best.tolist() == [[*PLANT, n_points]]
    assert reg.valid.tolist() == [n_points] and reg.score.tolist() == [n_points] and reg.fraction.tolist() == [1.0]
    assert abs(reg.angle_deg[0] - 2.0) < 1e-12 and reg.shift_cells.tolist() == [[2, -1]]
    C = M.correction_ref(*PLANT, M.CS, angles, (Ts[0, 0, 3], Ts[0, 1, 3]))
    assert np.allclose(reg.correction, C, atol=1e-15, rtol=0) and reg.corrections.shape == (1, 4, 4)
    assert reg.transforms.shape == (N_FRAMES, 4, 4) and np.allclose(reg.transforms, C @ Ts, atol=1e-15, rtol=0)
    assert not (sc / "vlmap").exists()                                       # nothing is written
    # the un-registered recording scores fewer points: the planted pose is not the prior
    calls.clear()
    per = vm.register_frames(sc, max_angle_deg=ANGLE, angle_step_deg=STEP, radius_m=RADIUS_M, joint=False, stride=2, batch=2)
    assert [k for k, _ in calls] == ["match"] * 3 and [len(c["depth"]) for _, c in calls] == [2, 2, 1] and not calls[0][1]["joint"]
    assert per.frames.tolist() == list(range(N_FRAMES)) and per.corrections.shape == (N_FRAMES, 4, 4) and np.array_equal(per.pivots, Ts[:, :2, 3])
    assert np.allclose(per.transforms, per.corrections @ Ts, atol=1e-15, rtol=0) and (per.fraction > 0.5).all()
    with pytest.raises(ValueError):
        per.correction
    for bad in (dict(radius_m=4.0), dict(batch=0), dict(max_frames=0), dict(stride=0), dict(h_band_m=(0.3, 0.2)), dict(angle_step_deg=0.0)):
        with pytest.raises(ValueError):
            vm.register_frames(sc, **bad)
    # the audit: the correction reaches the transforms of its directory, and only of that one
    calls.clear()
    vm.data_dir = tmp_path
    audit = vm.audit_visibility([sc, sc], stride=4, batch=8, corrections=[None, reg.correction])
    got = [c for k, c in calls if k == "audit"]
    assert len(got) == 4 and audit.frame_counts == [N_FRAMES, N_FRAMES]
    for a, b in ((got[0], got[1]), (got[2], got[3])):                        # pass A, pass B
        assert np.array_equal(a["transforms"], Ts) and np.array_equal(b["transforms"], reg.correction @ Ts)
        assert a["ids"].tolist() == list(range(N_FRAMES)) and b["ids"].tolist() == list(range(N_FRAMES, 2 * N_FRAMES))
    calls.clear()
    plain = vm.audit_visibility([sc], stride=4)
    assert np.array_equal(calls[0][1]["transforms"], Ts) and plain.frame_counts == [N_FRAMES]
    for bad in ([reg.correction], [None, np.eye(3)], [None, None, None]):
        with pytest.raises(ValueError):
            vm.audit_visibility([sc, sc], corrections=bad)


def test_the_app_accepts_the_register_flags_and_refuses_them_without_register():
    from avlmaps_amd.apps import audit_map
    base = ["--data-dir", "x", "--revisit", "y"]
    a = audit_map.parse_args(base)
    assert a.register is False and (a.register_angle, a.register_step, a.register_radius, a.register_min_fraction) == (10.0, 0.5, 0.5, 0.5)
    a = audit_map.parse_args(base + ["--register"])
    assert a.register is True and (a.register_angle, a.register_step, a.register_radius, a.register_min_fraction) == (10.0, 0.5, 0.5, 0.5)
    a = audit_map.parse_args(base + ["--register", "--register-angle", "5", "--register-step", "0.25", "--register-radius", "1.0",
                                     "--register-min-fraction", "0.8"])
    assert (a.register_angle, a.register_step, a.register_radius, a.register_min_fraction) == (5.0, 0.25, 1.0, 0.8)
    for flag in ("--register-angle", "--register-step", "--register-radius", "--register-min-fraction"):
        with pytest.raises(SystemExit):
            audit_map.parse_args(base + [flag, "1"])
    with pytest.raises(SystemExit):
        audit_map.parse_args(base + ["--register", "--prune"])               # (the old rule still holds)
