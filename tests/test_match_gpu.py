"""GPU tests of the correlative pose search (csrc/avl_match.hip): ops.match_frames against the restatement of tests/_match_ref.py
with np.array_equal -- scores, best and valid, no tolerance, no shift left out -- over the shapes at which the kernels take another
path: one shift, a partial lane tile and several tiles of shifts; lists stored plainly and lists split over blocks, a block taking
one chunk of points, several, and a last chunk that is not full (the split is pinned where a case is about it, so that what runs
does not depend on the library's own choice); one launch of frames and more than kRayFrames, one launch of angles and more than 64;
both modes; host and resident inputs."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import _match_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def scene():
    depth, Ts = M.scene(17)
    depth.setflags(write=False)
    Ts.setflags(write=False)
    return depth, Ts


@functools.lru_cache(maxsize=None)
def voxels(vh):
    pos = M.voxels(vh)
    pos.setflags(write=False)
    return pos


def angles(K):
    from avlmaps_amd import ops
    return {1: ops.match_angles(0, 1), 2: ops.match_angles(3, 3)[1:], 5: ops.match_angles(4, 2), 7: ops.match_angles(6, 2),
            65: ops.match_angles(3.2, 0.1)}[K]


def run_both(vh, R, K, F, joint, stride, h_band=(2, None), k0=None, pivot=None, depth=None, pos=None, resident=False, split=None):
    """-> (got, want): (scores, best, valid) of ops.match_frames and of the restatement on frames 0 .. F - 1 of the scene"""
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    d, Ts = scene()
    d = d[:F] if depth is None else depth
    pos = voxels(vh) if pos is None else pos
    kw = dict(stride=stride, h_band=h_band, joint=joint, k0=k0, pivot=pivot, **M.DEPTHS)
    want = M.match_ref(pos, M.GS, vh, d if d.dtype == np.float32 else (d / 1000.0).astype(np.float32), M.K, Ts[:F], M.CS, angles(K), R, **kw)
    with ops.cell_index(DeviceArray.from_numpy(pos) if resident else pos, M.GS, vh) as index:
        res = ops.match_frames(index, DeviceArray.from_numpy(d) if resident else d, M.K, Ts[:F], M.CS, angles(K), R, device=resident, split=split, **kw)
        got = (res.scores.numpy(), res.best.numpy(), res.valid.numpy()) if resident else (res.scores, res.best, res.valid)
    V, S = (1 if joint else F), 2 * R + 1
    assert got[0].shape == (V, K, S, S) and got[0].dtype == np.uint32 and got[1].shape == (V, 4) and got[1].dtype == np.int32
    assert got[2].shape == (V,) and got[2].dtype == np.uint32
    return got, want


def same(got, want):
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]), (got[1], want[1])


CHUNK = 256                             # kMatchChunk: the points a block of the correlate kernel stages at a time


def block_ranges(cap, split):
    """the ranges of a list of capacity `cap` (lattice pixels of the volume's frames) that the blocks of a pinned split take: the
    entry point gives a block whole chunks, ceil(cap / split) rounded up to a multiple of CHUNK"""
    per = -(-(-(-cap // split)) // CHUNK) * CHUNK
    return [(lo, min(cap, lo + per)) for lo in range(0, cap, per)]


# (vh, R, K, F, joint, stride, split): cells that straddle index words (vh 7 and 30), every tile shape of the shifts, a second launch
# of frames.  split None: the library's choice, which at these sizes is one chunk of at most 256 points per block or, for a frame of
# 88 pixels, the whole list in one block.  A pinned split says how many blocks share a list, whatever the library would choose
SHAPES = [
    (8, 0, 7, 3, False, 1, None),       # one shift: 64 rows of di in a wave
    (7, 1, 2, 17, False, 3, None),      # S = 3 in 4 lanes; 17 frames: a second launch; 88 pixels a frame: plain stores
    (30, 5, 7, 3, False, 1, None),      # S = 11 in 16 lanes
    (30, 20, 2, 3, True, 1, None),      # S = 41 in 64 lanes, three tiles of di; one list of three frames
    (8, 64, 1, 1, False, 3, None),      # S = 129: three tiles of dj, nine of di; plain stores
    (7, 64, 2, 3, True, 1, None),       # ... and split lists with 27 tiles each
    (8, 0, 2, 17, True, 1, None),       # 17 frames in one volume: lists of thousands of points
    (8, 5, 1, 17, True, 3, None),
    (30, 1, 7, 17, False, 1, None),     # 119 lists
    (8, 1, 65, 17, True, 3, None),      # 65 angles: a second rasterise launch with k_first = 64, and a second launch of frames
    (7, 1, 65, 3, False, 1, None),      # ... per frame
    (30, 5, 7, 3, False, 1, 1),         # whole lists of 630 .. 768 points: plain stores after three chunks, the last not full
    (30, 64, 5, 17, False, 1, 1),       # ... with 27 tiles of shifts
    (8, 0, 2, 17, True, 1, 1),          # one block walks a list of thousands of points: more than twenty chunks, plain stores
    (8, 64, 2, 17, True, 1, 4),         # atomics after 13 chunks a block; the list ends inside the second block, two blocks get nothing
    (30, 1, 7, 17, False, 1, 2),        # atomics: two chunks in the first block, a partial one in the second
]


@pytest.mark.parametrize("vh,R,K,F,joint,stride,split", SHAPES)
def test_scores_best_and_valid_equal_the_restatement(vh, R, K, F, joint, stride, split):
    got, want = run_both(vh, R, K, F, joint, stride, split=split)
    same(got, want)
    assert want[2].sum() > 20 * F // stride and want[0].any()
    if not joint and R:
        assert (want[0].reshape(F, -1).max(axis=1) > 0).all()
    if split is not None:
        # the case really takes a block past its first chunk and ends a block on a chunk that is not full: the lengths of the lists
        # of the zero angle (under it a list holds the points the restatement keeps), cut as the entry point cuts them
        depth, Ts = scene()
        rays = len(M.lattice(M.H, M.W, stride))
        vols = M.volumes(depth[:F], M.K, Ts[:F], M.CS, vh, stride, joint=joint, **M.DEPTHS)
        k0 = len(angles(K)) // 2
        lengths = [len(M.cells_of(points, *angles(K)[k0], px, py, M.GS, M.CS, R)) for points, (px, py) in vols]
        taken = [min(n, hi) - lo for n in lengths for lo, hi in block_ranges(rays * (F if joint else 1), split) if n > lo]
        assert max(taken) > CHUNK and any(t % CHUNK and t > CHUNK for t in taken)
        if split > 1:
            assert len(taken) > len(lengths)                                # more than one block of a list has points
        if split == 4:
            assert len(taken) == 2 * len(lengths)                           # ... and two of its four have none


def test_the_scene_holds_the_cases_it_is_there_for():
    depth, Ts = scene()
    rows, cols = [], []
    for f in range(7):
        (points, (px, py)), = M.volumes(depth[f], M.K, Ts[f], M.CS, 30, 1, h_band=(0, None), **M.DEPTHS)
        for k in (0, 6):
            cells = M.cells_of(points, *angles(7)[k], px, py, M.GS, M.CS, 64)
            rows += cells[:, 0].tolist()
            cols += cells[:, 1].tolist()
    assert -64 <= min(rows) < 0 and -64 <= min(cols) < 0                       # points beyond the first row and col that a shift brings in
    assert sum(r < 5 for r in rows) > 50 and sum(r > M.GS - 6 for r in rows) > 50 and sum(c < 12 for c in cols) > 50     # walls near three borders
    assert not np.isfinite(depth[0, 0, 1]) and depth[0, 0, 0] == 0 and depth[0, 0, 3] == 6.0 and depth[0, 0, 5] == 0.125 and depth[0, 0, 4] > 6.0
    pos = voxels(8)
    assert (pos[:, 0] < 0).any() and (pos[:, 2] >= 8).any() and len(np.unique(pos, axis=0)) < len(pos)


def test_resident_inputs_a_height_band_a_prior_index_and_a_pivot():
    same(*run_both(8, 5, 7, 3, False, 1, resident=True))
    same(*run_both(30, 5, 7, 3, True, 1, h_band=(4, 11), k0=5, pivot=(0.35, -0.6), resident=True))
    got, want = run_both(30, 1, 2, 17, False, 3, h_band=(5, 5), k0=0)
    same(got, want)
    assert 0 < want[2].sum() < 17 * 88 // 4


def test_uint16_depth_equals_float32():
    mm = (np.random.default_rng(5).integers(0, 28, (3, M.H, M.W)) * 125).astype(np.uint16)      # multiples of 1/8 m: value / 1000 is exact in float32
    mm[0, 0, :5] = [125, 6000, 0, 7500, 65500]                                                  # the two limits themselves and two far pixels: dropped
    f32 = (mm / 1000.0).astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), mm / 1000.0)
    got16, want = run_both(8, 5, 2, 3, False, 1, depth=mm)
    got32, _ = run_both(8, 5, 2, 3, False, 1, depth=f32)
    same(got16, want)
    same(got32, want)
    assert want[2].sum() > 500


def test_no_voxels_an_all_invalid_frame_and_no_frames():
    from avlmaps_amd import ops
    depth, Ts = scene()
    for joint in (False, True):
        got, want = run_both(8, 5, 7, 3, joint, 1, pos=np.zeros((0, 3), np.int32), k0=1)
        same(got, want)
        assert not got[0].any() and got[2].all() and got[1].tolist() == [[1, 0, 0, 0]] * len(got[1])
    bad = np.array(depth[:3])
    bad[1] = [0.0, np.nan, 7.0, 0.05] * (M.W // 4)
    got, want = run_both(8, 5, 7, 3, False, 1, depth=bad)
    same(got, want)
    assert got[2][1] == 0 and not got[0][1].any() and got[1][1].tolist() == [3, 0, 0, 0] and got[2][0] > 0 and got[2][2] > 0
    same(*run_both(8, 5, 7, 3, True, 1, depth=np.stack([bad[1]] * 3), k0=6))
    with ops.cell_index(voxels(8), M.GS, 8) as index:
        for joint, V in ((False, 0), (True, 1)):
            res = ops.match_frames(index, depth[:0], M.K, Ts[:0], M.CS, angles(7), 2, joint=joint, k0=4)
            assert res.scores.shape == (V, 7, 5, 5) and not res.scores.any() and res.best.tolist() == [[4, 0, 0, 0]] * V
            assert res.valid.tolist() == [0] * V and res.fraction.tolist() == [0.0] * V


@pytest.mark.parametrize("vh,k_star,di_star,dj_star", [(8, 5, 3, -2), (30, 1, -4, 5), (7, 3, 0, 0), (30, 6, 5, 5)])
def test_a_planted_pose_is_found_and_its_correction_is_the_planted_one(vh, k_star, di_star, dj_star):
    from avlmaps_amd import ops
    table, R, origin, yaw = angles(7), 5, (0.1, -0.2, 0.4), 30.0
    depth, T, pos = M.planted(table, k_star, di_star, dj_star, vh, R, origin=origin, yaw=yaw)
    with ops.cell_index(pos, M.GS, vh) as index:
        res = ops.match_frames(index, depth, M.K, T, M.CS, table, R, stride=1, **M.DEPTHS)
    assert res.valid[0] > 200 and res.best[0].tolist() == [k_star, di_star, dj_star, int(res.valid[0])] and res.fraction.tolist() == [1.0]
    assert int((res.scores == res.scores.max()).sum()) == 1
    corrected = res.corrections(M.CS, table, T[:, :2, 3])[0] @ T[0]
    theta = 2.0 * (k_star - 3)
    want = M.camera((origin[0] - di_star * M.CS, origin[1] - dj_star * M.CS, origin[2]), yaw=yaw + theta)
    assert np.allclose(corrected[:3, :3], want[:3, :3], atol=1e-12, rtol=0)
    assert np.abs(corrected[:3, 3] - want[:3, 3]).max() <= M.CS                # one cell, by construction


# ------------------------------------------------------------------ end to end
E_VH, E_FRAMES, E_PLANT = 16, 5, (3, 2, -1)             # 5 angles of -4 .. 4 degrees, R = 3: the recording is off by +2 degrees, (2, -1) cells


@pytest.fixture(scope="module")
def revisit(tmp_path_factory):
    """scene a: one frame and the saved map; scene b: a recording of the same room that is off by E_PLANT in the map's frame"""
    import yaml
    from avlmaps_amd import ops
    from avlmaps_amd.utils.mapping_utils import save_3d_map
    root = tmp_path_factory.mktemp("register")
    cfg = M.recording_config()
    table = ops.match_angles(4.0, 2.0)
    depth, Ts, pos, n_points, _ = M.recording(root / "b", cfg, E_FRAMES, table, E_PLANT, E_VH, list(range(E_FRAMES)))
    M.recording(root / "a", cfg, 1, table, (2, 0, 0), E_VH, [0])                       # the same first pose: the same map frame
    rng = np.random.default_rng(3)
    occupied = -np.ones((M.GS, M.GS, E_VH), np.int32)
    occupied[tuple(pos.T)] = np.arange(len(pos))
    (root / "a" / "vlmap").mkdir()
    save_3d_map(root / "a" / "vlmap" / "vlmaps.h5df", rng.standard_normal((len(pos), 16)).astype(np.float32), pos, np.ones(len(pos), np.float32),
                occupied, [0], rng.integers(0, 255, (len(pos), 3)).astype(np.uint8))
    (root / "cfg.yaml").write_text(yaml.safe_dump({"map_config": {"grid_size": M.GS, "cell_size": M.CS, "cam_calib_mat": [float(x) for x in M.K.reshape(-1)],
                                                                  "pose_info": {"camera_height": 0.4}}, "params": {"gs": M.GS, "cs": M.CS}}))
    return root, cfg, table, depth, Ts, pos, n_points


def test_register_frames_and_the_app_find_the_planted_correction(revisit):
    from avlmaps_amd.apps import audit_map
    from avlmaps_amd.map import VLMap
    root, cfg, table, depth, Ts, pos, n_points = revisit
    vm = VLMap(cfg)
    assert vm.load_map(str(root / "a")) and np.array_equal(vm.grid_pos, pos)
    kw = dict(max_angle_deg=4.0, angle_step_deg=2.0, radius_m=0.15, stride=1)
    reg = vm.register_frames(root / "b", **kw)
    assert reg.frames.tolist() == list(range(E_FRAMES)) and reg.best.tolist() == [[*E_PLANT, n_points]] and reg.fraction.tolist() == [1.0]
    C = M.correction_ref(*E_PLANT, M.CS, table, (Ts[0, 0, 3], Ts[0, 1, 3]))
    assert np.allclose(reg.correction, C, atol=1e-15, rtol=0) and np.allclose(reg.transforms, C @ Ts, atol=1e-15, rtol=0)
    # per frame: every frame on its own, about its own origin (one frame of a wall does not pin the pose as five do)
    per = vm.register_frames(root / "b", joint=False, batch=2, **kw)
    want = M.match_ref(pos, M.GS, E_VH, depth, M.K, Ts, M.CS, table, 3, stride=1, min_depth=0.1, max_depth=6.0, k0=2)
    assert np.array_equal(per.best, want[1]) and np.array_equal(per.valid, want[2]) and per.corrections.shape == (E_FRAMES, 4, 4)
    # the app: the audit of the revisit under the correction ends its rays on the map's voxels; without it, it does not
    base = ["--data-dir", str(root / "a"), "--revisit", str(root / "b"), "--stride", "1", "--config", str(root / "cfg.yaml")]
    res = audit_map.main(base + ["--register", "--register-angle", "4", "--register-step", "2", "--register-radius", "0.15"])
    (r,) = res["registration"]
    assert r["dir"] == str(root / "b") and abs(r["angle_deg"] - 2.0) < 1e-9 and r["shift_cells"] == [2, -1]
    assert r["score"] == r["valid"] == n_points and r["fraction"] == 1.0 and res["frames"] == [1, E_FRAMES]
    plain = audit_map.main(base)
    assert "registration" not in plain and res["hit"] >= 0.95 * len(pos) and plain["hit"] < 0.5 * len(pos)
    with pytest.raises(SystemExit, match="register-min-fraction"):
        audit_map.main(base + ["--register", "--register-angle", "0", "--register-radius", "0"])       # the prior itself: a poor pose
