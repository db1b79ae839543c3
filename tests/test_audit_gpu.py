"""GPU tests of the visibility audit (csrc/avl_audit.hip): the cell index against a dict, avl_audit_rays against the scalar
restatement of tests/_audit_ref.py with np.array_equal -- no tolerance, no ray or voxel left out -- its ties to the free-space carver
and to the builder, and Map.audit_visibility / VLMap.prune_voxels end to end.  Every scene asserts, through the restatement's own
bookkeeping, that it contains the cases it is there for."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import _audit_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

GS, VH, CS = 64, 8, 0.1
H, W = 24, 32
K = A.calib(8.0, 16.5, 12.5)            # pixel (12, 16) looks straight ahead; (12, 24), (20, 16), (20, 24) at exactly 45 degrees
H_MAX = 1.0                             # above the grid's top (VH * CS = 0.8): a ray may end on a surface the builder would not fuse
RANGE = dict(min_depth=0.125, max_depth=3.0)
PARAMS = dict(h_min=None, h_max=H_MAX, **RANGE)
CENTRE = (0.05, 0.05, 0.35)             # the centre of a cell in all three coordinates


# ------------------------------------------------------------------ the index
def index_cases():
    rng = np.random.default_rng(0)
    gs, vh = 70, 7                                                        # 34 300 cells: the last bitmap word is not full
    cells = gs * gs * vh
    yield gs, vh, np.zeros((0, 3), np.int32)
    yield gs, vh, np.array([[69, 69, 6]], np.int32)                       # the last cell alone
    lin = np.unique(np.concatenate([[0, 1, 31, 32, 33, 63, 64, 1023, 1024, 32767, 32768, cells - 33, cells - 32, cells - 1],
                                    rng.choice(cells, 4900, replace=False)]))      # both ends of the bitmap, both sides of word and block boundaries
    pos = np.stack(np.unravel_index(rng.permutation(lin), (gs, gs, vh)), axis=1).astype(np.int32)
    outside = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1], [70, 0, 0], [0, 70, 0], [0, 0, 7], [2 ** 31 - 1, 5, 5], [-2 ** 31, 5, 5],
                        [5, 2 ** 31 - 1, 1], [5, 5, -2 ** 31]], np.int64).astype(np.int32)
    dup = pos[rng.integers(0, len(pos), 5000 - len(pos) - len(outside))]  # cells held twice or more: the largest row wins
    yield gs, vh, rng.permutation(np.concatenate([pos, outside, dup]))
    yield 1, 1, np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1]], np.int32)     # the smallest grid; one cell held twice


def test_cell_index_equals_the_dict():
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    rng = np.random.default_rng(1)
    sizes = []
    for gs, vh, pos in index_cases():
        sizes.append(len(pos))
        every = np.stack(np.unravel_index(np.arange(gs * gs * vh), (gs, gs, vh)), axis=1).astype(np.int32)
        beyond = np.concatenate([rng.integers(-3, gs + 3, (200, 3)), [[gs, 0, 0], [0, gs, 0], [0, 0, vh], [-1, 0, 0], [2 ** 31 - 1, 0, 0],
                                                                      [-2 ** 31, -2 ** 31, -2 ** 31]]]).astype(np.int32)
        want, want_beyond = A.lookup_ref(pos, gs, vh, every), A.lookup_ref(pos, gs, vh, beyond)
        with ops.cell_index(pos, gs, vh) as index:
            assert (index.N, index.gs, index.vh) == (len(pos), gs, vh)
            got = ops.lookup_cells(index, every)
            assert got.dtype == np.int32 and np.array_equal(got, want)
            assert np.array_equal(ops.lookup_cells(index, beyond), want_beyond) and (want_beyond[-6:] == -1).all()
            assert ops.lookup_cells(index, np.zeros((0, 3), np.int32)).shape == (0,)
            dev = ops.lookup_cells(index, DeviceArray.from_numpy(every), device=True)
            assert np.array_equal(dev.numpy(), want)
        with ops.cell_index(DeviceArray.from_numpy(pos), gs, vh) as index:                        # a device-resident voxel list
            assert np.array_equal(ops.lookup_cells(index, every), want)
        if len(pos) > 1000:
            inside = (pos >= 0).all(axis=1) & (pos < (gs, gs, vh)).all(axis=1)
            assert (~inside).sum() >= 5 and len(np.unique(pos[inside], axis=0)) < inside.sum()   # rows outside, cells held twice
            owners = want[want >= 0]
            assert len(owners) == len(np.unique(pos[inside], axis=0)) and np.array_equal(pos[owners], every[want >= 0])
            assert want[0] >= 0 and want[-1] >= 0 and want[31] >= 0 and want[32] >= 0                 # the first and the last word, a word boundary
    assert sizes == [0, 1, 5000, 3]
    index = ops.cell_index(np.zeros((2, 3), np.int32), 4, 2)
    index.close()
    with pytest.raises(ValueError):
        ops.lookup_cells(index, np.zeros((1, 3), np.int32))


# ------------------------------------------------------------------ rays
def scene():
    """(depth (F, 24, 32) float32, transforms (F, 4, 4)): the frames of the ray tests"""
    rng = np.random.default_rng(2)
    Ts, depth = [], []

    def add(T, d):
        Ts.append(T)
        depth.append(np.asarray(d, np.float32))

    for yaw in (20.0, 110.0, 200.0, 290.0):                              # 0 - 7: every sign of row and column under either as the driving
        for pitch in (15.0, -15.0):                                       # axis, looking down (floor hits below z = 0) and up (ends above the grid)
            add(A.camera(CENTRE, yaw=yaw, pitch=pitch), rng.uniform(0.3, 3.4, (H, W)))
    add(A.camera((0.05, 0.05, 0.75), pitch=90.0), rng.uniform(0.2, 0.9, (H, W)))        # 8: straight down: the height drives
    add(A.camera((0.05, 0.05, 0.02), pitch=-90.0), rng.uniform(0.2, 1.2, (H, W)))       # 9: straight up, leaving through h_max
    d = rng.uniform(0.3, 2.9, (H, W))
    d[12, 16] = d[12, 24] = d[20, 16] = d[20, 24] = 1.0                   # straight ahead (level: dz == 0) and the 45-degree rays
    d[0, 0] = 0.13                                                        # ends in the camera's own cell: a point ray
    d[1, :6] = [0.0, np.nan, -1.0, 0.125, np.inf, 3.0]                    # zero, NaN, negative, exactly min_depth, infinite, exactly max_depth (far)
    add(A.camera(CENTRE), d)                                              # 10
    add(A.camera(CENTRE, yaw=90), d)                                      # 11: the same along the other axis
    add(A.camera((0.05, 0.05, H_MAX), yaw=180), rng.uniform(0.3, 2.9, (H, W)))          # 12: a camera exactly at h_max
    add(A.camera((-0.45, 0.25, 2.0), yaw=270), rng.uniform(0.5, 3.4, (H, W)))           # 13: above the band: level rays outside, falling ones enter from above
    add(A.camera((0.25, -0.35, -0.5), pitch=-30.0), rng.uniform(0.5, 3.4, (H, W)))      # 14: below the floor, looking up: enters from below
    add(A.camera((2.95, 0.05, 0.35), yaw=10.0), rng.uniform(0.3, 3.4, (H, W)))          # 15: near the border, looking out: rays leave the grid sideways
    add(A.camera((3.55, 0.05, 0.35), yaw=180.0), rng.uniform(0.3, 2.9, (H, W)))         # 16: outside the grid: every ray is skipped
    T = A.camera(CENTRE, yaw=45.0)
    T[:2, :3] *= 1.0e9                                                    # 17: no rigid motion: the rays end beyond 2^28 cells
    add(T, rng.uniform(0.3, 2.9, (H, W)))
    d = np.full((H, W), 2.0)
    d[20, 16] = 0.35 + 0.05                                               # 45 degrees down from z = 0.35: ends at z = -0.05, a hit in h = 0
    add(A.camera(CENTRE, yaw=180), d)                                     # 18
    return np.stack(depth), np.stack(Ts)


IDS = np.arange(19) * 2 + 3               # 3, 5, .. 39: not the frames' positions, and with gaps for `after`


@functools.lru_cache(maxsize=None)
def traced(stride):
    """(rays, stats) of the scene at a stride: traced once, folded by every test that needs it"""
    depth, Ts = scene()
    stats = {}
    return A.trace(GS, VH, depth, K, Ts, IDS, CS, stride=stride, stats=stats, **PARAMS), stats


@functools.lru_cache(maxsize=None)
def voxels():
    """the hit cells of every other frame, random cells, a few rows outside the grid and a few cells twice"""
    rng = np.random.default_rng(3)
    rays, _ = traced(1)
    hits = A.hit_cells([r for r in rays if (r[0] - 3) % 4 == 0])
    rand = np.stack(np.unravel_index(rng.permutation(GS * GS * VH)[:2500], (GS, GS, VH)), axis=1)
    pos = np.concatenate([np.array(hits).reshape(-1, 3), rand, [[-1, 3, 3], [3, GS, 3], [3, 3, VH]], rand[:5]]).astype(np.int32)
    return rng.permutation(pos)


def test_the_scene_contains_its_cases():
    _, stats = traced(1)
    assert len(stats["octants"]) == 24, sorted(stats["octants"])                                  # 8 sign octants under each driving axis
    assert stats["axis_aligned"] >= {0, 1, 2} and stats["diagonal"] >= 2 and stats["point"] >= 1
    for key in ("level_inside", "level_outside", "camera_at_h_max", "enters_from_above", "enters_from_below", "slab_leaves", "slab_empty",
                "leaves_grid", "far", "has_end", "cut", "hit", "hit_below_zero", "end_above_grid", "not_finite"):
        assert stats.get(key), (key, stats)
    assert stats["starts_outside"] >= H * W - 8 and stats["too_far"] >= 100 and stats["dropped"] >= 8
    for stride in (3, 5):
        assert traced(stride)[1].get("hit") and traced(stride)[1].get("far")


def run(stride=1, end_margin=2, last_hit=True, through=True, after=None, pos=None, frames=slice(None), ids=IDS, device=False, depth=None):
    """ops.audit_rays over (some of) the scene's frames from fresh outputs -> (last_hit, through)"""
    from avlmaps_amd import ops
    d, Ts = scene()
    pos = voxels() if pos is None else pos
    lh = np.full(len(pos), -1, np.int32) if last_hit is True else last_hit
    th = np.zeros(len(pos), np.uint32) if through is True else through
    with ops.cell_index(pos, GS, VH) as index:
        return ops.audit_rays(index, (d if depth is None else depth)[frames], K, Ts[frames], ids[frames], CS, stride=stride, end_margin=end_margin,
                              last_hit=lh if lh is not False else None, through=th if th is not False else None, after=after, device=device,
                              **PARAMS)


def want(stride=1, end_margin=2, after=None, pos=None, stats=None):
    pos = voxels() if pos is None else pos
    return A.fold(traced(stride)[0], pos, GS, VH, end_margin, np.full(len(pos), -1, np.int32), np.zeros(len(pos), np.uint32), after, stats)


@pytest.mark.parametrize("stride", [1, 3, 5])
def test_rays_equal_the_restatement(stride):
    stats = {}
    lh_want, th_want = want(stride, stats=stats)
    lh, th = run(stride)
    assert lh.dtype == np.int32 and th.dtype == np.uint32
    assert np.array_equal(lh, lh_want) and np.array_equal(th, th_want)
    assert stats["hit_recorded"] > 50 and stats["through_counted"] > 500 and stats["inside_margin"] > 20
    assert (lh_want >= 0).sum() > 20 and (th_want > 0).sum() > 200 and th_want.max() > 3


@pytest.mark.parametrize("end_margin", [0, 1, 1000])
def test_end_margin(end_margin):
    lh_want, th_want = want(1, end_margin)
    lh, th = run(1, end_margin)
    assert np.array_equal(lh, lh_want) and np.array_equal(th, th_want)
    assert not np.array_equal(th_want, want(1, 2)[1]) and np.array_equal(lh_want, want(1, 2)[0])
    if end_margin == 1000:                                                # only the rays without a surface at their end are left
        rays = [r for r in traced(1)[0] if not r[3]]
        assert np.array_equal(th_want, A.fold(rays, voxels(), GS, VH, 0, None, np.zeros(len(voxels()), np.uint32))[1]) and th_want.any()


def test_after_holds_back_the_frames_up_to_a_voxels_last_hit():
    rng = np.random.default_rng(4)
    after = rng.choice(np.concatenate([[-1, -1, -1], IDS, IDS - 1, [100]]), len(voxels())).astype(np.int32)
    stats = {}
    lh_want, th_want = want(after=after, stats=stats)
    for key in ("after_equal", "after_next", "after_never", "after_earlier", "after_later"):
        assert stats.get(key), (key, stats)
    lh, th = run(after=after)
    assert np.array_equal(lh, lh_want) and np.array_equal(th, th_want) and np.array_equal(lh_want, want()[0])
    assert (th_want <= want()[1]).all() and (th_want < want()[1]).any() and (th_want[after == 100] == 0).all()
    # the two passes of Map.audit_visibility: the hits first, then the rays of later frames
    lh2, th2 = run(last_hit=False, after=lh_want)
    assert lh2 is None and np.array_equal(th2, want(after=lh_want)[1]) and th2.any()


def test_each_output_may_be_absent():
    lh_want, th_want = want()
    lh, th = run(through=False)
    assert th is None and np.array_equal(lh, lh_want)
    lh, th = run(last_hit=False)
    assert lh is None and np.array_equal(th, th_want)
    assert run(last_hit=False, through=False) == (None, None)
    # no voxel at all, and no frame at all
    none = np.zeros((0, 3), np.int32)
    lh, th = run(pos=none)
    assert lh.shape == (0,) and th.shape == (0,)
    lh, th = run(frames=slice(0, 0))
    assert (lh == -1).all() and not th.any()


def test_uint16_depth_equals_float32():
    from avlmaps_amd import ops
    mm = (np.random.default_rng(5).integers(0, 28, (3, H, W)) * 125).astype(np.uint16)       # multiples of 1/8 m: value / 1000 is exact in float32
    f32 = (mm / 1000.0).astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), mm / 1000.0)
    _, Ts = scene()
    pos, kw = voxels(), dict(stride=1, end_margin=1, **PARAMS)
    got = []
    with ops.cell_index(pos, GS, VH) as index:
        for depth in (mm, f32):
            got.append(ops.audit_rays(index, depth, K, Ts[[0, 3, 8]], [4, 5, 6], CS, depth_div=1000.0, last_hit=np.full(len(pos), -1, np.int32),
                                      through=np.zeros(len(pos), np.uint32), **kw))
    ref = A.audit_ref(pos, GS, VH, f32, K, Ts[[0, 3, 8]], [4, 5, 6], CS, last_hit=np.full(len(pos), -1, np.int32),
                      through=np.zeros(len(pos), np.uint32), **kw)
    for a, b, c in zip(got[0], got[1], ref):
        assert np.array_equal(a, b) and np.array_equal(a, c) and (a != 0).any()


# ------------------------------------------------------------------ folds
def test_calls_continue_each_other_in_any_order():
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    lh_want, th_want = want()
    lh, th = run(frames=slice(0, 7))                                      # two calls, host arrays updated in place
    lh2, th2 = run(frames=slice(7, None), last_hit=lh, through=th)
    assert lh2 is lh and th2 is th and np.array_equal(lh, lh_want) and np.array_equal(th, th_want)
    back = slice(None, None, -1)                                          # reversed frame order
    lh, th = run(frames=back)
    assert np.array_equal(lh, lh_want) and np.array_equal(th, th_want)
    # 20 frames in one call are two launches: the scene and its first frame again under a later id
    d, Ts = scene()
    pos = voxels()
    more = dict(depth=np.concatenate([d, d[:1]]), transforms=np.concatenate([Ts, Ts[:1]]), ids=np.concatenate([IDS, [77]]))
    rays = traced(1)[0] + [(77,) + r[1:] for r in traced(1)[0] if r[0] == IDS[0]]
    lh20, th20 = A.fold(rays, pos, GS, VH, 2, np.full(len(pos), -1, np.int32), np.zeros(len(pos), np.uint32))
    assert (lh20 == 77).any()
    lh_dev, th_dev = DeviceArray.from_numpy(np.full(len(pos), -1, np.int32)), DeviceArray((len(pos),), np.uint32).zero_()
    with ops.cell_index(pos, GS, VH) as index:                            # device-resident outputs, updated in place
        out = ops.audit_rays(index, more["depth"], K, more["transforms"], more["ids"], CS, stride=1, last_hit=lh_dev, through=th_dev, **PARAMS)
        assert out[0] is lh_dev and out[1] is th_dev
        assert np.array_equal(lh_dev.numpy(), lh20) and np.array_equal(th_dev.numpy(), th20)
        # ... and continued: the same frames once more double every count and leave the maxima alone
        ops.audit_rays(index, DeviceArray.from_numpy(more["depth"]), K, more["transforms"], more["ids"], CS, stride=1, last_hit=lh_dev,
                       through=th_dev, **PARAMS)
        assert np.array_equal(lh_dev.numpy(), lh20) and np.array_equal(th_dev.numpy(), 2 * th20)
        host = np.zeros(len(pos), np.uint32)
        kept = ops.audit_rays(index, d[:2], K, Ts[:2], IDS[:2], CS, stride=1, through=host, device=True, **PARAMS)[1]
        assert isinstance(kept, DeviceArray) and not host.any() and kept.numpy().any()            # device=True: the staged copy comes back instead


def test_every_ray_of_four_frames_through_one_voxel():
    from avlmaps_amd import ops
    Ts = np.stack([A.camera(CENTRE, yaw=y, pitch=p) for y, p in ((0, 0.0), (90, 10.0), (180, -10.0), (270, 0.0))])
    depth = np.full((4, H, W), 5.0, np.float32)                           # every ray is far: no end to keep a margin from
    pos = np.array([[3, 3, 3], [32, 32, 3], [32, 32, 2]], np.int32)       # the camera's own cell: 32 - int(0.5) = 32 twice, int(3.5) = 3
    with ops.cell_index(pos, GS, VH) as index:
        _, th = ops.audit_rays(index, depth, K, Ts, [0, 1, 2, 3], CS, stride=1, through=np.zeros(3, np.uint32), **PARAMS)
    assert th[1] == 4 * H * W and th[2] == 0                              # (nothing looks straight down: the cell below stays uncrossed)
    assert np.array_equal(th, A.audit_ref(pos, GS, VH, depth, K, Ts, [0, 1, 2, 3], CS, stride=1, through=np.zeros(3, np.uint32), **PARAMS)[1])


# ------------------------------------------------------------------ ties to existing code
def test_one_layer_of_voxels_is_the_free_space_carver():
    from avlmaps_amd import ops
    depth, Ts = scene()
    frames = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 15, 16]
    every = np.stack(np.unravel_index(np.arange(GS * GS), (GS, GS, 1)), axis=1).astype(np.int32)
    kw = dict(stride=1, h_min=0.0, h_max=1.5, **RANGE)
    with ops.cell_index(every, GS, 1) as index:
        _, th = ops.audit_rays(index, depth[frames], K, Ts[frames], IDS[frames], CS, end_margin=0, through=np.zeros(GS * GS, np.uint32), **kw)
    first_seen = ops.carve_free_space(None, depth[frames], K, Ts[frames], IDS[frames], GS, CS, **kw)
    seen = th.reshape(GS, GS) > 0
    for T in Ts[frames]:
        r, c = int(GS / 2 - int(T[0, 3] / CS)), int(GS / 2 - int(T[1, 3] / CS))
        if 0 <= r < GS and 0 <= c < GS:
            seen[r, c] = True
    assert np.array_equal(seen, first_seen != ops.NEVER_SEEN) and 200 < seen.sum() < GS * GS


def test_a_built_maps_voxels_were_all_hit_by_the_frame_that_built_them():
    from avlmaps_amd import ops
    depth, Ts = scene()
    stride, D = 2, 8
    lattice = np.array([v * W + u for v, u in A.lattice(H, W, stride)], np.int32)
    for f in (0, 8, 18):
        acc = ops.VoxelAccumulator(GS, CS, VH, D)
        try:
            acc.integrate_frame(depth[f], K, Ts[f], lattice, np.ones((H, W, D), np.float32), np.zeros((H, W, 3), np.uint8), 0, **RANGE)
            pos = acc.finalize()["grid_pos"]
        finally:
            acc.close()
        # the builder fuses a point under the rule that makes a ray a hit: its voxels are among the restatement's hit cells
        hits = set(A.hit_cells(A.trace(GS, VH, depth[f], K, Ts[f], [41], CS, stride=stride, **RANGE)))
        assert 0 < len(pos) <= len(hits) and {tuple(p) for p in pos.tolist()} <= hits, (f, len(pos), len(hits))
        with ops.cell_index(pos, GS, VH) as index:                            # the default band: [-cs, vh * cs]
            lh, _ = ops.audit_rays(index, depth[f], K, Ts[f], [41], CS, stride=stride, last_hit=np.full(len(pos), -1, np.int32), **RANGE)
        assert (lh == 41).all(), (f, int((lh != 41).sum()), len(pos))


# ------------------------------------------------------------------ end to end
EG, ECS, EVH = 48, 0.25, 6              # the map of the end-to-end scene: 12 m x 12 m x 1.5 m
EK = [8.0, 0, 16.5, 0, 8.0, 12.5, 0, 0, 1]


def _config():
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": EG, "map_config.cell_size": ECS, "map_config.cam_calib_mat": EK}).map_config


def _render(T, with_box):
    """the depth image of a wall at x = 3.1 and (with_box) the front of a box at x = 1.1, |y| <= 0.5, z <= 1 before it, seen through
    the camera -> map transform T of a camera that looks along +x: analytic, per pixel"""
    Kinv = np.linalg.inv(np.array(EK).reshape(3, 3))
    depth = np.zeros((H, W), np.float32)
    O = T[:3, 3]
    for v in range(H):
        for u in range(W):
            d = T[:3, :3] @ (Kinv @ np.array([u + 0.5, v + 0.5, 1.0]))    # the map-frame ray per metre of camera depth
            best = (3.1 - O[0]) / d[0]
            if with_box:
                z = (1.1 - O[0]) / d[0]
                p = O + z * d
                if abs(p[1]) <= 0.5 and p[2] <= 1.0:
                    best = z
            depth[v, u] = best
    return depth


@pytest.fixture(scope="module")
def visit(tmp_path_factory):
    """scene A (a box in front of a wall) with a map of A's hit cells, and scene B: the same place later, the box gone"""
    from scipy.spatial.transform import Rotation
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.map.vlmap_builder import VLMapBuilder
    from avlmaps_amd.utils.mapping_utils import save_3d_map
    root = tmp_path_factory.mktemp("audit")
    cfg = _config()
    vm = VLMap(cfg)
    poses = {"a": [[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [-0.3, 0.0, 0.0]], "b": [[0.0, 0.0, 0.0], [0.2, 0.0, 0.1], [-0.2, 0.0, 0.1], [0.4, 0.0, 0.0]]}
    quat = Rotation.identity().as_quat()
    frames = {}
    for name in ("a", "b"):
        sc = root / name
        (sc / "depth").mkdir(parents=True)
        vecs = np.array([[*p, *quat] for p in poses[name]])
        np.savetxt(sc / "poses.txt", vecs)
        builder = VLMapBuilder(sc, cfg, sc / "poses.txt", [], [], vm.base2cam_tf, vm.base_transform)
        Ts = np.stack(builder.frame_transforms(np.concatenate([np.array([[*poses["a"][0], *quat]]), vecs])))[1:]
        depth = np.stack([_render(T, name == "a") for T in Ts])
        for i, d in enumerate(depth):
            np.save(sc / "depth" / f"{i:06d}.npy", d)
        frames[name] = (depth, Ts)
    rays = A.trace(EG, EVH, frames["a"][0], np.array(EK).reshape(3, 3), frames["a"][1], [0, 1, 2], ECS, stride=1)
    pos = np.array(A.hit_cells(rays), np.int32)
    rng = np.random.default_rng(6)
    occupied = -np.ones((EG, EG, EVH), np.int32)
    occupied[tuple(pos.T)] = np.arange(len(pos))
    (root / "a" / "vlmap").mkdir()
    save_3d_map(root / "a" / "vlmap" / "vlmaps.h5df", rng.standard_normal((len(pos), 128)).astype(np.float32), pos, np.ones(len(pos), np.float32),
                occupied, [0, 1, 2], rng.integers(0, 255, (len(pos), 3)).astype(np.uint8))
    return root, frames, pos


def test_a_revisit_finds_the_box_gone_and_the_pruned_map_answers_like_a_fresh_one(visit, tmp_path):
    from avlmaps_amd.apps import audit_map
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.utils.mapping_utils import save_3d_map
    root, frames, pos = visit
    Kmat = np.array(EK).reshape(3, 3)
    vm = VLMap(_config())
    assert vm.load_map(str(root / "a")) and vm.visibility is None
    audit = vm.audit_visibility([root / "a", root / "b"], stride=1, batch=2)
    # the restatement: pass A over both directories, then pass B with after = last_hit
    depth, Ts, ids = np.concatenate([frames["a"][0], frames["b"][0]]), np.concatenate([frames["a"][1], frames["b"][1]]), np.arange(7)
    rays = A.trace(EG, EVH, depth, Kmat, Ts, ids, ECS, stride=1)
    lh_want, _ = A.fold(rays, pos, EG, EVH, 2, np.full(len(pos), -1, np.int32), None)
    _, th_want = A.fold(rays, pos, EG, EVH, 2, None, np.zeros(len(pos), np.uint32), after=lh_want)
    assert np.array_equal(audit.last_hit, lh_want) and np.array_equal(audit.through, th_want)
    assert audit.frame_counts == [3, 4] and audit.params == dict(gs=EG, cs=ECS, vh=EVH, stride=1, end_margin=2, n_frames=7)
    assert vm.visibility is audit and (lh_want >= 0).all()                # every voxel is a hit cell of scene A
    stale = audit.stale()
    box = pos[:, 0] == EG // 2 - int(1.1 / ECS)                           # x = 1.1: row 24 - 4; the wall is row 24 - 12
    assert box.any() and (pos[~box, 0] == EG // 2 - int(3.1 / ECS)).all()
    assert (stale & box).any() and not stale[lh_want >= 3].any() and (lh_want >= 3).any() and (lh_want[stale] < 3).all()
    again = VLMap(_config())
    assert again.load_map(str(root / "a")) and np.array_equal(again.visibility.through, th_want)     # visibility.npz is picked up
    assert again.visibility.params == audit.params and again.visibility.frame_counts == [3, 4]
    # queries of the pruned map equal those of a freshly loaded copy of it
    q = np.random.default_rng(7).standard_normal((5, 128)).astype(np.float32)
    before = vm.index_queries(q)                                          # makes the resident copy that pruning has to drop
    removed = vm.prune_voxels(stale)
    assert removed == int(stale.sum()) and 0 < removed < len(pos) and vm.visibility is None
    out = tmp_path / "pruned"
    (out / "vlmap").mkdir(parents=True)
    save_3d_map(out / "vlmap" / "vlmaps.h5df", vm.grid_feat, vm.grid_pos, vm.weight, vm.occupied_ids, vm.mapped_iter_list, vm.grid_rgb)
    fresh = VLMap(_config())
    assert fresh.load_map(str(out)) and len(fresh.grid_pos) == len(pos) - removed
    am, sc = vm.index_queries(q, want_scores=True)
    am_fresh, sc_fresh = fresh.index_queries(q, want_scores=True)
    assert np.array_equal(am, am_fresh) and np.array_equal(sc, sc_fresh) and np.array_equal(am, before[~stale])
    from avlmaps_amd.apps.common import HashClip
    for m in (vm, fresh):                                                 # index_map's fused path and index_object's two steps: mask, then heat
        m.clip_feat_dim, m.clip_model = 128, HashClip(128)
    mask, mask_fresh = vm.index_map("chair", with_init_cat=False), fresh.index_map("chair", with_init_cat=False)
    assert mask.dtype == bool and mask.shape == (len(pos) - removed,) and np.array_equal(mask, mask_fresh)
    assert np.array_equal(vm.heatmap_from_mask(mask, ECS, 0.1).numpy(), fresh.heatmap_from_mask(mask_fresh, ECS, 0.1).numpy())
    for m in (vm, fresh):
        m.scores_mat, m.categories = (sc if m is vm else sc_fresh), ["a", "b", "c", "d", "e"]
        m._argmax_src = None
    assert np.array_equal(vm.index_map("b"), fresh.index_map("b"))
    assert np.array_equal(np.asarray(vm.heatmap_from_mask(vm.index_map("b"), ECS, 0.1).numpy()),
                          np.asarray(fresh.heatmap_from_mask(fresh.index_map("b"), ECS, 0.1).numpy()))
    # the app: the same counts, the pruned map under --out, the input map untouched
    res = audit_map.main(["--data-dir", str(root / "a"), "--revisit", str(root / "b"), "--stride", "1", "--prune", "--out", str(tmp_path / "app"),
                          "--render", str(tmp_path / "stale.png"), "--config", _config_file(tmp_path)])
    assert res["voxels"] == len(pos) and res["stale"] == removed == res["removed"] and res["frames"] == [3, 4]
    assert res["hit"] == len(pos) and res["seen_through"] == int((th_want > 0).sum())
    app = VLMap(_config())
    assert app.load_map(str(tmp_path / "app")) and np.array_equal(app.grid_pos, fresh.grid_pos)
    assert np.array_equal(app.occupied_ids, fresh.occupied_ids)
    untouched = VLMap(_config())
    assert untouched.load_map(str(root / "a")) and len(untouched.grid_pos) == len(pos)
    from PIL import Image
    img = np.asarray(Image.open(tmp_path / "stale.png"))
    assert img.shape == (EG, EG) and (img == 255).sum() > 0 and (img == 128).sum() > 0


def _config_file(tmp_path):
    import yaml
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump({"map_config": {"grid_size": EG, "cell_size": ECS, "cam_calib_mat": EK}, "params": {"gs": EG, "cs": ECS}}))
    return str(path)
