"""Cross-modal goals on the GPU (csrc/avl_goal.hip through ops.goal_fuse, AVLMap.index_goal and the apps) against a NumPy
restatement of what generated robot code does upstream (robot/habitat_lang_robot.py:377-430): widen every heat to float64,
multiply left to right, np.argmax, grid_pos[argmax].  Every term has a closed form, so the tests demand equality."""
import itertools
import json
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent / "tools"))

KINDS = ("dense32", "dense64", "field32", "field64", "cones")
GS, VH = 37, 5                                         # a grid that is not a multiple of the 16-cell tiles of the field kernels


# ------------------------------------------------------------------ the oracle
def np_product(values):
    acc = values[0].astype(np.float64)
    for v in values[1:]:
        acc = acc * v.astype(np.float64)
    return acc


def np_field(field, gp, gs, vh):
    """avl_field_lift: the min-max normalised field at the voxel's column in the field's precision, rounded to float32; 0 outside"""
    r, c, h = gp[:, 0], gp[:, 1], gp[:, 2]
    inside = (r >= 0) & (r < gs) & (c >= 0) & (c < gs) & (h >= 0) & (h < vh)
    mn, mx = field.min(), field.max()
    norm = ((field - mn) / (mx - mn)).astype(np.float32)
    out = np.zeros(len(gp), np.float32)
    out[inside] = norm[r[inside], c[inside]]
    return out


def np_cones(cells, peaks, decay, gp):
    """habitat_lang_robot.py:207-227 in cells: max over the points of clip(peak - decay * dist, 0, 1), float64"""
    best = None
    for (pr, pc), pk in zip(cells, peaks):
        dx, dy = gp[:, 0].astype(np.float64) - float(pr), gp[:, 1].astype(np.float64) - float(pc)
        v = np.clip(pk - decay * np.sqrt(dx * dx + dy * dy), 0, 1)
        best = v if best is None else np.maximum(best, v)
    return best


def _gf(field):
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    mm = np.array([field.min(), field.max()], dtype=field.dtype)
    return ops.GoalField(DeviceArray.from_numpy(field), DeviceArray.from_numpy(mm))


def make_positions(rng, N, gs=GS, vh=VH):
    """voxels inside and outside the grid: negative coordinates, rows / columns >= gs, heights >= vh"""
    gp = np.concatenate([rng.integers(-3, gs + 3, (N, 2)), rng.integers(-1, vh + 2, (N, 1))], 1).astype(np.int32)
    gp[0] = [gs // 2, gs // 3, 1]
    return gp


def make_term(kind, rng, gp, P=3, decay=0.07, gs=GS, vh=VH):
    """-> (ops.GoalTerm, the term's (N,) values by NumPy)"""
    from avlmaps_amd import ops
    N = len(gp)
    if kind == "dense32":
        v = rng.random(N).astype(np.float32)
        return ops.GoalTerm.dense(v), v
    if kind == "dense64":
        v = rng.random(N) * 1.5
        return ops.GoalTerm.dense(v), v
    if kind in ("field32", "field64"):
        field = (rng.random((gs, gs)) * 3 + 0.25).astype(np.float32 if kind == "field32" else np.float64)
        return ops.GoalTerm.field(_gf(field), vh), np_field(field, gp, gs, vh)
    cells = rng.integers(-5, gs + 5, (P, 2)).astype(np.int32)
    peaks = rng.random(P) * 1.3                                       # some peaks above 1: the cone is clipped
    if P >= 4:
        peaks[::4] = 0.0                                              # and some equal to 0: they contribute nothing
    return ops.GoalTerm.cones(cells, peaks, decay), np_cones(cells, peaks, decay, gp)


def check(terms, values, gp):
    from avlmaps_amd import ops
    want = np_product(values)
    idx = int(np.argmax(want))
    res = ops.goal_fuse(terms, gp)
    heat = res.heat.numpy()
    assert heat.dtype == np.float64 and np.array_equal(heat, want)
    assert res.index == idx and res.value == want[idx] and res.pos.dtype == np.int32 and res.pos.tolist() == gp[idx].tolist()
    lean = ops.goal_fuse(terms, gp, want_heat=False)
    assert lean.heat is None and (lean.index, lean.value, lean.pos.tolist()) == (res.index, res.value, res.pos.tolist())


# ------------------------------------------------------------------ ops level, bit for bit
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097, 300_000])
def test_every_kind_every_pair_and_eight_terms(N):
    rng = np.random.default_rng(N)
    gp = make_positions(rng, N)
    made = {k: make_term(k, rng, gp) for k in KINDS}
    for k in KINDS:                                                    # every kind alone
        check([made[k][0]], [made[k][1]], gp)
    for a, b in itertools.product(KINDS, KINDS):                       # every ordered pair of kinds
        ta, tb = made[a], made[b] if a != b else make_term(b, rng, gp)
        check([ta[0], tb[0]], [ta[1], tb[1]], gp)
    eight = [made[k] for k in KINDS] + [make_term(k, rng, gp, P=5) for k in ("cones", "field32", "dense64")]
    order = rng.permutation(8)
    check([eight[i][0] for i in order], [eight[i][1] for i in order], gp)


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_cone_counts_across_the_lds_chunks(P):
    rng = np.random.default_rng(P)
    gp = make_positions(rng, 4097)
    for decay in (0.07, 0.0, 2.5):
        t, v = make_term("cones", rng, gp, P=P, decay=decay)
        check([t], [v], gp)
        d, dv = make_term("dense32", rng, gp)
        check([d, t], [dv, v], gp)


def test_cone_peaks_above_one_and_zero():
    from avlmaps_amd import ops
    rng = np.random.default_rng(8)
    gp = make_positions(rng, 5000)
    cells = np.array([[5, 5], [20, 30], [-2, 40], [18, 18]], np.int32)
    for peaks in ([0.0, 0.0, 0.0, 0.0], [3.0, 0.0, 1.0, 1.0 + 2 ** -52], [0.5, 2.0, 0.0, 0.25]):
        for decay in (0.0, 0.11):
            peaks = np.array(peaks)
            check([ops.GoalTerm.cones(cells, peaks, decay)], [np_cones(cells, peaks, decay, gp)], gp)


def test_a_large_grid_and_real_heights():
    """gs = 1000 with a float64 and a float32 field, as the area and sound queries make them"""
    rng = np.random.default_rng(21)
    gs, vh, N = 1000, 30, 200_000
    gp = make_positions(rng, N, gs, vh)
    terms = [make_term(k, rng, gp, P=2, decay=0.01, gs=gs, vh=vh) for k in ("dense32", "field64", "field32", "cones")]
    check([t for t, _ in terms], [v for _, v in terms], gp)


# ------------------------------------------------------------------ ties and repeatability
def test_ties_go_to_the_smallest_index_and_runs_repeat():
    from avlmaps_amd import ops
    N = 300_000
    rng = np.random.default_rng(4)
    gp = make_positions(rng, N)
    ones_at = [299_999, 256 * 700 + 5, 70_001, 256 * 3 + 17, 123_456]      # spread over different workgroups, and over their steps
    a = (rng.random(N) * 0.5).astype(np.float32)
    a[ones_at] = 1.0
    b = np.full(N, 0.25)
    b[ones_at] = 1.0
    for terms, vals in (([ops.GoalTerm.dense(a)], [a]), ([ops.GoalTerm.dense(a), ops.GoalTerm.dense(b)], [a, b])):
        res = ops.goal_fuse(terms, gp)
        assert res.index == min(ones_at) == int(np.argmax(np_product(vals))) and res.value == 1.0
        again = ops.goal_fuse(terms, gp)
        assert (again.index, again.value, again.pos.tolist()) == (res.index, res.value, res.pos.tolist())
        assert np.array_equal(again.heat.numpy(), res.heat.numpy())
    # the modalities do not overlap: the product is 0 everywhere and the goal is voxel 0, as np.argmax returns it
    lo, hi = np.zeros(N, np.float32), np.zeros(N)
    lo[: N // 2] = rng.random(N // 2)
    hi[N // 2:] = rng.random(N - N // 2)
    res = ops.goal_fuse([ops.GoalTerm.dense(lo), ops.GoalTerm.dense(hi)], gp)
    assert res.index == 0 and res.value == 0.0 and res.pos.tolist() == gp[0].tolist() and not res.heat.numpy().any()


def test_device_arrays_are_used_in_place_and_sizes_are_checked():
    from avlmaps_amd import ops
    from avlmaps_amd.device import DeviceArray
    rng = np.random.default_rng(6)
    gp = make_positions(rng, 1000)
    v32, v64 = rng.random(1000).astype(np.float32), rng.random(1000)
    d32, d64, dgp = DeviceArray.from_numpy(v32), DeviceArray.from_numpy(v64), DeviceArray.from_numpy(gp)
    t = ops.GoalTerm.dense(d32)
    assert t.data == d32.ptr and t.kind == ops.GOAL_DENSE_F32 and ops.GoalTerm.dense(d64).kind == ops.GOAL_DENSE_F64
    res = ops.goal_fuse([t, ops.GoalTerm.dense(d64)], dgp)
    assert np.array_equal(res.heat.numpy(), np_product([v32, v64]))
    with pytest.raises(ValueError):
        ops.goal_fuse([ops.GoalTerm.dense(v32[:999])], gp)
    with pytest.raises(ValueError):
        ops.goal_fuse([t], np.zeros((0, 3), np.int32))
    with pytest.raises(TypeError):
        ops.GoalTerm.dense(DeviceArray.from_numpy(np.zeros(4, np.int32)))


# ------------------------------------------------------------------ each kind against its stand-alone kernel
def test_terms_equal_the_stand_alone_kernels():
    from avlmaps_amd import ops
    rng = np.random.default_rng(12)
    gs, vh = 203, 9
    gp = make_positions(rng, 50_000, gs, vh)
    for dtype in (np.float32, np.float64):
        gf = _gf((rng.random((gs, gs)) * 2 + 0.5).astype(dtype))
        res = ops.goal_fuse([ops.GoalTerm.field(gf, vh)], gp)
        lift = ops.field_lift(gf, gp, vh).numpy()
        assert lift.dtype == np.float32 and np.array_equal(res.heat.numpy(), lift.astype(np.float64))
        assert res.index == int(np.argmax(lift))
    for row, col, decay in ((100, 90, 0.01), (-20, 400, 0.001), (3, 7, 0.5)):
        res = ops.goal_fuse([ops.GoalTerm.cones([[row, col]], [1.0], decay)], gp)
        sim = ops.planar_decay(gp, row, col, decay).numpy()
        assert np.array_equal(res.heat.numpy(), sim) and res.index == int(np.argmax(sim))


# ------------------------------------------------------------------ end to end through AVLMap and the apps
OBJECTS = ("table", "rug")              # hashed text features: on this scene "table" beats "other" on 187 of the 9 845 voxels, "rug" on 2 719


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map
    from avlmaps_amd.apps.common import HashImageEncoder, load_config
    from avlmaps_amd.map.area_map import AreaMap
    tmp = tmp_path_factory.mktemp("goal")
    sc = make(tmp / "scene", frames=8, H=96, W=128)
    cfg_path = tmp / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                       "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(sc), "--config", str(cfg_path), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    AreaMap().create_map(sc, image_encoder=HashImageEncoder())
    rng = np.random.default_rng(11)
    db = {i: {"audio_features": rng.standard_normal(1024).astype(np.float32),
              "locations": [np.array([rng.uniform(-1.5, 1.5), 0.0, rng.uniform(-1.5, 1.5)]) for _ in range(1 + i % 5)]}
          for i in range(14)}
    (sc / "audio_video").mkdir()
    (sc / "audio_video" / "audio_data_level_3.pkl").write_bytes(pickle.dumps(db))
    return sc, cfg_path, load_config(str(cfg_path))


IMAGE_POSE = 5


def _avlmap(scene, localizer=True):
    from avlmaps_amd.apps.common import FixedPoseLocalizer, HashAudioText, HashClip
    from avlmaps_amd.map import AVLMap
    sc, _, cfg = scene
    av = AVLMap(cfg, data_dir=str(sc), area_text_model=HashClip(768), audio_text_model=HashAudioText())
    assert av.load_map(str(sc))
    vm = av.vlmap
    vm.clip_feat_dim = vm.grid_feat.shape[1]
    vm.clip_model = HashClip(vm.clip_feat_dim)
    if localizer:
        av.visual_map.localizer = FixedPoseLocalizer(np.loadtxt(sc / "poses.txt")[IMAGE_POSE], vm.base2cam_tf)
    return av


IMG = np.zeros((48, 64, 3), np.uint8)
f64 = lambda a: a.astype(np.float64)  # noqa: E731


def test_the_objects_of_the_fixture_match_voxels(scene):
    av = _avlmap(scene)
    for name in OBJECTS:
        heat = av.index_object(name)
        assert 0 < int((heat == 1.0).sum()) < len(heat)


def test_index_goal_equals_the_product_of_the_stand_alone_queries(scene):
    av = _avlmap(scene)
    gp = av.vlmap.grid_pos
    combos = [
        (dict(obj="table", sound="dog"), lambda: [av.index_object("table"), av.index_sound("dog")]),
        (dict(obj="table", area="kitchen"), lambda: [av.index_object("table"), av.index_area("kitchen")]),
        (dict(area="kitchen", sound="dog", img=IMG), lambda: [av.index_area("kitchen"), av.index_sound("dog"), av.index_image(IMG)]),
        (dict(obj="table", area="kitchen", sound="dog", img=IMG),
         lambda: [av.index_object("table"), av.index_area("kitchen"), av.index_sound("dog"), av.index_image(IMG)]),
        (dict(obj=["table", "rug"]), lambda: [av.index_object("table"), av.index_object("rug")]),
        (dict(obj=("table", 0.03), area=[("kitchen", 0.02), "bedroom"], sound="clock tick", decay_rates={"sound": 0.05}),
         lambda: [av.index_object("table", decay_rate=0.03), av.index_area("kitchen", decay_rate=0.02), av.index_area("bedroom"),
                  av.index_sound("clock tick", decay_rate=0.05)]),
    ]
    for kwargs, parts in combos:
        want = np_product(parts())
        goal = av.index_goal(**kwargs)
        assert goal.heat.dtype == np.float64 and np.array_equal(goal.heat, want), kwargs
        assert goal.voxel == int(np.argmax(want)) and goal.value == want[goal.voxel]
        assert goal.pos.tolist() == gp[goal.voxel].tolist() and goal.cell.tolist() == gp[goal.voxel][:2].tolist()
        lean = av.index_goal(want_heat=False, **kwargs)
        assert lean.heat is None and (lean.voxel, lean.value, lean.pos.tolist()) == (goal.voxel, goal.value, goal.pos.tolist())
    # caller-made heats come last, and get_max_pos_3d is grid_pos[first argmax]
    extra = np.random.default_rng(2).random(len(gp)).astype(np.float32)
    want = np_product([av.index_sound("dog"), extra])
    goal = av.index_goal(sound="dog", extra=[extra])
    assert np.array_equal(goal.heat, want) and goal.voxel == int(np.argmax(want))
    for heat in (want, extra):
        assert av.get_max_pos_3d(heat).tolist() == gp[int(np.argmax(heat))].tolist()
    with pytest.raises(ValueError):
        av.get_max_pos_3d(extra[:-1])


def test_index_goal_against_the_reference_arithmetic(scene):
    """every term from the reference's own arithmetic on the CPU (scores from a CPU matmul, scipy distance transforms, the
    occupied_ids loop, a brute-force nearest-target heat).  Each term lies in [0, 1] and the GPU's differs from it by at most
    e = 1e-5 (the bound the stand-alone end-to-end tests hold), so a product of K terms differs by at most K * e, and the voxel the
    GPU picks is within 2 * K * e of the reference's maximum."""
    from test_multimodal_gpu import ref_area_field, ref_image, ref_lift, ref_normalise, ref_sound_field, _ref_cells
    from avlmaps_amd.apps.common import HashAudioText, HashClip
    from avlmaps_amd.utils.clip_utils import get_text_feats
    from avlmaps_amd.utils.mapping_utils import cvt_pose_vec2tf
    e = 1e-5
    sc, _, _ = scene
    av = _avlmap(scene)
    vm = av.vlmap
    gp, N = vm.grid_pos, len(vm.grid_pos)
    poses = np.loadtxt(sc / "poses.txt")
    # object: argmax of the CPU score matmul == 0 (the name beats "other"), then visualize_utils.py:29-49 by brute force
    q = np.asarray(vm._text_feats(["table"]), dtype=np.float32)
    mask = np.argmax(np.asarray(vm.grid_feat, np.float32) @ q.T, axis=1) == 0
    tgt = gp[mask].astype(np.float64)
    d = np.concatenate([np.linalg.norm(tgt[None] - gp[i:i + 256, None, :].astype(np.float64), axis=2).min(1) / 0.05
                        for i in range(0, N, 256)])
    obj = np.clip(1 - d * 0.1, 0, 1).astype(np.float32)
    obj[mask] = 1.0
    # slow decays, so that the four modalities overlap on this 20 m scene and the maximum of the product is not 0
    rates = {"area": 0.01, "sound": 0.002, "img": 0.002}
    # area
    cells = _ref_cells([cvt_pose_vec2tf(p) for p in poses], sc, av)
    s = (av.area_map.clip_sparse_map @ get_text_feats(["kitchen"], HashClip(768), 768).T).flatten()
    s = (s - np.min(s)) / (np.max(s) - np.min(s))
    area = ref_lift(ref_normalise(ref_area_field(cells, s, 400, rates["area"])), vm.occupied_ids, N)
    # sound
    db = pickle.loads((sc / "audio_video" / "audio_data_level_3.pkl").read_bytes())
    A = np.stack([db[i]["audio_features"] for i in range(len(db))])
    cats = av.sound_map.sound_categories
    cell_lists = []
    for i in range(len(db)):
        tfs = []
        for p in db[i]["locations"]:
            tf = np.eye(4)
            tf[:3, 3] = p
            tfs.append(tf)
        cell_lists.append(_ref_cells(tfs, sc, av))
    p = ((np.float32(100.0) * A) @ HashAudioText().encode_text(cats).T)[:, cats.index("dog")]
    p = (p - np.min(p)) / (np.max(p) - np.min(p))
    sound = ref_lift(ref_normalise(ref_sound_field(cell_lists, p, 400, rates["sound"])), vm.occupied_ids, N)
    # image
    row, col = _ref_cells([cvt_pose_vec2tf(poses[IMAGE_POSE])], sc, av)[0]
    image = ref_image(gp, row, col, 1.5 / 0.05, rates["img"])
    for kwargs, parts in ((dict(obj="table", sound="dog"), [obj, sound]), (dict(area="kitchen", sound="dog", img=IMG), [area, sound, image]),
                          (dict(obj="table", area="kitchen", sound="dog", img=IMG), [obj, area, sound, image])):
        kwargs["decay_rates"] = rates
        K = len(parts)
        want = np_product(parts)
        goal = av.index_goal(**kwargs)
        err = float(np.abs(goal.heat - want).max())
        print(f"K = {K}: max |heat - reference| = {err:.3e}, reference at the goal {want[goal.voxel]!r}, reference maximum {want.max()!r}")
        assert err <= K * e
        assert want.max() > 0 and want[goal.voxel] >= want.max() - 2 * K * e


def test_index_goal_raises_what_the_stand_alone_queries_raise(scene):
    from avlmaps_amd.apps.common import HashClip
    from avlmaps_amd.map import AVLMap
    from avlmaps_amd.map.avlmap import MissingSubMap
    sc, _, cfg = scene
    av = _avlmap(scene, localizer=False)
    with pytest.raises(MissingSubMap):                                   # no localiser attached
        av.index_goal(obj="table", img=IMG)
    av.visual_map.localizer = lambda img, K: None
    with pytest.raises(ValueError, match="localised"):
        av.index_goal(sound="dog", img=IMG)
    with pytest.raises(KeyError):
        av.index_goal(obj="table", sound="zebra")
    bare = AVLMap(cfg, data_dir=str(sc), area_text_model=HashClip(768))   # no sound configuration at all
    assert bare.load_map(str(sc))
    with pytest.raises(MissingSubMap):
        bare.index_goal(area="kitchen", sound="dog")
    bare._area_loaded = False
    with pytest.raises(MissingSubMap):
        bare.index_goal(area="kitchen")
    # a degenerate field: every sound segment at one probability 0 -> the 2-D map is constant
    real = av.sound_map.get_distribution_and_locations
    av.sound_map.get_distribution_and_locations = lambda name: (np.zeros_like(real(name)[0]), real(name)[1])
    with pytest.raises(ValueError, match="constant"):
        av.index_sound("dog")
    with pytest.raises(ValueError, match="constant"):
        av.index_goal(obj="table", sound="dog")
    av.sound_map.get_distribution_and_locations = real
    # an object no voxel matches: the name loses against "other" everywhere
    vm = av.vlmap
    q = np.asarray(vm._text_feats(["table"]), dtype=np.float32)
    saved, vm.grid_feat = vm.grid_feat, np.tile(q[1], (len(vm.grid_pos), 1)).astype(np.float32)
    try:
        with pytest.raises(ValueError, match="argmin of an empty sequence"):
            av.index_object("table")
        with pytest.raises(ValueError, match="argmin of an empty sequence"):
            av.index_goal(obj="table", sound="dog")
    finally:
        vm.grid_feat = saved


def _reachable_start(vm, goal_of):
    """a free cell of the map's obstacle crop from which the planner reaches goal_of(start) in at least one step: the free cells
    nearest to the goal are tried first (a goal voxel can sit in a pocket that the rest of the map does not reach)"""
    from avlmaps_amd.navigator import Navigator
    from avlmaps_amd.utils.navigation_utils import NoPathError
    nav = Navigator()
    nav.build_visgraph(vm.obstacles_cropped, vm.rmin, vm.cmin)
    try:
        free = np.argwhere(vm.obstacles_cropped) + np.array([vm.rmin, vm.cmin])
        g0 = np.asarray(goal_of([float(free[0][0]), float(free[0][1])]), dtype=np.float64)
        order = np.argsort(((free - g0) ** 2).sum(1), kind="stable")
        for r, c in free[order][1:600]:
            start = [float(r), float(c)]
            g = goal_of(start)
            try:
                if len(nav.plan_to(start, [float(g[0]), float(g[1])])) >= 2:
                    return start
            except NoPathError:
                continue
    finally:
        nav.close()
    raise AssertionError("no free cell near the goal reaches it")


def test_apps(scene, capsys):
    from avlmaps_amd.apps import index_map, plan_path
    from avlmaps_amd.apps.common import FixedPoseLocalizer, load_config
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.apps.common import HashClip
    from avlmaps_amd.utils.mapping_utils import load_rgb_png
    sc, cfg_path, _ = scene
    av = _avlmap(scene)
    vm = av.vlmap
    base = ["--data-dir", str(sc), "--config", str(cfg_path), "--text-model", "hash"]
    img = sorted((sc / "rgb").glob("*.png"))[2]
    av.visual_map.localizer = FixedPoseLocalizer(np.loadtxt(sc / "poses.txt")[2], vm.base2cam_tf)
    save = sc / "fused.npy"
    heat = index_map.main(base + ["--modality", "fused", "--object", "table", "--object", "rug", "--area", "kitchen", "--sound", "dog",
                                  "--image", str(img), "--image-pose", "2", "--sound-decay", "0.02", "--save", str(save)])
    goal = av.index_goal(obj=["table", "rug"], area="kitchen", sound="dog", img=load_rgb_png(img), decay_rates={"sound": 0.02})
    assert heat.dtype == np.float64 and np.array_equal(heat, goal.heat) and np.array_equal(np.load(save), goal.heat)
    assert f"goal voxel id {goal.voxel} at grid_pos {goal.pos.tolist()}" in capsys.readouterr().out
    # plan_path: a cross-modal goal
    vm.init_categories(["table", "other"])
    vm.generate_obstacle_map()
    goal = av.index_goal(obj="table", sound="dog")
    start = _reachable_start(vm, lambda s: plan_path.clamp_cell(goal.cell, vm.rmin, vm.cmin, vm.obstacles_cropped.shape))
    argv = base + ["--query", "table", "--start", str(start[0]), str(start[1])]
    out = plan_path.main(argv + ["--sound", "dog"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    assert out["goal_cell"] == [float(goal.cell[0]), float(goal.cell[1])] and out["goal_voxel"] == goal.voxel
    assert out["goal_value"] == goal.value and out["path"][0] == start
    assert out["goal"] == [float(x) for x in plan_path.clamp_cell(goal.cell, vm.rmin, vm.cmin, vm.obstacles_cropped.shape)]
    H, W = vm.obstacles_cropped.shape
    assert vm.rmin <= out["goal"][0] < vm.rmin + H and vm.cmin <= out["goal"][1] < vm.cmin + W
    # without the new flags: Map.get_nearest_pos, as before
    ref = VLMap(load_config(str(cfg_path)).map_config, data_dir=str(sc))
    assert ref.load_map(str(sc))
    ref.clip_feat_dim = ref.grid_feat.shape[1]
    ref.clip_model = HashClip(ref.clip_feat_dim)
    ref.init_categories(["sofa", "other"])
    ref.generate_obstacle_map()
    start = _reachable_start(ref, lambda s: ref.get_nearest_pos(s, "sofa"))
    want = ref.get_nearest_pos(start, "sofa")
    old = plan_path.main(base + ["--query", "sofa", "--start", str(start[0]), str(start[1])])
    assert old["goal"] == [float(want[0]), float(want[1])] and set(old) == {"query", "start", "goal", "path"} and old["path"][0] == start


def test_plan_path_clamps_a_goal_outside_the_crop(scene, monkeypatch, capsys):
    """a goal voxel above the height band, in a column nothing inside the band reaches: its cell lies outside the cropped obstacle
    map, where plan_to_pos_v2 raises ValueError.  plan_path clamps the cell into the crop and reports both cells."""
    from avlmaps_amd.apps import plan_path
    from avlmaps_amd.map import AVLMap, Goal
    from avlmaps_amd.navigator import Navigator
    sc, cfg_path, _ = scene
    av = _avlmap(scene)
    vm = av.vlmap
    vm.generate_obstacle_map()
    H, W = vm.obstacles_cropped.shape
    far = np.array([vm.rmin + H + 6, vm.cmin - 4, 39], np.int32)
    start = _reachable_start(vm, lambda s: [vm.rmin + H - 1, vm.cmin])
    nav = Navigator()
    nav.build_visgraph(vm.obstacles_cropped, vm.rmin, vm.cmin)
    with pytest.raises(ValueError):
        nav.plan_to(start, [float(far[0]), float(far[1])])             # what an unclamped goal would do
    nav.close()
    monkeypatch.setattr(AVLMap, "index_goal", lambda self, **kw: Goal(None, 7, 0.5, far))
    out = plan_path.main(["--data-dir", str(sc), "--config", str(cfg_path), "--text-model", "hash", "--query", "table", "--sound", "dog",
                          "--start", str(start[0]), str(start[1])])
    assert out["goal_cell"] == [float(far[0]), float(far[1])] and out["goal"] == [float(vm.rmin + H - 1), float(vm.cmin)]
    assert out["goal_voxel"] == 7 and out["goal_value"] == 0.5 and out["path"][0] == start
