"""End-to-end GPU tests through the reference-shaped Python API (VLMapBuilder / VLMap / AVLMap)."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_host_mirror import Cfg, make_cfg  # noqa: E402


class MemoryBuilder:
    """VLMapBuilder fed from arrays instead of rgb/*.png + depth/*.npy"""

    @staticmethod
    def make(g, tmp_path, feats_as="numpy_chw"):
        from avlmaps_amd.map.map import Map
        from avlmaps_amd.map.vlmap_builder import VLMapBuilder
        cfg = make_cfg(g)
        m = Map(cfg)
        nfr = len(g["depths"])
        pose_path = tmp_path / "poses.txt"
        np.savetxt(pose_path, g["poses"])
        counter = {"i": 0}

        def extractor(rgb):
            f = g["feats"][counter["i"]][None]           # reference layout (1, D, Hf, Wf)
            counter["i"] += 1
            if feats_as == "torch_hwc":
                import torch
                return torch.from_numpy(np.ascontiguousarray(np.transpose(f[0], (1, 2, 0)))).cuda()
            if feats_as == "torch_refill":               # an extractor that REFILLS one output buffer: deferred fuse would read it late
                import torch
                t = torch.from_numpy(np.ascontiguousarray(np.transpose(f[0], (1, 2, 0))))
                if "buf" not in counter:
                    counter["buf"] = torch.empty(t.shape, dtype=t.dtype, device="cuda")
                counter["buf"].copy_(t)
                return counter["buf"]
            if feats_as == "torch_views":                # views at ALTERNATING offsets of one persistent buffer: different data
                import torch                             # pointers frame to frame, the same storage
                t = torch.from_numpy(np.ascontiguousarray(np.transpose(f[0], (1, 2, 0))))
                if "ring" not in counter:
                    counter["ring"] = torch.empty((2,) + tuple(t.shape), dtype=t.dtype, device="cuda")
                v = counter["ring"][(counter["i"] - 1) % 2]
                v.copy_(t)
                return v
            if feats_as == "torch_late_refill":          # fresh storage for the first three frames, then ONE buffer refilled
                import torch
                t = torch.from_numpy(np.ascontiguousarray(np.transpose(f[0], (1, 2, 0))))
                if counter["i"] <= 3:
                    return t.cuda()
                if "buf" not in counter:
                    counter["buf"] = torch.empty(t.shape, dtype=t.dtype, device="cuda")
                counter["buf"].copy_(t)
                return counter["buf"]
            return f

        b = VLMapBuilder(tmp_path, cfg, pose_path, [None] * nfr, [None] * nfr, m.base2cam_tf, m.base_transform,
                         feat_extractor=extractor)
        b.load_frame = lambda i: (g["rgbs"][i], g["depths"][i])
        b.capacity = 4000
        return b


@pytest.mark.parametrize("feats_as,batch", [("numpy_chw", 1), ("torch_hwc", 1), ("torch_hwc", 4), ("numpy_chw", 2),
                                            ("torch_hwc", "deferred"), ("numpy_chw", "deferred"), ("torch_refill", 1), ("torch_views", 1), ("torch_hwc", "off")])
def test_vlmapbuilder_reproduces_reference_map(golden, tmp_path, feats_as, batch):
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    g = golden("g2a_builder_small.npz")
    b = MemoryBuilder.make(g, tmp_path, feats_as)
    if batch == "deferred":                  # one launch per frame; checkpoints (save_every) flush the pending fusion
        b.deferred_fuse, b.save_every, batch = True, 3, 1
    elif batch == "off":
        b.deferred_fuse, batch = False, 1
    auto = b.deferred_fuse == "auto"
    b.batch_frames = batch
    np.random.seed(1234)                     # same global-RNG state the reference run had
    b.create_mobile_base_map()
    if auto and batch == 1:
        # deferred fuse is the default now, decided on probation: an extractor that hands out fresh storage per frame (any torch
        # model; NumPy features are staged by the builder) gets one launch per frame, one that refills a single buffer does not
        # (two views at alternating offsets of one buffer do not overlap: frame i - 1's features are fused by frame i's launch,
        # queued before the extractor refills that half for frame i + 1 -- compared by address range)
        assert b.deferred_fuse_active == (feats_as != "torch_refill")
    it, gf, gp, w, occ, rgb = load_3d_map(tmp_path / "vlmap" / "vlmaps.h5df")
    assert it == list(range(len(g["depths"])))
    assert np.array_equal(gp, g["grid_pos"]) and gp.dtype == np.int32
    nz = np.argwhere(occ != -1)
    assert np.array_equal(nz, g["occ_nz"]) and np.array_equal(occ[nz[:, 0], nz[:, 1], nz[:, 2]], g["occ_nz_vals"])
    np.testing.assert_allclose(gf, g["grid_feat"], rtol=2e-5, atol=3e-4)
    np.testing.assert_allclose(w, g["weight"], rtol=3e-7)
    assert np.array_equal(rgb, g["grid_rgb"])                     # replay log on by default: sequential uint8 colour
    assert gf.dtype == np.float32 and w.dtype == np.float32 and rgb.dtype == np.uint8 and occ.dtype == np.int32


@pytest.mark.parametrize("name,deferred", [("g2a_builder_small.npz", "auto"), ("g2b_builder_growth.npz", "auto"), ("g2b_builder_growth.npz", False)])
def test_vlmapbuilder_feeds_the_c_frame_loop(golden, tmp_path, name, deferred):
    """create_mobile_base_map hands consecutive staged frames to avl_builder_integrate_frames (the frame loop in C: K1's PreGather
    instantiations) once the extractor has been seen to hand out fresh storage; the map is the reference's, as with one call per frame"""
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    g = golden(name)
    b = MemoryBuilder.make(g, tmp_path, "torch_hwc")
    b.deferred_fuse, b.frame_loop_eager, b.frame_loop_max_extract_s = deferred, True, 60.0
    np.random.seed(1234 if name.startswith("g2a") else 99)
    b.create_mobile_base_map()
    nfr = len(g["depths"])
    assert b.build_times["c_loop_calls"] >= 1 and 2 <= b.build_times["frames_in_c_loop_calls"] <= nfr
    if nfr >= 16:
        assert b.build_times["frames_in_c_loop_calls"] >= 8
    it, gf, gp, w, occ, rgb = load_3d_map(tmp_path / "vlmap" / "vlmaps.h5df")
    assert it == list(range(nfr)) and np.array_equal(gp, g["grid_pos"])
    np.testing.assert_allclose(gf, g["grid_feat"], rtol=2e-5, atol=3e-4)
    if name.startswith("g2a"):
        assert np.array_equal(rgb, g["grid_rgb"])
        np.testing.assert_allclose(w, g["weight"], rtol=3e-7)
    # ... and bit for bit the map of one call per frame
    one = tmp_path / "one"
    one.mkdir()
    b1 = MemoryBuilder.make(g, one, "torch_hwc")
    b1.deferred_fuse, b1.frame_loop_frames = deferred, 1
    np.random.seed(1234 if name.startswith("g2a") else 99)
    b1.create_mobile_base_map()
    assert b1.build_times["c_loop_calls"] == 0
    ref = load_3d_map(one / "vlmap" / "vlmaps.h5df")
    for a, c in zip((it, gf, gp, w, occ, rgb), ref):
        assert np.array_equal(a, c)


def test_a_ring_of_feature_buffers_limits_the_frames_held_back(golden, tmp_path):
    """an extractor cycling through FOUR output buffers: the builder sees the recycling distance and never holds back (or defers)
    more frames than half of it -- the reference's map, no 'reused the storage' error"""
    import torch
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    g = golden("g2b_builder_growth.npz")
    b = MemoryBuilder.make(g, tmp_path, "torch_hwc")
    inner = b.feat_extractor
    ring, k = [None] * 4, [0]

    def extractor(rgb):
        t = inner(rgb)
        if ring[k[0] % 4] is None:
            ring[k[0] % 4] = torch.empty_like(t)
        ring[k[0] % 4].copy_(t)
        k[0] += 1
        return ring[(k[0] - 1) % 4]
    b.feat_extractor, b.frame_loop_eager, b.frame_loop_max_extract_s = extractor, True, 60.0
    np.random.seed(99)
    b.create_mobile_base_map()
    assert b.deferred_fuse_active and b.build_times["c_loop_calls"] >= 1
    assert b.build_times["frames_in_c_loop_calls"] <= 2 * b.build_times["c_loop_calls"]       # never more than two frames per call
    assert np.array_equal(load_3d_map(tmp_path / "vlmap" / "vlmaps.h5df")[2], g["grid_pos"])


def test_extractor_that_starts_recycling_late_fails_loudly(golden, tmp_path):
    """deferred fuse on probation saw fresh storage for the first frames; an extractor that LATER refills one buffer would have its
    features fused a frame late -- the builder notices the repeated storage and raises instead of writing a wrong map"""
    g = golden("g2a_builder_small.npz")
    if len(g["depths"]) < 6:
        pytest.skip("needs six frames")
    b = MemoryBuilder.make(g, tmp_path, "torch_late_refill")
    np.random.seed(1234)
    with pytest.raises(RuntimeError, match="reused the storage"):
        b.create_mobile_base_map()


def test_incremental_checkpoints_write_the_same_file(golden, tmp_path):
    """save_every = 2 over the golden sequence: the first checkpoint is a full write, the later ones and the final save only
    write changed + new rows (MapFileWriter); the finished file is the one a single full save produces = the reference's map"""
    from avlmaps_amd.utils import h5lite
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    if not h5lite.available():
        pytest.skip("libhdf5 not found")
    g = golden("g2a_builder_small.npz")
    files = {}
    for mode in ("incremental", "full"):
        d = tmp_path / mode
        d.mkdir()
        b = MemoryBuilder.make(g, d)
        b.save_every = 2
        b.skip_busy_checkpoints = False          # every checkpoint is written, like upstream (the default skips one that finds the writer busy)
        b.incremental_checkpoints = mode == "incremental"
        np.random.seed(1234)
        b.create_mobile_base_map()
        files[mode] = load_3d_map(d / "vlmap" / "vlmaps.h5df")
        if mode == "incremental":
            st = b._map_writer.stats
            assert [s["mode"] for s in st] == ["full", "incremental", "incremental", "incremental"]     # 3 checkpoints + the final save
            assert all(s["rows_written"] <= s["rows_total"] for s in st) and st[-1]["rows_written"] == 0    # nothing fused since
            assert st[1]["rows_written"] <= st[1]["rows_total"] and st[1]["rows_dirty"] < st[1]["rows_total"]   # whole 64-row chunks go out
    a, f = files["incremental"], files["full"]
    assert a[0] == f[0] == list(range(len(g["depths"])))
    for x, y, k in zip(a[1:], f[1:], ("grid_feat", "grid_pos", "weight", "occupied_ids", "grid_rgb")):
        assert np.array_equal(x, y) and x.dtype == y.dtype, k
    assert np.array_equal(a[2], g["grid_pos"]) and np.array_equal(a[5], g["grid_rgb"])


def test_resume_appends_on_top_of_saved_map(golden, tmp_path):
    """second run finds the map file, imports it and fuses all frames again (upstream resume semantics)"""
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    g = golden("g2a_builder_small.npz")
    np.random.seed(1234)
    MemoryBuilder.make(g, tmp_path).create_mobile_base_map()
    first = load_3d_map(tmp_path / "vlmap" / "vlmaps.h5df")
    np.random.seed(1234)
    MemoryBuilder.make(g, tmp_path).create_mobile_base_map()
    second = load_3d_map(tmp_path / "vlmap" / "vlmaps.h5df")
    assert np.array_equal(second[2], first[2])                       # same voxels, same ids
    np.testing.assert_allclose(second[3], 2 * first[3], rtol=1e-5)   # every weight doubled
    # second pass: no voxel is new, so row = (old_row * W + sum alpha*f) / 2W = old_row + a1(1-a1) f1 / 2W:
    # identical direction, bounded by the largest feature magnitude (14.29 * alpha quirk aside)
    assert np.isfinite(second[1]).all() and np.abs(second[1]).max() <= 14.3
    # opt-in fix of the upstream quirk: skip the frames the file already lists -> nothing is fused again, the map is unchanged
    np.random.seed(1234)
    b = MemoryBuilder.make(g, tmp_path)
    b.skip_mapped_frames = True
    b.create_mobile_base_map()
    third = load_3d_map(tmp_path / "vlmap" / "vlmaps.h5df")
    assert third[0] == second[0] and np.array_equal(third[2], second[2])
    np.testing.assert_allclose(third[3], second[3], rtol=1e-6)
    np.testing.assert_allclose(third[1], second[1], rtol=1e-5, atol=1e-5)


class FakeClip:
    """OpenAI-CLIP shaped stub: tokenize() -> ids, encode_text(ids) -> rows of a fixed table"""

    def __init__(self, D, seed=0):
        self.D, self.rng, self.vocab, self.rows = D, np.random.default_rng(seed), {}, []

    def tokenize(self, texts):
        import torch
        ids = []
        for t in texts:
            if t not in self.vocab:
                self.vocab[t] = len(self.rows)
                self.rows.append(self.rng.standard_normal(self.D).astype(np.float32))
            ids.append(self.vocab[t])
        return torch.tensor(ids, dtype=torch.int64)

    def encode_text(self, ids):
        import torch
        return torch.from_numpy(np.stack([self.rows[i] for i in ids.cpu().tolist()])).to(ids.device)


def test_vlmap_index_and_avlmap_index_object(golden):
    from avlmaps_amd.map import AVLMap, VLMap
    from avlmaps_amd.utils.clip_utils import get_lseg_score, get_text_feats, multiple_templates
    from oracle import avl_oracle as O
    g3, g4 = golden("g3_similarity.npz"), golden("g4_heatmap.npz")
    cfg = Cfg(map_config=Cfg(map_type="vlmap", grid_size=1000, cell_size=0.05,
                             pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                                           base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0])),
              params=Cfg(cs=0.05))
    av = AVLMap(cfg)
    vm = av.vlmap
    n = len(g4["grid_pos"])
    vm.grid_feat = g3["feat"][:n] if len(g3["feat"]) >= n else np.resize(g3["feat"], (n, 512))
    vm.grid_pos = g4["grid_pos"]
    vm.clip_model = FakeClip(512)
    vm.clip_feat_dim = 512
    # expected through the oracle on the same text features
    prompts = [t.format(lm) for lm in ["sofa", "other"] for t in multiple_templates]
    tf = get_text_feats(prompts, vm.clip_model, 512)
    assert np.allclose(np.linalg.norm(tf, axis=1), 1, atol=1e-6)
    q = O.template_mean(tf.reshape(2, 63, 512))
    ref = O.sim_scores(vm.grid_feat, q)
    mask = vm.index_map("sofa", with_init_cat=False)
    margin = np.abs(ref[:, 0] - ref[:, 1]) > 1e-4
    assert mask.dtype == bool and np.array_equal(mask[margin], (np.argmax(ref, 1) == 0)[margin])
    sc = get_lseg_score(vm.clip_model, ["sofa"], vm.grid_feat, 512, use_multiple_templates=True, add_other=True)
    assert sc.shape == (n, 2) and sc.dtype == np.float32 and np.abs(sc - ref).max() < 1e-4
    # avg_mode=1: average of per-template scores
    sc1 = get_lseg_score(vm.clip_model, ["sofa"], vm.grid_feat, 512, use_multiple_templates=True, avg_mode=1)
    assert np.abs(sc1 - (vm.grid_feat @ tf.T).reshape(n, 2, 63).mean(2)).max() < 1e-4
    # init_categories caches (N, Q) scores; "other" is appended only when missing
    sm = vm.init_categories(["chair", "table", "other"])
    assert sm.shape == (n, 3) and vm.scores_mat is sm
    assert np.array_equal(vm.index_map("table"), np.argmax(sm, 1) == 1)
    with pytest.raises(KeyError):
        vm.index_map("zebra")
    # AVLMap.index_object = mask -> nearest-target decay heat
    heat = av.index_object("sofa", decay_rate=0.01)
    assert heat.shape == (n,) and heat.dtype == np.float32
    assert np.array_equal(heat, O.heatmap_from_mask(vm.grid_pos, mask, 0.05, 0.01))
    plan = vm._heat_plan()                       # the map's cell order is computed once and answers the next query too
    assert plan is not None and np.array_equal(av.index_object("sofa", decay_rate=0.1), O.heatmap_from_mask(vm.grid_pos, mask, 0.05, 0.1))
    assert vm._heat_plan() is plan
    for fn in (av.index_sound, av.index_area, av.index_image):
        with pytest.raises(NotImplementedError):
            fn("x")


def test_config1_through_the_api(golden):
    """the same case through the mirrored API: get_lseg_score + VLMap.index_map(with_init_cat=False) with the text features the
    reference was given (a stand-in text tower that looks them up), on the 50 000-voxel map"""
    from avlmaps_amd.map.vlmap import VLMap
    from avlmaps_amd.utils import clip_utils as cu
    g = golden("g9_config1.npz")
    feat = np.random.default_rng(0).standard_normal((50_000, 512)).astype(np.float32)
    table = {}
    for li, lm in enumerate(("sofa", "other")):
        for ti, t in enumerate(cu.multiple_templates):
            table[t.format(lm)] = g["template_feats"][li, ti]
        table[lm] = g["single_feats"][li]

    def lookup(in_text, clip_model, clip_feat_dim, batch_size=64):
        return np.stack([table[t] for t in in_text]).astype(np.float32)

    old = cu.get_text_feats
    cu.get_text_feats = lookup
    try:
        sc = cu.get_lseg_score(None, ["sofa"], feat, 512, use_multiple_templates=True, add_other=True)
        np.testing.assert_allclose(np.asarray(sc), g["scores"], rtol=0, atol=1e-5)
        sc1 = cu.get_lseg_score(None, ["sofa"], feat, 512, use_multiple_templates=False, add_other=True)
        np.testing.assert_allclose(np.asarray(sc1), g["single_scores"], rtol=0, atol=1e-5)
        vm = VLMap(Cfg(map_type="vlmap", grid_size=1000, cell_size=0.05,
                       pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                                     base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0])))
        vm.grid_feat, vm.clip_model, vm.clip_feat_dim = feat, None, 512
        mask = np.asarray(vm.index_map("sofa", with_init_cat=False))
    finally:
        cu.get_text_feats = old
    clear = np.abs(g["scores"][:, 0] - g["scores"][:, 1]) > 2e-5
    assert mask.dtype == bool and mask.shape == (50_000,)
    assert np.array_equal(mask[clear], g["index_map_mask"][clear])


def test_vlmap_with_the_compact_resident_copy(golden):
    """VLMap.compact_map (default) keeps the 3-byte resident copy, False the 4-byte one: index_map / init_categories / index_object
    agree wherever the top-2 gap exceeds 2e-5, scores within 1e-5 of each other (g3 features)"""
    from avlmaps_amd.map import AVLMap
    from avlmaps_amd.ops import PreparedMap
    g3, g4 = golden("g3_similarity.npz"), golden("g4_heatmap.npz")
    cfg = Cfg(map_config=Cfg(map_type="vlmap", grid_size=1000, cell_size=0.05,
                             pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                                           base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0])),
              params=Cfg(cs=0.05))
    n = len(g4["grid_pos"])
    feat = g3["feat"][:n] if len(g3["feat"]) >= n else np.resize(g3["feat"], (n, 512))
    res = {}
    for compact in (False, True):
        av = AVLMap(cfg)
        vm = av.vlmap
        vm.compact_map = compact
        vm.grid_feat, vm.grid_pos, vm.clip_model, vm.clip_feat_dim = feat, g4["grid_pos"], FakeClip(512), 512
        mask = vm.index_map("sofa", with_init_cat=False)
        assert isinstance(vm._dev_feat, PreparedMap) and vm._dev_feat.compact == compact
        sm = vm.init_categories(["chair", "table", "sofa", "other"])
        heat = av.index_object("sofa", decay_rate=0.01)
        res[compact] = (mask, sm, heat)
    (m0, s0, h0), (m1, s1, h1) = res[False], res[True]
    assert np.abs(s1 - s0).max() < 1e-5                                    # measured ~2e-6
    gap = np.sort(s0, axis=1)
    clear = gap[:, -1] - gap[:, -2] > 2e-5
    assert np.array_equal(np.argmax(s1, 1)[clear], np.argmax(s0, 1)[clear]) and np.mean(m0 == m1) > 0.999
    assert h1.shape == h0.shape and np.mean(h0 == h1) > 0.99


def test_dynamic_obstacles_map_matches_numpy_restatement(golden):
    """index_utils.py:138-184 on the GPU vs a NumPy evaluation of the same definition"""
    from avlmaps_amd.utils.clip_utils import landmark_text_feats
    from avlmaps_amd.utils.index_utils import get_dynamic_obstacles_map_3d
    from oracle import avl_oracle as O
    g3, g4 = golden("g3_similarity.npz"), golden("g4_heatmap.npz")
    pos = g4["grid_pos"]
    n = len(pos)
    feat = np.resize(g3["feat"], (n, 512)).astype(np.float32)
    clip = FakeClip(512, seed=3)
    potential = ["chair", "wall", "wall above the door", "table", "window", "floor", "stairs", "other"]
    obstacles = ["wall", "chair", "table", "window", "stairs", "other"]
    rmin, cmin = int(pos[:, 0].min()), int(pos[:, 1].min())
    cropped = np.ones((int(pos[:, 0].max()) - rmin + 1, int(pos[:, 1].max()) - cmin + 1), dtype=bool)
    cropped[pos[::2, 0] - rmin, pos[::2, 1] - cmin] = False          # every other voxel column is an obstacle cell
    got = get_dynamic_obstacles_map_3d(clip, cropped, potential, obstacles, feat, pos, rmin, cmin, 512)
    q, _ = landmark_text_feats(clip, list(potential), 512, True, True)
    sc = O.sim_scores(feat, q)
    srt = np.sort(sc, axis=1)
    safe = (srt[:, -1] - srt[:, -2]) > 1e-4                           # ignore numerically tied rows
    predict = np.argmax(sc, axis=1)
    ids = [potential.index(o) for o in obstacles]
    want = np.zeros_like(cropped)
    sel = np.isin(predict, ids)
    want[pos[sel, 0] - rmin, pos[sel, 1] - cmin] = True
    want = ~(want & (cropped == 0))
    if safe.all():
        assert np.array_equal(got, want)
    assert got.dtype == bool and got.shape == cropped.shape and (got != want).mean() < 0.01


def test_cli_create_then_index_on_disk_dataset(tmp_path):
    """apps.create_map + apps.index_map on a synthetic scene in the reference's on-disk layout (png / npy / poses.txt)"""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map, index_map
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    scene = make(tmp_path / "scene", frames=6, H=96, W=128)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                  "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(scene), "--config", str(cfg), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    it, gf, gp, w, occ, rgb = load_3d_map(scene / "vlmap" / "vlmaps.h5df")
    assert it == list(range(6)) and gf.shape[1] == 64 and len(gp) > 500 and occ.shape == (400, 400, 30)
    assert (occ >= 0).sum() == len(gp) and np.array_equal(occ[gp[:, 0], gp[:, 1], gp[:, 2]], np.arange(len(gp)))
    heat = index_map.main(["--data-dir", str(scene), "--config", str(cfg), "--query", "sofa", "--text-model", "hash"])
    assert heat.shape == (len(gp),) and heat.max() == 1.0
    # the voxels that match are the ones the float64 product ranks first -- including the many rows of magnitude 1e-7 this
    # scene has (voxels seen once from far away, feat * exp(-r^2/1.2)): the unscaled fp16 split of round 1 flushed them to
    # zero and called them "other"
    from avlmaps_amd.apps.common import HashClip
    from avlmaps_amd.utils.clip_utils import landmark_text_feats
    q, _ = landmark_text_feats(HashClip(64), ["sofa"], 64, use_multiple_templates=True, add_other=True)
    ref = gf.astype(np.float64) @ q.astype(np.float64).T
    clear = np.abs(ref[:, 0] - ref[:, 1]) > 1e-5 * np.abs(ref).max(axis=1)
    assert np.abs(gf).max(axis=1).min() < 1e-5 and clear.mean() > 0.9
    assert np.array_equal((heat == 1.0)[clear], (ref.argmax(axis=1) == 0)[clear])
    # host-side pipelining (frame decode threads, sampler thread, batched launches) must not change a single bit:
    # the default above ran with prefetch 4; inline loading and 3-frame batches give the same file contents
    first = (it, gf, gp, w, occ, rgb)
    for extra in (["--prefetch", "0"], ["--prefetch", "2", "--batch-frames", "3"]):
        for f in (scene / "vlmap").iterdir():
            f.unlink()
        create_map.main(["--data-dir", str(scene), "--config", str(cfg), "--features", "hash", "--feat-dim", "64", "--seed", "3"] + extra)
        again = load_3d_map(scene / "vlmap" / "vlmaps.h5df")
        assert again[0] == first[0]
        for a, b, name in zip(again[1:], first[1:], ("grid_feat", "grid_pos", "weight", "occupied_ids", "grid_rgb")):
            if name == "grid_feat" and extra[-2:] == ["--batch-frames", "3"]:
                np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6)     # fp64 sums in a different order
            else:
                assert np.array_equal(a, b), (name, extra)


def test_multi_floor_builder_reproduces_reference_map(golden, tmp_path):
    """VLMapBuilderMultiFloor.create_global_map vs the reference run (two passes, np.round indices, capacity doubling)"""
    check_multi_floor_builder(golden("g6_multi_floor.npz"), tmp_path)


def check_multi_floor_builder(g, tmp_path):
    """the product's two-pass builder on the frames, poses and seed of a reference run (tools/gen_golden.py) against its arrays"""
    from avlmaps_amd.map import VLMapBuilderMultiFloor
    nfr = len(g["depths_u16"])
    cfg = Cfg(cell_size=float(g["cs"]), depth_sample_rate=int(g["rate"]), skip_frame=1, grid_size=1000,
              cam_calib_mat=[float(x) for x in g["calib"]], pose_info=Cfg(camera_height=1.5, building_init_height=0.0))
    counter = {"i": 0}

    def extractor(rgb):
        f = g["feats"][counter["i"]][None]
        counter["i"] += 1
        return f

    b = VLMapBuilderMultiFloor(tmp_path, cfg, [None] * nfr, [None] * nfr, [None] * nfr, None, None, feat_extractor=extractor)
    b.load_frame = lambda i: (g["rgbs"][i], g["depths_u16"][i])
    b.load_pose = lambda i: g["poses"][i]
    b.capacity = 8000
    np.random.seed(777)                      # the seed the reference run had (tools/gen_golden.py)
    b.create_global_map()
    assert np.array_equal(b.pcd_min, g["pcd_min"]) and np.array_equal(b.pcd_max, g["pcd_max"])      # bit-exact bbox
    assert np.array_equal(b.grid_size, g["grid_size"])
    it, gf, gp, w, occ, rgb, pmin, pmax, cs = VLMapBuilderMultiFloor.load_3d_map(tmp_path / "vlmap_multi_floor" / "vlmaps_multi_floor.h5df")
    assert it == list(range(nfr)) and cs == float(g["cs"]) and np.array_equal(pmin, g["pcd_min"])
    assert np.array_equal(gp, g["grid_pos"])                                                         # ids + order
    assert tuple(occ.shape) == tuple(g["occ_shape"])
    nz = np.argwhere(occ != -1)
    assert np.array_equal(nz, g["occ_nz"]) and np.array_equal(occ[nz[:, 0], nz[:, 1], nz[:, 2]], g["occ_nz_vals"])
    np.testing.assert_allclose(gf, g["grid_feat"], rtol=2e-5, atol=3e-4)
    # the builder keeps the replay log: weight and grid_rgb are the reference's sequential values, bit for bit, across the
    # dtype switch (float32 running weight, then float64 once the map outgrew grid_size[0] * grid_size[2] rows)
    assert np.array_equal(w, g["weight"].astype(np.float32))
    assert np.array_equal(rgb, np.floor(g["grid_rgb"]).astype(np.uint8))


def test_get_lseg_feat_protocol_on_the_gpu(golden):
    """the sliding-window LSeg evaluation (lseg_utils.py:20-119) with the image, crops, flips and the averaged output all
    resident on the GPU, channels-last, against the reference run (fake model)"""
    import sys
    from pathlib import Path
    import torch
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    from gen_golden import FakeLSeg
    from avlmaps_amd.utils.lseg_utils import get_lseg_feat

    class CudaFake(FakeLSeg):
        def __call__(self, x, labels):
            f, logits = FakeLSeg.__call__(self, x.cpu(), labels)     # same arithmetic as the generator, result moved back
            return f.to(x.device), logits.to(x.device)

    g = golden("g5_lseg_protocol.npz")
    for name in ("pad_short", "grid_2x3", "tall"):
        crop, base = (int(x) for x in g[f"{name}_cfg"])
        ref = g[f"{name}_feat"]
        fake = CudaFake()
        calls = []
        counted = lambda x, labels: calls.append(int(x.shape[0])) or fake(x, labels)
        counted.out_c = fake.out_c
        f = get_lseg_feat(counted, g[f"{name}_img"], ["example"], None, "cuda", crop, base)
        assert f.is_cuda and f.is_contiguous() and tuple(f.shape) == (ref.shape[2], ref.shape[3], ref.shape[1])
        assert len(calls) == 1 and calls[0] in (2, 6)                 # ONE model call for all windows of the frame
        # the resize runs on the GPU here and on the CPU in the reference run (bilinear weights to the last bit of float32)
        np.testing.assert_allclose(f.cpu().numpy(), np.transpose(ref[0], (1, 2, 0)), rtol=1e-5, atol=1e-5)
        # window by window (what upstream does) gives the same map bit for bit: the merge sums in window order
        f1 = get_lseg_feat(fake, g[f"{name}_img"], ["example"], None, "cuda", crop, base, window_batch_size=1)
        assert torch.equal(f, f1)
        # reference layout on request
        fr = get_lseg_feat(fake, g[f"{name}_img"], ["example"], None, "cuda", crop, base, channels_last=False)
        assert tuple(fr.shape) == ref.shape and torch.equal(fr[0].permute(1, 2, 0), f)
    # the merge kernel alone against its definition, float32 and float16 windows, a channel count that is not a multiple of 64
    from avlmaps_amd.utils.lseg_utils import WindowPlan, merge_windows
    plan = WindowPlan.make(72, 108, 48, 100)
    G, D = len(plan.origins), 70
    win = torch.randn((G, D, 48, 48), device="cuda")
    for w in (win, win.half()):
        acc = torch.zeros((D,) + plan.canvas, device="cuda")
        cnt = torch.zeros((1,) + plan.canvas, device="cuda")
        for (h0, w0), o in zip(plan.origins, w.float()):
            acc[:, h0:h0 + 48, w0:w0 + 48] += o
            cnt[:, h0:h0 + 48, w0:w0 + 48] += 1
        want = (acc / cnt)[:, :plan.height, :plan.width].permute(1, 2, 0)
        assert torch.equal(merge_windows(w, plan), want)


def test_vlmap_indexes_a_fused_visual_audio_map_with_block_queries():
    """BASELINE config 5 through the product: a VLMap whose grid_feat is 512 visual | 1024 audio columns keeps the compact
    resident copy (3 bytes per element) and scores text / audio queries against their own column blocks
    (VLMap.index_queries); results = NumPy's grid_feat @ q.T and its argmax (clip_utils.py:227-229, vlmap.py:123)"""
    from test_host_mirror import Cfg
    from avlmaps_amd.map.vlmap import VLMap
    rng = np.random.default_rng(12)
    N, D, Q = 5000, 1536, 128
    feat = rng.standard_normal((N, D)).astype(np.float32)
    feat *= (14.2857 * (0.05 + 0.95 * rng.random((N, 1)))) / np.linalg.norm(feat, axis=1, keepdims=True)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[0::2, 512:] = 0                      # text queries (interleaved with the audio ones)
    q[1::2, :512] = 0
    cfg = Cfg(map_type="vlmap", grid_size=1000, cell_size=0.05,
              pose_info=Cfg(camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1], base_forward_axis=[0, 0, -1],
                            base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0]))
    vm = VLMap(cfg)
    vm.grid_feat = feat
    am, sc = vm.index_queries(q, want_scores=True)
    assert vm._dev_feat.compact and tuple(vm._dev_feat.feat.shape) == (N, 3 * D)
    want = feat.astype(np.float64) @ q.astype(np.float64).T
    assert sc.shape == (N, Q) and np.abs(sc - want).max() < 2e-5
    assert np.array_equal(am, np.argmax(sc, axis=1))
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-4
    assert np.array_equal(am[clear], np.argmax(want, axis=1)[clear]) and clear.mean() > 0.9
    assert np.array_equal(vm.index_queries(q), am)
    with pytest.raises(ValueError):
        vm.index_queries(q[:, :512])


def test_lseg_adapter_with_a_stub_upstream_model(tmp_path, monkeypatch):
    """lseg_adapter.load_upstream_lseg end to end against a stand-in for the upstream package: same import path, constructor
    call and checkpoint format as vlmap_builder.py:226-264 (LSegEncNet("", arch_option=0, block_depth=0, activation="lrelu",
    crop_size=480), state_dict keys prefixed "net."), a forward that is batch-general like lseg_net.py:287-337.  The real
    weights are not on this machine; what runs here is everything around them: checkpoint loading, the window batch, ONE model
    call per frame, the device merge, channels-last output on the GPU."""
    import sys
    import types
    import torch
    calls = []

    class LSegEncNet(torch.nn.Module):
        out_c = 24

        def __init__(self, labels, arch_option=0, block_depth=0, activation="lrelu", crop_size=480):
            super().__init__()
            assert labels == "" and crop_size == 480 and activation == "lrelu"
            self.conv = torch.nn.Conv2d(3, self.out_c, 3, padding=1)

        def forward(self, x, labelset):
            calls.append(tuple(x.shape))
            f = self.conv(x)
            f = 14.2857 * f / f.norm(dim=1, keepdim=True)
            return f.half().float(), f[:, :1]

    pkg = types.ModuleType("avlmaps")
    pkg.__file__ = str(tmp_path / "avlmaps" / "__init__.py")
    pkg.__path__ = [str(tmp_path / "avlmaps")]
    mods = {"avlmaps": pkg}
    for name in ("avlmaps.lseg", "avlmaps.lseg.modules", "avlmaps.lseg.modules.models", "avlmaps.lseg.modules.models.lseg_net"):
        m = types.ModuleType(name)
        m.__path__ = []
        mods[name] = m
    mods["avlmaps.lseg.modules.models.lseg_net"].LSegEncNet = LSegEncNet
    for k, v in mods.items():
        monkeypatch.setitem(sys.modules, k, v)
    torch.manual_seed(0)
    ref_model = LSegEncNet("")
    ckpt = tmp_path / "avlmaps" / "lseg" / "checkpoints" / "demo_e200.ckpt"
    ckpt.parent.mkdir(parents=True)
    torch.save({"state_dict": {"net." + k: v for k, v in ref_model.state_dict().items()}}, ckpt)
    from avlmaps_amd.lseg_adapter import load_upstream_lseg
    extract = load_upstream_lseg()                                 # default path: <avlmaps>/lseg/checkpoints/demo_e200.ckpt
    rgb = np.random.default_rng(0).integers(0, 256, (72, 108, 3), dtype=np.uint8)
    f = extract(rgb)
    assert f.is_cuda and f.dtype == torch.float32 and f.is_contiguous() and tuple(f.shape) == (347, 520, 24)
    assert calls == [(2, 3, 480, 480)]                            # both windows of the frame in ONE call
    nrm = f.norm(dim=2)                                           # unit directions x logit scale, averaged where the windows overlap
    assert float(nrm.max()) < 14.2857 + 0.05
    single = torch.cat([nrm[:, :320], nrm[:, 480:]], dim=1)       # columns covered by ONE window (window 0: [0, 480), window 1: [320, 800))
    assert torch.allclose(single, torch.full_like(single, 14.2857), atol=0.05)
    # the builder takes it as is
    from avlmaps_amd import ops
    acc = ops.VoxelAccumulator(200, 0.05, 30, 24, capacity=4096)
    depth = np.full((72, 108), 1.0, np.float32)               # z = 1 m -> height cell 20 of 30
    acc.integrate_frame(depth, np.array([54, 0, 54, 0, 54, 36, 0, 0, 1.0]), np.eye(4), np.arange(0, 72 * 108, 7, dtype=np.int32), f, rgb, frame_idx=0)
    assert acc.num_voxels() > 0


def test_bench_line_contract():
    """bench.py prints ONE JSON line with the fields the driver reads (metric/value/unit/n_gpus/steps/warmup/ms_per_step/
    higher_is_better/scaling/vs_baseline/dtype/data/config) plus the roofline object; small shapes, a few steps"""
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    for extra, metric in ((["--voxels", "60000", "--settle-steps", "2", "--no-build-extra", "--no-cpu", "--no-pmc"], "voxel_query_similarities_per_sec"),
                          (["--workload", "build", "--no-cpu"], "map_build_frames_per_sec")):
        r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config", "roofline"):
            assert k in d, k
        assert d["metric"] == metric and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["vs_baseline"] is None
        assert d["value"] > 0 and d["higher_is_better"] is True and d["data"] == "synthetic"
        assert d["scaling"] == ("strong" if metric.startswith("map_build") else "weak")
        assert "traffic" in d["roofline"] and "traffic_source" in d["roofline"]
        if metric.startswith("map_build"):
            ex = d["extra"]
            assert ex["total_frames"] == 3 and ex["merge_finalize_seconds"] > 0 and ex["voxels_merged"] == ex["voxels_local"] > 0
            assert abs(d["value"] - 3 / ex["seconds"]) < 1e-6 * d["value"]          # the finalisation is inside the timed region
            assert ex["single_gpu_merge_path"]["merged_voxels"] == ex["voxels_merged"]
        assert "workload" in d["config"] and "model" not in d["config"]
        rf = d["roofline"]
        assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: what the timed path computed in its last step, as float32 / float64 .npy files of at most 64 MB in all;
    the inputs are seeded, so two runs with the same arguments return the same row argmax"""
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent

    def run(extra, out):
        r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu",
                            "--dump-outputs", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        files = {p.stem: np.load(p) for p in out.glob("*.npy")}
        assert set(files) == set(d["dumped_outputs"]) and all(list(a.shape) == d["dumped_outputs"][k] for k, a in files.items())
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(p.stat().st_size for p in out.glob("*.npy")) <= 64 << 20
        return d, files

    index = ["--voxels", "60000", "--settle-steps", "2", "--no-build-extra", "--no-pmc"]
    _, a = run(index, tmp_path / "a")
    _, b = run(index, tmp_path / "b")
    am = a["argmax"]
    assert am.shape == (60000,) and np.array_equal(am, np.round(am)) and am.min() >= 0 and am.max() < 64
    assert np.array_equal(am, b["argmax"])
    d, m = run(["--workload", "build"], tmp_path / "build")
    n = int(m["num_rows"][0])
    assert n == d["extra"]["voxels_merged"] > 0 and n <= 16384               # 3 frames: every row of the map
    assert np.array_equal(m["row_index"], np.arange(n))
    assert m["grid_feat"].shape == (n, 512) and m["grid_pos"].shape == (n, 3) and m["weight"].shape == (n,) and m["grid_rgb"].shape == (n, 3)
    assert np.isfinite(m["grid_feat"]).all() and np.isfinite(m["weight"]).all() and (m["weight"] >= 0).all() and m["grid_pos"].min() >= 0
    assert len(np.unique(m["grid_pos"], axis=0)) == n
    assert m["occupied_ids"].shape == m["occupied_ids_index"].shape and m["occupied_ids"].max() < n


def test_bench_measures_hbm_traffic_in_the_run():
    """roofline.traffic comes from counter passes of the SAME command on the SAME box (bench.py re-executes itself under
    rocprofv3 --pmc FETCH_SIZE, then --pmc WRITE_SIZE: counter-only runs) -- and the resident-copy lines carry their own roofline"""
    import json
    import shutil
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    base = [sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--voxels", "400000", "--settle-steps", "2",
            "--no-build-extra", "--no-cpu"]
    if shutil.which("rocprofv3") or Path("/opt/rocm/bin/rocprofv3").exists():
        r = subprocess.run(base, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        rf = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["roofline"]
        assert rf["traffic_source"].startswith("in-run"), rf
        alg = 400000 * 512 * 4
        assert 0.9 * alg < rf["traffic_read_bytes"] < 1.25 * alg and rf["traffic"] >= rf["traffic_read_bytes"]
        assert any("sim_split_f16_kernel" in k for k in rf["traffic_kernels"])
    for form, bytes_per_el in (("prepared", 4), ("compact", 3)):
        r = subprocess.run(base + ["--no-pmc", "--resident", form], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["config"]["resident_form"] == form and form in d["config"]["workload"]
        assert abs(d["roofline"]["algorithmic_bytes"] - (400000 * 512 * bytes_per_el + 400000 * 4 + 64 * 512 * 4 + 400000 * 4)) < 1
        assert d["roofline"]["float32_equivalent_speed_frac"] >= d["roofline"]["frac"] * (0.99 if bytes_per_el == 4 else 1.2)
        assert d["extra"]["parity_sample"]["max_abs_err_vs_fp64"] < 1e-4


MAX_RANKS_ON_ONE_GPU = 4      # every rank opens the one GPU, and so do the torch.distributed.run launcher and this test process:
                              # at most six processes on the device


def _run_ranks(nproc, args, port, timeout=900, **env_extra):
    import os
    import subprocess
    import sys
    from pathlib import Path
    assert nproc <= MAX_RANKS_ON_ONE_GPU, nproc
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, AVLMAPS_DIST_BACKEND="gloo")        # several ranks share this box's single GPU
    env.update({k: str(v) for k, v in env_extra.items()})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(root / "tests" / "dist_build_worker.py")] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])


@pytest.mark.parametrize("nproc,n_frames,name,mode", [(2, 6, "g2a_builder_small.npz", "sharded"), (3, 4, "g2a_builder_small.npz", "sharded"),
                                                      (2, 16, "g2b_builder_growth.npz", "sharded"), (3, 16, "g2b_builder_growth.npz", "sharded"),
                                                      (4, 16, "g2b_builder_growth.npz", "sharded"),
                                                      (3, 16, "g2b_builder_growth.npz", "sharded, exchange in chunks of 40 rows"),
                                                      (4, 16, "g2b_builder_growth.npz", "sharded, exchange in chunks of 9 rows"),
                                                      (2, 6, "g2a_builder_small.npz", "reduce"), (2, 16, "g2b_builder_growth.npz", "reduce")])
def test_seeded_multi_rank_build_equals_the_single_rank_map(golden, tmp_path, nproc, n_frames, name, mode):
    """VLMapBuilder under N ranks (one process each, frames sharded contiguously; the device merge -- row-sharded all_to_all of
    every rank's own voxel rows, or ONE dense sum-reduce -- and the chained colour replay) with the global NumPy RNG seeded like
    the reference run: the map file rank 0 writes is the single-rank map -- grid_pos / occupied_ids / grid_rgb / weight
    bit-exact, grid_feat to float64 rounding (identical float32 values but for the odd last bit) -- and, for the full sequence,
    the reference's own map (golden).  (3 ranks, 4 frames: the last shard is empty.)"""
    import json
    from avlmaps_amd import parallel
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    GOLDEN_DIR = Path(__file__).resolve().parent / "golden"
    one, many = tmp_path / "one", tmp_path / "many"
    seed = 1234 if name.startswith("g2a") else 99              # what tools/gen_golden.py seeded the reference run with
    _run_ranks(1, [GOLDEN_DIR / name, one, n_frames, "replay", seed], 29541)
    chunk_rows = int(mode.split()[-2]) if "chunks" in mode else 0        # the payload exchange of every merge in chunks (merge2.merge_sharded_v2)
    mode = mode.split(",")[0]
    _run_ranks(nproc, [GOLDEN_DIR / name, many, n_frames, "replay", seed], 29542, AVL_TEST_MERGE_MODE=mode,
               **(dict(AVLMAPS_MERGE_CHUNK_ROWS=chunk_rows) if chunk_rows else {}))
    a = load_3d_map(one / "vlmap" / "vlmaps.h5df")
    b = load_3d_map(many / "vlmap" / "vlmaps.h5df")
    assert a[0] == b[0] == list(range(n_frames))
    for i, k in ((2, "grid_pos"), (3, "weight"), (4, "occupied_ids"), (5, "grid_rgb")):
        assert np.array_equal(a[i], b[i]), k
        assert a[i].dtype == b[i].dtype
    np.testing.assert_allclose(b[1], a[1], rtol=1e-6, atol=1e-7)
    assert np.mean(a[1] == b[1]) > 0.999                       # (p + q) + r against p + (q + r) in float64, rounded to float32 once
    tim = json.loads((many / "merge_timings.json").read_text())
    assert tim["exact_rgb"] is True and tim["merged_voxels"] == len(a[2]) and tim["local_voxels"] <= tim["merged_voxels"]
    if mode == "sharded":
        M, D = len(a[2]), a[1].shape[1]
        sent = rows = 0
        for r in range(nproc):
            t = json.loads((many / f"merge_timings_rank{r}.json").read_text())
            assert t["mode"].startswith("row-sharded") and t["world_size"] == nproc and t["backend"] == "gloo"
            assert tuple(t["shard_rows"]) == parallel.shard_rows(M, r, nproc) and t["shard_feat_shape"] == [t["own_rows"], D]
            assert t["plan"].startswith("gather plan")           # contiguous frame shards: two all_gathers, one payload all_to_all (merge2.py)
            assert (t["exchange_chunks"] > 1 and t["exchange_chunk_rows"] == chunk_rows) if chunk_rows else t["exchange_chunks"] == 1
            assert t["rows_sent"] <= t["local_voxels"] and t["payload_bytes_fp64_form"] == t["rows_sent"] * ((D + 4) * 8 + 8)
            # mixed payload: 64 B of side record per row + a float32 row (voxels of this rank alone) or a float64 row (shared)
            assert t["rows_sent"] * (64 + D * 4) <= t["payload_bytes_sent"] <= t["rows_sent"] * (64 + D * 8)
            assert t["single_rank_voxels"] + t["shared_voxels_local"] == t["local_voxels"]
            assert t["bytes_sent_per_rank"] >= t["payload_bytes_sent"]
            assert abs(t["compute_total_s"] + t["in_collectives_total_s"] - sum(v for k, v in t["wall_s"].items() if k != "gather")) < 1e-6
            sent += t["payload_bytes_sent"]
            rows += t["local_voxels"]
        # the exchange moves what the ranks hold -- at most every local row once -- not ws dense copies of the map
        assert sent <= 1.3 * rows * (D + 4) * 8
        assert rows * (D + 4) * 8 < nproc * tim["dense_reduce_payload_bytes"]
    g = golden(name)
    if n_frames == len(g["depths"]):
        assert np.array_equal(b[2], g["grid_pos"])
        if name.startswith("g2a"):                       # g2b: upstream's arrays changed dtype when they doubled (float32 colour)
            assert np.array_equal(b[5], g["grid_rgb"])
    # without the RNG fast-forward the shards sample other pixels: the faithful mode is what makes the maps equal
    if nproc == 2 and n_frames == 6:
        ind = tmp_path / "independent"
        _run_ranks(nproc, [GOLDEN_DIR / name, ind, n_frames, "independent", seed], 29543)
        c = load_3d_map(ind / "vlmap" / "vlmaps.h5df")
        assert not (c[2].shape == a[2].shape and np.array_equal(c[2], a[2]))


def test_a_failing_rank_takes_the_others_down_instead_of_hanging_them(tmp_path):
    """a rank that fails in its frame loop (here: rank 1 cannot read its second frame) joins the status collective the
    others reach next with its failure flag set; every rank raises promptly -- nobody sits in a merge collective until the timeout"""
    import os
    import subprocess
    import sys
    import time
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, AVLMAPS_DIST_BACKEND="gloo", AVL_TEST_FAIL_RANK="1", AVL_TEST_SAVE_EVERY="3")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29571", str(root / "tests" / "dist_build_worker.py"), str(root / "tests" / "golden" / "g2b_builder_growth.npz"),
           str(tmp_path / "out"), "16", "replay", "99"]
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and time.time() - t0 < 120
    assert "disk gone (simulated on rank 1)" in r.stderr                       # the rank that failed says why ...
    assert "another rank reported a failure" in r.stderr                       # ... and rank 0 stops because of it, not by a timeout


def test_multi_rank_checkpoints_and_resume(golden, tmp_path):
    """Several ranks, like upstream's loop (vlmap_builder.py:181-183, :212-222): every save_every local frames the ranks merge
    and rank 0 writes the map file; a run that dies after such a checkpoint is resumed by the same number of ranks -- rank 0
    imports the file, everybody skips the frames it lists, the merge keeps the file's voxel ids -- and ends with the map of
    the uninterrupted build: same cells, same weights, same features (to the float32 round trip of the checkpoint)."""
    from avlmaps_amd.utils.mapping_utils import load_3d_map, map_checkpoint_complete, read_map_dataset
    GOLDEN_DIR = Path(__file__).resolve().parent / "golden"
    name, n_frames, seed = "g2b_builder_growth.npz", 16, 99
    whole, cut = tmp_path / "whole", tmp_path / "cut"
    _run_ranks(2, [GOLDEN_DIR / name, whole, n_frames, "replay", seed], 29561, AVL_TEST_SAVE_EVERY=3)
    a = load_3d_map(whole / "vlmap" / "vlmaps.h5df")
    assert a[0] == list(range(n_frames)) and map_checkpoint_complete(whole / "vlmap" / "vlmaps.h5df")
    # interrupted after 5 local frames per rank: ONE checkpoint round (after the 3rd local frame) has been written
    _run_ranks(2, [GOLDEN_DIR / name, cut, n_frames, "replay", seed], 29562, AVL_TEST_SAVE_EVERY=3, AVL_TEST_STOP_AFTER=5)
    part = read_map_dataset(cut / "vlmap" / "vlmaps.h5df", "mapped_iter_list").tolist()
    assert part == [0, 1, 2, 8, 9, 10]
    n_part = len(read_map_dataset(cut / "vlmap" / "vlmaps.h5df", "grid_pos"))
    assert 0 < n_part < len(a[2])
    # resumed by two ranks, skipping what the file already holds
    _run_ranks(2, [GOLDEN_DIR / name, cut, n_frames, "replay", seed], 29563, AVL_TEST_SAVE_EVERY=3, AVL_TEST_SKIP_MAPPED=1)
    b = load_3d_map(cut / "vlmap" / "vlmaps.h5df")
    assert b[0] == list(range(n_frames)) and len(b[2]) == len(a[2])
    part_pos = read_map_dataset(cut / "vlmap" / "vlmaps.h5df", "grid_pos")[:n_part]
    cells = lambda pos: (pos[:, 0].astype(np.int64) * 100000 + pos[:, 1]) * 1000 + pos[:, 2]
    ca, cb = cells(a[2]), cells(b[2])
    assert np.array_equal(np.sort(ca), np.sort(cb))                       # the same voxels ...
    ia, ib = np.argsort(ca), np.argsort(cb)
    np.testing.assert_allclose(b[3][ib], a[3][ia], rtol=2e-6)              # ... the same weights (sum of alpha: order-free)
    # ... and the same features, except where the interruption changed WHICH sample is a voxel's first touch: the reference
    # stores feat * alpha at the first touch of a voxel and treats it as a mean afterwards (vlmap_builder.py:166-174, SURVEY.md
    # 8a-5), so its map depends on the frame order; the checkpoint holds frames {0,1,2,8,9,10}, and a voxel frame 9 created
    # that frame 4 would have created in the uninterrupted order keeps frame 9's first-touch weighting.  (Upstream's own resume
    # re-fuses every frame on top of the loaded map: it does not reproduce the uninterrupted map either.)
    close = np.isclose(b[1][ib], a[1][ia], rtol=2e-5, atol=2e-6).all(axis=1)
    assert close.mean() > 0.97, close.mean()
    # colour: the frames fused after a resume enter as the exact weighted mean (no replay log survives a map file), upstream
    # truncates to uint8 at every update -- a downward bias of up to one step per update on voxels that are hit often
    dc = np.abs(b[5][ib].astype(int) - a[5][ia].astype(int))[close]
    assert dc.max() <= 16 and dc.mean() < 1.5, (dc.max(), dc.mean())
    # the checkpoint's voxels keep their ids; occupied_ids is consistent with grid_pos
    assert np.array_equal(b[2][:n_part], part_pos)
    assert np.array_equal(b[4][b[2][:, 0], b[2][:, 1], b[2][:, 2]], np.arange(len(b[2])))


def test_checkpoint_rounds_with_uneven_shards_do_not_change_the_map(golden, tmp_path):
    """3 ranks, 16 frames (shards of 6, 6 and 4), a checkpoint round every 3 local frames: the short shard joins the second
    round at the end of its frames, the merges are non-destructive -- the final map is the map of the run without periodic
    checkpoints, array for array"""
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    GOLDEN_DIR = Path(__file__).resolve().parent / "golden"
    plain, ck = tmp_path / "plain", tmp_path / "ck"
    _run_ranks(3, [GOLDEN_DIR / "g2b_builder_growth.npz", plain, 16, "replay", 99], 29581)
    _run_ranks(3, [GOLDEN_DIR / "g2b_builder_growth.npz", ck, 16, "replay", 99], 29582, AVL_TEST_SAVE_EVERY=3)
    a, b = load_3d_map(plain / "vlmap" / "vlmaps.h5df"), load_3d_map(ck / "vlmap" / "vlmaps.h5df")
    assert a[0] == b[0] == list(range(16))
    for x, y in zip(a[1:6], b[1:6]):
        assert np.array_equal(x, y)


def test_sharded_build_feeds_the_sharded_index_without_an_upload(golden, tmp_path):
    """after a 2-rank build every rank's block of the merged map is already in its HBM (VLMapBuilder.map_shard): VLMap.load_map
    in the same process adopts it as the resident copy (no second upload) and index_map returns what float64 NumPy returns on
    the file's features"""
    GOLDEN_DIR = Path(__file__).resolve().parent / "golden"
    out = tmp_path / "adopt"
    _run_ranks(2, [GOLDEN_DIR / "g2b_builder_growth.npz", out, 16, "replay", 99], 29571, AVL_TEST_ADOPT=1)
    z = np.load(out / "adopt.npz")
    assert bool(z["adopted"]) and z["rows"][0] == 0 and 0 < z["rows"][1] < len(z["mask"])
    assert z["mask"].dtype == np.bool_ and np.mean(z["mask"] == z["want"]) > 0.999 and z["want"].any() and (~z["want"]).any()


def test_uniform_pixel_sampling(golden, tmp_path):
    """pixel_sampling = "uniform": ceil(H*W / rate) distinct pixels per frame from a generator seeded by one draw of the global
    RNG and the frame index -- reproducible under np.random.seed, other pixels than the reference's shuffle, and the same map
    whether the frames are built by one rank or by two (no RNG fast-forward needed)"""
    from avlmaps_amd.utils.mapping_utils import load_3d_map
    GOLDEN_DIR = Path(__file__).resolve().parent / "golden"
    g = golden("g2a_builder_small.npz")
    maps = []
    for rep in range(2):
        d = tmp_path / f"rep{rep}"
        d.mkdir()
        b = MemoryBuilder.make(g, d)
        b.pixel_sampling = "uniform"
        drawn = []
        orig = b._draw_samples
        b._draw_samples = lambda i, n, r: drawn.append(orig(i, n, r)) or drawn[-1]
        np.random.seed(1234)
        b.create_mobile_base_map()
        maps.append(load_3d_map(d / "vlmap" / "vlmaps.h5df"))
        H, W = g["depths"][0].shape
        for s in drawn:
            assert s.dtype == np.int32 and len(s) == len(g["samples"][0]) == len(set(s.tolist())) and 0 <= s.min() and s.max() < H * W
    for x, y in zip(maps[0][1:], maps[1][1:]):
        assert np.array_equal(x, y)                                                   # seeded -> reproducible
    assert not (maps[0][2].shape == g["grid_pos"].shape and np.array_equal(maps[0][2], g["grid_pos"]))      # not the shuffle's pixels
    n_frames = len(g["depths"])
    one, two = tmp_path / "one", tmp_path / "two"
    _run_ranks(1, [GOLDEN_DIR / "g2a_builder_small.npz", one, n_frames, "uniform", 1234], 29545)
    _run_ranks(2, [GOLDEN_DIR / "g2a_builder_small.npz", two, n_frames, "uniform", 1234], 29546)
    a, c = load_3d_map(one / "vlmap" / "vlmaps.h5df"), load_3d_map(two / "vlmap" / "vlmaps.h5df")
    for i in (2, 3, 4, 5):
        assert np.array_equal(a[i], c[i]), i
    np.testing.assert_allclose(c[1], a[1], rtol=1e-6, atol=1e-7)


def test_row_sharded_vlmap_indexing(golden, tmp_path):
    """VLMap under 2 ranks: every rank keeps and scores only its block of voxel rows (prepared, per-row scaled), the per-voxel
    results are all-gathered -- index_map / init_categories return what the single process and the reference return (g3)"""
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    g = golden("g3_similarity.npz")
    env = dict(os.environ, AVLMAPS_DIST_BACKEND="gloo")
    out = tmp_path / "sharded.npz"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29551", str(root / "tests" / "dist_index_worker.py"), str(root / "tests" / "golden" / "g3_similarity.npz"), str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    z = np.load(out)
    assert z["rows"].tolist() == [0, 512]
    assert np.array_equal(z["mask"], g["index_map_sofa_mask"])
    np.testing.assert_allclose(z["scores"], g["init_categories_scores"], rtol=0, atol=1e-4)
    assert np.array_equal(z["m7"], np.argmax(z["scores"], axis=1) == 7)


def test_bench_two_ranks_share_one_gpu():
    """the N > 1 launch path of bench.py (torch.distributed.run, one rank per process, barrier + max-over-ranks timing) with
    two ranks on this box's single GPU: gloo instead of RCCL via AVLMAPS_DIST_BACKEND, everything else as the driver runs it"""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, AVLMAPS_DIST_BACKEND="gloo")
    for extra, metric in ((["--voxels", "60000", "--settle-steps", "2", "--build-frames", "12", "--standin-frames", "8", "--no-pmc"], "voxel_query_similarities_per_sec"),
                          (["--workload", "build"], "map_build_frames_per_sec")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", "29533", str(root / "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]          # rank 0 only
        d = json.loads(lines[0])
        assert d["metric"] == metric and d["n_gpus"] == 2 and d["steps"] == 4 and d["value"] > 0
        ex = d["extra"] if metric.startswith("map_build") else d["extra"]["map_build_strong"]
        # strong scaling of a fixed sequence; the sparse merge (reduce + chained replay) ran INSIDE the timed region and
        # rank 0 finalised the union
        assert ex["voxels_merged"] >= ex["voxels_local"] > 0 and ex["frames_per_gpu"] * 2 == ex["total_frames"]
        mb = ex["merge_breakdown"]
        assert mb["exact_rgb"] is True and mb["merged_voxels"] == ex["voxels_merged"]
        # the N-GPU line says what the merge moved and what carried it: per-phase seconds AND bytes, per rank
        assert mb["mode"].startswith("row-sharded") and ex["merge_finalize_seconds"] >= mb["exchange_s"] > 0
        assert mb["world_size"] == 2 and len(mb["per_rank"]) == 2
        assert all(p["bytes_sent_per_rank"] >= p["payload_bytes_sent"] >= 0 and p["rows_sent"] <= p["local_voxels"] for p in mb["per_rank"])
        assert sum(p["payload_bytes_sent"] for p in mb["per_rank"]) <= 1.3 * sum(p["local_voxels"] for p in mb["per_rank"]) * (512 + 4) * 8
        col = d["extra"]["collectives"]
        assert col["backend"] == "gloo" and col["world_size"] == 2 and [r["rank"] for r in col["ranks"]] == [0, 1]
        if not metric.startswith("map_build"):
            assert "no data-path collective" in d["config"]["parallelism"].lower()
            sv = d["extra"]["map_build_strong_vit_standin"]
            assert sv["feature_standin"] == "vit-l16" and "NOT LSeg" in sv["note"] and sv["total_frames"] >= 4
            assert d["extra"]["merge_breakdown"]["bytes_sent_per_rank"] > 0
            # the N-GPU line answers north_star's strong-scaling question at top level: N-rank frames/s next to the
            # single-GPU reference of the same frames measured in the same run, the merge's phases, and what carried it
            bl = d["build"]
            assert bl["n_gpus"] == 2 and bl["frames"] == 12 and bl["frames_per_s"] > 0 and bl["single_gpu_frames_per_s"] > 0
            assert abs(bl["speedup_vs_single_gpu"] - bl["frames_per_s"] / bl["single_gpu_frames_per_s"]) < 1e-9
            assert bl["merge_breakdown"]["world_size"] == 2 and bl["merge_breakdown"]["plan"].startswith("gather plan")
            assert bl["with_extractor_standin"]["speedup_vs_single_gpu"] > 0 and "NOT LSeg" in bl["with_extractor_standin"]["note"]
            assert d["scaling"] == "weak" and "no data-path collective" in d["scaling_note"]
        if metric.startswith("map_build"):
            assert d["scaling"] == "strong" and abs(d["value"] - 4 / ex["seconds"]) < 1e-6 * d["value"]


def test_randomised_parity_sweep():
    """tools/fuzz_parity.py with a fixed seed and case count: random similarity shapes / strides / modes / column windows against
    float64, random builder scenes frame-by-frame vs deferred vs batched vs the sequential oracle (the long form runs for minutes;
    2 x 2 699 cases were clean at the end of round 2)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "120", "2", "80"], capture_output=True, text=True,
                       timeout=300, cwd=root)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
