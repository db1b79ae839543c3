"""CPU checks of the area / sound / image side of AVLMap: the Habitat pose conversions against a float64 restatement, the area-map
file, the sound database, category lookups, and the errors of queries whose sub-map is absent.  No GPU needed."""
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


def _cfg():
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": 400, "map_config.cell_size": 0.05, "params.gs": 400})


def _scene(tmp_path, frames=6):
    from make_synth_dataset import make
    return make(tmp_path / "scene", frames=frames, H=48, W=64)


def _quat_tf(p, yaw_deg, roll_deg=0.0):
    from scipy.spatial.transform import Rotation as R
    tf = np.eye(4)
    tf[:3, :3] = R.from_euler("yx", [yaw_deg, roll_deg], degrees=True).as_matrix()
    tf[:3, 3] = p
    return tf


def ref_full_map_pose(tf_hab, poses0, base_transform, gs, cs):
    """habitat_dataloader.py:115-121 + mapping_utils.base_pos2grid_id_3d, restated in float64"""
    from avlmaps_amd.utils.mapping_utils import cvt_pose_vec2tf
    bt = base_transform
    init = bt @ cvt_pose_vec2tf(poses0) @ np.linalg.inv(bt)
    tf = np.linalg.inv(init) @ bt @ tf_hab @ np.linalg.inv(bt)
    x, y = tf[0, 3], tf[1, 3]
    theta = np.rad2deg(np.arctan2(tf[1, 0], tf[0, 0]))
    return int(gs / 2 - int(x / cs)), int(gs / 2 - int(y / cs)), theta


def _loader(scene, cfg):
    from avlmaps_amd.dataloader import VLMapsDataloaderHabitat
    from avlmaps_amd.map.map import Map
    m = Map(cfg.map_config, data_dir=scene)
    return VLMapsDataloaderHabitat(scene, cfg.map_config, m), m


def test_pose_conversions_match_float64_restatement(tmp_path):
    cfg = _cfg()
    scene = _scene(tmp_path)
    dl, m = _loader(scene, cfg)
    poses = np.loadtxt(scene / "poses.txt")
    rng = np.random.default_rng(0)
    for _ in range(200):
        tf = _quat_tf(rng.uniform(-9, 9, 3), rng.uniform(-180, 180))
        dl.from_habitat_tf(tf)
        row, col, th = dl.to_full_map_pose()
        rr, rc, rth = ref_full_map_pose(tf, poses[0], m.base_transform, 400, 0.05)
        assert (row, col) == (rr, rc) and th == rth
    cells = dl.habitat_tfs_to_cells([_quat_tf([0.3 * k, 0, -0.2 * k], 10 * k) for k in range(5)])
    assert cells.tolist() == [list(ref_full_map_pose(_quat_tf([0.3 * k, 0, -0.2 * k], 10 * k), poses[0], m.base_transform, 400, 0.05)[:2])
                              for k in range(5)]
    # from_camera_tf: the camera pose of a base pose lands on the cell of base_transform @ inv_init @ base2cam @ cam
    cam = _quat_tf([0.5, 0.1, -0.7], 30)
    dl.from_camera_tf(cam)
    want = ref_full_map_pose(m.base_transform @ dl.inv_init_base_tf @ m.base2cam_tf @ cam, poses[0], m.base_transform, 400, 0.05)
    assert dl.to_full_map_pose()[:2] == list(want[:2])
    # the full-map conversions never built the obstacle map
    assert m.obstacles_map is None


def test_pose_round_trip_like_the_reference(tmp_path):
    """habitat_dataloader.py:155-173: habitat tf -> full-map pose -> habitat tf stays within 1 (Frobenius)"""
    from avlmaps_amd.utils.mapping_utils import cvt_pose_vec2tf
    cfg = _cfg()
    scene = _scene(tmp_path, frames=10)
    dl, _ = _loader(scene, cfg)
    for i in range(len(dl.base_poses)):
        base = cvt_pose_vec2tf(dl.base_poses[i])
        dl.from_habitat_tf(base)
        dl.from_full_map_pose(*dl.to_full_map_pose())
        assert np.linalg.norm(base - dl.to_habitat_tf()) < 1


def test_cropped_pose_offsets(tmp_path):
    cfg = _cfg()
    dl, m = _loader(_scene(tmp_path), cfg)
    m.obstacles_map = np.ones((400, 400), bool)
    m.obstacles_cropped = np.ones((5, 5), bool)
    m.rmin, m.rmax, m.cmin, m.cmax = 10, 14, 20, 24
    dl.from_cropped_map_pose(1, 2, 45.0)
    assert dl.to_full_map_pose() == [11, 22, 45.0] and dl.to_cropped_map_pose() == [1, 2, 45.0]
    assert dl.get_obstacles_cropped() is m.obstacles_cropped


def test_base_rot_mat2theta():
    from avlmaps_amd.utils.mapping_utils import base_rot_mat2theta
    for a in (-170.0, -45.0, 0.0, 30.0, 179.0):
        t = np.deg2rad(a)
        rot = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
        assert abs(np.rad2deg(base_rot_mat2theta(rot)) - a) < 1e-9


def test_area_map_file_round_trip(tmp_path):
    from avlmaps_amd.apps.common import HashImageEncoder
    from avlmaps_amd.map.area_map import AreaMap
    from avlmaps_amd.utils.mapping_utils import cvt_pose_vec2tf, load_rgb_png
    scene = _scene(tmp_path)
    enc = HashImageEncoder()
    a = AreaMap()
    a.create_map(scene, image_encoder=enc)
    assert AreaMap.map_exists(scene)
    b = AreaMap()
    assert b.load_map(scene)
    poses = np.loadtxt(scene / "poses.txt")
    rgbs = sorted((scene / "rgb").glob("*.png"))
    assert b.clip_sparse_map.shape == (6, 768) and b.clip_sparse_map.dtype == np.float32
    assert np.array_equal(b.clip_sparse_map, np.stack([enc(load_rgb_png(p)) for p in rgbs]))
    assert np.array_equal(b.robot_pose_list, np.stack([cvt_pose_vec2tf(p) for p in poses]))
    assert np.allclose(np.linalg.norm(b.clip_sparse_map, axis=1), 1, atol=1e-6)
    assert not AreaMap().load_map(tmp_path / "nowhere")


def _sound_db(rng, S=5, D=1024):
    return {i: {"audio_features": rng.standard_normal(D).astype(np.float32),
                "locations": [rng.uniform(-2, 2, 3) for _ in range(1 + i % 4)]} for i in range(S)}


def test_sound_database_round_trip(tmp_path):
    from avlmaps_amd.apps.common import HashAudioText
    from avlmaps_amd.map.sound_map import SoundMap
    from avlmaps_amd.utils.audio_utils import get_level_categories
    cfg = _cfg()
    sm = SoundMap(str(tmp_path), cfg.sound_config, cfg.sound_data_collect_params, audio_text_model=HashAudioText())
    db = _sound_db(np.random.default_rng(1))
    path = sm.sound_map_path(tmp_path)
    assert path.name == "audio_data_level_3.pkl"
    path.parent.mkdir(parents=True)
    path.write_bytes(pickle.dumps(db))
    assert sm.load_sound_map(tmp_path).keys() == db.keys()
    feats, locs = sm.get_all_audio_features_and_locations()
    assert feats.shape == (5, 1024) and np.array_equal(feats, np.stack([db[i]["audio_features"] for i in range(5)]))
    assert [len(l) for l in locs] == [1, 2, 3, 4, 1] and np.array_equal(locs[2][1], db[2]["locations"][1])
    cats = get_level_categories("level_3", cfg.sound_config)
    assert sm.sound_categories == cats == sorted(cats) and len(cats) == 30 and "door wood knock" in cats and "dog" in cats
    assert get_level_categories("level_1", cfg.sound_config) == sorted(get_level_categories("level_1", cfg.sound_config))
    assert sm.logit_scale() == np.float32(100.0)


def test_category_lookup_errors(tmp_path):
    from avlmaps_amd.apps.common import HashAudioText
    from avlmaps_amd.map.area_map import AreaMap
    from avlmaps_amd.map.sound_map import SoundMap
    a = AreaMap()
    a.categories, a.scores_mat = ["kitchen", "bedroom"], np.arange(6, dtype=np.float32).reshape(3, 2)
    assert np.array_equal(a.index_map("bedroom"), [1, 3, 5])
    with pytest.raises(KeyError):
        a.index_map("garage")
    b = AreaMap()
    with pytest.raises(Exception, match="init_categories"):
        b.index_map("kitchen", with_init_cat=True)
    cfg = _cfg()
    sm = SoundMap(str(tmp_path), cfg.sound_config, cfg.sound_data_collect_params, audio_text_model=HashAudioText())
    sm.audio_database = _sound_db(np.random.default_rng(2))
    with pytest.raises(KeyError):
        sm.get_distribution_and_locations("zebra")


def test_absent_submaps_raise_not_implemented_subclass(tmp_path):
    from avlmaps_amd.map import AVLMap
    from avlmaps_amd.map.avlmap import MissingSubMap
    assert issubclass(MissingSubMap, NotImplementedError)
    av = AVLMap(_cfg())
    for fn, what in ((av.index_area, "area map"), (av.index_area_2d, "area map"), (av.index_sound, "sound map"),
                     (av.index_sound_2d, "sound map"), (av.index_image, "localiser")):
        with pytest.raises(MissingSubMap, match=what):
            fn("x")
    # a config without the sound settings says so
    from avlmaps_amd.apps.common import to_cfg
    bare = to_cfg({"map_config": dict(_cfg().map_config), "params": {"cs": 0.05}})
    with pytest.raises(NotImplementedError, match="sound_config"):
        AVLMap(bare).index_sound("dog")
    # sound map loaded but no audio-text model attached
    av._sound_loaded = True
    with pytest.raises(MissingSubMap, match="audio-text model"):
        av.index_sound("dog")


def test_index_map_cli_arguments():
    from avlmaps_amd.apps import index_map
    with pytest.raises(SystemExit):
        index_map.main(["--data-dir", ".", "--modality", "area"])          # no --query
    with pytest.raises(SystemExit):
        index_map.main(["--data-dir", ".", "--modality", "image"])         # no --image
    assert index_map.DEFAULT_DECAY == {"object": 0.01, "area": 0.1, "sound": 0.01, "image": 0.01}
