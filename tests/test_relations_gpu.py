"""The spatial-relation goals end to end on the GPU: Map.get_pos_in_between / get_left_pos on a VLMap whose islands come from the device
path (csrc/avl_islands.hip) and whose nearest contour pair comes from ops.contour_nearest_pair, against the same calls with the host
island path and the NumPy nearest pair; and apps.plan_path --relation on a synthetic scene."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(ROOT / "tools"))
from test_islands_gpu import g8_vlmap  # noqa: E402
from test_relations_host import numpy_nearest_pair  # noqa: E402

HEADINGS = (0.0, 45.0, 90.0, 135.0, 180.0, -135.0, -90.0, -45.0)


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return list(a) == list(b) if a[0] is None or b[0] is None else np.array_equal(a, b)


def test_in_between_and_left_equal_the_host_paths(golden, monkeypatch):
    from avlmaps_amd import ops
    vm, _ = g8_vlmap(golden, monkeypatch)
    centre = [(vm.rmin + vm.rmax) / 2, (vm.cmin + vm.cmax) / 2]
    device_pair = ops.contour_nearest_pair
    found_between = found_left = 0
    for pos in (centre, [float(vm.rmin), float(vm.cmin)]):
        for h in HEADINGS:
            vm.island_path = "device"
            got = (vm.get_pos_in_between(pos, h, "wall", "table"), vm.get_left_pos(pos, h, "table"), vm.get_left_pos(pos, h, "wall"))
            vm.island_path = "host"
            monkeypatch.setattr(ops, "contour_nearest_pair", numpy_nearest_pair)
            want = (vm.get_pos_in_between(pos, h, "wall", "table"), vm.get_left_pos(pos, h, "table"), vm.get_left_pos(pos, h, "wall"))
            monkeypatch.setattr(ops, "contour_nearest_pair", device_pair)
            assert all(same(a, b) for a, b in zip(got, want)), (pos, h, got, want)
            found_between += want[0] is not None
            found_left += want[1][0] is not None or want[2][0] is not None
    assert found_between and found_left                        # the comparison is not one of None with None throughout


@pytest.fixture(scope="module")
def synth_scene(tmp_path_factory):
    """a synthetic scene with its map (the recipe of test_morph2d_gpu)"""
    import yaml
    from make_synth_dataset import make
    tmp = tmp_path_factory.mktemp("relations")
    scene_dir = make(tmp / "scene", frames=6, H=96, W=128)
    cfg = tmp / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                  "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    from avlmaps_amd.apps import create_map
    create_map.main(["--data-dir", str(scene_dir), "--config", str(cfg), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    from avlmaps_amd.apps.common import HashClip, load_config
    from avlmaps_amd.map import VLMap
    vm = VLMap(load_config(str(cfg)).map_config, data_dir=str(scene_dir))
    assert vm.load_map(str(scene_dir))
    vm.clip_feat_dim = vm.grid_feat.shape[1]
    vm.clip_model = HashClip(vm.clip_feat_dim)
    vm.init_categories(["sofa", "chair", "other"])
    vm.generate_obstacle_map()
    return vm, scene_dir, cfg


def test_plan_path_relation_between_in_a_child_process(synth_scene):
    from avlmaps_amd.apps import plan_path
    from avlmaps_amd.navigator import Navigator, NoPathError
    vm, scene_dir, cfg = synth_scene
    free = np.argwhere(vm.get_obstacle_cropped())
    pairs = [("sofa", "chair"), ("sofa", "other"), ("chair", "other"), ("sofa", "sofa"), ("chair", "chair"), ("other", "other")]
    found = nothing = None
    nav = Navigator()
    nav.build_visgraph(vm.get_obstacle_cropped(), vm.rmin, vm.cmin)
    try:
        for c in free[:: max(1, len(free) // 12)]:
            start = [float(c[0] + vm.rmin), float(c[1] + vm.cmin)]
            for h in HEADINGS:
                for qa, qb in pairs:
                    goal = vm.get_pos_in_between(start, h, qa, qb)
                    if goal is None:
                        nothing = nothing or (start, h, qa, qb)
                        continue
                    if found is None:
                        try:
                            g = plan_path.clamp_point(goal, vm.rmin, vm.cmin, vm.obstacles_cropped.shape)
                            found = (start, h, qa, qb, [float(goal[0]), float(goal[1])], g, nav.plan_to(start, g))
                        except NoPathError:
                            pass
                if found and nothing:
                    break
            if found and nothing:
                break
    finally:
        nav.close()
    assert found is not None, "no start and heading of the scene has two sizeable objects in front"
    start, h, qa, qb, cell, goal, path = found
    base = [sys.executable, "-m", "avlmaps_amd.apps.plan_path", "--data-dir", str(scene_dir), "--config", str(cfg), "--text-model", "hash",
            "--categories", "sofa,chair,other"]
    r = subprocess.run(base + ["--query", qa, "--query-b", qb, "--relation", "between", "--heading", str(h), "--start", str(start[0]),
                               str(start[1])], capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["relation"] == "between" and out["goal_cell"] == cell and out["goal"] == goal
    assert len(out["path"]) >= 1 and out["path"] == [[float(p[0]), float(p[1])] for p in path]
    # nothing in front: a message and a non-zero status, no plan to None (in process: the child above is what starts processes)
    args = ["--data-dir", str(scene_dir), "--config", str(cfg), "--text-model", "hash", "--categories", "sofa,chair,other"]
    assert nothing is not None, "every start and heading of the scene has objects in front"
    nstart, nh, na, nb = nothing
    with pytest.raises(SystemExit) as e:
        plan_path.main(args + ["--query", na, "--query-b", nb, "--relation", "between", "--heading", str(nh), "--start", str(nstart[0]),
                               str(nstart[1])])
    assert e.value.code not in (0, None) and "in front" in str(e.value.code)
    out = plan_path.main(args + ["--query", qa, "--relation", "face", "--heading", "10", "--start", str(start[0]), str(start[1])])
    assert -180.0 <= out["turn_right_deg"] <= 180.0 and "path" not in out
