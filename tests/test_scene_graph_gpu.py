"""Object relations on the GPU (csrc/avl_relations.hip through ops.object_relations, VLMap.get_scene_graph,
AVLMap.index_related_object and apps.index_map --relations).

Oracle: tests/_scene_graph_ref.py, the definition of include/avlmaps_hip.h (24) restated with a dense owner array and one NumPy
step per offset.  Every result is an integer minimum or count, so the table and P are compared with np.array_equal in every case."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
from _scene_graph_ref import offset_code, reference_relations  # noqa: E402
from test_host_mirror import Cfg  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


def run(ops, pos, labels, n, R, gs, vh, **kw):
    pos, labels = np.asarray(pos, np.int32).reshape(-1, 3), np.asarray(labels, np.int32)
    with ops.cell_index(pos, gs, vh) as index:
        return ops.object_relations(index, pos, labels, n, R, **kw)


def check(ops, pos, labels, n, R, gs, vh, **kw):
    want, P = reference_relations(pos, labels, n, R, gs, vh)
    got = run(ops, pos, labels, n, R, gs, vh, **kw)
    assert got.P == P, (got.P, P)
    assert got.table.dtype == np.int64 and got.table.shape == (P, ops.RELATION_TABLE_COLS)
    assert np.array_equal(got.table, want), (got.table, want)
    assert (got.radius, got.n) == (R, n)
    return got


# ------------------------------------------------------------------ 1. nothing to relate
def test_empty_and_one_object_inputs(ops):
    none = np.zeros((0, 3), np.int32)
    assert check(ops, none, np.zeros(0, np.int32), 3, 2, 8, 4).P == 0                   # N = 0
    pos = np.argwhere(np.ones((3, 3, 2), bool)).astype(np.int32)
    assert check(ops, pos, np.ones(len(pos), np.int32), 0, 2, 8, 4).P == 0              # n = 0
    assert check(ops, pos, np.ones(len(pos), np.int32), 1, 2, 8, 4).P == 0              # one object only
    assert check(ops, pos, np.zeros(len(pos), np.int32), 5, 2, 8, 4).P == 0             # labels all 0
    got = run(ops, pos, np.zeros(len(pos), np.int32), 5, 2, 8, 4)
    assert got.table.shape == (0, 8) and got.pair(1, 2) is None


# ------------------------------------------------------------------ 2. the radius is exact
@pytest.mark.parametrize("R", [1, 2, 15])
def test_two_voxels_at_the_radius_and_just_beyond(ops, R):
    gs, vh = 40, 20
    labels = np.array([1, 2], np.int32)
    at = np.array([[3, 4, 2], [3 + R, 4, 2]], np.int32)                                 # |d|^2 = R^2: the offsets (R, 0, 0) and (-R, 0, 0)
    got = run(ops, at, labels, 2, R, gs, vh)
    assert got.P == 1 and got.table.tolist() == [[1, 2, R * R, 0, 1, 0, 0, 2 if R == 1 else 0]]     # (a contact counts from both sides)
    beyond = np.array([[3, 4, 2], [3 + R, 5, 2]], np.int32)                             # |d|^2 = R^2 + 1
    got = run(ops, beyond, labels, 2, R, gs, vh)
    assert got.P == 0 and got.table.shape == (0, 8)
    if R < 15:
        check(ops, at, labels, 2, R, gs, vh)
        check(ops, beyond, labels, 2, R, gs, vh)
    else:
        # the corner offsets (15, 15, 15) are not scanned: the largest code in use is that of (15, 0, 0), and a voxel there is found
        assert offset_code(15, 0, 0, 15) < 2 ** 15 and 15 * 15 < 2 ** 8
        corner = np.array([[3, 4, 2], [18, 19, 17]], np.int32)
        assert run(ops, corner, labels, 2, R, gs, vh).P == 0
        check(ops, np.concatenate([at, corner[1:]]), np.array([1, 2, 2], np.int32), 2, R, gs, vh)


# ------------------------------------------------------------------ 3. the edges of the grid
def test_neighbours_across_the_edges_of_the_grid_are_not_neighbours(ops):
    gs, vh = 9, 5
    labels = np.array([1, 2], np.int32)
    # the linear cell after (r, c, vh - 1) is (r, c + 1, 0): a true distance of 1^2 + 4^2 = 17, never 1
    pos = np.array([[2, 3, vh - 1], [2, 4, 0]], np.int32)
    for R in (1, 4, 5):
        got = check(ops, pos, labels, 2, R, gs, vh)
        assert got.P == (1 if R >= 5 else 0) and (got.P == 0 or got.table[0, 2] == 17)
    # and after (r, gs - 1, h) comes (r + 1, 0, h): 1^2 + 8^2 = 65
    pos = np.array([[2, gs - 1, 1], [3, 0, 1]], np.int32)
    for R in (1, 8, 9):
        got = check(ops, pos, labels, 2, R, gs, vh)
        assert got.P == (1 if R >= 9 else 0) and (got.P == 0 or got.table[0, 2] == 65)
    # voxels in the corners: no read outside the grid, and the table is the reference's
    corners = np.array([[0, 0, 0], [0, 1, 0], [gs - 1, gs - 1, vh - 1], [gs - 1, gs - 2, vh - 1], [0, gs - 1, 0], [1, gs - 1, 1]], np.int32)
    for R in (1, 3, 15):
        check(ops, corners, np.array([1, 2, 3, 4, 5, 6], np.int32), 6, R, gs, vh)


# ------------------------------------------------------------------ 4. rows that share a cell
def test_rows_that_share_a_cell(ops):
    pos = np.array([[4, 4, 2], [4, 4, 2]], np.int32)
    got = check(ops, pos, np.array([1, 2], np.int32), 2, 1, 8, 4)
    assert got.table.tolist() == [[1, 2, 0, 0, 1, 0, 0, 0]]                             # row 0 scans and sees the owner, row 1, at d = 0
    got = check(ops, pos, np.array([2, 1], np.int32), 2, 1, 8, 4)
    assert got.table.tolist() == [[1, 2, 0, 0, 1, 0, 0, 0]]
    # the smaller row's object is seen only as scanner: object 3 above the shared cell sees object 2 (the owner) alone
    pos = np.array([[4, 4, 2], [4, 4, 2], [4, 4, 3]], np.int32)
    got = check(ops, pos, np.array([1, 2, 3], np.int32), 3, 1, 8, 4)
    assert got.table.tolist() == [[1, 2, 0, 0, 1, 0, 0, 0], [1, 3, 1, 0, 2, 0, 0, 1], [2, 3, 1, 1, 2, 0, 1, 2]]


# ------------------------------------------------------------------ 5. the witness
def test_the_witness_tie_breaks_by_row_then_code(ops):
    # two voxels of object 1 (rows 3 and 1) equally near the one voxel of object 2 (row 2): the smallest scanning row wins
    pos = np.array([[9, 9, 9], [5, 4, 3], [5, 5, 3], [5, 6, 3]], np.int32)
    labels = np.array([0, 1, 2, 1], np.int32)
    got = check(ops, pos, labels, 2, 2, 12, 12)
    assert got.table[0, 2:5].tolist() == [1, 1, 2]
    # two offsets from one voxel (row 0) equally near two voxels of object 2: the smallest code wins, (0, -1, 0) before (0, 1, 0)
    pos = np.array([[5, 5, 3], [5, 6, 3], [5, 4, 3]], np.int32)
    labels = np.array([1, 2, 2], np.int32)
    got = check(ops, pos, labels, 2, 2, 12, 12)
    assert got.table[0, 2:5].tolist() == [1, 0, 2]
    # the sides: the scanning row belongs to hi here, and the SceneGraph puts it there
    from types import SimpleNamespace
    from avlmaps_amd.map.scene_graph import SceneGraph
    pos = np.array([[5, 5, 3], [5, 7, 3]], np.int32)
    labels = np.array([2, 1], np.int32)
    got = check(ops, pos, labels, 2, 2, 12, 12)
    assert got.table.tolist() == [[1, 2, 4, 0, 1, 0, 0, 0]]
    objs = SimpleNamespace(objects=[SimpleNamespace(label=1, voted_name="a"), SimpleNamespace(label=2, voted_name="b")], n=2, min_voxels=0)
    e = SceneGraph(objs, got, 0.05, 2, labels=labels).edges[0]
    assert (e.a, e.b, e.voxel_a, e.voxel_b) == (1, 2, 1, 0)


# ------------------------------------------------------------------ 6. support and contacts
@pytest.mark.parametrize("upper", [1, 2])
def test_two_slabs_stacked(ops, upper):
    cells = np.argwhere(np.ones((64, 64, 2), bool))
    cells = cells[np.random.default_rng(3).permutation(len(cells))].astype(np.int32)
    labels = np.where(cells[:, 2] == 1, upper, 3 - upper).astype(np.int32)             # the upper slab is object `upper`
    got = check(ops, cells + np.array([3, 2, 1], np.int32), labels, 2, 2, 70, 4)
    on = got.table[0, 5:7].tolist()
    assert on == ([4096, 0] if upper == 1 else [0, 4096])
    # every voxel sees the 3 x 3 block of the other slab, cut at the slab's edges: (3 * 64 - 2)^2 per side
    assert got.table[0, 7] == 2 * (3 * 64 - 2) ** 2 and got.table[0, 2] == 1


# ------------------------------------------------------------------ 7. the pair table's bound
@functools.lru_cache(maxsize=None)
def chain():
    """2 000 one-voxel objects along a path that touches itself nowhere else: rows 0, 2, 4 .. of a 64-cell grid joined at
    alternating ends, numbered along the path and shuffled"""
    path = []
    for k in range(31):
        cols = range(64) if k % 2 == 0 else range(63, -1, -1)
        path += [(2 * k, c, 0) for c in cols] + [(2 * k + 1, 63 if k % 2 == 0 else 0, 0)]
    path = np.array(path[:2000], np.int32)
    perm = np.random.default_rng(4).permutation(2000)
    pos, labels = path[perm], (perm + 1).astype(np.int32)
    want, P = reference_relations(pos, labels, 2000, 1, 64, 1)
    assert P == 1999
    for a in (pos, labels, want):
        a.setflags(write=False)
    return pos, labels, want


def test_a_chain_of_objects_and_the_bound_of_the_pair_table(ops):
    from avlmaps_amd import _lib
    from avlmaps_amd.device import DeviceArray
    pos, labels, want = chain()
    got = run(ops, pos, labels, 2000, 1, 64, 1, max_pairs=1999)
    assert got.P == 1999 and np.array_equal(got.table, want)
    got = run(ops, pos, labels, 2000, 1, 64, 1)                                         # the default, max(1024, 16 n), holds them
    assert got.P == 1999 and np.array_equal(got.table, want)
    assert got.pair(7, 8).tolist() == want[(want[:, 0] == 7) & (want[:, 1] == 8)][0].tolist() and got.pair(8, 7) is not None
    assert got.pair(7, 9) is None and got.pair(0, 1) is None and got.pair(2000, 2001) is None
    with pytest.raises(_lib.AvlError, match=r"\d+ pairs were counted, more than max_pairs = 1998"):
        run(ops, pos, labels, 2000, 1, 64, 1, max_pairs=1998)
    # the C entry point: one pair too many is a count above max_pairs, not an error code
    lib = _lib.load()
    nws = C.c_size_t(0)
    assert lib.avl_object_relations_work_bytes(1998, C.byref(nws)) == 0
    ws, table, count = DeviceArray((nws.value,), np.uint8), DeviceArray((1998, 8), np.int64), DeviceArray((1,), np.int64)
    dp, dl = DeviceArray.from_numpy(pos), DeviceArray.from_numpy(labels)
    with ops.cell_index(dp, 64, 1) as index:
        rc = lib.avl_object_relations(index.ptr, index.nbytes, 2000, 64, 1, dp.ptr, dl.ptr, 2000, 1, 1998, table.ptr, count.ptr, ws.ptr, nws.value, None)
        assert rc == 0, lib.avl_last_error()
        assert count.numpy()[0] > 1998


def test_the_default_pair_table_grows(ops):
    """64 one-voxel objects in an 8 x 8 plate, every one within 15 cells of every other: 2 016 pairs, more than the 1 024 the default
    starts with, and exactly n (n - 1) / 2, the bound it may grow to"""
    from avlmaps_amd import _lib
    pos = np.argwhere(np.ones((8, 8, 1), bool)).astype(np.int32) + np.array([2, 3, 1], np.int32)
    labels = (np.random.default_rng(5).permutation(64) + 1).astype(np.int32)
    got = check(ops, pos, labels, 64, 15, 16, 3)
    assert got.P == 64 * 63 // 2 > 1024
    with pytest.raises(_lib.AvlError, match=r"\d+ pairs were counted, more than max_pairs = 1024"):
        run(ops, pos, labels, 64, 15, 16, 3, max_pairs=1024)


# ------------------------------------------------------------------ 8. fuzz
@functools.lru_cache(maxsize=None)
def blobs(seed):
    """about 3 000 voxels in and around a 24 x 24 x 8 grid: about 40 blob-shaped labels (the nearest of 40 seeds), some rows that
    share cells, some rows outside the grid, some labels 0 or above n"""
    rng = np.random.default_rng(seed)
    gs, vh, n = 24, 8, 40
    cells = np.argwhere(rng.random((gs, gs, vh)) < 0.6)
    seeds = rng.integers(0, [gs, gs, vh], (n, 3))
    labels = 1 + np.argmin(((cells[:, None, :] - seeds[None]) ** 2).sum(2), axis=1)
    extra = rng.integers(0, len(cells), 150)                                            # rows that share a cell, under other labels
    outside = rng.integers(-3, [gs + 3, gs + 3, vh + 3], (150, 3))
    outside = outside[np.any((outside < 0) | (outside >= [gs, gs, vh]), axis=1)]
    pos = np.concatenate([cells, cells[extra], outside])
    labels = np.concatenate([labels, rng.integers(1, n + 1, len(extra)), rng.integers(1, n + 1, len(outside))])
    labels[rng.random(len(labels)) < 0.05] = 0
    labels[rng.random(len(labels)) < 0.03] = n + 1 + rng.integers(0, 5)
    labels[rng.random(len(labels)) < 0.02] = -2
    perm = rng.permutation(len(pos))
    pos, labels = pos[perm].astype(np.int32), labels[perm].astype(np.int32)
    for a in (pos, labels):
        a.setflags(write=False)
    return pos, labels, n, gs, vh


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("R", [1, 2, 3, 5])
def test_fuzz(ops, R, seed):
    pos, labels, n, gs, vh = blobs(seed)
    assert 2500 < len(pos) < 3500
    got = check(ops, pos, labels, n, R, gs, vh)
    assert got.P > n and (got.table[:, 2] == 0).any()                                   # many pairs, shared cells among them


# ------------------------------------------------------------------ 9. the same bytes
def test_the_same_bytes_on_every_run_and_from_device_inputs(ops):
    from avlmaps_amd.device import DeviceArray
    pos, labels, n, gs, vh = blobs(0)
    first = run(ops, pos, labels, n, 3, gs, vh)
    again = run(ops, pos, labels, n, 3, gs, vh)
    assert first.P == again.P and first.table.tobytes() == again.table.tobytes()
    dp, dl = DeviceArray.from_numpy(pos), DeviceArray.from_numpy(labels)
    with ops.cell_index(dp, gs, vh) as index:
        dev = ops.object_relations(index, dp, dl, n, 3, device=True)
        assert isinstance(dev.table, DeviceArray) and dev.table.shape == (first.P, 8) and dev.P == first.P
        assert dev.table.numpy().tobytes() == first.table.tobytes()
        assert dev.pair(int(first.table[5, 1]), int(first.table[5, 0])).tolist() == first.table[5].tolist()
        small = ops.object_relations(index, dp, dl, n, 3, max_pairs=first.P)           # a table that is exactly full
        assert small.table.tobytes() == first.table.tobytes()


# ------------------------------------------------------------------ 10. map layer
NAMES = ["table", "mug", "chair"]


@functools.lru_cache(maxsize=None)
def synthetic_map():
    """a 10 x 10 table top at height 4, a 4 x 4 x 4 mug on it, a 4 x 4 x 4 chair beside it (one free column between them, its top one
    cell below the table top), at (20, 30, 0) of a 100-cell map; scores whose row maximum and whose mean both say the category"""
    cat = -np.ones((30, 30, 12), np.int32)
    cat[5:15, 5:15, 4] = 0
    cat[8:12, 8:12, 5:9] = 1
    cat[5:9, 16:20, 0:4] = 2
    rng = np.random.default_rng(9)
    cells = np.argwhere(cat >= 0)
    cells = cells[rng.permutation(len(cells))]
    c = cat[cells[:, 0], cells[:, 1], cells[:, 2]]
    scores = (rng.integers(0, 64, (len(cells), 3)) / 128).astype(np.float32)
    scores[np.arange(len(cells)), c] += 1
    return (cells + np.array([20, 30, 0])).astype(np.int32), np.ascontiguousarray(scores), c


def synthetic_avlmap():
    from avlmaps_amd.map import AVLMap
    grid_pos, scores, _ = synthetic_map()
    cfg = Cfg(map_config=Cfg(map_type="vlmap", grid_size=100, cell_size=0.05,
                             pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                                           base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0])),
              params=Cfg(cs=0.05))
    av = AVLMap(cfg)
    av.vlmap.grid_pos, av.vlmap.scores_mat, av.vlmap.categories = grid_pos.copy(), scores.copy(), list(NAMES)
    return av


def test_the_mug_on_the_table(ops):
    from avlmaps_amd.map.scene_graph import Relation, SceneGraph, relations_from_json
    grid_pos, scores, cat = synthetic_map()
    av = synthetic_avlmap()
    vm = av.vlmap
    graph = vm.get_scene_graph()
    assert isinstance(graph, SceneGraph) and graph.R == 5 and graph.cs == 0.05
    scene = graph.objects
    assert scene is vm.get_objects() and [(it.voted_name, it.count) for it in scene.objects] == [("table", 100), ("chair", 64), ("mug", 64)]
    table, chair, mug = scene.objects
    labels = scene.voxel_objects.labels.numpy()
    want, P = reference_relations(grid_pos, labels, scene.n, 5, 100, int(grid_pos[:, 2].max()) + 1)
    assert graph.relations.P == P == 2 and np.array_equal(graph.relations.table, want)
    hits = graph.find("mug", "on", "table")
    assert len(hits) == 1 and hits[0][0] == mug and hits[0][1] == table
    rel = hits[0][2]
    assert isinstance(rel, Relation) and (rel.a, rel.b, rel.d2, rel.a_on_b, rel.b_on_a) == (mug.label, table.label, 1, 16, 0)
    assert rel.distance == 0.05 and labels[rel.voxel_a] == mug.label and labels[rel.voxel_b] == table.label
    assert rel.contacts == 2 * 16 * 9                    # the mug's 16 bottom voxels and the 3 x 3 table cells under each, from both sides
    mirror = graph.find("table", "under", "mug")
    assert len(mirror) == 1 and mirror[0][0] == table and mirror[0][1] == mug and mirror[0][2] == rel.mirrored()
    assert graph.find("chair", "on", "table") == [] and graph.find("table", "on", "mug") == []
    near = graph.find("chair", "near", "table")
    assert len(near) == 1 and near[0][2].d2 == 5 and near[0][2].contacts == 0           # (0, 2, 1): one free column, one cell lower
    assert graph.find("chair", "near", "mug") == [] and graph.relation(chair.label, mug.label) is None
    assert [e.b for e in graph.neighbors(table.label)] == [mug.label, chair.label]      # nearest first
    assert [e.b for e in graph.rests_on(mug.label)] == [table.label] and [e.b for e in graph.supports(table.label)] == [mug.label]
    assert [e.b for e in graph.touching(table.label)] == [mug.label] and graph.touching(chair.label) == []
    assert relations_from_json(graph.to_json()) == graph.edges and len(graph.edges) == 2
    # the heat of the related object is the heat of that object
    heat = av.index_related_object("mug", "on", "table")
    assert heat.dtype == np.float32 and heat.tobytes() == av.index_scene_object(mug.label).tobytes()
    assert np.array_equal(heat == 1.0, cat == 1)
    with pytest.raises(LookupError):
        av.index_related_object("chair", "on", "table")
    goal = av.index_goal(extra=[heat])
    assert goal.value == 1 and cat[goal.voxel] == 1
    # a smaller radius loses the chair, and the radius is clamped to 1 .. 15 cells
    assert len(vm.get_scene_graph(radius=0.1).edges) == 1 and vm.get_scene_graph(radius=0.1).R == 2
    assert vm.get_scene_graph(radius=0.001).R == 1 and vm.get_scene_graph(radius=10.0).R == 15


# ------------------------------------------------------------------ 11. the app
def test_index_map_relations_flags_on_a_disk_dataset(tmp_path, capsys):
    """apps.index_map --inventory --relations --relations-json on a synthetic scene in the on-disk layout: the printed edges are
    those of the JSON, they are the scene graph's of the same map, and --related returns that object's heat"""
    import re
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import yaml
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map, index_map
    from avlmaps_amd.map.scene_graph import relations_from_json
    scene = make(tmp_path / "scene", frames=6, H=96, W=128)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                  "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(scene), "--config", str(cfg), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    base = ["--data-dir", str(scene), "--config", str(cfg), "--query", "sofa", "--text-model", "hash", "--categories", "sofa,table,chair"]
    path = tmp_path / "relations.json"
    heat = index_map.main(base + ["--inventory", "--relations", "--relations-json", str(path), "--relation-radius", "0.15",
                                  "--min-voxels", "1", "--connectivity", "6"])
    out = capsys.readouterr().out
    edges = relations_from_json(path.read_text())
    lines = re.findall(r"relation (\d+) '\w+' - (\d+) '\w+': gap [\d.]+ m \(d2 (\d+)\) between voxels (\d+) and (\d+), (\d+) contacts, (\d+) / (\d+) voxels", out)
    assert len(lines) == len(edges) > 0 and f"wrote {path}: {len(edges)} relations" in out
    assert [tuple(int(v) for v in ln) for ln in lines] == [(e.a, e.b, e.d2, e.voxel_a, e.voxel_b, e.contacts, e.a_on_b, e.b_on_a) for e in edges]
    assert all(e.a < e.b and e.d2 <= 9 for e in edges) and edges == sorted(edges, key=lambda e: (e.a, e.b))
    # --related: the heat of the first hit's subject, whatever it is; the plain query's heat otherwise
    import json
    names = json.loads(path.read_text())["names"]
    e = edges[0]
    heat2 = index_map.main(base + ["--related", f"{names[str(e.a)]} near {names[str(e.b)]}", "--relation-radius", "0.15", "--min-voxels", "1",
                                   "--connectivity", "6"])
    out = capsys.readouterr().out
    assert "related " in out and heat2.shape == heat.shape and (heat2 == 1.0).any()
