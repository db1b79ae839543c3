"""CPU tests of the ground-truth label map: the restatement the GPU tests compare against (on a scene worked out by hand),
ops.map_scores on hand-made matrices, the obj2cls table from every source, the GTMap file round trip, the argument checks of the
four C calls and of their ops (all before any device work), and SciPy's definition of binary_closing the port relies on."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import _gtmap_ref as R  # noqa: E402


# ------------------------------------------------------------------ the restatement, by hand
def test_known_answer_wall():
    # The camera of vote_scene's frame 0: at (0.0125, 0.0125, 0.2125) looking along +x; a flat wall at depth 0.3 puts every pixel at
    # x = 0.3125 -> int(6.25) = 6 -> row 32 - 6 = 26.  Sideways: y = 0.0125 - (u + 0.5 - 16) / 32 * 0.3; up: z = 0.2125 - (v + 0.5 - 12)
    # / 32 * 0.3.  With one object id everywhere and a full index every lattice pixel votes, all of them in row 26.
    depth = np.full((1, R.H, R.W), 0.3, np.float32)
    sem = np.full((1, R.H, R.W), 7, np.int32)
    table = np.full(9, -1, np.int32)
    table[7] = 2
    occupied = np.arange(R.GS * R.GS * R.VH, dtype=np.int32).reshape(R.GS, R.GS, R.VH)
    N = occupied.size
    T = R.camera((0.0125, 0.0125, 0.2125))[None]
    for stride in (1, 3):
        stats = {}
        votes, counts = R.vote_ref(None, depth, sem, R.K, T, occupied, N, 3, R.CS, stride=stride, obj2cls=table, stats=stats, **R.DEPTHS)
        lattice_v, lattice_u = range(stride // 2, R.H, stride), range(stride // 2, R.W, stride)
        assert counts.tolist() == [0, 0, 0, len(lattice_v) * len(lattice_u)] and set(stats) == {"max_votes_one_counter_one_frame"}
        assert votes[:, [0, 1]].sum() == 0 and votes.sum() == counts[3]
        want = np.zeros((R.GS, R.GS, R.VH), np.int64)
        for v in lattice_v:
            for u in lattice_u:
                y = 0.0125 - (u + 0.5 - 16.0) / 32.0 * np.float64(np.float32(0.3))
                z = 0.2125 - (v + 0.5 - 12.0) / 32.0 * np.float64(np.float32(0.3))
                want[26, 32 - int(y / R.CS), int(z / R.CS)] += 1
        hit = votes[:, 2].reshape(R.GS, R.GS, R.VH)
        assert np.array_equal(hit, want)                                 # every count is the number of lattice pixels that fall there
        assert (hit[26] > 0).sum() == (hit > 0).sum() and hit[:, :, :].max() >= (30 if stride == 1 else 4)
    # a pixel with another object, one without a voxel and one out of the depth range
    sem[0, 0, 0], depth[0, 0, 1] = 8, 9.0
    occupied = occupied.copy()
    occupied[26, 29, 4] = -1
    votes2, counts2 = R.vote_ref(None, depth, sem, R.K, T, occupied, N, 3, R.CS, obj2cls=table, **R.DEPTHS)
    full, _ = R.vote_ref(None, np.full((1, R.H, R.W), 0.3, np.float32), np.full((1, R.H, R.W), 7, np.int32), R.K, T, np.arange(N, dtype=np.int32).reshape(occupied.shape), N, 3,
                         R.CS, obj2cls=table, **R.DEPTHS)
    gone = int(want_at(26, 29, 4, full))
    assert counts2.tolist() == [1, 1, gone, R.H * R.W - 2 - gone] and gone > 0


def want_at(row, col, h, votes):
    return votes[:, 2].reshape(R.GS, R.GS, R.VH)[row, col, h]


def test_restatement_of_labels_pool_and_confusion_by_hand():
    votes = np.array([[0, 0, 0], [1, 3, 3], [2, 0, 2], [0, 0, 4], [2 ** 32 - 1, 2, 0]], np.uint32)
    label, support = R.labels_ref(votes)
    assert label.tolist() == [-1, 1, 0, 2, 0] and support.tolist() == [0, 7, 4, 4, 1]
    occupied = np.full((2, 2, 3), -1, np.int32)
    occupied[0, 0] = [1, 0, -1]             # the top voxel (id 0) is unlabelled, the one below it has label 1
    occupied[0, 1] = [-1, -1, -1]           # no voxel
    occupied[1, 0] = [0, -1, 0]             # unlabelled voxels only
    occupied[1, 1] = [3, 2, 4]              # the top one wins
    assert R.pool_ref(label, occupied).tolist() == [[1, -1], [-1, 0]]
    assert R.pool_ref(label, occupied, (1, 1, 0, 1)).tolist() == [[-1, 0]]
    conf, skipped = R.confusion_ref([0, 0, 1, -1, -1, 1], [0, 2, -1, 1, -1, 1], 2, 3)
    assert conf.tolist() == [[1, 0, 1], [0, 1, 0]] and skipped.tolist() == [2, 1]
    with pytest.raises(IndexError):
        R.confusion_ref([2], [0], 2, 3)


# ------------------------------------------------------------------ map_scores
def test_map_scores_by_hand():
    from avlmaps_amd import ops
    # three GT classes (class 1 has no ground truth) against four predicted ones ("other" is the last)
    conf = np.array([[6, 1, 0, 1],
                     [0, 0, 0, 0],
                     [2, 0, 5, 1]], np.uint64)
    s = ops.map_scores(conf)
    assert s.pixel_acc == 11 / 16
    assert s.acc[0] == 6 / 8 and np.isnan(s.acc[1]) and s.acc[2] == 5 / 8
    assert s.iou[0] == 6 / (8 + 8 - 6) and np.isnan(s.iou[1]) and s.iou[2] == 5 / (8 + 5 - 5)
    assert s.mean_acc == float(np.mean([6 / 8, 5 / 8])) and s.miou == float(np.mean([6 / 10, 5 / 8]))
    assert s.fwiou == (8.0 * (6 / 10) + 8.0 * (5 / 8)) / 16
    assert s.support.tolist() == [8, 0, 8]
    want = R.scores_ref(conf)
    assert (s.pixel_acc, s.mean_acc, s.miou, s.fwiou) == (want["pixel_acc"], want["mean_acc"], want["miou"], want["fwiou"])
    # fewer predicted classes than GT classes: class 2 has no column and no diagonal
    t = ops.map_scores(np.array([[1, 1], [0, 2], [3, 0]]))
    assert t.pixel_acc == 3 / 7 and t.acc.tolist() == [1 / 2, 1.0, 0.0] and t.iou.tolist() == [1 / (2 + 4 - 1), 2 / (2 + 3 - 2), 0.0]
    # an empty matrix: NaN, not an exception
    e = ops.map_scores(np.zeros((3, 4), np.int64))
    assert all(np.isnan(x) for x in (e.pixel_acc, e.mean_acc, e.miou, e.fwiou)) and np.isnan(e.acc).all() and np.isnan(e.iou).all()
    assert e.as_dict()["pixel_acc"] is None
    with pytest.raises(ValueError):
        ops.map_scores(np.zeros((3, 4), np.float64))
    rng = np.random.default_rng(0)
    for _ in range(20):
        m = rng.integers(0, 50, (7, 8)) * (rng.random((7, 1)) < 0.7)
        s, want = ops.map_scores(m), R.scores_ref(m)
        assert (s.pixel_acc, s.mean_acc, s.miou, s.fwiou) == (want["pixel_acc"], want["mean_acc"], want["miou"], want["fwiou"]) or m.sum() == 0
        assert np.array_equal(s.iou, want["iou"], equal_nan=True) and np.array_equal(s.acc, want["acc"], equal_nan=True)


# ------------------------------------------------------------------ obj2cls
def test_obj2cls_from_every_source(tmp_path):
    from avlmaps_amd import ops
    want = np.array([4, -1, 0, 7], np.int32)
    assert ops.obj2cls_table(None) is None
    for src in (want, want.astype(np.int64), want.tolist()):
        got = ops.obj2cls_table(src)
        assert got.dtype == np.int32 and np.array_equal(got, want)
    tuples = {0: (4, "chair"), 2: (0, "void"), 3: (7, "table")}           # dataset/README.md:80-90's obj2cls
    assert np.array_equal(ops.obj2cls_table(tuples), want)
    assert np.array_equal(ops.obj2cls_table({0: 4, 2: 0, 3: 7}), want)
    (tmp_path / "t.json").write_text(json.dumps({str(k): list(v) for k, v in tuples.items()}))
    assert np.array_equal(ops.obj2cls_table(tmp_path / "t.json"), want)
    (tmp_path / "l.json").write_text(json.dumps(want.tolist()))
    assert np.array_equal(ops.obj2cls_table(str(tmp_path / "l.json")), want)
    np.save(tmp_path / "t.npy", want.astype(np.int16))
    assert np.array_equal(ops.obj2cls_table(tmp_path / "t.npy"), want)
    for bad in (np.array([0, 2 ** 31], np.int64), {2 ** 31: 1}, {1: 2 ** 31}, {1: (2 ** 31, "x")}, {-1: 0}):
        with pytest.raises(ValueError):
            ops.obj2cls_table(bad)
    with pytest.raises(TypeError):
        ops.obj2cls_table(np.array([0.5, 1.0]))
    with pytest.raises(ValueError):
        ops.obj2cls_table(tmp_path / "t.txt")


# ------------------------------------------------------------------ GTMap file
GS, CS = 48, 0.25


def _config():
    from avlmaps_amd.apps.common import load_config
    return load_config(overrides={"map_config.grid_size": GS, "map_config.cell_size": CS}).map_config


class FakeVLMap:
    def __init__(self, n):
        self.grid_pos = np.zeros((n, 3), np.int32)
        self.occupied_ids = -np.ones((GS, GS, 6), np.int32)


def test_gtmap_file_round_trip_and_wrong_n(tmp_path):
    from avlmaps_amd.map import GTMap
    cfg = _config()
    gt = GTMap(cfg)
    assert not gt.load_map(tmp_path, vlmap=FakeVLMap(5)) and gt.grid_gt is None
    with pytest.raises(RuntimeError, match="no GT map"):
        gt.get_gt_cropped()
    gt.labels = np.array([2, -1, 0, 1, 1], np.int32)
    gt.support = np.array([9, 0, 1, 2 ** 32 - 1, 4], np.uint32)
    gt.grid_gt = np.full((GS, GS), -1, np.int32)
    gt.grid_gt[10:20, 5:9] = np.arange(40).reshape(10, 4) % 3
    gt.stats = np.array([7, 5, 3, 2 ** 40], np.uint64)
    gt.categories = ["void", "wall", "floor"]
    gt.gt_params = dict(cs=CS, stride=1, min_depth=0.1, max_depth=6.0, gs=GS, n_classes=3, n_voxels=5, n_frames=2)
    (tmp_path / "vlmap").mkdir()
    gt.save_map(tmp_path / "vlmap" / GTMap.GT_FILE)
    other = GTMap(cfg)
    assert other.load_map(tmp_path, vlmap=FakeVLMap(5)) is True
    for k in ("labels", "support", "grid_gt", "stats"):
        assert getattr(other, k).dtype == getattr(gt, k).dtype and np.array_equal(getattr(other, k), getattr(gt, k)), k
    assert other.categories == gt.categories and other.gt_params == gt.gt_params
    wrong = GTMap(cfg)
    with pytest.raises(ValueError, match="do not belong"):
        wrong.load_map(tmp_path, vlmap=FakeVLMap(6))
    assert wrong.labels is None
    with pytest.raises(ValueError, match="does not belong"):
        GTMap({**cfg, "grid_size": GS + 2}).load_map(tmp_path, vlmap=FakeVLMap(5))


def test_create_map_needs_semantic_frames(tmp_path):
    from avlmaps_amd.map import GTMap
    (tmp_path / "depth").mkdir()
    with pytest.raises(FileNotFoundError, match="semantic"):
        GTMap(_config()).create_map(tmp_path)


def test_app_flags():
    from avlmaps_amd.apps import create_map, evaluate_map
    a = evaluate_map.parse_args(["--data-dir", "scene", "--categories-file", "c.txt"])
    assert a.dim == "3d" and a.text_model == "clip" and a.json is None
    assert evaluate_map.parse_args(["--data-dir", "s", "--categories-file", "c", "--dim", "2d", "--text-model", "hash"]).dim == "2d"
    for bad in (["--data-dir", "s"], ["--data-dir", "s", "--categories-file", "c", "--dim", "4d"]):
        with pytest.raises(SystemExit):
            evaluate_map.parse_args(bad)
    with pytest.raises(SystemExit):
        create_map.main(["--data-dir", "s", "--obj2cls", "t.json"])         # belongs to --gt


# ------------------------------------------------------------------ arguments: everything is checked before the device is touched
def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    lib = _lib.load()
    kinv, T = np.eye(3), np.eye(4)
    vote = lambda **kw: [kw.get(k, d) for k, d in (("depth", 1), ("u16", 0), ("div", 1000.0), ("sem", 1), ("F", 1), ("H", 6), ("W", 8),      # noqa: E731
                                                    ("kinv", kinv.ctypes.data), ("T", T.ctypes.data), ("gs", 64), ("cs", 0.05), ("vh", 8),
                                                    ("stride", 1), ("dmin", 0.1), ("dmax", 6.0), ("table", None), ("n_obj", 0), ("C", 5),
                                                    ("occ", 1), ("N", 10), ("votes", 1), ("stats", 1), ("err", None), ("stream", None))]
    for bad, word in ((dict(stride=0), b"stride"), (dict(gs=0), b"grid size"), (dict(gs=16385), b"grid size"), (dict(cs=-1.0), b"cell size"),
                      (dict(vh=0), b"voxel height"), (dict(H=0), b"bad batch"), (dict(dmax=0.05), b"depth range"), (dict(C=0), b"classes"),
                      (dict(C=4097), b"classes"), (dict(N=-1), b"voxels"), (dict(N=2 ** 38), b"voxels"), (dict(n_obj=3), b"object table"),
                      (dict(table=1), b"object table"), (dict(u16=1, div=0.0), b"depth_div"), (dict(sem=None), b"null"),
                      (dict(votes=None), b"null"), (dict(stats=None), b"null"), (dict(occ=None), b"null")):
        assert lib.avl_gt_vote(*vote(**bad)) != 0 and word in lib.avl_last_error(), bad
    assert lib.avl_gt_vote(*vote(F=0, depth=None, sem=None)) == 0            # no frames: nothing to do
    assert lib.avl_gt_labels(1, 10, 0, 1, 1, None) != 0 and b"classes" in lib.avl_last_error()
    assert lib.avl_gt_labels(1, 2 ** 38, 5, 1, 1, None) != 0 and b"voxels" in lib.avl_last_error()
    assert lib.avl_gt_labels(None, 10, 5, 1, 1, None) != 0 and b"null" in lib.avl_last_error()
    assert lib.avl_gt_labels(None, 0, 5, None, None, None) == 0
    pool = lambda **kw: [kw.get(k, d) for k, d in (("label", 1), ("N", 10), ("occ", 1), ("gs", 64), ("vh", 8), ("r0", 0), ("r1", 63), ("c0", 0),      # noqa: E731
                                                    ("c1", 63), ("out", 1), ("err", None), ("stream", None))]
    for bad, word in ((dict(gs=0), b"grid size"), (dict(vh=0), b"voxel height"), (dict(r1=64), b"window"), (dict(r0=5, r1=4), b"window"),
                      (dict(c0=-1), b"window"), (dict(c1=64), b"window"), (dict(N=-1), b"voxels"), (dict(out=None), b"null"),
                      (dict(label=None), b"null"), (dict(occ=None), b"null")):
        assert lib.avl_pool_labels_2d(*pool(**bad)) != 0 and word in lib.avl_last_error(), bad
    conf = lambda **kw: [kw.get(k, d) for k, d in (("gt", 1), ("pred", 1), ("n", 10), ("Cg", 5), ("Cp", 6), ("conf", 1), ("skipped", 1),      # noqa: E731
                                                    ("err", None), ("stream", None))]
    for bad, word in ((dict(Cg=0), b"matrix"), (dict(Cp=65537), b"matrix"), (dict(Cg=65536, Cp=65536), b"matrix"), (dict(n=-1), b"pairs"),
                      (dict(gt=None), b"null"), (dict(pred=None), b"null"), (dict(conf=None), b"null"), (dict(skipped=None), b"null")):
        assert lib.avl_label_confusion(*conf(**bad)) != 0 and word in lib.avl_last_error(), bad
    assert lib.avl_label_confusion(*conf(n=0, gt=None, pred=None)) == 0
    assert lib.avl_label_confusion_limits(None) != 0 and b"null" in lib.avl_last_error()


def test_confusion_limits_are_readable_without_a_device():
    from avlmaps_amd import ops
    lds = ops.label_confusion_limits()
    assert lds == 16384 and lds * 4 <= 64 * 1024                           # uint32 counters in the 64 KB a block may take


def _vote_args():
    return dict(votes=None, depth=np.ones((2, 6, 8), np.float32), semantic=np.ones((2, 6, 8), np.int32), calib=R.calib(4.0, 4.0, 3.0),
                transforms=np.stack([np.eye(4)] * 2), occupied_ids=np.zeros((16, 16, 4), np.int32), n_voxels=10, n_classes=5, cs=0.25)


@pytest.mark.parametrize("change, error", [
    (dict(depth=np.ones((2, 6, 8), np.float64)), TypeError),
    (dict(semantic=np.ones((2, 6, 8), np.float32)), TypeError),
    (dict(semantic=np.full((2, 6, 8), 2 ** 31, np.int64)), ValueError),
    (dict(semantic=np.full((2, 6, 8), 2 ** 32 - 1, np.uint32)), ValueError),
    (dict(semantic=np.ones((2, 6, 9), np.int32)), ValueError),
    (dict(occupied_ids=np.zeros((16, 16, 4), np.int64)), TypeError),
    (dict(occupied_ids=np.zeros((16, 15, 4), np.int32)), ValueError),
    (dict(transforms=np.stack([np.eye(4)] * 3)), ValueError),
    (dict(calib=np.eye(4)), ValueError),
    (dict(stride=0), ValueError),
    (dict(n_classes=0), ValueError),
    (dict(n_classes=4097), ValueError),
    (dict(n_voxels=2 ** 38), ValueError),
    (dict(cs=0.0), ValueError),
    (dict(min_depth=2.0, max_depth=1.0), ValueError),
    (dict(obj2cls=np.array([0.5])), TypeError),
    (dict(obj2cls=np.zeros((2, 2), np.int32)), ValueError),
    (dict(votes=np.zeros((10, 5), np.int32)), TypeError),
    (dict(votes=np.zeros((10, 4), np.uint32)), ValueError),
    (dict(stats=np.zeros(4, np.int64)), TypeError),
])
def test_gt_vote_rejects_bad_arguments(change, error, monkeypatch):
    from avlmaps_amd import _lib, ops
    monkeypatch.setattr(_lib, "require_gpu", lambda: (_ for _ in ()).throw(AssertionError("the device was reached")))
    with pytest.raises(error):
        ops.gt_vote(**{**_vote_args(), **change})


def test_the_other_ops_reject_bad_arguments():
    from avlmaps_amd import ops
    with pytest.raises(TypeError):
        ops.gt_labels(np.zeros((4, 3), np.int64))
    with pytest.raises(ValueError):
        ops.gt_labels(np.zeros((4,), np.uint32))
    with pytest.raises(ValueError):
        ops.gt_labels(np.zeros((4, 4097), np.uint32))
    occ = np.zeros((8, 8, 2), np.int32)
    with pytest.raises(TypeError):
        ops.pool_labels_2d(np.zeros(4, np.float32), occ)
    with pytest.raises(TypeError):
        ops.pool_labels_2d(np.zeros(4, np.int32), occ.astype(np.int64))
    with pytest.raises(ValueError):
        ops.pool_labels_2d(np.zeros(4, np.int32), occ, (0, 8, 0, 7))
    with pytest.raises(ValueError):
        ops.pool_labels_2d(np.zeros((4, 1), np.int32), occ)
    with pytest.raises(ValueError):
        ops.label_confusion(np.zeros(4, np.int32), np.zeros(5, np.int32), 3, 3)
    with pytest.raises(ValueError):
        ops.label_confusion(np.zeros(4, np.int32), np.zeros(4, np.int32), 0, 3)
    with pytest.raises(TypeError):
        ops.label_confusion(np.zeros(4, np.float32), np.zeros(4, np.int32), 3, 3)
    with pytest.raises(ValueError):
        ops.label_confusion(np.full(4, 2 ** 31, np.int64), np.zeros(4, np.int32), 3, 3)


# ------------------------------------------------------------------ SciPy's closing
def test_binary_closing_is_dilate_then_erode():
    """GTMap.get_predict_mask runs ops.binary_morph(dilate, 3) then (erode, 3); this pins that it is SciPy's definition of
    binary_closing(iterations=3), border value 0, on masks with set cells on the border (where a border value of 1 would differ)"""
    from scipy.ndimage import binary_closing, binary_dilation, binary_erosion
    rng = np.random.default_rng(4)
    differs_from_border_one = 0
    for shape in ((9, 11), (20, 33), (5, 5), (1, 9)):
        for density in (0.1, 0.3, 0.6):
            m = rng.random(shape) < density
            m[0, :] |= rng.random(shape[1]) < 0.7
            m[:, -1] |= rng.random(shape[0]) < 0.7
            want = binary_closing(m, iterations=3)
            assert np.array_equal(want, binary_erosion(binary_dilation(m, iterations=3), iterations=3))
            assert np.array_equal(want, binary_erosion(binary_dilation(m, iterations=3, border_value=0), iterations=3, border_value=0))
            differs_from_border_one += int(not np.array_equal(want, binary_erosion(binary_dilation(m, iterations=3), iterations=3, border_value=1)))
    assert differs_from_border_one > 0
