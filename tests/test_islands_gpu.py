"""Object islands on the GPU (csrc/avl_islands.hip through ops.label_islands, trace_islands, contour_nearest_pair,
navigation_utils.get_segment_islands_pos_device and VLMap.get_pos).

Oracles: scipy.ndimage.label / find_objects / sum for the labels, the count and the table; the project's own host tracer
(navigation_utils.get_segment_islands_pos without OpenCV) for the contours; a NumPy expression for the nearest pair.  Every
comparison is np.array_equal: all results are integers that are unique by definition."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_host_mirror import Cfg  # noqa: E402

BOX = np.ones((3, 3), int)


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


# ------------------------------------------------------------------ inputs
def serpentine(H, W):
    """a one-pixel-wide line that runs along every second row and turns at alternating ends"""
    m = np.zeros((H, W), np.uint8)
    m[::2] = 1
    for k, r in enumerate(range(1, H - 1, 2)):
        m[r, W - 1 if k % 2 == 0 else 0] = 1
    return m


def spiral(H, W):
    """a one-pixel-wide square spiral with one-pixel gaps, from the outer border inwards"""
    m = np.zeros((H, W), np.uint8)
    r, c, dr, dc = 0, 0, 0, 1
    m[r, c] = 1
    turns = 0
    while turns < 2:
        nr, nc = r + dr, c + dc
        ahead2r, ahead2c = r + 2 * dr, c + 2 * dc
        blocked = not (0 <= nr < H and 0 <= nc < W) or (0 <= ahead2r < H and 0 <= ahead2c < W and m[ahead2r, ahead2c])
        if blocked:
            dr, dc = dc, -dr
            turns += 1
            continue
        r, c = nr, nc
        m[r, c] = 1
        turns = 0
    return m


@functools.lru_cache(maxsize=None)
def structured():
    rng = np.random.default_rng(20261018)
    eye = np.eye(130, dtype=np.uint8)
    anti = np.fliplr(np.eye(128, dtype=np.uint8))
    rr, cc = np.mgrid[0:63, 0:65]
    lattice = np.zeros((63, 65), np.uint8)
    lattice[::2, ::2] = 1
    frame = np.zeros((50, 70), np.uint8)
    frame[0], frame[-1], frame[:, 0], frame[:, -1] = 1, 1, 1, 1
    frame[20:25, 30:41] = 1                                    # an island of its own inside the one that touches all four borders
    lines = np.zeros((40, 40), np.uint8)
    lines[5, 3:30] = 1                                         # one-pixel-wide lines: the trace passes their pixels twice
    lines[10:35, 35] = 1
    lines[np.arange(12, 30), np.arange(2, 20)] = 1
    lines[38, 1] = 1                                           # and one-pixel islands
    lines[0, 39] = 1
    corner_main = np.zeros((130, 130), np.uint8)               # two blobs whose only link is the diagonal step across (64, 64), the
    corner_main[40:64, 40:64], corner_main[64:90, 64:90] = 1, 1    # common corner of four tiles of any size up to 64
    corner_anti = np.zeros((130, 130), np.uint8)
    corner_anti[40:64, 64:90], corner_anti[64:90, 40:64] = 1, 1
    return {
        "one_set": np.ones((1, 1), np.uint8), "one_clear": np.zeros((1, 1), np.uint8),
        "row_1x37": (rng.random((1, 37)) < 0.6).astype(np.uint8), "col_37x1": (rng.random((37, 1)) < 0.6).astype(np.uint8),
        "row_ones": np.ones((1, 37), np.uint8), "col_ones": np.ones((37, 1), np.uint8),
        "empty": np.zeros((40, 50), np.uint8), "ones_33x65": np.ones((33, 65), np.uint8),
        "random_63x65": (rng.random((63, 65)) < 0.5).astype(np.uint8), "random_130x67": (rng.random((130, 67)) < 0.5).astype(np.uint8),
        "diagonal": eye, "antidiagonal": anti, "cross": eye[:128, :128] | anti, "corner_main": corner_main, "corner_anti": corner_anti,
        "checkerboard": ((rr + cc) % 2 == 0).astype(np.uint8), "lattice": lattice,
        "serpentine_130x67": serpentine(130, 67), "spiral_131x133": spiral(131, 133),
        "frame": frame, "lines": lines,
    }


@functools.lru_cache(maxsize=None)
def big_structured():
    """more than 4 x 4 tiles of any size up to 64: many merge rounds, chains far longer than one flatten step"""
    return {"serpentine_257x261": serpentine(257, 261), "spiral_259x262": spiral(259, 262)}


FILLS = (0.2, 0.45, 0.6, 0.8)


@functools.lru_cache(maxsize=None)
def random_masks(fill):
    rng = np.random.default_rng(int(fill * 100))
    out = []
    for k in range(10):
        H, W = (200, 200) if k == 0 else (int(rng.integers(1, 201)), int(rng.integers(1, 201)))
        out.append((rng.random((H, W)) < fill).astype(np.uint8))
    return out


def expected_table(mask):
    lab, n = ndimage.label(mask, structure=BOX)
    table = np.zeros((n, 8), np.int32)
    if n:
        idx = np.arange(1, n + 1)
        table[:, 0] = ndimage.sum(mask, lab, index=idx)
        for k, sl in enumerate(ndimage.find_objects(lab)):
            table[k, 1:5] = sl[0].start, sl[0].stop - 1, sl[1].start, sl[1].stop - 1
        first = np.unique(lab.ravel(), return_index=True)[1][-n:]          # the first pixel of every label in raster order
        table[:, 5], table[:, 6] = first // mask.shape[1], first % mask.shape[1]
    return lab.astype(np.int32), n, table


def check_labels(ops, mask, what):
    lab, n, table = expected_table(mask)
    with ops.label_islands(mask) as isl:
        assert isl.n == n, what
        assert isl.labels.dtype == np.int32 and np.array_equal(isl.labels, lab), what
        assert isl.table.dtype == np.int32 and isl.table.shape == (n, 8) and np.array_equal(isl.table, table), what


def check_contours(ops, mask, what):
    from avlmaps_amd.device import DeviceArray
    from avlmaps_amd.utils.navigation_utils import get_segment_islands_pos, get_segment_islands_pos_device
    want_c, want_cen, want_box, _ = get_segment_islands_pos(mask, 1)
    got_c, got_cen, got_box, hier = get_segment_islands_pos_device(DeviceArray.from_numpy(mask), 1)
    assert hier is None and len(got_c) == len(want_c) == len(got_cen) == len(got_box), what
    for k in range(len(want_c)):
        assert got_c[k].dtype == want_c[k].dtype and np.array_equal(got_c[k], want_c[k]), (what, k)
        assert got_cen[k] == want_cen[k] and got_box[k] == want_box[k], (what, k)
        assert [type(v) for v in got_cen[k] + got_box[k]] == [type(v) for v in want_cen[k] + want_box[k]], (what, k)


# ------------------------------------------------------------------ labels, count, table
def test_the_structured_masks_are_what_they_claim():
    s = structured()
    assert ndimage.label(s["checkerboard"], structure=BOX)[1] == 1 and ndimage.label(s["checkerboard"])[1] > 1000
    assert ndimage.label(s["lattice"], structure=BOX)[1] == 32 * 33
    for name in ("corner_main", "corner_anti"):
        assert ndimage.label(s[name], structure=BOX)[1] == 1 and ndimage.label(s[name])[1] == 2, name
    for name, m in list(big_structured().items()) + [(k, s[k]) for k in ("serpentine_130x67", "spiral_131x133")]:
        assert ndimage.label(m, structure=BOX)[1] == 1 and m.sum() > m.size // 3, name
        assert ndimage.binary_erosion(m, structure=np.ones((2, 2))).sum() == 0, name       # one pixel wide


@pytest.mark.parametrize("name", sorted(structured()))
def test_labels_of_structured_masks(ops, name):
    check_labels(ops, structured()[name], name)


@pytest.mark.parametrize("name", sorted(big_structured()))
def test_labels_of_long_chains(ops, name):
    check_labels(ops, big_structured()[name], name)


@pytest.mark.parametrize("fill", FILLS)
def test_labels_of_random_masks(ops, fill):
    for k, mask in enumerate(random_masks(fill)):
        check_labels(ops, mask, (fill, k, mask.shape))


def test_labels_of_the_largest_crop(ops):
    mask = (np.random.default_rng(1000).random((1000, 1000)) < 0.45).astype(np.uint8)
    check_labels(ops, mask, "1000 x 1000")


def test_labels_over_two_rounds_of_the_offsets_scan(ops):
    """1025 x 1024 pixels are 1025 scan blocks of 1024 pixels, one more than the offsets workgroup has threads: its loop (and the
    barrier between its rounds) runs twice"""
    mask = (np.random.default_rng(1025).random((1025, 1024)) < 0.05).astype(np.uint8)
    check_labels(ops, mask, "1025 x 1024")


def test_bool_device_and_two_runs_give_identical_bytes(ops):
    from avlmaps_amd.device import DeviceArray
    mask = random_masks(0.45)[0]
    runs = []
    for m in (mask, mask.astype(bool), DeviceArray.from_numpy(mask)):
        with ops.label_islands(m, device=True) as isl:
            assert isinstance(isl.labels, DeviceArray)
            runs.append((isl.n, isl.labels.numpy().tobytes(), isl.table.tobytes()))
    assert runs[0] == runs[1] == runs[2]


def test_bad_arguments_are_error_statuses(ops):
    from avlmaps_amd import _lib
    lib = _lib.load()
    n = C.c_size_t(0)
    for H, W in ((0, 5), (5, 0), (-1, 5), (5, 16385), (16385, 5)):
        assert lib.avl_label_islands_work_bytes(H, W, C.byref(n)) != 0, (H, W)
        assert lib.avl_label_islands(None, W, H, W, None, None, None, 0, None) != 0, (H, W)
        assert lib.avl_island_table(None, H, W, 1, None, None) != 0 and lib.avl_trace_islands(None, H, W, 1, None, None, None, 0, None) != 0
    assert lib.avl_label_islands_work_bytes(16384, 16384, C.byref(n)) == 0 and n.value >= 4 << 28        # 2^28 cells: the limit itself
    assert lib.avl_label_islands_work_bytes(8, 8, None) != 0
    assert lib.avl_label_islands(None, 8, 8, 8, None, None, None, 0, None) != 0 and b"null" in lib.avl_last_error()
    assert lib.avl_island_table(None, 8, 8, 3, None, None) != 0 and lib.avl_island_table(None, 8, 8, 17, None, None) != 0
    assert lib.avl_trace_islands(None, 8, 8, 3, None, None, None, 0, None) != 0
    assert lib.avl_nearest_pair_work_bytes(0, 5, C.byref(n)) != 0 and lib.avl_nearest_pair_work_bytes(5, 0, C.byref(n)) != 0
    assert lib.avl_nearest_pair_i32(None, 4, None, 4, None, None, 0, None) != 0
    with pytest.raises(_lib.AvlError):
        ops.label_islands(np.zeros((0, 7), np.uint8))
    with pytest.raises(ValueError):
        ops.contour_nearest_pair(np.zeros((0, 2), np.int32), np.zeros((3, 2), np.int32))


# ------------------------------------------------------------------ contours
@pytest.mark.parametrize("name", sorted(structured()))
def test_contours_of_structured_masks(ops, name):
    check_contours(ops, structured()[name], name)


@pytest.mark.parametrize("fill", FILLS)
def test_contours_of_random_masks(ops, fill):
    for k, mask in enumerate(random_masks(fill)):
        check_contours(ops, mask, (fill, k, mask.shape))


def test_trace_fills_the_length_column_and_a_line_is_passed_twice(ops):
    mask = structured()["lines"]
    with ops.label_islands(mask) as isl:
        assert not isl.table[:, 7].any()
        contours = ops.trace_islands(isl)
        assert [len(c) for c in contours] == isl.table[:, 7].tolist() and all(c.dtype == np.int32 for c in contours)
        row = int(np.flatnonzero((isl.table[:, 1] == 5) & (isl.table[:, 2] == 5))[0])       # the horizontal line of 27 pixels
        assert isl.table[row, 0] == 27 and len(contours[row]) == 2 * 27 - 2
        assert sorted(len(c) for c in contours)[:2] == [1, 1]


# ------------------------------------------------------------------ nearest pair
def numpy_pair(a, b):
    d = np.linalg.norm(a[:, None].astype(np.int64) - b[None].astype(np.int64), axis=2)
    i, j = np.unravel_index(np.argmin(d), d.shape)
    return int(i), int(j), int(((a[i].astype(np.int64) - b[j]) ** 2).sum())


@pytest.mark.parametrize("na,nb,hi", [(1, 1, 1000), (1, 5000, 1000), (5000, 1, 1000), (300, 300, 8), (3000, 2500, 1001)])
def test_nearest_pair(ops, na, nb, hi):
    rng = np.random.default_rng(na * 7 + nb)
    a, b = rng.integers(0, hi, (na, 2)).astype(np.int32), rng.integers(0, hi, (nb, 2)).astype(np.int32)
    assert ops.contour_nearest_pair(a, b) == numpy_pair(a, b)
    if hi == 8:
        d2 = ((a[:, None].astype(np.int64) - b[None]) ** 2).sum(2)
        assert (d2 == d2.min()).sum() > 50                     # many equal minima: the first-minimum rule decides
        assert ops.contour_nearest_pair(a.astype(np.int64), b.astype(np.float64)) == numpy_pair(a, b)     # what get_pos hands over


def test_nearest_pair_at_the_far_corners(ops):
    a = np.array([[-32768, -32768], [5, 5]], np.int32)
    b = np.array([[32768, 32768]], np.int32)
    assert ops.contour_nearest_pair(a[:1], b) == (0, 0, 2 * 65536 ** 2)             # the largest distance the domain allows: 2^33
    assert ops.contour_nearest_pair(a, b) == numpy_pair(a, b)
    with pytest.raises(ValueError):
        ops.contour_nearest_pair(a, b + 1)


# ------------------------------------------------------------------ VLMap.get_pos
def g8_vlmap(golden, monkeypatch):
    """the VLMap of g8_map2d.npz with the text features of the reference run (the set-up of test_map2d_gpu)"""
    import avlmaps_amd.map.vlmap as vlmap_mod
    from avlmaps_amd.map.vlmap import VLMap
    from avlmaps_amd.utils import clip_utils
    g = golden("g8_map2d.npz")
    mean = {lm: v for lm, v in zip(list(g["dyn_potential"]), g["dyn_mean_feats"])}

    def fake(clip_model, landmarks, clip_feat_dim, use_multiple_templates=False, add_other=True):
        lms = list(landmarks)
        if add_other and lms[-1] != "other":
            lms = lms + ["other"]
        return np.stack([mean[lm] for lm in lms]).astype(np.float32), lms
    monkeypatch.setattr(clip_utils, "landmark_text_feats", fake)
    monkeypatch.setattr(vlmap_mod, "landmark_text_feats", fake)
    gs, vh = int(g["gs"]), int(g["vh"])
    occ = -np.ones((gs, gs, vh), np.int32)
    nz = g["occupied_ids_nz"]
    occ[nz[:, 0], nz[:, 1], nz[:, 2]] = g["occupied_ids_vals"]
    cfg = Cfg(map_type="vlmap", grid_size=gs, cell_size=float(g["cs"]),
              pose_info=Cfg(camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1], base_forward_axis=[0, 0, -1],
                            base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0]))
    vm = VLMap(cfg)
    vm.grid_feat, vm.grid_pos, vm.occupied_ids, vm.grid_rgb = g["grid_feat"], g["grid_pos"], occ, g["grid_rgb"]
    vm.clip_model, vm.clip_feat_dim = None, g["grid_feat"].shape[1]
    vm.generate_obstacle_map(0, 1.5)
    vm.init_categories(list(g["get_pos_categories"]))
    return vm, g


def test_get_pos_device_path_equals_host_path(ops, golden, monkeypatch):
    vm, g = g8_vlmap(golden, monkeypatch)
    islands = 0
    for name in ("wall", "table"):
        vm.island_path = "host"
        want = vm.get_pos(name)
        vm.island_path = "device"
        got = vm.get_pos(name)
        assert np.array_equal(vm._last_foreground, g[f"get_pos_{name}_foreground"]) and vm._last_foreground.dtype == bool
        assert len(got[0]) == len(want[0]) == len(got[1]) == len(got[2])
        islands += len(want[0])
        for k in range(len(want[0])):
            assert got[0][k].dtype == want[0][k].dtype and np.array_equal(got[0][k], want[0][k]), (name, k)
            assert got[1][k] == want[1][k] and got[2][k] == want[2][k], (name, k)
    assert islands > 0
    try:
        import cv2  # noqa: F401
    except Exception:
        vm.island_path = None
        assert vm._island_path() == "device"                   # without OpenCV the device path is the default
