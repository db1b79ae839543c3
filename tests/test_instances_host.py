"""The 3-D instance entry points without a GPU (csrc/avl_instances.hip, ops/instances.py, apps/index_map.py): argument checks that
happen before any device work, the workspace size as recorded from the library as built, the host arithmetic of Instance3D, the
app's flags, and that there is no CPU fallback."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    build()
    return _lib.load()


def _fails(lib, rc, *words):
    msg = lib.avl_last_error().decode()
    assert rc == 1, (rc, msg)                                    # AVL_ERR_INVALID
    for w in words:
        assert w in msg, (w, msg)


def test_symbols_source_and_signatures(lib):
    from avlmaps_amd import _lib, build
    for name in ("avl_label_voxels_work_bytes", "avl_label_voxels", "avl_voxel_instance_table"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert build.SOURCES["avl_instances.hip"] == ["-ffp-contract=off"]


def test_label_voxels_rejects_bad_arguments_before_any_device_work(lib):
    one = C.c_void_p(256)                                        # never dereferenced: every call below fails in its checks
    n = C.c_size_t(0)
    _fails(lib, lib.avl_label_voxels_work_bytes(4, None), "avl_label_voxels_work_bytes", "null")
    _fails(lib, lib.avl_label_voxels_work_bytes(-1, C.byref(n)), "avl_label_voxels_work_bytes", "N = -1")
    _fails(lib, lib.avl_label_voxels_work_bytes(1 << 31, C.byref(n)), "N = 2147483648")
    _fails(lib, lib.avl_label_voxels(one, one, -1, 26, one, one, one, 1 << 20, None), "avl_label_voxels", "N = -1")
    for connectivity in (7, 0, 27, -6):
        _fails(lib, lib.avl_label_voxels(one, one, 4, connectivity, one, one, one, 1 << 20, None), "avl_label_voxels", f"connectivity {connectivity}")
    for k in (0, 1, 4, 5):
        args = [one, one, 4, 26, one, one, one, 1 << 20, None]
        args[k] = None
        _fails(lib, lib.avl_label_voxels(*args), "avl_label_voxels", "null", ("d_grid_pos", "d_mask", "", "", "d_labels", "d_n")[k])
    _fails(lib, lib.avl_label_voxels(one, one, 4, 26, one, one, None, 1 << 20, None), "avl_label_voxels", "workspace (ws)")
    _fails(lib, lib.avl_label_voxels(one, one, 4, 26, one, one, one, 16, None), "workspace (ws) of 16 bytes")


def test_instance_table_rejects_bad_arguments_before_any_device_work(lib):
    one = C.c_void_p(256)
    _fails(lib, lib.avl_voxel_instance_table(one, one, None, -1, 1, one, one, None), "avl_voxel_instance_table", "N = -1")
    _fails(lib, lib.avl_voxel_instance_table(one, one, None, 4, -1, one, one, None), "avl_voxel_instance_table", "n = -1")
    _fails(lib, lib.avl_voxel_instance_table(one, one, None, 4, 5, one, one, None), "n = 5 instances among 4")
    for k in (0, 1, 5, 6):
        args = [one, one, None, 4, 2, one, one, None]
        args[k] = None
        _fails(lib, lib.avl_voxel_instance_table(*args), "avl_voxel_instance_table", "null",
               ("d_grid_pos", "d_labels", "", "", "", "d_table", "d_best_score")[k])
    assert lib.avl_voxel_instance_table(None, None, None, 4, 0, None, None, None) == 0       # no instance: nothing to do


# recorded from the library as built: 256 bytes of header, two uint64 and three int32 per voxel and one int32 per 1024 voxels, each
# piece padded to 256 bytes.  N = 1, N = 5 (every piece is padded) and N = 65 (8 N = 520 and 4 N = 260: just above 512 and 256)
@pytest.mark.parametrize("N,expected", [(0, 256), (1, 1792), (5, 1792), (65, 3584), (1025, 30464)])
def test_work_bytes_are_the_recorded_sizes(lib, N, expected):
    n = C.c_size_t(0)
    assert lib.avl_label_voxels_work_bytes(N, C.byref(n)) == 0, lib.avl_last_error()
    assert n.value == expected


def test_instance3d_center_and_cell():
    from avlmaps_amd import ops
    assert ops.INSTANCE_TABLE_COLS == 12 and ops.INSTANCES_MAX_BOX_SIDE == 1 << 20
    row = np.array([4, 10, 12, 20, 21, 0, 3, 42, 82, 6, 17, 5], np.int64)
    it = ops.Instance3D.from_row(3, row, np.float32(0.75))
    assert it == ops.Instance3D(3, 4, (10, 12, 20, 21, 0, 3), (10.5, 20.5, 1.5), 5, 0.75, (10, 20))       # halves go to the even cell
    assert all(isinstance(v, float) for v in it.center) and all(isinstance(v, int) for v in it.cell + it.bbox)
    it = ops.Instance3D.from_row(1, [3, 0, 0, 0, 0, 0, 0, 35, -34, 1, 0, -1])
    assert it.center == (35 / 3, -34 / 3, 1 / 3) and it.cell == (12, -11) and it.best_voxel == -1 and it.best_score == 0.0
    big = (1 << 53) + 2                                          # the sums are integers: the centre is one exact float64 division
    it = ops.Instance3D.from_row(1, [2, 0, 0, 0, 0, 0, 0, big, 2, 0, 0, 0])
    assert it.center[0] == float(big // 2)


def test_index_map_lists_the_instance_flags(capsys):
    from avlmaps_amd.apps import index_map
    with pytest.raises(SystemExit) as e:
        index_map.parse_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--instances", "--instance K", "--min-voxels", "--connectivity"):
        assert flag in text, flag
    base = ["--data-dir", "x", "--query", "chair"]
    args = index_map.parse_args(base + ["--categories", "chair,table", "--instances", "--instance", "2", "--connectivity", "18"])
    assert args.instances and args.instance == 2 and args.min_voxels == 50 and args.connectivity == 18
    assert index_map.parse_args(base).instances is False and index_map.parse_args(base).instance is None
    for bad in (["--instances"], ["--instance", "1"], ["--categories", "chair", "--instances", "--connectivity", "7"]):
        with pytest.raises(SystemExit):
            index_map.parse_args(base + bad)                     # both need --categories; 7 is no connectivity


def test_no_cpu_fallback_without_gpu(lib):
    from avlmaps_amd import _lib, ops
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.AvlError):
        ops.label_voxels(np.zeros((4, 3), np.int32), np.ones(4, np.uint8))
    with pytest.raises(ValueError):
        ops.label_voxels(np.zeros((4, 3), np.int32), np.ones(4, np.uint8), connectivity=7)
