"""The workspace size queries that are pure arithmetic return fixed numbers: no GPU needed.

The constants were recorded from the library before the entry points moved onto the shared workspace carver (csrc/avl_common.h);
what this pins is that a layout change never changes a size the Python side or a C caller allocates by.  Three shapes per query:
the smallest legal one, one where every piece needs padding to 256 bytes, and one just above an alignment boundary."""
import ctypes as C

import pytest

# query -> [(arguments, bytes)]
SIZES = {
    "avl_dilate_map_work_bytes": [((1, 1), 1024), ((5, 7), 2048), ((5, 13), 3584)],
    "avl_mask_foreground_work_bytes": [((1, 1), 768), ((5, 7), 1024), ((1, 257), 3328)],
    "avl_edt2d_work_bytes": [((1, 1), 256), ((5, 7), 256), ((1, 65), 512)],
    "avl_label_islands_work_bytes": [((1, 1), 512), ((5, 7), 512), ((1, 1025), 4608)],
    "avl_nearest_pair_work_bytes": [((1, 1), 256), ((5, 7), 256), ((2561, 1), 512)],
    "avl_audio_segment_work_bytes": [((1,), 1024), ((4097,), 1024), ((262145,), 2304)],
    "avl_render_topdown_work_bytes": [((1, 1), 16), ((5, 7), 560), ((1, 17), 272)],
    "avl_render_view_work_bytes": [((1, 1), 8), ((5, 7), 280), ((33, 1), 264)],
    "avl_pnp_ransac_work_bytes": [((1,), 96), ((5,), 480), ((3,), 288)],
    "avl_merge2_fold_work_bytes": [((0, 1), 1024), ((5, 3), 1024), ((65, 1), 1792)],
}


@pytest.fixture(scope="module")
def lib():
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    build()
    return _lib.load()


@pytest.mark.parametrize("name", sorted(SIZES))
def test_work_bytes_are_the_recorded_sizes(lib, name):
    for args, expected in SIZES[name]:
        n = C.c_size_t(0)
        assert getattr(lib, name)(*args, C.byref(n)) == 0, (name, args, lib.avl_last_error())
        assert n.value == expected, (name, args, n.value, expected)
