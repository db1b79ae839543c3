"""The workspace size queries return fixed numbers, and none of them goes unheld.

The constants were recorded from the library before the entry points moved onto the shared workspace carver (csrc/avl_common.h),
and for the queries added since from the library of the commit before they were pinned; what this pins is that a layout change
never changes a size the Python side or a C caller allocates by.  Three shapes per query: the smallest legal one, one where every
piece needs padding to 256 bytes, and one just above an alignment boundary (four where a flag of the query changes the layout).

SIZES: the queries that are pure arithmetic, or ask rocPRIM for a sort's temporary storage, which it answers without a device: no
GPU needed.  DEVICE_SIZES: avl_merge_rows_work_bytes and avl_merge2_work_bytes also ask rocPRIM for a scan's storage, which it
answers only with a device present (hipErrorNoDevice otherwise): the same pins in a test marked gpu.

test_every_size_query_is_pinned_and_held lists the exported symbols that are size queries and asserts that each is pinned here and
named in the registry of tests/test_work_exact_gpu.py: an entry point with a workspace cannot be added without its exact-size
case.  avl_merge2_max_chunks counts chunks, not bytes: the pattern does not match it."""
import ctypes as C
import re

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
    "avl_merge_work_bytes": [((1,), 1536), ((300,), 5888), ((65,), 2560)],
    "avl_merge2_prepare_work_bytes": [((1,), 768), ((300,), 1792), ((65,), 1024)],
    "avl_argsort_bits_work_bytes": [((1, 4, 1), 1024), ((300, 8, 40), 5632), ((65, 4, 5), 1792)],
    "avl_sim_workspace_bytes_n": [((1, 1, 1), 1024), ((257, 512, 65), 334080), ((8193, 1536, 100), 1427712)],
    "avl_sim_workspace_bytes": [((1, 1), 256), ((512, 65), 200192), ((1536, 100), 811520)],
    "avl_resize_work_bytes": [((1, 1, 1, 1, 0), 256), ((1, 1, 1, 1, 1), 512), ((2, 5, 3, 4, 1), 512), ((1, 65, 4, 1, 1), 768)],
    "avl_label_voxels_work_bytes": [((1,), 1792), ((300,), 9472), ((1025,), 30464)],
    "avl_label_classes_work_bytes": [((1,), 1792), ((300,), 9472), ((1025,), 30464)],
    "avl_colselect_workspace_bytes": [((1,), 133376), ((65,), 133376), ((300,), 133376)],
    "avl_cell_index_work_bytes": [((1, 2, 1), 1280), ((300, 8, 7), 2304), ((300, 33, 31), 10496)],
    "avl_match_ws_bytes": [((1, 1, 1, 1, 1, 0, 0), 1024), ((17, 24, 32, 3, 2, 1, 0), 12800), ((17, 24, 32, 3, 1, 5, 1), 6912)],
    "avl_pool_rows_work_bytes": [((1, 1, 1), 1792), ((32, 32, 32), 9728), ((513, 7, 3), 10240)],
    "avl_object_relations_work_bytes": [((1,), 2304), ((5,), 2560), ((513,), 95744)],
    "avl_travel2d_workspace_bytes": [((1, 1), 1280), ((5, 7), 1536), ((33, 65), 20480)],
    "avl_grow_labels_workspace_bytes": [((1, 1), 3072), ((5, 7), 3584), ((33, 65), 51968)],
    "avl_room_seeds_workspace_bytes": [((1, 1), 2048), ((5, 7), 2048), ((1, 2049), 20480)],
    "avl_room_doors_workspace_bytes": [((1,), 5632), ((2,), 5632), ((40,), 82432)],
}
# the two queries that need a device to answer (see the module docstring)
DEVICE_SIZES = {
    "avl_merge_rows_work_bytes": [((1,), 3072), ((300,), 14592), ((65,), 5632)],
    "avl_merge2_work_bytes": [((1, 1, 1, 0), 7936), ((300, 300, 2, 0), 34304), ((65, 65, 3, 1), 14336), ((500, 300, 2, 0), 39936)],
}
SIZE_QUERY = re.compile(r"_(work|workspace|ws)_bytes(_n)?$")


@pytest.fixture(scope="module")
def lib():
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    build()
    return _lib.load()


def _check_sizes(lib, name, table):
    for args, expected in table[name]:
        n = C.c_size_t(0)
        assert getattr(lib, name)(*args, C.byref(n)) == 0, (name, args, lib.avl_last_error())
        assert n.value == expected, (name, args, n.value, expected)


@pytest.mark.parametrize("name", sorted(SIZES))
def test_work_bytes_are_the_recorded_sizes(lib, name):
    _check_sizes(lib, name, SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DEVICE_SIZES))
def test_work_bytes_that_need_a_device_are_the_recorded_sizes(name):
    from avlmaps_amd import _lib                         # (the built library, as every GPU test loads it)
    _lib.require_gpu()
    _check_sizes(_lib.load(), name, DEVICE_SIZES)


def test_every_size_query_is_pinned_and_held():
    """every exported size query is pinned above and has its exact-size case in tests/test_work_exact_gpu.py (or a stated exemption
    there), and that module's registry names only tests that exist"""
    from avlmaps_amd import _lib
    import test_work_exact_gpu as exact
    queries = sorted(s for s in _lib.EXPORTED_SYMBOLS if SIZE_QUERY.search(s))
    assert len(queries) >= 29 and "avl_merge2_max_chunks" not in queries
    assert not set(SIZES) & set(DEVICE_SIZES)
    pinned = set(SIZES) | set(DEVICE_SIZES)
    assert pinned <= set(queries), sorted(pinned - set(queries))
    for q in queries:
        assert q in pinned, f"{q} has no recorded sizes in tests/test_work_bytes_host.py"
        assert all(len(args) == len(_lib._SIGS[q][1]) - 1 for args, _ in (SIZES.get(q) or DEVICE_SIZES[q])), q
        assert (q in exact.REGISTRY) != (q in exact.EXEMPT), f"{q}: no exact-size case in tests/test_work_exact_gpu.py (REGISTRY), or a stated exemption"
    assert set(exact.REGISTRY) | set(exact.EXEMPT) <= set(queries)
    assert all(isinstance(reason, str) and len(reason) > 20 for reason in exact.EXEMPT.values())
    for q, tests in exact.REGISTRY.items():
        assert tests, q
        for t in tests:
            assert callable(getattr(exact, t, None)), (q, t)
