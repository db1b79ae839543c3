"""The host side of the batched travel fields, without a GPU: the tour order (map/tour.held_karp) against a brute force over
permutations on reference matrices, the argument checks of ops.travel_fields and of the C entry points (before any device work),
the app's flag combinations, and that the batch kernel's geometry is the single field's."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
AVL_ERR_INVALID = 1
sys.path.insert(0, str(HERE))
from _travel_ref import pair_less  # noqa: E402
from _travel_many_ref import arrivals_ref, fields_ref, tour_ref  # noqa: E402


def matrix(free, sets):
    A, B = fields_ref(free, sets)
    a, b, _, _ = arrivals_ref(free, A, B, sets)
    assert np.array_equal(a, a.T) and np.array_equal(b, b.T)
    return a, b


def rooms_map():
    free = np.ones((20, 24), np.uint8)
    free[:, 11] = 0
    free[8:10, 11] = 1                                                            # a wall with a door
    free[14, 15:21] = free[18, 15:21] = 0
    free[14:19, 15] = free[14:19, 20] = 0                                         # a sealed pocket, rows 15 .. 17, cols 16 .. 19
    free[3:6, 3:6] = 0                                                            # a block: a goal on obstacle cells
    return free


# ------------------------------------------------------------------ Held-Karp
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("closed", [False, True])
def test_held_karp_equals_brute_force(n, closed):
    from avlmaps_amd.map.tour import held_karp
    rng = np.random.default_rng(100 * n + closed)
    free = rooms_map()
    for trial in range(3):
        sets = [[(10, 2)]]                                                        # the start
        pool = [[(4, 4), (3, 3)], [(16, 17)], [(2, 20)], [(18, 2), (18, 3)], [(1, 12)], [(12, 22)], [(8, 11)], [(19, 10)], [(0, 0)]]
        for k in rng.permutation(len(pool))[:n]:
            sets.append(pool[k])
        a, b = matrix(free, sets)
        want = tour_ref(a, b, closed)
        got = held_karp(a, b, closed)
        assert got[0] == want[0] and tuple(got[1]) == tuple(want[1]) and got[2] == want[2], (n, closed, trial, sets)
        if any(s == [(16, 17)] for s in sets):
            assert got[2] == [sets.index([(16, 17)])]                              # the goal in the pocket is skipped
        tot = [0, 0]
        for u, v in zip([0] + got[0], got[0] + ([0] if closed and got[0] else [])):
            tot[0] += int(a[u, v])
            tot[1] += int(b[u, v])
        assert tuple(tot) == tuple(got[1])


def test_held_karp_ties_go_to_the_smallest_order():
    from avlmaps_amd.map.tour import held_karp
    free = np.ones((21, 21), np.uint8)
    sets = [[(10, 10)], [(10, 15)], [(10, 5)], [(15, 10)], [(5, 10)]]            # four goals at (5, 0) from the start, a square around it
    a, b = matrix(free, sets)
    for closed in (False, True):
        order, total, skipped = held_karp(a, b, closed)
        want = tour_ref(a, b, closed)
        assert (order, tuple(total), skipped) == (want[0], tuple(want[1]), [])
    assert held_karp(a, b, True)[0][0] == 1                                      # every rotation and reflection ties: the smallest comes first
    # all goals out of reach: nothing to order
    free = rooms_map()
    a, b = matrix(free, [[(10, 2)], [(16, 17)], [(16, 18)]])
    assert held_karp(a, b) == ([], (0, 0), [1, 2])
    with pytest.raises(ValueError, match="at most"):
        held_karp(np.zeros((12, 12), np.int32), np.zeros((12, 12), np.int32))


def test_held_karp_compares_sums_exactly():
    """(7, 0) against (0, 5): 7 < 5 sqrt(2) = 7.071; and sums whose floats would tie are told apart"""
    from avlmaps_amd.map.tour import held_karp, pair_less as less
    assert less((7, 0), (0, 5)) and not less((0, 5), (7, 0)) and not less((3, 4), (3, 4))
    big = 10 ** 12
    assert less((big, big), (big + 1, big)) and less((big, big), (big, big + 1)) and pair_less((big, big), (big + 1, big))
    a = np.array([[0, 7, 0], [7, 0, 1], [0, 1, 0]], np.int64)
    b = np.array([[0, 0, 5], [0, 0, 0], [5, 0, 0]], np.int64)
    order, total, _ = held_karp(a, b)
    assert order == [1, 2] and total == (8, 0)                                    # 7 + 1 < 5 sqrt(2) + 1


# ------------------------------------------------------------------ argument checks
def test_travel_fields_argument_errors():
    from avlmaps_amd import ops
    free = np.ones((6, 9), np.uint8)
    with pytest.raises(ValueError, match="one cell or more"):
        ops.travel_fields(free, [0, 1, 1], [[0, 0]])                              # an empty set
    with pytest.raises(ValueError, match="CSR"):
        ops.travel_fields(free, [1, 2], [[0, 0], [1, 1]])                         # does not start at 0
    with pytest.raises(ValueError, match="CSR"):
        ops.travel_fields(free, [0, 1], [[0, 0], [1, 1]])                         # does not end at L
    with pytest.raises(ValueError, match="CSR"):
        ops.travel_fields(free, [0, 2, 1, 3], [[0, 0], [1, 1], [2, 2]])           # not monotonic
    with pytest.raises(ValueError, match="CSR"):
        ops.travel_fields(free, [], np.zeros((0, 2), np.int32))
    for cell in ([6, 0], [0, 9], [-1, 0]):
        with pytest.raises(ValueError, match="outside"):
            ops.travel_fields(free, [0, 1], [cell])
    with pytest.raises(ValueError, match="outside"):
        ops.travel_fields(free, [0, 1], [[3, 3]], window=(0, 3, 0, 9))            # inside the map, outside the window
    with pytest.raises(ValueError, match="integers"):
        ops.travel_fields(free, [0, 1], [[0.5, 1.0]])
    with pytest.raises(ValueError, match="window"):
        ops.travel_fields(free, [0, 1], [[0, 0]], window=(0, 7, 0, 9))
    with pytest.raises(ValueError, match="peaks"):
        ops.sound_travel_field(free, [0, 1], [[0, 0]], [0.5, 0.5], 0.01)
    with pytest.raises(ValueError, match="chunk"):
        ops.sound_travel_field(free, [0, 1], [[0, 0]], [0.5], 0.01, chunk=0)


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    from avlmaps_amd import _lib
    lib = _lib.load()
    one = 0x1000                                                                  # never dereferenced: every check below is on the host

    def many(K, ws=one, ws_bytes=1 << 30, free=one, H=5, W=7, L=None):
        return lib.avl_travel2d_many(free, W, H, W, one, one, K, K if L is None else L, one, one, one, ws, ws_bytes, None)
    for K, word in ((0, b"fields"), (1025, b"fields"), (-1, b"fields")):
        assert many(K) == AVL_ERR_INVALID and word in lib.avl_last_error(), K
    assert many(2, free=None) == AVL_ERR_INVALID and b"null" in lib.avl_last_error()
    assert many(2, ws=None) == AVL_ERR_INVALID and b"workspace" in lib.avl_last_error()
    assert many(2, ws_bytes=2 * 1536 - 1) == AVL_ERR_INVALID and b"need 3072" in lib.avl_last_error()      # K x the single query
    assert many(2, L=1) == AVL_ERR_INVALID and b"cells" in lib.avl_last_error()
    assert many(1, H=0) == AVL_ERR_INVALID and many(1, W=16385) == AVL_ERR_INVALID
    assert lib.avl_travel_arrive(one, 7, 5, 7, one, one, 0, one, one, 1, 1, one, one, one, one, None) == AVL_ERR_INVALID
    assert lib.avl_travel_arrive(one, 7, 5, 7, one, one, 1, one, one, 1025, 1, one, one, one, one, None) == AVL_ERR_INVALID
    assert lib.avl_travel_arrive(one, 7, 5, 7, one, one, 1, one, one, 1, 1, None, one, one, one, None) == AVL_ERR_INVALID
    assert lib.avl_travel_arrive(one, 6, 5, 7, one, one, 1, one, one, 1, 1, one, one, one, one, None) == AVL_ERR_INVALID
    assert lib.avl_travel_sound2d(one, one, 0, 5, 7, one, 0.01, 1, one, one, None) == AVL_ERR_INVALID
    assert lib.avl_travel_sound2d(one, one, 1, 5, 7, one, -0.01, 1, one, one, None) == AVL_ERR_INVALID
    assert lib.avl_travel_sound2d(one, one, 1, 5, 7, None, 0.01, 1, one, one, None) == AVL_ERR_INVALID
    assert lib.avl_travel_sound_normalize(one, None, 5, 7, one, None) == AVL_ERR_INVALID


def test_the_batch_kernel_has_the_single_fields_geometry():
    from avlmaps_amd import ops
    """... because there is one geometry and one body: the header's, which the sources of all four families use and none repeats"""
    csrc = ROOT / "avlmaps_amd" / "csrc"
    head = (csrc / "avl_travel_tile.h").read_text()
    many = (csrc / "avl_travel_many.hip").read_text()

    def const(text, name):
        return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))
    assert const(head, "kTravelTile") == ops.TRAVEL_TILE and const(head, "kTravelSweeps") == ops.TRAVEL_SWEEPS
    assert const(head, "kTravelThreads") == 256 and const(head, "kTravelMaxSide") == ops.TRAVEL_MAX_SIDE
    assert const(many, "kManyMaxFields") == ops.TRAVEL_MANY_MAX_FIELDS
    for name in ("avl_travel.hip", "avl_costfield.hip", "avl_travel_many.hip", "avl_rooms.hip"):
        src = (csrc / name).read_text()
        assert not re.search(r"constexpr int k(Travel|Cost|Many|Grow)(Tile|Threads|Cells|Sweeps|Halo|MaxSide)\b", src), name
        assert "bool travel_less" not in src and "cost_less" not in src, name
        if name != "avl_rooms.hip":                                               # the three field families: no sweep loop of their own
            assert '#include "avl_travel_tile.h"' in src and "travel_tile_relax<" in src and "__syncthreads_or" not in src, name
    assert head.count("bool travel_less") == 1 and "cost_less" not in head          # one definition, in the header
    assert "travel_less" in many                                                    # (the arrivals compare with it)


# ------------------------------------------------------------------ the app's flags
def test_plan_path_flag_combinations():
    from avlmaps_amd.apps import plan_path as P
    base = ["--data-dir", "x", "--start", "1", "2"]
    a = P.parse_args(base + ["--tour", "sofa, table,lamp", "--tour-closed"])
    assert a.tour == ["sofa", "table", "lamp"] and a.tour_closed and a.query is None
    a = P.parse_args(base + ["--tour", "sofa", "--customize-obstacles"])
    assert a.tour == ["sofa"] and not a.tour_closed
    a = P.parse_args(base + ["--query", "sofa", "--goal-2d", "--travel", "--sound", "dog", "--sound-travel"])
    assert a.sound_travel and a.tour is None
    assert not P.parse_args(base + ["--query", "sofa", "--goal-2d", "--travel", "--sound", "dog"]).sound_travel
    bad = [["--tour", "sofa", "--query", "table"], ["--tour", "sofa", "--goal", "frontier"], ["--tour", "sofa", "--relation", "left", "--heading", "0"],
           ["--tour", "sofa", "--area", "kitchen"], ["--tour", "sofa", "--sound", "dog"], ["--tour", "sofa", "--goal-2d"], ["--tour", "sofa", "--view"],
           ["--tour", "sofa", "--nearest", "path"], ["--tour", "sofa", "--room", "1"], ["--tour", "sofa", "--planner", "cost"],
           ["--tour", "sofa", "--render", "x.png"], ["--tour", "sofa", "--known-free"], ["--tour", " , "],
           ["--tour", ",".join("abcdefghijk")], ["--query", "sofa", "--tour-closed"],
           ["--query", "sofa", "--sound-travel"], ["--query", "sofa", "--goal-2d", "--sound", "dog", "--sound-travel"],
           ["--query", "sofa", "--goal-2d", "--travel", "--sound-travel"], ["--query", "sofa", "--sound", "dog", "--sound-travel"]]
    for flags in bad:
        with pytest.raises(SystemExit):
            P.parse_args(base + flags)
