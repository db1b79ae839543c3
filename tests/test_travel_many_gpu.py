"""K travel fields in one batch on the GPU (csrc/avl_travel_many.hip through ops.travel_fields, travel_arrivals and
sound_travel_field, and their users Map.get_travel_fields / get_travel_matrix / plan_tour, VLMap.plan_object_tour and
AVLMap.index_sound_2d_travel / index_goal_2d_sound_travel) against tests/_travel_many_ref.py: a loop of the heap
Dijkstra on integer pairs per set, the arrival rule as plain loops, the sound sum in NumPy step by step, tours by brute force.

Every comparison is np.array_equal, float32 through its uint32 view.  T = 32 cells per tile side, C = 64 sweeps per round."""
import ctypes as C_
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tools"))
sys.path.insert(0, str(HERE))
from _travel_ref import check_walk, pair_less, serpentine, travel_ref  # noqa: E402
from _travel_many_ref import arrivals_ref, csr, fields_ref, set_mask, sound_ref, tour_ref  # noqa: E402

T, C = 32, 64
SHAPES = [(T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, 3 * T - 1)]


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    assert (ops.TRAVEL_TILE, ops.TRAVEL_SWEEPS) == (T, C)
    return ops


def random_sets(rng, H, W, K):
    """K sets of 1 .. 4 cells wherever they fall: some on obstacle cells, some cells twice"""
    return [[(int(rng.integers(H)), int(rng.integers(W))) for _ in range(int(rng.integers(1, 5)))] for _ in range(K)]


@functools.lru_cache(maxsize=None)
def world(shape, K):
    """(free, sets, A, B) of one case: a random map at 25 % obstacles, K random sets, the reference planes -- computed once and
    shared by the tests that need them; nobody writes to them"""
    H, W = shape
    rng = np.random.default_rng(H * 1009 + W * 17 + K)
    free = (rng.random((H, W)) >= 0.25).astype(np.uint8)
    sets = random_sets(rng, H, W, K)
    A, B = fields_ref(free, sets)
    for a in (free, A, B):
        a.setflags(write=False)
    return free, sets, A, B


def equal_fields(ops, tf, A, B, name=""):
    assert tf.straight.dtype == np.int32 and tf.diagonal.dtype == np.int32 and tf.straight.shape == A.shape
    assert np.array_equal(tf.straight, A), (name, int((tf.straight != A).sum()))
    assert np.array_equal(tf.diagonal, B), (name, int((tf.diagonal != B).sum()))
    assert np.array_equal(tf.reached, (A >= 0).sum(axis=(1, 2))), name


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(ops, shape, K):
    free, sets, A, B = world(shape, K)
    tf = ops.travel_fields(free, *csr(sets))
    equal_fields(ops, tf, A, B, (shape, K))
    assert tf.K == K and tf.rounds >= 1 and tf.tile_runs >= tf.rounds
    for k, s in enumerate(sets):                                                 # byte for byte the single field of the set
        one = ops.travel_field(free, np.array(s, np.int32))
        assert tf.straight[k].tobytes() == one.straight.tobytes() and tf.diagonal[k].tobytes() == one.diagonal.tobytes(), k
        assert int(tf.reached[k]) == one.reached


def test_one_cell(ops):
    for v in (0, 1):
        tf = ops.travel_fields(np.full((1, 1), v, np.uint8), [0, 1], [[0, 0]])
        assert tf.straight.tolist() == [[[0]]] and tf.diagonal.tolist() == [[[0]]] and tf.reached.tolist() == [1]


# ------------------------------------------------------------------ 2. tile borders
def test_tile_borders_on_the_empty_map(ops):
    H, W = 2 * T + 5, 3 * T - 3
    srcs = [(T - 1, T), (T, T - 1), (H - 1, W - 1)]
    A, B = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    for r in range(H):
        for c in range(W):
            best = None
            for r0, c0 in srcs:                                                  # the closed form of the empty map, per source
                dr, dc = abs(r - r0), abs(c - c0)
                p = (abs(dr - dc), min(dr, dc))
                if best is None or pair_less(p, best):
                    best = p
            A[r, c], B[r, c] = best
    tf = ops.travel_fields(np.ones((H, W), np.uint8), *csr([srcs, [(0, 0)]]))
    assert np.array_equal(tf.straight[0], A) and np.array_equal(tf.diagonal[0], B)
    rr, cc = np.indices((H, W))
    assert np.array_equal(tf.straight[1], np.abs(rr - cc)) and np.array_equal(tf.diagonal[1], np.minimum(rr, cc))
    assert tf.reached.tolist() == [H * W, H * W]


# ------------------------------------------------------------------ 3. fields of unequal length
def unequal_world():
    """(T - 1) x T: a serpentine in the left columns, a column of obstacles, and to its right obstacles with a sealed pocket"""
    H, W, Ws = T - 1, T, T - 8
    free = np.zeros((H, W), np.uint8)
    free[:, :Ws] = serpentine(H, Ws)
    free[20:23, Ws + 3:Ws + 5] = 1                                                # the pocket: 6 cells, obstacles all around
    return free, [[(0, 0)], [(5, Ws + 3)], [(21, Ws + 3)]]


@pytest.mark.parametrize("reverse", [False, True])
def test_fields_of_unequal_length(ops, reverse):
    free, sets = unequal_world()
    singles = [ops.travel_field(free, np.array(s, np.int32)) for s in sets]
    assert singles[0].straight.max() + singles[0].diagonal.max() > 2 * C and singles[0].rounds > 1
    assert singles[1].reached == 1 and singles[2].reached == 6 and singles[1].rounds <= 1 and singles[2].rounds == 1
    A, B = fields_ref(free, sets)
    order = [2, 1, 0] if reverse else [0, 1, 2]
    tf = ops.travel_fields(free, *csr([sets[k] for k in order]))
    equal_fields(ops, tf, A[order], B[order], reverse)
    for at, k in enumerate(order):
        assert np.array_equal(tf.straight[at], singles[k].straight) and np.array_equal(tf.diagonal[at], singles[k].diagonal)
    print("rounds", tf.rounds, [s.rounds for s in singles], "tile runs", tf.tile_runs, [s.tile_runs for s in singles])
    # one tile per field: a field's schedule in the batch is its own, so the batch runs as long as its slowest field
    assert tf.rounds == max(s.rounds for s in singles)
    assert tf.tile_runs == sum(s.tile_runs for s in singles)


# ------------------------------------------------------------------ 4. set order
def test_set_order(ops):
    free, sets, A, B = world((T + 1, T + 1), 5)
    o, c = csr(sets)
    base = ops.travel_fields(free, o, c)
    twice = ops.travel_fields(free, *csr([sets[3], sets[3]]))
    assert np.array_equal(twice.straight[0], twice.straight[1]) and np.array_equal(twice.diagonal[0], twice.diagonal[1])
    assert np.array_equal(twice.straight[0], A[3]) and twice.reached[0] == twice.reached[1]
    perm = [4, 0, 3, 1, 2]
    p = ops.travel_fields(free, *csr([sets[k] for k in perm]))
    assert np.array_equal(p.straight, base.straight[perm]) and np.array_equal(p.diagonal, base.diagonal[perm])
    assert np.array_equal(p.reached, base.reached[perm])
    rep = ops.travel_fields(free, *csr([s + [s[0], s[-1], s[0]] for s in sets]))  # repeated cells inside every set
    assert np.array_equal(rep.straight, base.straight) and np.array_equal(rep.diagonal, base.diagonal)
    assert np.array_equal(rep.reached, base.reached)


# ------------------------------------------------------------------ 5. more fields than a wave has lanes
def test_sixty_five_fields(ops):
    H, W, K = 40, 44, 65
    rng = np.random.default_rng(65)
    free = (rng.random((H, W)) >= 0.25).astype(np.uint8)
    sets = random_sets(rng, H, W, K)
    tf = ops.travel_fields(free, *csr(sets))
    for k in (0, 1, 31, 63, 64):
        a, b = travel_ref(free, set_mask((H, W), sets[k]))
        assert np.array_equal(tf.straight[k], a) and np.array_equal(tf.diagonal[k], b), k
    for k, s in enumerate(sets):
        one = ops.travel_field(free, np.array(s, np.int32))
        assert np.array_equal(tf.straight[k], one.straight) and np.array_equal(tf.diagonal[k], one.diagonal), k
        assert int(tf.reached[k]) == one.reached


# ------------------------------------------------------------------ 6. strides
def test_windows_and_device_inputs(ops):
    from avlmaps_amd.device import DeviceArray
    rng = np.random.default_rng(6)
    big = (rng.random((90, 101)) >= 0.3).astype(np.uint8)
    r0, r1, c0, c1 = 7, 7 + T + 9, 11, 11 + 2 * T + 3
    free = big[r0:r1, c0:c1].copy()
    sets = random_sets(rng, r1 - r0, c1 - c0, 3)
    A, B = fields_ref(free, sets)
    o, c = csr(sets)
    want = arrivals_ref(free, A, B, sets)
    for f_in in (big, DeviceArray.from_numpy(big), big.astype(np.float32)):
        for device in (False, True):
            tf = ops.travel_fields(f_in, o, c, window=(r0, r1, c0, c1), device=device)
            a, b = tf.planes()
            assert np.array_equal(a, A) and np.array_equal(b, B) and isinstance(tf.straight, DeviceArray) == device
            arr = ops.travel_arrivals(tf, o, c)                                  # reads the free map through the same window
            for got, ref in zip((arr.a, arr.b, arr.cell, arr["from"]), want):
                assert np.array_equal(got, ref)
    f1 = tf.field(1)                                                             # a device batch hands out TravelFields
    assert np.array_equal(f1.planes()[0], A[1]) and f1.reached == int((A[1] >= 0).sum())
    assert np.array_equal(ops.travel_decay_2d(f1, 0.05), ops.travel_decay_2d(ops.travel_field(free, np.array(sets[1], np.int32)), 0.05))
    cell = tuple(np.argwhere(A[1] >= 0)[-1])
    check_walk(free, set_mask(free.shape, sets[1]), A[1], B[1], f1.descend(cell))
    with pytest.raises(ValueError, match="outside"):
        ops.travel_fields(big, [0, 1], [[r1 - r0, 0]], window=(r0, r1, c0, c1))


# ------------------------------------------------------------------ 7. the workspace
def test_workspace_is_k_times_the_single_query(ops):
    from test_work_exact_gpu import dev, exact_and_short, filled
    from avlmaps_amd import _lib
    from avlmaps_amd.device import DeviceArray
    lib = _lib.load()
    env = (_lib, lib, ops, DeviceArray)
    for shape, K in (((T + 1, T + 1), 3), ((5, 7), 2), ((T, T), 1)):
        free, sets, A, B = world(shape, 5)
        H, W = shape
        o, c = csr(sets[:K])
        nb = C_.c_size_t(0)
        _lib.check(lib.avl_travel2d_workspace_bytes(H, W, C_.byref(nb)), "query")
        d_free, d_o, d_c = dev(DeviceArray, free), dev(DeviceArray, o), dev(DeviceArray, c)

        def check(outs):
            assert np.array_equal(outs[0].numpy(), A[:K]) and np.array_equal(outs[1].numpy(), B[:K])
            assert np.array_equal(outs[2].numpy()[2:], (A[:K] >= 0).sum(axis=(1, 2)))

        exact_and_short(env, K * nb.value, (),
                        lambda ws, n, out: lib.avl_travel2d_many(d_free.ptr, W, H, W, d_o.ptr, d_c.ptr, K, len(c), out[0].ptr, out[1].ptr,
                                                                 out[2].ptr, ws, n, None),
                        lambda: [filled(DeviceArray, (K, H, W), np.int32), filled(DeviceArray, (K, H, W), np.int32),
                                 filled(DeviceArray, (2 + K,), np.int64)], check, aligns_base=True)


# ------------------------------------------------------------------ 8. arrivals
@pytest.mark.parametrize("shape", SHAPES)
def test_arrivals_equal_the_reference_and_are_symmetric(ops, shape):
    free, sets, A, B = world(shape, 5)
    o, c = csr(sets)
    arr = ops.travel_arrivals(ops.travel_fields(free, o, c, device=True), o, c)
    for got, ref, name in zip((arr.a, arr.b, arr.cell, arr["from"]), arrivals_ref(free, A, B, sets), "a b cell from".split()):
        assert got.dtype == np.int32 and got.shape == (5, 5) and np.array_equal(got, ref), name
    assert np.array_equal(arr.a, arr.a.T) and np.array_equal(arr.b, arr.b.T)
    assert np.all(np.diag(arr.a) == 0) and np.all(np.diag(arr.b) == 0) and np.all(np.diag(arr["from"]) == -1)
    want = arr.a.astype(np.float64) + arr.b.astype(np.float64) * np.sqrt(2.0)
    want[arr.a < 0] = np.inf
    assert np.array_equal(arr.length(), want)


def test_arrivals_on_obstacles_and_out_of_reach(ops):
    H, W = 40, 44
    free = np.ones((H, W), np.uint8)
    free[10:20, 12:25] = 0                                                        # a block
    free[28, 30:41] = free[36, 30:41] = 0
    free[28:37, 30] = free[28:37, 40] = 0                                         # a closed box around rows 29 .. 35, cols 31 .. 39
    sets = [[(2, 3)],                       # free, outside
            [(14, 18), (15, 18)],           # buried in the block: no walk leaves or reaches it
            [(10, 18), (10, 19)],           # on the block's edge: wholly on obstacles, beside free cells
            [(32, 35)],                     # inside the sealed box
            [(28, 33)],                     # on the box's wall: an obstacle cell that touches both sides
            [(5, 40), (14, 18)]]            # overlaps set 1, and has a free cell
    A, B = fields_ref(free, sets)
    o, c = csr(sets)
    arr = ops.travel_arrivals(ops.travel_fields(free, o, c), o, c)
    for got, ref in zip((arr.a, arr.b, arr.cell, arr["from"]), arrivals_ref(free, A, B, sets)):
        assert np.array_equal(got, ref)
    assert np.array_equal(arr.a, arr.a.T) and np.array_equal(arr.b, arr.b.T)
    assert arr.a[0, 1] == arr.b[0, 1] == arr.cell[0, 1] == arr["from"][0, 1] == -1 and arr.a[1, 0] == -1      # buried: -1 on both sides
    assert arr.a[0, 3] == -1 and arr.a[3, 0] == -1 and np.isinf(arr.length()[0, 3])                              # sealed: -1 on both sides
    assert arr.a[0, 2] > 0 and arr.a[0, 4] > 0 and arr.a[3, 4] >= 0 and arr.a[4, 3] >= 0                        # the wall cell is reached from both sides
    assert (arr.a[1, 5], arr.b[1, 5], arr.cell[1, 5], arr["from"][1, 5]) == (0, 0, int(o[5]) + 1, -1)           # overlap: (0, 0), no direction
    assert (arr.a[5, 1], arr.b[5, 1], arr.cell[5, 1], arr["from"][5, 1]) == (0, 0, int(o[1]), -1)


def test_arrival_steps_and_ties(ops):
    def run(free, sources, targets):
        tf = ops.travel_fields(free, *csr(sources))
        arr = ops.travel_arrivals(tf, *csr(targets))
        ref = arrivals_ref(free, *fields_ref(free, sources), targets)
        for got, want in zip((arr.a, arr.b, arr.cell, arr["from"]), ref):
            assert np.array_equal(got, want)
        return arr
    free = np.ones((12, 12), np.uint8)
    free[5, 5] = free[5, 6] = 0                                                   # two obstacle cells side by side
    arr = run(free, [[(5, 5)]], [[(5, 6)]])
    assert (arr.a[0, 0], arr.b[0, 0], arr["from"][0, 0]) == (1, 0, 4)             # one straight step, from the west
    free = np.ones((12, 12), np.uint8)
    free[5, 5] = free[6, 6] = 0                                                   # diagonal neighbours, both edge-sharing cells free
    arr = run(free, [[(5, 5)]], [[(6, 6)]])
    assert (arr.a[0, 0], arr.b[0, 0], arr["from"][0, 0]) == (0, 1, 3)             # one diagonal step, from the north-west
    free[5, 6] = 0                                                                # one of the two blocked: the diagonal step is refused
    arr = run(free, [[(5, 5)]], [[(6, 6)]])
    assert (arr.a[0, 0], arr.b[0, 0], arr["from"][0, 0]) == (2, 0, 4)             # around: (5, 5) -> (6, 5) -> (6, 6)
    free = np.ones((20, 20), np.uint8)
    arr = run(free, [[(10, 10)]], [[(3, 3)], [(13, 10), (10, 7), (10, 13)], [(12, 11)]])
    assert (arr.a[0, 1], arr.b[0, 1], arr.cell[0, 1]) == (3, 0, 1)                # three cells at (3, 0): the first in CSR order
    assert (arr.a[0, 2], arr.b[0, 2], arr["from"][0, 2]) == (1, 1, 2)             # N and NW both give (1, 1): N comes first
    many = [(10, 10 + 3 * (1 if k % 2 else -1)) if k >= 70 else (0, k % 20) for k in range(150)]     # more cells than lanes; ties past lane 64
    arr = run(free, [[(10, 10)]], [many])
    assert (arr.a[0, 0], arr.b[0, 0], arr.cell[0, 0]) == (3, 0, 70)


# ------------------------------------------------------------------ 9. sound
def sound_world():
    """two rooms with a door, a sealed pocket in the right room; 7 segments of 1 .. 3 locations"""
    H, W, wall = 36, 50, 25
    free = np.ones((H, W), np.uint8)
    free[0, :] = free[H - 1, :] = free[:, 0] = free[:, W - 1] = 0
    free[:, wall] = 0
    free[13:16, wall] = 1
    free[24:31, 36:45] = 0
    free[25:30, 37:44] = 1                                                        # the pocket: walls one cell thick
    sets = [[(5, 23)], [(30, 5), (31, 6), (20, 40)], [(8, 30), (9, 30)], [(0, 10)],                 # (0, 10): on the border, an obstacle
            [(27, 40)], [(17, 12), (27, 41)], [(33, 47), (2, 2), (2, 47)]]                           # (27, 40), (27, 41): in the pocket
    peaks = np.array([0.9, 0.31, 0.0, 0.55, 0.77, 0.128, 0.4], np.float32)
    return free, sets, peaks, wall


def test_sound_equals_numpy_for_every_chunk(ops):
    free, sets, peaks, wall = sound_world()
    decay = 0.02
    A, B = fields_ref(free, sets)
    assert A[4, 5, 5] < 0 and A[3].max() > 0 and (A[0] < 0).any()
    want = sound_ref(A, B, peaks, decay)
    o, c = csr(sets)
    got = {}
    for chunk in (1, 3, 64):
        gf = ops.sound_travel_field(free, o, c, peaks, decay, chunk=chunk)
        f = gf.field.numpy()
        assert f.dtype == np.float32 and f.shape == free.shape
        assert np.array_equal(f.view(np.uint32), want.view(np.uint32)), (chunk, int((f != want).sum()))
        assert np.array_equal(gf.minmax.numpy().view(np.uint32), np.array([want.min(), want.max()], np.float32).view(np.uint32)), chunk
        got[chunk] = f.tobytes()
        norm = ops.sound_travel_normalize(gf).numpy()
        assert np.array_equal(norm.view(np.uint32), ((want - want.min()) / (want.max() - want.min())).view(np.uint32))
    assert got[1] == got[3] == got[64]
    win = (3, 30, 4, 47)                                                           # a window: locations relative to it
    sub = free[win[0]:win[1], win[2]:win[3]]
    wsets = [[(20, 18)], [(5, 30), (2, 2)]]
    wa, wb = fields_ref(sub, wsets)
    gw = ops.sound_travel_field(free, *csr(wsets), peaks[:2], decay, window=win).field.numpy()
    assert np.array_equal(gw.view(np.uint32), sound_ref(wa, wb, peaks[:2], decay).view(np.uint32))


def test_sound_is_quieter_behind_the_wall(ops):
    free, sets, peaks, wall = sound_world()
    (r, c), = sets[0]                                                             # two cells from the wall, far from the door
    one = ops.sound_travel_field(free, [0, 1], [[r, c]], peaks[:1], 0.02).field.numpy()
    cb, cm = 2 * wall - c, 3 * c - 2 * wall                                       # straight behind the wall, and as far on this side
    assert cb - c == c - cm and free[r, cb] and free[r, cm] and 0 < one[r, cb] < one[r, cm]
    euclid = ops.sound_field([0, 1], [[r, c]], peaks[:1], 50, 0.02).field.numpy()  # the Euclidean field cannot tell them apart
    assert euclid[r, cb] == euclid[r, cm] > 0


# ------------------------------------------------------------------ 10. the map layer
from test_travel_gpu import avmap, smoothed  # noqa: E402,F401  (the synthetic AVLMap of the travel tests, one more instance)
from _travel_ref import legal_step  # noqa: E402


@pytest.fixture()
def pocket_map(avmap):
    """the two rooms with a sealed one-cell pocket in the right room's bottom, for the duration of a test -> (av, vm, free, pocket)"""
    av, wall, box = avmap
    vm = av.vlmap
    saved = vm.obstacles_cropped
    rooms = np.array(saved, copy=True)
    h, w = rooms.shape
    rooms[h - 5:h - 2, wall + 2:wall + 5] = 0
    rooms[h - 4, wall + 3] = 1
    vm.obstacles_cropped = rooms
    try:
        yield av, vm, np.asarray(rooms) != 0, (h - 4, wall + 3)
    finally:
        vm.obstacles_cropped = saved


def tour_world(ops, vm, free, pocket):
    """(start, goals as plan_tour takes them, the same as crop-cell sets): a point per room corner, the sofa's mask (obstacle
    cells), a two-point goal, and the pocket"""
    h, w = free.shape
    off = np.array([int(vm.rmin), int(vm.cmin)])
    sofa = smoothed(ops, vm, "sofa")
    crop_goals = [[(h - 3, 3)], [(5, w - 4)], None, [(h - 3, w - 3), (2, w - 3)], [pocket], [(2, 2)]]
    goals, sets = [], []
    for g in crop_goals:
        if g is None:
            goals.append(sofa)
            sets.append([tuple(c) for c in np.argwhere(sofa)])
        else:
            goals.append([[r + off[0] + 0.3, c + off[1] + 0.6] for r, c in g])   # points: their int() cells
            sets.append(g)
    start = (12, 3)
    return [start[0] + off[0] + 0.5, start[1] + off[1] + 0.2], goals, [[start]] + sets


def test_travel_matrix_equals_the_reference(ops, pocket_map):
    av, vm, free, pocket = pocket_map
    start, goals, sets = tour_world(ops, vm, free, pocket)
    A, B = fields_ref(free, sets)
    arr = vm.get_travel_matrix([[start]] + goals)
    for got, ref in zip((arr.a, arr.b, arr.cell, arr["from"]), arrivals_ref(free, A, B, sets)):
        assert np.array_equal(got, ref)
    assert np.array_equal(arr.a, arr.a.T) and np.array_equal(arr.b, arr.b.T) and arr.a[0, 5] == -1 and arr.a[0, 3] > 0
    tf = vm.get_travel_fields([[start]] + goals)
    assert np.array_equal(tf.straight, A) and np.array_equal(tf.diagonal, B)
    one = vm.get_travel_field(goals[2])
    assert np.array_equal(tf.straight[3], one.straight) and np.array_equal(tf.diagonal[3], one.diagonal)
    with pytest.raises(ValueError, match="outside"):
        vm.get_travel_fields([[[vm.rmin - 1, vm.cmin]]])
    with pytest.raises(ValueError, match="empty"):
        vm.get_travel_fields([np.zeros(free.shape, np.uint8)])


@pytest.mark.parametrize("n,closed", [(4, False), (5, True), (6, False), (6, True)])
def test_plan_tour_gives_the_brute_force_order_and_legal_legs(ops, pocket_map, n, closed):
    av, vm, free, pocket = pocket_map
    start, goals, sets = tour_world(ops, vm, free, pocket)
    goals, sets = goals[6 - n:], [sets[0]] + sets[1 + 6 - n:]                     # the last n: the pocket is always among them
    A, B = fields_ref(free, sets)
    a, b, _, _ = arrivals_ref(free, A, B, sets)
    order, total, skipped = tour_ref(a, b, closed)
    tour = vm.plan_tour(start, goals, closed=closed)
    assert tour.order == [g - 1 for g in order] and tour.matrix_pair == tuple(total) and len(order) == n - 1
    assert tour.skipped == [g - 1 for g in skipped] == [sets.index([pocket]) - 1]
    assert tour.matrix_length == total[0] + total[1] * np.sqrt(2.0)
    off = (int(vm.rmin), int(vm.cmin))
    at, driven = sets[0][0], [0, 0]
    stops = order + ([0] if closed else [])
    assert len(tour.legs) == len(tour.driven_pairs) == len(stops)
    for leg, pair, g in zip(tour.legs, tour.driven_pairs, stops):
        walk = [(r - off[0], c - off[1]) for r, c in leg]
        assert walk[0] == at and free[walk[-1]]
        src = set_mask(free.shape, sets[g])
        diag = sum(1 for u, v in zip(walk[:-1], walk[1:]) if u[0] != v[0] and u[1] != v[1])
        assert pair == (len(walk) - 1 - diag, diag)                              # the leg's own step counts
        if src[walk[-1]]:
            check_walk(free, src, A[g], B[g], walk)                              # legal steps, the start's pair, ends on the goal
        else:                                                                    # a goal of obstacle cells: the walk stops one step in front of it
            for v, u in zip(walk[:-1], walk[1:]):
                assert legal_step(free, src, u, v), (u, v)
            left = (int(A[g][walk[0]]) - pair[0], int(B[g][walk[0]]) - pair[1])
            assert left in ((1, 0), (0, 1))
        at = walk[-1]
        driven[0] += pair[0]
        driven[1] += pair[1]
    assert not pair_less(tuple(driven), tuple(total))                             # the driven length is never below the matrix length
    assert tour.driven_length == driven[0] + driven[1] * np.sqrt(2.0)
    if closed:
        assert at == sets[0][0] and tour.closed
    with pytest.raises(ValueError, match="goals"):
        vm.plan_tour(start, [])


def test_plan_object_tour(ops, pocket_map):
    av, vm, free, pocket = pocket_map
    h, w = free.shape
    start = [int(vm.rmin) + h - 3, int(vm.cmin) + w - 3]                          # in the right room: the table comes first
    tour = vm.plan_object_tour(start, ["sofa", "table"])
    sets = [[(h - 3, w - 3)]] + [[tuple(c) for c in np.argwhere(smoothed(ops, vm, name))] for name in ("sofa", "table")]
    a, b, _, _ = arrivals_ref(free, *fields_ref(free, sets), sets)
    order, total, skipped = tour_ref(a, b)
    assert tour.names == [("sofa", "table")[g - 1] for g in order] == ["table", "sofa"] and tour.skipped_names == []
    assert tour.matrix_pair == tuple(total) and len(tour.legs) == 2
    with pytest.raises(ValueError, match="no target"):
        vm.plan_object_tour(start, ["sofa", "lamp"])


def test_index_sound_2d_travel_and_the_goal_with_it(ops, avmap):
    av = avmap[0]
    vm = av.vlmap
    free = np.asarray(vm.obstacles_cropped) != 0
    h, w = free.shape
    r0, c0 = int(vm.rmin), int(vm.cmin)
    av.index_sound_2d("dog")                                                      # lists the segments' cells
    offsets, cells = av._sound_cells
    peaks = np.asarray(av.sound_map.get_distribution_and_locations("dog")[0], np.float32)
    sets, kept = [], []
    for s in range(len(peaks)):
        own = [(int(r) - r0, int(c) - c0) for r, c in cells[offsets[s]:offsets[s + 1]] if r0 <= r < r0 + h and c0 <= c < c0 + w]
        if own:
            sets.append(own)
            kept.append(peaks[s])
    assert len(sets) >= 3
    for rate in (0.01, 0.05):
        raw = sound_ref(*fields_ref(free, sets), np.array(kept, np.float32), rate)
        want = (raw - raw.min()) / (raw.max() - raw.min())
        got = av.index_sound_2d_travel("dog", rate)
        assert got.dtype == np.float32 and got.shape == (h, w) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), rate
        assert got.max() == 1.0 and got.min() == 0.0
    win = (slice(r0, r0 + h), slice(c0, c0 + w))
    # index_goal_2d_travel is what it was: its sound factor is the Euclidean one, the product of the stand-alone calls bit for bit
    plain = av.index_goal_2d_travel(obj="table", sound=[("dog", 0.05)], area="kitchen")
    was = vm.get_travel_distribution_map("table", 0.1).astype(np.float64)
    was = was * av.index_area_2d("kitchen")[win].astype(np.float64)
    was = was * av.index_sound_2d("dog", 0.05)[win].astype(np.float64)
    assert np.array_equal(plain.heat.view(np.uint64), was.view(np.uint64))
    nosound = dict(obj="sofa", area="kitchen", start=[r0 + h - 3, c0 + 3])      # without a sound the two calls are one
    a, b = av.index_goal_2d_travel(**nosound), av.index_goal_2d_sound_travel(**nosound)
    assert np.array_equal(a.heat.view(np.uint64), b.heat.view(np.uint64)) and a.cell.tolist() == b.cell.tolist() and a.value == b.value
    goal = av.index_goal_2d_sound_travel(obj="table", sound=[("dog", 0.05)], area="kitchen")
    want = vm.get_travel_distribution_map("table", 0.1).astype(np.float64)
    want = want * av.index_area_2d("kitchen")[win].astype(np.float64)
    want = want * av.index_sound_2d_travel("dog", 0.05).astype(np.float64)
    assert np.array_equal(goal.heat.view(np.uint64), want.view(np.uint64))
    r, c = np.unravel_index(np.argmax(want), want.shape)
    assert goal.cell.tolist() == [r + r0, c + c0] and goal.value == want[r, c]
    lean = av.index_goal_2d_sound_travel(obj="table", sound=[("dog", 0.05)], area="kitchen", want_heat=False)
    assert lean.heat is None and lean.cell.tolist() == goal.cell.tolist() and lean.value == goal.value
    # slow decays, so that the product is not zero everywhere: the two sound factors then give different goals' heats
    goal = av.index_goal_2d_sound_travel(obj=[("table", 0.01)], sound="dog")
    want = vm.get_travel_distribution_map("table", 0.01).astype(np.float64) * av.index_sound_2d_travel("dog", 0.01).astype(np.float64)
    was = av.index_goal_2d_travel(obj=[("table", 0.01)], sound="dog").heat
    print("goal with the sound around walls: max", want.max(), "cells that differ from the Euclidean goal", int((want != was).sum()))
    assert np.array_equal(goal.heat.view(np.uint64), want.view(np.uint64)) and want.max() > 0 and not np.array_equal(want, was)
    r, c = np.unravel_index(np.argmax(want), want.shape)
    assert goal.cell.tolist() == [r + r0, c + c0] and goal.value == want[r, c]
