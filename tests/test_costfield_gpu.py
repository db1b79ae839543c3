"""The cost-weighted travel field and the layered costmap on the GPU (csrc/avl_costfield.hip through ops.cost_field, CostField,
build_costmap and their users Map.get_costmap / get_cost_field / plan_cost_path) against the heap Dijkstra on integer pairs and the
NumPy costmap of tests/_costfield_ref.py.

Every comparison is np.array_equal on both integer planes: the price of a walk is A + B sqrt(2) with integer A and B, different
pairs differ in price, and the kernel orders pairs exactly in integers.  T = ops.TRAVEL_TILE = 32 cells per tile side and
C = ops.TRAVEL_SWEEPS = 64 sweeps per tile and round are the kernel's constants (test_costfield_host.py checks that the source says
the same).  The largest reference Dijkstra here runs on 95 x 94 cells: the serpentine over 3 x 3 tiles needs 3T - 1 rows, and only
every other row of it is free.  Measured on an MI355X with --durations: every test of this module, its reference included, takes
less than 0.7 s (the slowest are the end-to-end plan_path run, 0.6 s, and the 16 MB table of the 4096^2 case, 0.15 s); the whole
module 4 s."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tools"))
sys.path.insert(0, str(HERE))
from _costfield_ref import check_walk, cost_ref, costmap_ref, passable_ref, price_ref  # noqa: E402
from _travel_ref import UNREACHED, serpentine, spiral, travel_ref  # noqa: E402

T, C = 32, 64


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    assert (ops.TRAVEL_TILE, ops.TRAVEL_SWEEPS) == (T, C)
    return ops


def one(H, W, *cells):
    m = np.zeros((H, W), np.uint8)
    for r, c in cells:
        m[r, c] = 1
    return m


def random_map(seed, H, W, density=0.25, n_sources=2):
    """25 % obstacles, prices 0 .. 255 (about 1 free cell in 256 is lethal), sources wherever they fall"""
    rng = np.random.default_rng(seed)
    free = (rng.random((H, W)) >= density).astype(np.uint8)
    cost = rng.integers(0, 256, (H, W)).astype(np.uint8)
    src = np.zeros((H, W), np.uint8)
    src.ravel()[rng.choice(H * W, size=min(n_sources, H * W), replace=False)] = 1
    return free, cost, src


def random_prices(seed, free):
    """1 .. 255 on every cell: a corridor stays a corridor"""
    return np.random.default_rng(seed).integers(1, 256, free.shape).astype(np.uint8)


def check(ops, free, cost, src, name=""):
    """both planes equal the reference; returns (field, A, B)"""
    A, B = cost_ref(free, cost, src)
    f = ops.cost_field(free, cost, src)
    assert f.straight.dtype == np.int32 and f.diagonal.dtype == np.int32 and f.shape == A.shape
    assert np.array_equal(f.straight, A), (name, int((f.straight != A).sum()))
    assert np.array_equal(f.diagonal, B), (name, int((f.diagonal != B).sum()))
    assert f.reached == int((A >= 0).sum()), name
    return f, A, B


# ------------------------------------------------------------------ shapes, price 1 and the closed form
@pytest.mark.parametrize("shape", [(1, 1), (1, 45), (39, 1), (T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, 3 * T - 1)])
def test_shapes(ops, shape):
    H, W = shape
    check(ops, *random_map(H * 131 + W, H, W), shape)


def test_price_one_is_the_travel_field(ops):
    H, W = 2 * T + 1, 3 * T - 1
    free, _, src = random_map(77, H, W)
    f = ops.cost_field(free, np.ones((H, W), np.uint8), src)
    t = ops.travel_field(free, src)                                              # GPU against GPU
    assert np.array_equal(f.straight, t.straight) and np.array_equal(f.diagonal, t.diagonal) and f.reached == t.reached
    A, B = travel_ref(free, src)
    assert np.array_equal(f.straight, A) and np.array_equal(f.diagonal, B)
    assert np.array_equal(f.cost(), t.distance())


def test_uniform_price_255_has_255_times_the_closed_form(ops):
    H, W = 2 * T + 5, 3 * T - 3
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    free, cost = np.ones((H, W), np.uint8), np.full((H, W), 255, np.uint8)
    for r0, c0 in ((0, 0), (H - 1, W - 1), (T - 1, T), (T, T - 1), (T, 2 * T), (H // 2, W // 2)):      # corners, tile borders, centre
        f = ops.cost_field(free, cost, one(H, W, (r0, c0)))
        dr, dc = np.abs(rr - r0), np.abs(cc - c0)
        assert np.array_equal(f.straight, 255 * np.abs(dr - dc)) and np.array_equal(f.diagonal, 255 * np.minimum(dr, dc)), (r0, c0)
        assert f.reached == H * W and f.rounds >= 1 and f.tile_runs >= f.rounds


# ------------------------------------------------------------------ the rule
def test_a_step_costs_the_cell_it_enters(ops):
    src = one(1, 3, (0, 0))
    for free, prices in (([1, 1, 1], [7, 3, 5]), ([1, 1, 1], [0, 3, 5]), ([0, 1, 1], [7, 3, 5]), ([0, 1, 1], [0, 3, 5])):
        f, A, B = check(ops, np.array([free], np.uint8), np.array([prices], np.uint8), src, (free, prices))
        assert f.straight.tolist() == [[0, 3, 8]] and f.diagonal.tolist() == [[0, 0, 0]]       # the source's own price never counts
    f = ops.cost_field(np.ones((1, 3), np.uint8), np.array([[5, 3, 7]], np.uint8), one(1, 3, (0, 2)))
    assert f.straight.tolist() == [[8, 3, 0]]                                    # the reverse walk: 8 + (7 - 5) would be the other end's
    f = ops.cost_field(np.ones((2, 2), np.uint8), np.array([[1, 9], [9, 4]], np.uint8), one(2, 2, (0, 0)))
    assert (f.straight[1, 1], f.diagonal[1, 1]) == (0, 4)                        # a diagonal step puts the price on the diagonal sum


def test_lethal_cells_block_like_obstacles(ops):
    free = np.ones((6, 6), np.uint8)
    cost = np.full((6, 6), 3, np.uint8)
    cost[2, 3] = cost[3, 2] = 0                                                  # the diagonal (2, 2) - (3, 3) runs between two lethal cells
    f, A, B = check(ops, free, cost, one(6, 6, (2, 2)), "diagonal between lethal cells")
    assert (A[3, 3], B[3, 3]) != (0, 3) and A[3, 3] > 0 and A[2, 3] == UNREACHED
    free = np.ones((40, 44), np.uint8)
    cost = np.full((40, 44), 2, np.uint8)
    cost[10:20, 12:25] = 0
    f, A, B = check(ops, free, cost, one(40, 44, (14, 18)), "buried in lethal cells")
    assert f.reached == 1 and (A[14, 18], B[14, 18]) == (0, 0)
    f, A, B = check(ops, free, cost, one(40, 44, (10, 12)), "on the lethal blob's corner")
    assert (A[9, 11], B[9, 11]) == (0, 2) and A[10, 13] == UNREACHED
    free = np.ones((36, 36), np.uint8)
    cost = random_prices(5, free)
    for k in range(36):
        cost[k, 35 - k] = 0                                                      # an anti-diagonal wall of lethal cells
    f, A, B = check(ops, free, cost, one(36, 36, (3, 4)), "lethal wall")
    assert A[35, 35] == UNREACHED and f.reached == 36 * 35 // 2
    cost[17, 18] = 9                                                             # one wall cell missing: a way through
    f, A, B = check(ops, free, cost, one(36, 36, (3, 4)), "lethal wall with a door")
    assert A[35, 35] >= 0 and f.reached == 36 * 36 - 35


def band_corridor(k, p):
    """A one-cell corridor along row 4 from column 0 to column W - 1, crossed by a band of k cells of price p, and a way around it:
    down column 10 to row 34, along it to column W - 11 and up again, 60 steps longer.  Everything else is obstacle, all other
    prices are 1.  Through the band the far end costs (W - 1) + k (p - 1), around it (W - 1) + 60: the break-even is k (p - 1) = 60."""
    H, W = T + 8, 2 * T + 10
    free = np.zeros((H, W), np.uint8)
    free[4, :] = 1
    free[4:35, 10] = free[4:35, W - 11] = 1
    free[34, 10:W - 10] = 1
    cost = np.ones((H, W), np.uint8)
    cost[4, 30:30 + k] = p
    return free, cost, (4, 0), (4, W - 1)


def test_the_detour_decides_by_price(ops):
    for k, p, through in ((6, 10, True), (6, 12, False), (1, 60, True), (1, 62, False)):
        free, cost, start, end = band_corridor(k, p)
        W = free.shape[1]
        f, A, B = check(ops, free, cost, one(*free.shape, start), (k, p))
        assert B[end] == 0 and A[end] == ((W - 1) + k * (p - 1) if through else (W - 1) + 60), (k, p, A[end])     # the reference decides
        assert (f.straight[end], f.diagonal[end]) == (A[end], 0)


# ------------------------------------------------------------------ scheduling
def test_serpentine_inside_one_tile_longer_than_the_cap(ops):
    free = serpentine(T - 1, T)
    f, A, B = check(ops, free, random_prices(1, free), one(T - 1, T, (0, 0)), "serpentine in a tile")
    assert f.rounds > 4 and f.tile_runs == f.rounds and f.reached == int(free.sum())


def test_serpentine_over_three_by_three_tiles(ops):
    free = serpentine(3 * T - 1, 3 * T - 2)                                      # every corridor row crosses all three tile columns
    f, A, B = check(ops, free, random_prices(2, free), one(3 * T - 1, 3 * T - 2, (0, 0)), "serpentine over 3 x 3 tiles")
    assert f.reached == int(free.sum())
    free = serpentine(3 * T - 2, 3 * T - 1).T.copy()                             # and columnwise
    check(ops, free, random_prices(3, free), one(3 * T - 1, 3 * T - 2, (3 * T - 2, 0)), "serpentine over 3 x 3 tiles, transposed")


def test_spiral(ops):
    n = 2 * T + 9
    free = spiral(n)
    f, A, B = check(ops, free, random_prices(4, free), one(n, n, (0, 0)), "spiral inwards")
    assert f.reached == int(free.sum())


# ------------------------------------------------------------------ windows, the workspace, determinism
GUARD = 0xA5


class Raw:
    """avl_costfield2d called directly: three device images with their own row lengths, result planes with a guarded tail of 4096
    bytes each, a guarded stats buffer and a workspace of exactly `ws_bytes` with a guard of 4096 bytes behind it"""

    def __init__(self, free, cost, src, origin, H, W, ws_delta=0):
        from avlmaps_amd import _lib
        from avlmaps_amd.device import DeviceArray
        lib = _lib.load()
        n = ctypes.c_size_t(0)
        assert lib.avl_travel2d_workspace_bytes(H, W, ctypes.byref(n)) == 0        # the travel field's query is this field's
        self.ws_bytes = n.value + ws_delta
        imgs = [DeviceArray.from_numpy(np.ascontiguousarray(a, np.uint8)) for a in (free, cost, src)]
        ptr = [d.ptr + o[0] * a.shape[1] + o[1] for d, a, o in zip(imgs, (free, cost, src), origin)]
        plane = np.full(H * W * 4 + 4096, GUARD, np.uint8)
        a, b = DeviceArray.from_numpy(plane), DeviceArray.from_numpy(plane)
        stats = DeviceArray.from_numpy(np.full(4 * 8 + 64, GUARD, np.uint8))
        ws = DeviceArray.from_numpy(np.full(self.ws_bytes + 4096, GUARD, np.uint8))
        self.rc = lib.avl_costfield2d(ptr[0], free.shape[1], ptr[1], cost.shape[1], ptr[2], src.shape[1], H, W, a.ptr, b.ptr, stats.ptr,
                                      ws.ptr, self.ws_bytes, None)
        self.error = lib.avl_last_error().decode()
        assert lib.avl_stream_sync(None) == 0
        a, b, stats, ws = a.numpy(), b.numpy(), stats.numpy(), ws.numpy()
        self.A, self.B = a[:H * W * 4].view(np.int32).reshape(H, W), b[:H * W * 4].view(np.int32).reshape(H, W)
        self.raw_planes = (a[:H * W * 4], b[:H * W * 4])
        self.tails = (a[H * W * 4:], b[H * W * 4:], stats[32:], ws[self.ws_bytes:])
        self.stats, self.raw_stats = stats[:32].view(np.int64), stats[:32]


def test_windows_of_three_images_with_three_row_lengths(ops):
    from avlmaps_amd.device import DeviceArray
    rng = np.random.default_rng(17)
    H, W = T + 9, 2 * T + 3
    free, cost, src = random_map(18, H, W, n_sources=5)
    assert src.any()
    A, B = cost_ref(free, cost, src)
    bigs, origins = [], ((7, 11), (0, 3), (4, 0))
    for img, (r0, c0), shape in zip((free, cost, src), origins, ((90, 101), (H + 2, W + 30), (H + 4, W + 1))):
        big = rng.integers(0, 256, shape).astype(np.uint8)                       # junk around the window
        big[r0:r0 + H, c0:c0 + W] = img
        bigs.append(big)
    raw = Raw(*bigs, origins, H, W)
    assert raw.rc == 0, raw.error
    assert np.array_equal(raw.A, A) and np.array_equal(raw.B, B)                 # the result of the copied window
    assert all(np.all(t == GUARD) for t in raw.tails)                            # nothing behind the planes, the stats or the workspace
    assert raw.stats[2] == int((A >= 0).sum()) and raw.stats[3] == 1
    # ops.cost_field's window applies to all three planes of one shape
    big_free, big_cost, big_src = random_map(19, 90, 101, n_sources=60)
    r0, r1, c0, c1 = 7, 7 + H, 11, 11 + W
    wf, wc, wsrc = (np.ascontiguousarray(a[r0:r1, c0:c1]) for a in (big_free, big_cost, big_src))
    assert wsrc.any()
    A, B = cost_ref(wf, wc, wsrc)
    for f_in, c_in, s_in in ((big_free, big_cost, big_src),
                             (DeviceArray.from_numpy(big_free), DeviceArray.from_numpy(big_cost), DeviceArray.from_numpy(big_src))):
        f = ops.cost_field(f_in, c_in, s_in, window=(r0, r1, c0, c1))
        assert np.array_equal(f.straight, A) and np.array_equal(f.diagonal, B)
    f = ops.cost_field(big_free, big_cost, np.argwhere(wsrc), window=(r0, r1, c0, c1))       # cells are relative to the window
    assert np.array_equal(f.straight, A) and np.array_equal(f.diagonal, B)
    with pytest.raises(ValueError, match="no source"):
        ops.cost_field(big_free, big_cost, one(90, 101, (0, 0)), window=(r0, r1, c0, c1))
    with pytest.raises(ValueError, match="no source"):
        ops.cost_field(DeviceArray.from_numpy(wf), DeviceArray.from_numpy(wc), DeviceArray.from_numpy(np.zeros_like(wsrc)))


def test_the_travel_workspace_serves_to_the_byte(ops):
    H, W = T + 5, 2 * T + 1
    free, cost, src = random_map(29, H, W)
    A, B = cost_ref(free, cost, src)
    origins = ((0, 0),) * 3
    raw = Raw(free, cost, src, origins, H, W)                                    # exactly avl_travel2d_workspace_bytes
    assert raw.rc == 0, raw.error
    assert np.array_equal(raw.A, A) and np.array_equal(raw.B, B)
    assert all(np.all(t == GUARD) for t in raw.tails)
    short = Raw(free, cost, src, origins, H, W, ws_delta=-1)                     # one byte short: refused, nothing touched
    assert short.rc != 0 and "workspace" in short.error and f"need {raw.ws_bytes}" in short.error
    assert all(np.all(p == GUARD) for p in short.raw_planes) and np.all(short.raw_stats == GUARD)
    assert all(np.all(t == GUARD) for t in short.tails)


def test_two_runs_and_both_result_kinds_give_the_same_bytes(ops):
    from avlmaps_amd.device import DeviceArray
    free, cost, src = random_map(23, 2 * T + 3, 2 * T + 5, density=0.35, n_sources=5)
    a, b = ops.cost_field(free, cost, src), ops.cost_field(free, cost, src)
    assert a.straight.tobytes() == b.straight.tobytes() and a.diagonal.tobytes() == b.diagonal.tobytes() and a.reached == b.reached
    d = ops.cost_field(free, cost, src, device=True)
    assert isinstance(d.straight, DeviceArray) and isinstance(d.diagonal, DeviceArray)
    assert np.array_equal(d.straight.numpy(), a.straight) and np.array_equal(d.diagonal.numpy(), a.diagonal)
    assert np.array_equal(d.reachable(), a.straight >= 0) and np.array_equal(d.cost(), price_ref(a.straight, a.diagonal))


def test_descend_on_device_fields(ops):
    rng = np.random.default_rng(41)
    free, cost, src = random_map(41, 2 * T + 1, T + 9, n_sources=4)
    f = ops.cost_field(free, cost, src, device=True)
    A, B = f.planes()
    cells = np.argwhere(A >= 0)
    assert len(cells) > 20
    for r, c in cells[rng.choice(len(cells), 20, replace=False)]:
        walk = f.descend((r, c))
        assert walk[0] == (r, c)
        check_walk(free, cost, src, A, B, walk)                                  # legal steps, the prices add up to the pair, ends on a source
        way = f.descend((r, c), waypoints=True)
        it = iter(walk)
        assert way[0] == walk[0] and way[-1] == walk[-1] and all(p in it for p in way)       # a subsequence with the same ends
    unreached = np.argwhere(A < 0)
    with pytest.raises(ValueError, match="not reached"):
        f.descend(tuple(unreached[0]))


# ------------------------------------------------------------------ the costmap
def random_layers(ops, seed, H, W, n, device):
    """n (plane, table) pairs: the planes are EDTs of random masks (distances up to a few cells), the tables random with lengths from
    1 up, so that the index clamps at the last entry in most of them; about every tenth entry is 255"""
    rng = np.random.default_rng(seed)
    layers = []
    for k in range(n):
        mask = rng.random((H, W)) < 0.97
        plane = ops.distance_transform_edt(mask, device=device)
        table = rng.integers(0, 90, int(rng.integers(1, 12))).astype(np.uint8)
        table[rng.random(len(table)) < 0.1] = 255
        layers.append((plane, table))
    return layers


@pytest.mark.parametrize("n_layers", [0, 1, 2, 8])
def test_costmap_equals_the_numpy_restatement(ops, n_layers):
    H, W = T + 7, 2 * T + 1
    free = (np.random.default_rng(n_layers).random((H, W)) >= 0.25).astype(np.uint8)
    layers = random_layers(ops, 50 + n_layers, H, W, n_layers, device=True)
    host = [(p.numpy(), t) for p, t in layers]
    want = costmap_ref(free, host)
    got = ops.build_costmap(free, layers)
    assert got.dtype == np.uint8 and got.shape == (H, W) and np.array_equal(got, want), int((got != want).sum())
    assert np.all(got[free == 0] == 0)
    if n_layers == 0:
        assert np.array_equal(got, free)                                         # no layer: price 1 on every free cell
    else:
        assert np.array_equal(ops.build_costmap(free != 0, host, device=True).numpy(), want)  # host planes, a bool map, a device result
    if n_layers == 8:
        assert (want == 254).any() and (want[free != 0] == 0).any()              # the sum clamps; a 255 in any layer is lethal


def test_costmap_clamps_the_index_the_sum_and_lethal_entries(ops):
    free = np.array([[1, 1, 0, 1, 1]], np.uint8)
    d = np.array([[2.0, 1.0, 0.0, 1.0, 3.0]])
    t = np.array([255, 40, 7], np.uint8)
    assert ops.build_costmap(free, [(d, t)]).tolist() == [[8, 41, 0, 41, 8]]     # d^2 = 4 and 9 read the last entry
    assert ops.build_costmap(free, [(d, t), (np.zeros((1, 5)), t)]).tolist() == [[0, 0, 0, 0, 0]]
    assert ops.build_costmap(free, [(np.zeros((1, 5)), t), (d, t)]).tolist() == [[0, 0, 0, 0, 0]]      # in any layer
    big = np.array([200, 254], np.uint8)
    assert ops.build_costmap(free, [(d, big), (d, big)]).tolist() == [[254, 254, 0, 254, 254]]
    assert ops.build_costmap(free, [(d, np.array([9], np.uint8))]).tolist() == [[10, 10, 0, 10, 10]]   # a table of one entry


def test_costmap_recovers_squared_distances_up_to_4096_squared(ops):
    W = 4097
    free = np.ones((1, W), np.uint8)
    free[0, W - 1] = 0                                                           # the clearance of column c is 4096 - c
    plane = ops.distance_transform_edt(free, device=True)
    i = np.arange(4096 * 4096 + 1, dtype=np.int64)
    table = ((i * 40503 >> 5) % 250).astype(np.uint8)                            # neighbours in d^2 almost always differ
    got = ops.build_costmap(free, [(plane, table)])
    want = 1 + table[(4096 - np.arange(W, dtype=np.int64)) ** 2].astype(np.int64)
    want[W - 1] = 0
    assert np.array_equal(got[0], want)
    assert np.array_equal(got, costmap_ref(free, [(plane.numpy(), table)]))
    # and squared distances that are no squares: every r^2 + c^2 of a 70 x 90 map with its one obstacle in the corner
    H, W = 70, 90
    free = np.ones((H, W), np.uint8)
    free[0, 0] = 0
    rr, cc = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    d2 = rr * rr + cc * cc
    assert len(np.unique(d2)) > 2000 and d2.max() == 69 * 69 + 89 * 89
    got = ops.build_costmap(free, [(ops.distance_transform_edt(free, device=True), table[:d2.max() + 1])])
    want = 1 + table[d2].astype(np.int64)
    want[0, 0] = 0
    assert np.array_equal(got, want)


def test_costmap_reads_a_free_map_with_long_rows(ops):
    from avlmaps_amd import _lib
    from avlmaps_amd.device import DeviceArray
    lib = _lib.load()
    H, W = T + 3, T + 14
    rng = np.random.default_rng(61)
    big = rng.integers(0, 2, (H + 9, W + 21)).astype(np.uint8)
    r0, c0 = 5, 13
    free = np.ascontiguousarray(big[r0:r0 + H, c0:c0 + W])
    layers = random_layers(ops, 62, H, W, 2, device=True)
    tables = [DeviceArray.from_numpy(t) for _, t in layers]
    from avlmaps_amd.ops.costmap import _CostLayerC
    # an array of 8 whose entries past n_layers = 2 are null with empty tables: they are never looked at, on the host or in the kernel
    arr = (_CostLayerC * 8)(*[_CostLayerC(p.ptr, d.ptr, len(t)) for (p, t), d in zip(layers, tables)])
    assert all(arr[k].d_distance is None and arr[k].d_table is None and arr[k].n_table == 0 for k in range(2, 8))
    dbig = DeviceArray.from_numpy(big)
    out = DeviceArray.from_numpy(np.full(H * W + 4096, GUARD, np.uint8))
    rc = lib.avl_costmap2d(dbig.ptr + r0 * big.shape[1] + c0, big.shape[1], H, W, arr, 2, out.ptr, None)
    assert rc == 0, lib.avl_last_error().decode()
    got = out.numpy()
    assert np.array_equal(got[:H * W].reshape(H, W), costmap_ref(free, [(p.numpy(), t) for p, t in layers]))
    assert np.all(got[H * W:] == GUARD)


# ------------------------------------------------------------------ the map layer
CS, ROBOT = 0.05, 0.15                 # metres per cell; the robot's radius: 3 cells
RMIN, CMIN = 20, 15
WALL, NARROW, WIDE = 40, (10, 17), (40, 56)      # the dividing wall's column and the rows of its two gaps
START, GOAL = (13, 10), (13, 70)       # crop cells, level with the narrow gap


def two_ways():
    """60 x 80 cells: a border of obstacles and a wall along column 40 with two gaps -- rows 10 .. 16, 7 cells = 0.35 m, wider
    than the robot's 0.30 m but narrow, straight between start and goal; and rows 40 .. 55, 16 cells, a long way round"""
    free = np.ones((60, 80), np.uint8)
    free[0, :] = free[-1, :] = free[:, 0] = free[:, -1] = 0
    free[:, WALL] = 0
    free[NARROW[0]:NARROW[1], WALL] = free[WIDE[0]:WIDE[1], WALL] = 1
    return free


def carpet_mask(full):
    """a carpet across the straight way in the right room; full: from wall to wall, no way around it"""
    m = np.zeros((60, 80), np.uint8)
    m[1:59 if full else 30, 50:61] = 1
    return m


@pytest.fixture(scope="module")
def vmap(ops):
    """a VLMap whose obstacle crop is two_ways() at (RMIN, CMIN) of a 128-cell map, with "carpet" voxels on carpet_mask(False)"""
    from avlmaps_amd.map import VLMap
    pose = dict(camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1], base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0],
                base_up_axis=[0, 1, 0])
    vm = VLMap({"map_type": "vlmap", "grid_size": 128, "cell_size": CS, "pose_info": pose})
    vm.obstacles_cropped = two_ways() != 0
    vm.rmin, vm.cmin = RMIN, CMIN
    vm.rmax, vm.cmax = RMIN + 59, CMIN + 79
    cells = np.argwhere(carpet_mask(False)) + (RMIN, CMIN)
    floor = np.argwhere(two_ways())[::5] + (RMIN, CMIN)
    pos = np.concatenate([np.c_[cells, np.full(len(cells), 1)], np.c_[floor, np.zeros(len(floor), np.int64)]]).astype(np.int32)
    scores = np.zeros((len(pos), 2), np.float32)
    scores[:len(cells), 0] = 1.0
    scores[len(cells):, 1] = 1.0
    vm.grid_pos, vm.categories, vm.scores_mat = pos, ["carpet", "other"], scores
    return vm


def full(cell):
    return [float(cell[0] + RMIN), float(cell[1] + CMIN)]


def crop_cells(path):
    return [(int(p[0]) - RMIN, int(p[1]) - CMIN) for p in path]


def gap_of(cells):
    rows = [r for r, c in cells if c == WALL]
    assert len(rows) == 1, rows
    return "narrow" if NARROW[0] <= rows[0] < NARROW[1] else "wide"


def ref_costmap(ops, free, inflation_radius=0.5, cost_scaling=5.0, peak=100, avoid=()):
    """Map.get_costmap restated on the host: SciPy's EDTs, ops' tables, the NumPy costmap"""
    from scipy.ndimage import distance_transform_edt
    layers = [(distance_transform_edt(free), ops.inflation_table(ROBOT / CS, inflation_radius / CS, cost_scaling * CS, peak))]
    for mask, radius, penalty, lethal in avoid:
        layers.append((distance_transform_edt(mask == 0), ops.penalty_table(radius / CS, penalty, lethal)))
    return costmap_ref(free, layers)


def ref_walk(free, cost):
    """the reference's own cheapest walk from START to GOAL (grown from the goal): its cells, by CostField.descend on reference planes"""
    from avlmaps_amd import ops
    A, B = cost_ref(free, cost, one(60, 80, GOAL))
    field = ops.CostField(A, B, A.shape, int((A >= 0).sum()), 0, 0, passable_ref(free, cost), cost)
    return (A, B), (field.descend(START) if A[START] >= 0 else None)


def test_plan_cost_path_takes_the_narrow_gap_only_when_it_is_cheap(ops, vmap):
    from scipy.ndimage import distance_transform_edt
    free = two_ways()
    clearance = distance_transform_edt(free)
    for kw, way in ((dict(inflation_radius=ROBOT, peak=0), "narrow"), (dict(), "wide")):
        cost = ref_costmap(ops, free, **kw)
        (A, B), walk = ref_walk(free, cost)
        assert gap_of(walk) == way, kw                                           # the reference Dijkstra decides by itself
        assert np.array_equal(vmap.get_costmap(**kw), cost)
        f = vmap.get_cost_field([full(GOAL)], **kw)
        assert np.array_equal(f.straight, A) and np.array_equal(f.diagonal, B)
        path, price = vmap.plan_cost_path(full(START), full(GOAL), waypoints=False, with_cost=True, **kw)
        cells = crop_cells(path)
        assert cells == walk and gap_of(cells) == way
        assert price == price_ref(A, B)[START]
        assert all(clearance[c] * CS >= ROBOT for c in cells)                    # never closer to an obstacle than the robot's radius
        short = vmap.plan_cost_path(full(START), full(GOAL), **kw)               # waypoints: the default
        assert crop_cells(short) == ops.drop_collinear(walk) and short[0] == full(START) and short[-1] == full(GOAL)
        assert vmap.plan_cost_path(full(START), full(GOAL), costmap=cost) == short       # a costmap made before serves


def test_plan_cost_path_snaps_and_refuses(ops, vmap):
    from avlmaps_amd.utils.navigation_utils import NoPathError
    path = vmap.plan_cost_path(full((13, 1)), full(GOAL), waypoints=False)       # the start is inside the robot's radius of the border
    assert crop_cells(path)[0] == (13, 3) and crop_cells(path)[-1] == GOAL       # snapped to the nearest passable cell
    sealed = two_ways()
    sealed[:, WALL] = 0
    saved = vmap.obstacles_cropped
    try:
        vmap.obstacles_cropped = sealed != 0
        with pytest.raises(NoPathError):
            vmap.plan_cost_path(full(START), full(GOAL))
    finally:
        vmap.obstacles_cropped = saved
    with pytest.raises(ValueError, match="outside"):
        vmap.plan_cost_path([RMIN - 1.0, CMIN + 3.0], full(GOAL))
    with pytest.raises(ValueError, match="would be ignored"):
        vmap.plan_cost_path(full(START), full(GOAL), costmap=vmap.get_costmap(), peak=3)


def test_avoid_moves_the_path_off_the_carpet_while_it_can(ops, vmap):
    from avlmaps_amd.map import Map
    from avlmaps_amd.utils.navigation_utils import NoPathError
    free = two_ways()
    base = dict(inflation_radius=ROBOT, peak=0)                                  # without the carpet: straight through the narrow gap
    plain = crop_cells(vmap.plan_cost_path(full(START), full(GOAL), waypoints=False, **base))
    part, whole = carpet_mask(False), carpet_mask(True)
    assert any(part[c] for c in plain)                                           # the straight way crosses the carpet
    for mask, crosses in ((part, False), (whole, True)):
        cost = ref_costmap(ops, free, ROBOT, peak=0, avoid=[(mask, 0.3, 200, False)])
        (A, B), walk = ref_walk(free, cost)
        assert any(mask[c] for c in walk) == crosses                             # the reference: around it while a carpet-free way exists
        assert np.array_equal(vmap.get_costmap(avoid=[(mask, 0.3, 200)], **base), cost)
        cells = crop_cells(vmap.plan_cost_path(full(START), full(GOAL), waypoints=False, avoid=[(mask, 0.3, 200)], **base))
        assert cells == walk and any(mask[c] for c in cells) == crosses
    with pytest.raises(NoPathError):
        vmap.plan_cost_path(full(START), full(GOAL), avoid=[(whole, 0.3, 200, True)], **base)
    lethal = vmap.plan_cost_path(full(START), full(GOAL), waypoints=False, avoid=[(part, 0.3, 200, True)], **base)
    assert not any(part[c] for c in crop_cells(lethal))
    # by name: VLMap resolves "carpet" on the device, a plain Map refuses; an empty mask adds nothing
    assert np.array_equal(vmap.get_predict_mask("carpet") != 0, part != 0)
    named = vmap.get_costmap(avoid=[("carpet", 0.3, 200)], **base)
    assert np.array_equal(named, ref_costmap(ops, free, ROBOT, peak=0, avoid=[(part, 0.3, 200, False)]))
    assert np.array_equal(vmap.get_costmap(avoid=[(np.zeros_like(part), 0.3, 200)], **base), vmap.get_costmap(**base))
    with pytest.raises(ValueError, match="needs a VLMap"):
        Map._avoid_distance(vmap, "carpet")


def test_plan_path_cost_planner_prints_the_path_its_cost_and_clearance(ops, tmp_path):
    """apps.plan_path --planner cost on a --features hash scene, in process: the JSON line is Map.plan_cost_path's walk without its
    collinear cells, its price and its smallest clearance; without the flag nothing of it appears"""
    import yaml
    from PIL import Image
    from scipy.ndimage import distance_transform_edt
    from make_synth_dataset import make
    from avlmaps_amd.apps import create_map, plan_path
    from avlmaps_amd.apps.common import HashClip, load_config
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.navigator import NoPathError
    sc = make(tmp_path / "scene", frames=8, H=96, W=128)
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump({"map_config": {"cam_calib_mat": [64, 0, 64, 0, 64, 48, 0, 0, 1], "depth_sample_rate": 3,
                                                       "grid_size": 400, "cell_size": 0.05}, "params": {"gs": 400, "cs": 0.05}}))
    create_map.main(["--data-dir", str(sc), "--config", str(cfg_path), "--features", "hash", "--feat-dim", "64", "--seed", "3"])
    vm = VLMap(load_config(str(cfg_path)).map_config, data_dir=str(sc))
    assert vm.load_map(str(sc))
    vm.clip_feat_dim = vm.grid_feat.shape[1]
    vm.clip_model = HashClip(vm.clip_feat_dim)
    vm.init_categories(["sofa", "other", "carpet"])                              # plan_path's list: the query, "other", the names to avoid
    vm.generate_obstacle_map(0.0, 1.5)
    free = np.asarray(vm.get_obstacle_cropped()) != 0
    cells = np.argwhere(free)
    base = ["--data-dir", str(sc), "--config", str(cfg_path), "--text-model", "hash", "--query", "sofa"]
    flags = ["--planner", "cost", "--robot-radius", "0.1", "--avoid", "carpet:0.3:200", "--render", str(tmp_path / "p.png")]
    out = plain = None
    for r, c in cells[:: max(1, len(cells) // 8)]:                                # the first start BOTH planners find a way from
        start = [float(r + vm.rmin), float(c + vm.cmin)]
        where = ["--start", str(start[0]), str(start[1])]
        try:
            plain = plan_path.main(base + where)                                  # the default planner
        except NoPathError:                                                       # the one thing that may go wrong here: no way from this start
            continue
        try:
            out = plan_path.main(base + flags + where)
            break
        except SystemExit as e:                                                   # likewise, in the cost planner's words; anything else is a failure
            assert str(e.code).startswith("--planner cost: no passable way"), e.code
    assert out is not None and plain is not None, "no start of the scene has a way for both planners"
    assert plain["path"] and not {"planner", "path_cost", "min_clearance_m"} & set(plain)      # the default line has nothing of this
    assert out["planner"] == "cost" and out["render"] == str(tmp_path / "p.png")
    goal = vm.get_nearest_pos(start, "sofa")
    assert out["goal"] == [float(goal[0]), float(goal[1])]
    costmap = vm.get_costmap(0.1, 0.5, 5.0, avoid=[("carpet", 0.3, 200)])
    walk, price = vm.plan_cost_path(start, goal, costmap=costmap, waypoints=False, with_cost=True)
    assert out["path"] == [list(p) for p in ops.drop_collinear([tuple(p) for p in walk])] and out["path_cost"] == price
    clearance = distance_transform_edt(free)
    least = min(clearance[int(p[0]) - int(vm.rmin), int(p[1]) - int(vm.cmin)] for p in walk) * float(vm.cs)
    assert out["min_clearance_m"] == least and least >= 0.1
    assert np.asarray(Image.open(tmp_path / "p.png")).shape == free.shape + (3,)
