"""avl_heat.hip at its edges, against the float64 brute force (oracle/avl_oracle.py: heatmap_from_mask) and a closed form: columns of
more than one 64-bit grid word (nearest_bit and the w0..w1 loop), windows whose column bits straddle two column-map words, the
kernels without the LDS coarse grid, and the brute-force kernel around its 1024-target tile.  Every comparison is bit for bit, of
the stateless call and of the planned call separately -- never of the two with each other."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CS = 0.05


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


@pytest.fixture(scope="module")
def O():
    from oracle import avl_oracle
    return avl_oracle


def check_both(ops, plan, pos, mask, decay, want, what):
    got = ops.heatmap_from_mask(pos, mask, CS, decay)
    assert got.dtype == np.float32 and np.array_equal(got, want), ("stateless",) + what + (np.flatnonzero(got != want)[:8],)
    got = plan(mask, CS, decay).numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want), ("planned",) + what + (np.flatnonzero(got != want)[:8],)


COLUMN_TARGETS = [(0,), (63,), (64,), (127, 128), (191,), (63, 64), (0, 191)] + [(z,) for z in range(60, 69)]


@pytest.mark.parametrize("decay,R", [(0.01, 5), (0.003125, 16)])
def test_single_column_of_three_words_is_the_closed_form(ops, O, decay, R):
    """192 voxels (0, 0, z) -- three grid words -- and one at (1, 0, 0): heat = clip(1 - |z - nearest target| / cs * decay, 0, 1) in
    float64, exactly 0 from R = cs / decay cells on.  The target sets put the nearest target in the voxel's own word, in the word
    below and above, on bits 0 and 63, and exactly R away: every branch of nearest_bit()."""
    assert int(np.ceil(CS / decay)) == R and (2 * R + 1) ** 3 <= 40000          # the windowed kernel, not the brute force
    z = np.arange(192)
    pos = np.concatenate([np.stack([0 * z, 0 * z, z], 1), [[1, 0, 0]]]).astype(np.int32)
    plan = ops.HeatPlan(pos)
    for targets in COLUMN_TARGETS:
        mask = np.zeros(193, bool)
        mask[list(targets)] = True
        d = np.abs(z[:, None] - np.asarray(targets)[None]).min(axis=1).astype(np.float64)
        closed = np.clip(1.0 - d / CS * decay, 0.0, 1.0)
        assert (closed[d >= R] == 0).all() and (closed[d == R - 1] > 0).all() and (d == R).any()
        want = O.heatmap_from_mask(pos, mask, CS, decay)
        assert np.array_equal(want[:192], closed.astype(np.float32)), targets      # the oracle is the closed form on the column
        check_both(ops, plan, pos, mask, decay, want, (targets, decay))
    plan.close()


def tall_box(nz, seed):
    """~6000 distinct voxels of a 12 x 80 x nz box at z offset -3, its eight corners among them"""
    rng = np.random.default_rng(seed)
    nx, ny = 12, 80
    corners = np.array([(x * ny + y) * nz + z for x in (0, nx - 1) for y in (0, ny - 1) for z in (0, nz - 1)])
    n = min(6000, nx * ny * nz // 4)
    lin = np.unique(np.concatenate([corners, rng.choice(nx * ny * nz, n, replace=False)]))
    lin = lin[rng.permutation(len(lin))]                                       # voxel ids are in no spatial order
    pos = np.stack([lin // (ny * nz) + 400, (lin // nz) % ny + 450, lin % nz - 3], 1).astype(np.int32)
    N = len(pos)
    centre = pos[rng.integers(0, N, 3)]
    masks = dict(clustered=(np.abs(pos[:, None, :] - centre[None]).max(axis=2) <= 6).any(axis=1), uniform=rng.random(N) < 0.02,
                 one=np.arange(N) == 777, corners=np.isin(lin, corners), empty=np.zeros(N, bool), full=np.ones(N, bool))
    assert masks["corners"].sum() == 8 and 0 < masks["clustered"].sum() < N and masks["uniform"].sum() > 20
    return pos, masks


# 0.003125: R = 16, the largest window (33^3 <= 40000); 0.003: R = 17, 35^3 > 40000 -> brute force; 1e-4: R >= 64 -> brute force
TALL_DECAYS = (0.05, 0.01, 0.004, 0.003125, 0.003, 1e-4)


@pytest.mark.parametrize("nz", [150, 64, 65])
def test_tall_random_box_equals_the_oracle(ops, O, nz):
    """nz = 150: three words per column; 64 | 65: the last one-word and the first two-word map.  ny = 80 > 64, so the column bits
    of a window straddle two column-map words.  Every mask and decay, the whole heat vector against the float64 brute force."""
    pos, masks = tall_box(nz, 20 + nz)
    assert tuple(np.ptp(pos, axis=0) + 1) == (12, 80, nz) and pos[:, 2].min() == -3
    plan = ops.HeatPlan(pos)
    for name, mask in masks.items():
        for decay in TALL_DECAYS:
            want = O.heatmap_from_mask(pos, mask, CS, decay)
            check_both(ops, plan, pos, mask, decay, want, (nz, name, decay))
    plan.close()


def test_sprawling_map_runs_without_the_lds_coarse_grid(ops, O):
    """A 2000 x 2000 x 20 bounding box has 251 x 251 coarse bytes, more than the 48 KiB the window kernels keep in LDS: the
    <false, ...> instantiations read the coarse grid from global memory.  ~4000 voxels, most of them around the ~40 targets so
    that their windows hold something, the rest anywhere."""
    rng = np.random.default_rng(31)
    corners = np.array([[0, 0, 0], [1999, 1999, 19], [0, 1999, 0], [1999, 0, 19]])
    centres = np.stack([rng.integers(0, 2000, 40), rng.integers(0, 2000, 40), rng.integers(0, 20, 40)], 1)
    centres[:4, :2] = [[0, 0], [1999, 1999], [63, 64], [1000, 7]]                    # windows clipped by the box, a column-word edge
    near = centres[rng.integers(0, 40, 3200)] + rng.integers(-5, 6, (3200, 3))
    far = np.stack([rng.integers(0, 2000, 800), rng.integers(0, 2000, 800), rng.integers(0, 20, 800)], 1)
    allp = np.concatenate([corners, centres, near, far])
    allp = allp[((allp >= 0) & (allp < [2000, 2000, 20])).all(axis=1)]
    allp = np.unique(allp, axis=0)
    pos = (allp[rng.permutation(len(allp))] + [-100, 50, -2]).astype(np.int32)
    assert tuple(np.ptp(pos, axis=0) + 1) == (2000, 2000, 20) and 3000 < len(pos) < 4100
    assert ((2000 >> 3) + 1) ** 2 > 48 * 1024
    mask = (pos[:, None, :] == (centres + [-100, 50, -2])[None]).all(axis=2).any(axis=1)
    assert 30 <= mask.sum() <= 40
    want = O.heatmap_from_mask(pos, mask, CS, 0.01)
    assert ((want > 0) & (want < 1)).sum() > 500                                     # the windows are not empty
    plan = ops.HeatPlan(pos)
    check_both(ops, plan, pos, mask, 0.01, want, ("sprawl",))
    plan.close()


@pytest.mark.parametrize("nt", [1023, 1024, 1025, 2049])
def test_brute_force_around_its_target_tile(ops, O, nt):
    """heat_brute_kernel stages the targets through LDS 1024 at a time.  Targets on a line (t, 0, 0), 300 other voxels at (t, 1, 0)
    over a run of 300 consecutive targets: the voxel above target t is at distance 1 from it and sqrt(2) from the next best, so a
    target lost at a tile edge shows wherever it sits in the compacted list; the runs together cover every target.  Then the same
    counts in a random box."""
    decay = 1e-4
    t = np.arange(nt)
    tpos = np.stack([t, 0 * t, 0 * t], 1)
    mask = np.arange(nt + 300) < nt
    for start in range(0, nt, 300):
        x = (start + np.arange(300)) % nt
        pos = np.concatenate([tpos, np.stack([x, 0 * x + 1, 0 * x], 1)]).astype(np.int32)
        want = O.heatmap_from_mask(pos, mask, CS, decay)
        assert (want[nt:] == np.float32(1.0 - 1.0 / CS * decay)).all()
        got = ops.heatmap_from_mask(pos, mask, CS, decay)
        assert np.array_equal(got, want), (nt, start, np.flatnonzero(got != want)[:8])
    rng = np.random.default_rng(nt)
    lin = rng.choice(40 * 40 * 40, nt + 300, replace=False)
    pos = np.stack([lin // 1600, (lin // 40) % 40, lin % 40], 1).astype(np.int32)
    mask = rng.permutation(nt + 300) < nt
    want = O.heatmap_from_mask(pos, mask, CS, decay)
    plan = ops.HeatPlan(pos)                                                         # (the plan hands such a decay to the same kernel)
    check_both(ops, plan, pos, mask, decay, want, (nt, "box"))
    plan.close()
