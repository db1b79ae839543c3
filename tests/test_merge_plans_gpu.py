"""The directory and general merge plans of avlmaps_amd/parallel.py on the GPU with SEVERAL ranks: every rank a thread of this process
with its own device tensors or VoxelAccumulator, the collectives an in-process stand-in with parallel._Coll's interface
(tests/thread_world.py).  With one rank every cell has one contributor; only a world of two or more runs the neighbour logic of
csrc/avl_merge.hip, the point-to-point replay hops, the shared-row lists and the general plan's chain.

(a) the plan kernels against the brute-force oracle of tests/merge_worlds.py and against the tensor code;
(b) the directory plan through parallel.merge_accumulator_sharded against the single-process map and the CPU twin;
(c) the general plan, forced and as the fall-back for first-touch keys that are not ordered by rank."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))

from merge_worlds import (OVERLAPPING, PLAN_WORLDS, assert_overlap_conditions, assert_plan_equal, build_shards, cell_holders,  # noqa: E402
                          oracle_plans, plan_world, run_plan_world)
from thread_world import run_ranks, thread_groups  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


# ---- (a) the plan kernels with real neighbours

GPU_PLAN_WORLDS = [n for n in PLAN_WORLDS if n != "ws16"]          # ws in {2, 3, 8}, sizes in {0, 1, 777, 20 003} mixed


def plans_on_device(cells, keys, grow_row, kernels, monkeypatch):
    """the world's plans on device tensors with AVLMAPS_MERGE_KERNELS = kernels; also checks that the setting chose the path"""
    from avlmaps_amd import parallel
    took, orig = [], parallel._merge_hip

    def spy(t):
        lib = orig(t)
        took.append(lib is not None)
        return lib
    monkeypatch.setattr(parallel, "_merge_hip", spy)
    got, aux = run_plan_world(cells, keys, grow_row, device="cuda", AVLMAPS_MERGE_KERNELS=kernels)
    monkeypatch.setattr(parallel, "_merge_hip", orig)
    assert len(took) == len(cells) and all(t == (kernels == "1") for t in took), (kernels, took)
    return got, aux


@pytest.mark.parametrize("name", GPU_PLAN_WORLDS)
def test_plan_kernels_with_neighbours_equal_the_oracle_and_the_tensor_code(ops, monkeypatch, name):
    """plan_merge_directory for 2, 3 and 8 ranks: every ShardPlan field on every rank equals the brute-force oracle, with the kernels
    of csrc/avl_merge.hip and with the tensor code, and the two equal each other.  20 003 voxels on a rank take the library's radix
    sort in _argsort_bits, 777 torch's.  A world named in OVERLAPPING holds a cell of every (non-empty) rank, a cell of the first and
    the last rank only and >= 50 cells of exactly two ranks: asserted from the inputs.  (ws = 2 cannot have both an empty rank and
    a shared cell, and a rank with ONE voxel can only hold the cell that everybody holds: hence several worlds per rank count.)"""
    sizes = PLAN_WORLDS[name]
    cells, keys = plan_world(sizes, seed=len(name))
    if name in OVERLAPPING:
        assert_overlap_conditions(cells, sizes)
    M = len(cell_holders(cells))
    for grow_row in (M // 2,) + ((M,) if name == "ws3-one-voxel-rank" else ()):          # inside the map; once beyond its last row
        runs = {}
        for kernels in ("1", "0"):
            runs[kernels], aux = plans_on_device(cells, keys, grow_row, kernels, monkeypatch)
        want = oracle_plans(cells, keys, grow_row, aux)
        assert want[0]["M"] == M and (want[0]["grow_key"] == (1 << 64) - 1) == (grow_row >= M)
        for r in range(len(sizes)):
            for kernels in ("1", "0"):
                assert_plan_equal(runs[kernels][r], want[r], f"{name} rank {r} grow_row {grow_row} AVLMAPS_MERGE_KERNELS={kernels}")
            assert_plan_equal(runs["1"][r], runs["0"][r], f"{name} rank {r} grow_row {grow_row} kernels against tensor code")


def test_plan_kernels_report_keys_that_are_not_rank_monotone(ops, monkeypatch):
    cells, keys = plan_world([777, 0, 777], seed=5, swap=(0, 2))
    for kernels in ("1", "0"):
        got, aux = plans_on_device(cells, keys, 10, kernels, monkeypatch)
        want = oracle_plans(cells, keys, 10, aux)
        for r in range(3):
            assert got[r]["monotone"] is False and want[r]["monotone"] is False
            assert_plan_equal(got[r], want[r], f"rank {r} AVLMAPS_MERGE_KERNELS={kernels}")


# ---- (b), (c) the plans through the product entry point

GS = 100                  # the scene's 12 622 voxels outgrow gs * gs = 10 000: the growth key of the colour replay lies INSIDE the map
_worlds = {}


class World:
    """the ranks' accumulators of one scene, the single-process map and the raw exports -- built once, shared, never changed"""

    def __init__(self, ops, ws, D, nfr, blocks):
        import torch
        self.ws, self.D = ws, D
        self.whole, self.shards, self.gs, self.vh = build_shards(ops, ws, D=D, nfr=nfr, gs=GS, blocks=blocks)
        self.want = self.whole.finalize()
        self.M = len(self.want["grid_pos"])
        self.raws = []
        for acc in self.shards:
            raw = acc.export_raw()
            raw["first_key"] = raw["first_key"].astype(np.int64)
            self.raws.append({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in raw.items()})
        self.holders = cell_holders([r["cell"] for r in self.raws])


@pytest.fixture(scope="module", autouse=True)
def release_worlds():
    yield
    for w in _worlds.values():
        for acc in [w.whole] + w.shards:
            acc.close()
    _worlds.clear()


def world(ops, ws, D, nfr=24, blocks=None):
    key = (ws, D, nfr, blocks)
    if key not in _worlds:
        _worlds[key] = World(ops, ws, D, nfr, blocks)
    return _worlds[key]


def merge_on_device(w, gather_to, exact_rgb=True, **env):
    """parallel.merge_accumulator_sharded on every rank's accumulator -> per rank (the result as host arrays, its timings)"""
    import torch
    from avlmaps_amd import parallel

    def host(d):
        return {k: (v.cpu().numpy() if torch.is_tensor(v) else host(v) if isinstance(v, dict) else v) for k, v in d.items()}

    def rank_fn(r, coll):
        tim = {}
        out = parallel.merge_accumulator_sharded(w.shards[r], group=coll, exact_rgb=exact_rgb, timings=tim, gather_to=gather_to)
        torch.cuda.synchronize()
        return host(out), tim
    with thread_groups(AVLMAPS_MERGE_KERNELS=None, **env):
        return run_ranks(w.ws, rank_fn)


def merge_twin(w, **env):
    """the CPU twin: parallel.merge_raw_sharded on the ranks' exported accumulators, a second world of threads"""
    from avlmaps_amd import parallel
    with thread_groups(**env):
        return run_ranks(w.ws, lambda r, coll: parallel.merge_raw_sharded(w.raws[r], group=coll))


def check_against_single_process_and_twin(w, outs, twin, gather_to, plan_name, colours=True):
    """what (b) and (c) assert on the blocks in rank order and on the gathered map of rank gather_to"""
    from avlmaps_amd import parallel
    import torch
    ws, M, want = w.ws, w.M, w.want
    for r, (out, tim) in enumerate(outs):
        assert tim["plan"].startswith(plan_name), (r, tim["plan"])
        assert out["M"] == M and tuple(out["rows"]) == parallel.shard_rows(M, r, ws), (r, out["rows"])
        assert ("full" in out) == (r == gather_to)
        assert twin[r]["plan"] == plan_name and twin[r]["rows"] == parallel.shard_rows(M, r, ws)
    blocks = {k: np.concatenate([o[0][k] for o in outs]) for k in ("grid_feat", "grid_pos", "weight", "grid_rgb", "cell")}
    blocks["occupied_ids"] = parallel.occupied_ids_from_cells(torch.from_numpy(blocks.pop("cell")), w.gs, w.gs, w.vh).numpy()
    twin_feat = np.concatenate([t["grid_feat"].numpy() for t in twin])
    for what, got in (("blocks", blocks), ("full", outs[gather_to][0]["full"])):
        for k in ("grid_pos", "occupied_ids") + (("weight", "grid_rgb") if colours else ()):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)          # bit for bit
        # against the single-process map: a voxel of one rank is bit-identical, a shared one differs by the float64 summation order
        np.testing.assert_allclose(got["grid_feat"], want["grid_feat"], rtol=1e-6, atol=1e-6)
        assert np.mean(got["grid_feat"] == want["grid_feat"]) > 0.99, what
        # against the twin: the same float64 expression, summed peer by peer in rank order, rounded once
        assert np.array_equal(got["grid_feat"], twin_feat), (what, float(np.abs(got["grid_feat"] - twin_feat).max()))
    return blocks


def assert_scene_conditions(w):
    counts = [len(h) for h in w.holders.values()]
    assert sum(1 for c in counts if c >= 2) > 50                   # voxels several ranks touched
    assert sum(1 for c in counts if c == 1) > 0                    # ... and voxels of one rank alone (they travel as finished rows)
    assert w.M > GS * GS - 1                                       # the growth key is a key of the map
    if w.ws == 8:
        assert any(c >= 3 for c in counts)                         # a middle contributor of three: prev >= 0 and next >= 0


@pytest.mark.parametrize("ws,D,nfr,gather_to", [(2, 64, 24, 0), (3, 30, 24, 0), (8, 64, 24, 0), (8, 5, 24, 0), (3, 64, 2, 0), (8, 64, 24, 7)],
                         ids=["ws2-D64", "ws3-D30", "ws8-D64", "ws8-D5", "ws3-D64-last-rank-empty", "ws8-D64-gather-to-last"])
def test_directory_plan_through_the_product(ops, ws, D, nfr, gather_to):
    """AVLMAPS_MERGE_PLAN=directory, merge_accumulator_sharded for ws ranks: ids, weights and colours (replay log on, growth key
    inside the map) bit for bit the single-process map, features within its summation-order tolerance and bit for bit the CPU twin.
    D = 30 and 5 take index_copy_ instead of avl_scatter_rows; with two frames for three ranks the last rank holds nothing."""
    w = world(ops, ws, D, nfr)
    if nfr == 24:
        assert_scene_conditions(w)
    else:
        assert [len(r["cell"]) > 0 for r in w.raws] == [True, True, False]
        assert sum(1 for h in w.holders.values() if len(h) == 2) > 50
    outs = merge_on_device(w, gather_to, AVLMAPS_MERGE_PLAN="directory")
    twin = merge_twin(w, AVLMAPS_MERGE_PLAN="directory")
    check_against_single_process_and_twin(w, outs, twin, gather_to, "directory")
    for r, (out, tim) in enumerate(outs):
        assert tim["directory_entries"] > 0 and tim["exact_rgb"] and tim["world_size"] == ws, (r, tim["directory_entries"])
        assert tim["local_voxels"] == len(w.raws[r]["cell"]) and tim["merged_voxels"] == w.M
        assert tim["single_rank_voxels"] == sum(1 for c in w.raws[r]["cell"].tolist() if len(w.holders[c]) == 1)
        assert tim["shared_voxels_local"] == tim["local_voxels"] - tim["single_rank_voxels"]
    assert sum(tim["single_rank_voxels"] for _, tim in outs) > 0


@pytest.mark.parametrize("D", [64, 30])
@pytest.mark.parametrize("ws", [2, 3, 8])
def test_general_plan_forced_through_the_product(ops, ws, D):
    """AVLMAPS_MERGE_PLAN=general on contiguous frame shards (the dense replay chain then runs in frame order): everything the
    directory plan's test asserts, weights and colours bit for bit included -- avl_builder_scatter_merge with non-owner ranks,
    avl_rows_add_f64 peer by peer, avl_finalize_merged at row0 != 0, avl_replay_state_apply on a block"""
    w = world(ops, ws, D)
    assert_scene_conditions(w)
    outs = merge_on_device(w, 0, AVLMAPS_MERGE_PLAN="general")
    twin = merge_twin(w, AVLMAPS_MERGE_PLAN="general")
    check_against_single_process_and_twin(w, outs, twin, 0, "general")
    assert all(tim["exact_rgb"] and tim["world_size"] == ws and tim["chain_bytes_sent"] == 24 * w.M for _, tim in outs)
    assert sum(out["rows"][0] != 0 and out["rows"][1] > out["rows"][0] for out, _ in outs) == ws - 1


@pytest.mark.parametrize("ws,D", [(3, 64), (8, 30)])
def test_general_plan_is_the_fallback_when_keys_are_not_ordered_by_rank(ops, ws, D):
    """default environment, ranks 0 and 1 hold each other's frame blocks (frame indices kept): the gather plan declines and the
    general plan runs.  Ids equal the single-process map, features are bit for bit the twin.  Without the log, weight and colour
    are finalize_kernel's arithmetic (csrc/avl_finalize.hip) on the twin's summed [alpha, alpha rgb], restated in NumPy float64.
    With the log the chain runs in RANK order, which is not frame order here by design: colours are not compared with the
    single-process map."""
    blocks = (1, 0) + tuple(range(2, ws))
    w = world(ops, ws, D, blocks=blocks)
    assert_scene_conditions(w)
    assert int(w.raws[0]["first_key"].min()) > int(w.raws[1]["first_key"].max())          # not ordered by rank
    twin = merge_twin(w, AVLMAPS_MERGE_PLAN=None)
    w4 = np.concatenate([t["w4"].numpy() for t in twin])
    for exact_rgb in (False, True):
        outs = merge_on_device(w, ws - 1, exact_rgb=exact_rgb, AVLMAPS_MERGE_PLAN=None)
        got = check_against_single_process_and_twin(w, outs, twin, ws - 1, "general", colours=False)
        assert all(tim["exact_rgb"] == exact_rgb for _, tim in outs)
        if not exact_rgb:
            for g in (got, outs[ws - 1][0]["full"]):
                assert g["weight"].dtype == np.float32 and np.array_equal(g["weight"], w4[:, 0].astype(np.float32))
                assert g["grid_rgb"].dtype == np.uint8
                assert np.array_equal(g["grid_rgb"], np.clip(w4[:, 1:4] / w4[:, :1] + 1e-9, 0.0, 255.0).astype(np.uint8))
