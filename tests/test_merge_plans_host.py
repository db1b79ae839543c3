"""The directory and general merge plans of avlmaps_amd/parallel.py on CPU tensors for several ranks of ONE process (threads,
tests/thread_world.py): the whole choreography of merge_raw_sharded against the brute-force merge of the raw lists, and the plan
itself (plan_merge_directory) against a brute-force oracle that shares nothing with the tensor code (tests/merge_worlds.py).
No GPU, no process group."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from avlmaps_amd import parallel  # noqa: E402
from merge_worlds import (OVERLAPPING, PLAN_WORLDS, assert_overlap_conditions, assert_plan_equal, cell_holders, oracle_plans,  # noqa: E402
                          plan_world, run_plan_world)
from test_parallel_gloo import _fake_replay, expected_merge, make_rank_raw  # noqa: E402
from thread_world import ThreadColl, run_ranks, thread_groups  # noqa: E402


# ---- the stand-in itself

@pytest.mark.parametrize("ws", [1, 2, 5])
def test_thread_collectives(ws):
    """all_reduce in place with MIN / MAX / SUM (own members and torch.distributed's), reduce, broadcast, send / recv into a slice"""
    import torch.distributed as dist

    def rank_fn(r, coll):
        R = ThreadColl._Dist.ReduceOp
        for ops_, want in (((R.MIN, dist.ReduceOp.MIN), 3), ((R.MAX, dist.ReduceOp.MAX), 3 + 2 * (ws - 1)), ((R.SUM, dist.ReduceOp.SUM), 3 * ws + ws * (ws - 1))):
            for op in ops_:
                t = torch.tensor([3 + 2 * r, -(3 + 2 * r)], dtype=torch.int64)
                back = coll.all_reduce(t, op)
                assert back is t and int(t[0]) == want, (op, t)
        with pytest.raises(ValueError):
            coll.all_reduce(torch.zeros(1), dist.ReduceOp.PRODUCT)
        # a float64 sum is folded in rank order on every rank: the same bits everywhere
        x = torch.tensor([0.1 * (r + 1), 1e16 if r == 0 else 1.0], dtype=torch.float64)
        coll.all_reduce(x, dist.ReduceOp.SUM)
        want = torch.tensor([0.1, 1e16], dtype=torch.float64)
        for k in range(1, ws):
            want = want + torch.tensor([0.1 * (k + 1), 1.0], dtype=torch.float64)
        assert torch.equal(x, want)
        y = torch.tensor([float(r + 1)], dtype=torch.float64)
        assert coll.reduce(y, ws - 1, dist.ReduceOp.SUM) is y
        assert float(y) == (ws * (ws + 1) / 2 if r == ws - 1 else r + 1)          # only the destination holds the sum
        z = torch.full((3,), r, dtype=torch.int32)
        assert coll.broadcast(z, ws // 2) is z and z.tolist() == [ws // 2] * 3
        # point to point: FIFO per ordered pair, send does not wait, recv fills the tensor it is given (a slice of a larger one)
        for d in range(ws):
            if d != r:
                coll.send(torch.tensor([[10 * r + d, 1]]), d)
                coll.send(torch.tensor([[10 * r + d, 2]]), d)
        buf = torch.zeros((2 * ws, 2), dtype=torch.int64)
        for s in range(ws):
            if s != r:
                coll.recv(buf[2 * s:2 * s + 1], s)
                coll.recv(buf[2 * s + 1:2 * s + 2], s)
        assert buf.tolist() == [[0, 0] if s == r else [10 * s + r, k] for s in range(ws) for k in (1, 2)]
        return True
    assert run_ranks(ws, rank_fn) == [True] * ws


def test_a_failing_rank_releases_a_rank_that_waits_in_recv():
    def rank_fn(r, coll):
        if r == 0:
            raise KeyError("rank 0 fails")
        coll.recv(torch.zeros(1), 0)
    with pytest.raises(KeyError):
        run_ranks(3, rank_fn)


def test_thread_groups_puts_everything_back(monkeypatch):
    import os
    monkeypatch.setenv("AVLMAPS_MERGE_PLAN", "gather")
    monkeypatch.delenv("AVLMAPS_MERGE_KERNELS", raising=False)
    saved = parallel._Coll, parallel._dist_on
    with pytest.raises(ZeroDivisionError):
        with thread_groups(AVLMAPS_MERGE_PLAN="general", AVLMAPS_MERGE_KERNELS=0):
            assert os.environ["AVLMAPS_MERGE_PLAN"] == "general" and os.environ["AVLMAPS_MERGE_KERNELS"] == "0"
            marker = object()
            assert parallel._Coll(marker) is marker and parallel._dist_on(marker) and not parallel._dist_on() and not parallel._dist_on(None)
            1 / 0
    assert (parallel._Coll, parallel._dist_on) == saved
    assert os.environ["AVLMAPS_MERGE_PLAN"] == "gather" and "AVLMAPS_MERGE_KERNELS" not in os.environ


# ---- merge_raw_sharded as threads: the assertions of test_parallel_gloo._sharded_worker

def sharded_world(ws, monotone):
    D = 12
    rng = np.random.default_rng(7)
    # contiguous frame shards see mostly disjoint voxels, a few shared ones (some by three and more ranks); one rank may hold nothing
    cellsets = [sorted(set(rng.integers(0, 400, 40 + 10 * (k % 3)).tolist())) for k in range(ws)]
    if ws >= 3:
        cellsets[2] = []
    lo = [1000 * k for k in range(ws)]
    if not monotone:
        lo[0], lo[1] = lo[1], lo[0]                # frames NOT sharded contiguously: the general plan must take over
    raws = [make_rank_raw(20 + k, D, cellsets[k], frame_lo=lo[k]) for k in range(ws)]
    return D, cellsets, raws


@pytest.mark.parametrize("monotone", [True, False], ids=["monotone", "swapped"])
@pytest.mark.parametrize("ws", [2, 3, 8, 16])
def test_row_sharded_merge_over_threads(ws, monotone):
    """parallel.merge_raw_sharded for ws ranks as threads: the directory plan with its point-to-point replay hops (rank-monotone
    keys), the general plan when the frame ranges of ranks 0 and 1 are swapped; merge_raw's dense reduce and gather_row_shards ride
    along.  Every block against the brute-force merge of the raw lists."""
    D, cellsets, raws = sharded_world(ws, monotone)
    cells, table = expected_merge(raws)
    M = len(cells)
    holders = {c: [k for k in range(ws) if c in cellsets[k]] for c in cells}

    def rank_fn(rank, coll):
        dense = parallel.merge_raw(raws[rank], dst=0, group=coll)
        sh = parallel.merge_raw_sharded(raws[rank], group=coll, replay_fn=_fake_replay(rank, raws[rank]["cell"]) if monotone else None, gs2=7)
        r0, r1 = sh["rows"]
        shard = dict(grid_feat=sh["grid_feat"], grid_pos=torch.arange(r0, r1, dtype=torch.int32)[:, None].repeat(1, 3),
                     weight=sh["w4"][:, 0].float().contiguous(), grid_rgb=torch.full((r1 - r0, 3), rank, dtype=torch.uint8))
        fullmap = parallel.gather_row_shards(shard, ws - 1, coll, rank, ws)
        return dense, sh, fullmap
    with thread_groups(AVLMAPS_MERGE_PLAN=None):
        outs = run_ranks(ws, rank_fn)
    for rank, (dense, sh, fullmap) in enumerate(outs):
        assert sh["plan"] == ("directory" if monotone else "general")
        assert sh["M"] == M and sh["rows"] == parallel.shard_rows(M, rank, ws)
        r0, r1 = sh["rows"]
        assert sh["cell"].tolist() == cells[r0:r1] and sh["grid_feat"].shape == (r1 - r0, D)
        part = {int(r): i for i, r in enumerate(sh["part_rows"].tolist())}
        for i in range(r0, r1):
            e = table[cells[i]]
            want = e["want"]
            np.testing.assert_allclose(sh["w4"][i - r0].numpy(), e["w4"], rtol=1e-15, atol=1e-15)
            assert int(sh["first_key"][i - r0]) == e["key"]
            if monotone and len(holders[cells[i]]) == 1:
                # a voxel of ONE rank: finished where it was accumulated, in float64, rounded once -- the single-process value
                assert (i - r0) not in part
                assert np.array_equal(sh["grid_feat"][i - r0].numpy(), (want / e["w4"][0]).astype(np.float32))
            else:
                np.testing.assert_allclose(sh["part_acc"][part[i - r0]].numpy(), want, rtol=1e-13, atol=1e-13)
                np.testing.assert_allclose(sh["grid_feat"][i - r0].numpy(), (want / e["w4"][0]).astype(np.float32), rtol=2e-7)
        assert (dense is not None) == (rank == 0)
        if monotone:
            # the key after which the reference's arrays change dtype: first-touch key of voxel id gs2 - 1
            assert sh["grow_key"] == (table[cells[6]]["key"] if M >= 7 else (1 << 64) - 1)
            # replay state: continued by every contributor of a voxel in rank order, delivered to the row's owner
            for i in range(r0, r1):
                c, s0 = cells[i], 0
                for k in holders[c]:
                    s0 = s0 * 31 + (k + 1) * 1000 + c
                assert sh["state"][i - r0].tolist() == [s0, len(holders[c]), 1 << 32], (i, holders[c])
            # traffic: 64 B of side record per row that leaves, + 4 B x D (single-rank voxels) or 8 B x D (shared)
            away = [c for c in cellsets[rank] if not (r0 <= cells.index(c) < r1)]
            single = sum(1 for c in away if len(holders[c]) == 1)
            assert sh["bytes_sent"] == len(away) * 64 + single * D * 4 + (len(away) - single) * D * 8
            assert sh["payload_bytes_fp64_form"] == len(away) * ((D + 4) * 8 + 8)
        # gather of finished row blocks to one rank
        if rank == ws - 1:
            assert fullmap["grid_pos"][:, 0].tolist() == list(range(M)) and fullmap["grid_feat"].shape == (M, D)
            assert fullmap["grid_rgb"][:, 0].tolist() == [min(i // max(1, (M + ws - 1) // ws), ws - 1) for i in range(M)]
        else:
            assert fullmap is None
    # the blocks, gathered, are the dense reduce of merge_raw
    gf = np.concatenate([o[1]["grid_feat"].numpy() for o in outs], axis=0)
    w4 = np.concatenate([o[1]["w4"].numpy() for o in outs], axis=0)
    dacc = outs[0][0]["acc"].numpy()
    assert outs[0][0]["cell"].tolist() == cells
    np.testing.assert_allclose(w4, dacc[:, D:], rtol=1e-15, atol=1e-15)
    np.testing.assert_allclose(gf, (dacc[:, :D] / dacc[:, D:D + 1]).astype(np.float32), rtol=2e-7, atol=0)
    if monotone:
        assert sum(o[1]["bytes_sent"] for o in outs) <= 1.3 * sum(len(c) for c in cellsets) * (D + 4) * 8
    # the dense voxel-id grid from the gathered cell blocks
    occ = parallel.occupied_ids_from_cells(torch.tensor(sum((o[1]["cell"].tolist() for o in outs), []), dtype=torch.int32), 1, 20, 20)
    assert occ.shape == (1, 20, 20) and int((occ >= 0).sum()) == M and int(occ.view(-1)[cells[3]]) == 3


def test_general_plan_forced_over_threads():
    """AVLMAPS_MERGE_PLAN=general with rank-monotone keys: the general plan's blocks equal the directory plan's"""
    ws = 3
    D, cellsets, raws = sharded_world(ws, True)
    with thread_groups(AVLMAPS_MERGE_PLAN="general"):
        gen = run_ranks(ws, lambda r, coll: parallel.merge_raw_sharded(raws[r], group=coll))
    with thread_groups(AVLMAPS_MERGE_PLAN=None):
        dire = run_ranks(ws, lambda r, coll: parallel.merge_raw_sharded(raws[r], group=coll))
    for g, d in zip(gen, dire):
        assert g["plan"] == "general" and d["plan"] == "directory" and g["rows"] == d["rows"] and g["M"] == d["M"]
        assert torch.equal(g["cell"], d["cell"]) and torch.equal(g["first_key"], d["first_key"]) and torch.equal(g["w4"], d["w4"])
        shared = torch.zeros(g["grid_feat"].shape[0], dtype=torch.bool)
        shared[d["part_rows"]] = True
        assert torch.equal(g["grid_feat"][shared], d["grid_feat"][shared])          # the same float64 sums in the same (rank) order
        np.testing.assert_allclose(g["grid_feat"].numpy(), d["grid_feat"].numpy(), rtol=2e-7, atol=0)


# ---- plan_merge_directory (tensor code) against the brute-force oracle

@pytest.mark.parametrize("name", list(PLAN_WORLDS))
def test_directory_plan_equals_the_brute_force_oracle(name):
    sizes = PLAN_WORLDS[name]
    cells, keys = plan_world(sizes, seed=len(name))
    if name in OVERLAPPING:
        assert_overlap_conditions(cells, sizes)
    M = len(cell_holders(cells))
    for grow_row in (M // 2, M - 1, M, None):                 # inside the map, its last row, just beyond it, not asked for
        got, aux = run_plan_world(cells, keys, grow_row)
        want = oracle_plans(cells, keys, grow_row, aux)
        assert want[0]["M"] == M and (want[0]["grow_key"] == (1 << 64) - 1) == (grow_row is None or grow_row >= M)
        for r in range(len(sizes)):
            assert_plan_equal(got[r], want[r], f"{name} rank {r} grow_row {grow_row}")


def test_directory_plan_reports_keys_that_are_not_rank_monotone():
    cells, keys = plan_world([777, 0, 777], seed=5, swap=(0, 2))
    got, aux = run_plan_world(cells, keys, 10)
    want = oracle_plans(cells, keys, 10, aux)
    for r in range(3):
        assert got[r]["monotone"] is False and want[r]["monotone"] is False
        assert_plan_equal(got[r], want[r], f"rank {r}")
