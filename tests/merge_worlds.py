"""What the multi-rank merge tests share (test_merge2_gpu, test_merge_plans_host, test_merge_plans_gpu): the scene whose frame shards
the ranks build, synthetic worlds of per-rank (cell, first-touch key) lists for the merge PLAN alone, and a brute-force oracle of
parallel.plan_merge_directory written with Python dicts and lists -- it shares nothing with the tensor code or the kernels."""
import numpy as np

U64_ALL_ONES = (1 << 64) - 1


def build_shards(ops, ws, D=64, nfr=24, seed=7, rate=5, cs=0.1, gs=400, replay=True, blocks=None):
    """one VoxelAccumulator over all nfr frames (120 x 160, features 58 x 77 x D) and one per rank over the rank's contiguous block of
    frames.  blocks: rank r fuses the frames of block blocks[r] instead of its own (frame indices kept: first-touch keys that are
    not ordered by rank)"""
    from oracle import avl_oracle as O
    from test_builder_gpu import synth_scene
    rng = np.random.default_rng(seed)
    H, W, Hf, Wf = 120, 160, 58, 77
    cam_h = 1.5
    calib = np.array([W / 2, 0, W / 2, 0, W / 2, H / 2, 0, 0, 1.0])
    depths, rgbs, feats, poses = synth_scene(rng, nfr, H, W, Hf, Wf, D)
    b2c, bt = O.setup_transforms([1, 0, 0, 0, -1, 0, 0, 0, -1], cam_h, [0, 0, -1], [-1, 0, 0], [0, 1, 0])
    Ts = O.pc_transforms(poses, bt, b2c)
    rs = np.random.RandomState(3)
    samples = [O.sample_indices(rs, H * W, rate) for _ in range(nfr)]
    fs = [np.ascontiguousarray(np.transpose(f, (1, 2, 0))) for f in feats]
    vh = int(cam_h / cs)
    from avlmaps_amd import parallel

    def build(lo, hi):
        acc = ops.VoxelAccumulator(gs, cs, vh, D, capacity=1 << 16)
        if replay:
            acc.enable_replay_log(max(1, (hi - lo) * len(samples[0])))
        for i in range(lo, hi):
            acc.integrate_frame(depths[i], calib, Ts[i], samples[i], fs[i], rgbs[i], frame_idx=i)
        return acc
    whole = build(0, nfr)
    shards = [build(*parallel.shard_frames(nfr, r if blocks is None else blocks[r], ws)) for r in range(ws)]
    return whole, shards, gs, vh


# ---------------------------------------------------------------------------------------------------------------------------------
# the merge plan alone: synthetic worlds and the oracle

def plan_world(sizes, seed, swap=None):
    """Per-rank voxel lists for a world of len(sizes) ranks, rank r holding sizes[r] voxels: (cells, keys) = lists of int32 / int64
    arrays in slot order.  Cells are distinct inside a rank and spread over all 31 bits.  A rank's cells are private ones plus
    shared ones, dealt so that (ranks with >= 700 voxels are "large")
        * cell 0 is held by EVERY rank that holds anything (two more such cells by every large rank),
        * cell 2^31 - 2 and four more by rank 0 and the last rank ONLY, if both are large (their neighbours are then not adjacent),
        * 60 cells by exactly two large ranks each, 40 by three.
    Keys are (frame << 32) | sample, unique inside a rank, rank r's frames in [100 r, 100 r + 50): rank-monotone -- unless
    swap = (a, b) exchanges the frame ranges of ranks a and b."""
    rng = np.random.default_rng(seed)
    ws = len(sizes)
    large = [r for r in range(ws) if sizes[r] >= 700]
    pool = np.unique(rng.integers(1, 2**31 - 2, 2 * (sum(sizes) + 200)))
    rng.shuffle(pool)
    pool = pool.tolist()
    held = [[] for _ in range(ws)]
    for r in range(ws):
        if sizes[r]:
            held[r].append(0)
    for _ in range(2):
        c = pool.pop()
        for r in large:
            held[r].append(c)
    if ws > 2 and 0 in large and ws - 1 in large:
        for c in [2**31 - 2] + [pool.pop() for _ in range(4)]:
            held[0].append(c)
            held[ws - 1].append(c)
    for k, count in ((2, 60), (3, 40)):
        if len(large) >= k:
            for _ in range(count):
                c = pool.pop()
                for r in rng.choice(large, k, replace=False).tolist():
                    held[r].append(c)
    cells, keys = [], []
    lo = [100 * r for r in range(ws)]
    if swap:
        a, b = swap
        lo[a], lo[b] = lo[b], lo[a]
    for r in range(ws):
        n = sizes[r]
        assert len(held[r]) <= max(n, 1), (r, n, len(held[r]))
        held[r] = held[r][:n] + [pool.pop() for _ in range(n - len(held[r][:n]))]
        c = np.array(held[r], np.int64)[rng.permutation(n)] if n else np.zeros(0, np.int64)
        cells.append(c.astype(np.int32))
        keys.append(((lo[r] + rng.integers(0, 50, n)).astype(np.int64) << 32) | rng.permutation(n).astype(np.int64))
    return cells, keys


def cell_holders(cells):
    """cell -> the sorted ranks that hold it"""
    holders = {}
    for r, cs in enumerate(cells):
        for c in (cs.tolist() if hasattr(cs, "tolist") else cs):
            holders.setdefault(int(c), []).append(r)
    assert all(len(set(h)) == len(h) for h in holders.values())          # a rank lists a cell once
    return {c: sorted(h) for c, h in holders.items()}


def oracle_plans(cells, keys, grow_row=None, aux=None):
    """What plan_merge_directory has to return on every rank, by brute force.  Per cell, the ranks that hold it, sorted: prev / next
    of a rank's voxel are its neighbours in that list, is_new marks the lowest holder.  The final rows are the NEW voxels ordered by
    (rank, first-touch key); a shared voxel has the row of its first holder.  counts / bases / M / n_prev / n_next / grow_key follow;
    dir_entries counts the (rank, cell) pairs whose cell hashes to the directory rank.  aux: per rank, the integers it passes."""
    ws = len(cells)
    cells = [[int(c) for c in cs] for cs in cells]
    keys = [[int(k) for k in ks] for ks in keys]
    aux_all = np.array([[int(a) for a in (aux[r] if aux else ())] for r in range(ws)], np.int64).reshape(ws, -1)
    last, monotone = -1, True
    for r in range(ws):
        if cells[r]:
            if min(keys[r]) <= last:
                monotone = False
            last = max(keys[r])
    if not monotone:
        return [dict(monotone=False, aux_all=aux_all) for _ in range(ws)]
    holders = cell_holders(cells)
    key_of = [dict(zip(cells[r], keys[r])) for r in range(ws)]
    new = [sorted((c for c in cells[r] if holders[c][0] == r), key=lambda c, r=r: key_of[r][c]) for r in range(ws)]
    counts = [len(x) for x in new]
    bases = [sum(counts[:r]) for r in range(ws)]
    M = sum(counts)
    row_of_cell, row_key = {}, []
    for r in range(ws):
        for j, c in enumerate(new[r]):
            row_of_cell[c] = bases[r] + j
            row_key.append(key_of[r][c])
    grow_key = (row_key[grow_row] & U64_ALL_ONES) if (grow_row is not None and 0 <= grow_row < M) else U64_ALL_ONES
    entries = [0] * ws
    for r in range(ws):
        for c in cells[r]:
            entries[(((c * 2654435761) & 0xFFFFFFFF) >> 12) % ws] += 1        # the directory rank of a cell (a multiplicative hash)
    plans = []
    for r in range(ws):
        prev, nxt = [], []
        for c in cells[r]:
            h = holders[c]
            j = h.index(r)
            prev.append(h[j - 1] if j > 0 else -1)
            nxt.append(h[j + 1] if j + 1 < len(h) else -1)
        plans.append(dict(monotone=True, aux_all=aux_all, M=M, bases=bases, counts=counts, grow_key=grow_key, dir_entries=entries[r],
                          row_of_slot=[row_of_cell[c] for c in cells[r]], is_new=[p < 0 for p in prev], prev=prev, next=nxt,
                          n_prev=[prev.count(q) for q in range(ws)], n_next=[nxt.count(q) for q in range(ws)]))
    return plans


def plan_fields(plan):
    """a ShardPlan as plain Python values (lists, ints, one NumPy array), whatever device its tensors live on"""
    out = dict(monotone=bool(plan.monotone), aux_all=np.asarray(plan.aux_all).astype(np.int64))
    if not plan.monotone:
        return out
    for f in ("row_of_slot", "is_new", "prev", "next"):
        out[f] = getattr(plan, f).cpu().tolist()
    for f in ("bases", "counts", "n_prev", "n_next"):
        out[f] = [int(v) for v in getattr(plan, f)]
    out.update(M=int(plan.M), grow_key=int(plan.grow_key), dir_entries=int(plan.dir_entries))
    return out


def assert_plan_equal(got, want, what=""):
    """got, want: plan_fields / oracle_plans dicts of one rank; every field equal"""
    assert got["monotone"] == want["monotone"], (what, "monotone")
    assert got["aux_all"].shape == want["aux_all"].shape and np.array_equal(got["aux_all"], want["aux_all"]), (what, "aux_all")
    if not want["monotone"]:
        return
    for f in ("M", "bases", "counts", "grow_key", "dir_entries", "n_prev", "n_next", "is_new", "prev", "next", "row_of_slot"):
        if got[f] != want[f]:
            where = next((i for i, (a, b) in enumerate(zip(got[f], want[f])) if a != b), None) if isinstance(want[f], list) else None
            raise AssertionError(f"{what}: ShardPlan.{f} differs from the oracle"
                                 + (f" at index {where}: {got[f][where]} != {want[f][where]}" if where is not None
                                    else f": {got[f]} != {want[f]}"))


PLAN_WORLDS = {                                  # per-rank voxel counts; 20 003 >= 8192: the size at which the GPU sorts change kernels
    "ws2": [20003, 777],
    "ws2-rank0-empty": [0, 777],
    "ws3-one-voxel-rank": [20003, 1, 777],
    "ws3-empty-middle": [777, 0, 20003],
    "ws8": [777, 20003, 0, 1, 777, 777, 777, 20003],
    "ws16": [777, 1, 40, 777, 3, 777, 60, 0, 777, 777, 5, 777, 777, 1, 777, 777],
}
OVERLAPPING = ("ws2", "ws3-one-voxel-rank", "ws8", "ws16")


def assert_overlap_conditions(cells, sizes):
    """what a world with overlaps must contain, read from the inputs: a cell held by every rank that holds anything (at most one
    rank holds nothing), a cell held by rank 0 and the last rank only, at least 50 cells held by exactly two ranks"""
    ws = len(sizes)
    holders = cell_holders(cells)
    nonempty = [r for r in range(ws) if sizes[r]]
    assert len(nonempty) >= ws - 1
    assert any(h == nonempty for h in holders.values())
    assert any(h == [0, ws - 1] for h in holders.values())
    assert sum(1 for h in holders.values() if len(h) == 2) >= 50
    if ws >= 3:
        assert any(len(h) >= 3 for h in holders.values())     # a middle contributor: prev >= 0 and next >= 0
    return holders


def run_plan_world(cells, keys, grow_row, device="cpu", **env):
    """plan_merge_directory for every rank of the world as threads (tensors on `device`; env: thread_groups' variables) -> (the ranks'
    plans as plan_fields dicts, the aux integers every rank passed)"""
    import torch
    from avlmaps_amd import parallel
    from thread_world import run_ranks, thread_groups
    ws = len(cells)
    aux = [(r % 2, 7 + r) for r in range(ws)]
    tc = [torch.from_numpy(c).to(device) for c in cells]
    tk = [torch.from_numpy(k).to(device) for k in keys]
    with thread_groups(**env):
        plans = run_ranks(ws, lambda r, coll: plan_fields(parallel.plan_merge_directory(tc[r], tk[r], group=coll, grow_row=grow_row, aux=aux[r])))
    return plans, aux
