"""GPU box: time the ground-truth label map's kernels (csrc/avl_gtmap.hip) against a vectorised NumPy restatement on the same box.
Prints one JSON object (and writes it to --out).

    probe_gtmap.py [--reps 30] [--warmup 3] [--host-reps 3] [--host-frames 16] [--out profiles/gtmap_probe.txt]

720 x 1080 float32 depth frames and int32 semantic frames (object ids in patches of 24 x 24 pixels, 60 objects, 40 classes) of a
synthetic room (walls 2 - 5.5 m away, a band of pixels beyond max_depth), gs = 1000, cs = 0.05, vh = 30, stride 1 (777 600 votes
attempted per frame), poses turning on the spot, a voxel index of 2 M voxels that holds 70 % of the cells the frames reach, batches
of 1, 16 and 64 resident frames:
  vote_resident    ops.gt_vote with depth, semantic frames, table, index, votes and statistics already on the device: the kernel
                   launches alone (the error flag is shared and not read inside the time)
  vote_upload      the same with the batch's depth and semantic frames uploaded from host arrays first (what GTMap.create_map pays per
                   batch)
  numpy_vote       the host path: back-projection, pose, cell, class and voxel of all pixels of a frame at once, then np.add.at, frame by
                   frame; the first --host-frames frames only (it takes a third of a second per frame), --host-reps times for one frame
  labels_device    ops.gt_labels over the (2 M, 40) votes of the 64-frame batch, resident     / labels_numpy: argmax, max and sum of the rows
  confusion_device ops.label_confusion over 2 M pairs at 40 x 41, resident                    / confusion_numpy: np.bincount of gt * 41 + pred
  pool_device      ops.pool_labels_2d over the whole 1000 x 1000 grid, resident               / pool_numpy: one np.where per height, top down
`same` says the device result equals NumPy's; for the votes `entries_differing` is reported rather than assumed zero, because the
NumPy path multiplies and adds where the kernel has K1's fma chain: a last-bit difference in a point can move a vote to the next cell.
Every device figure is the median of `reps` synchronised calls after `warmup` (host clock), minimum and maximum next to it."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from avlmaps_amd import _lib, ops  # noqa: E402
from avlmaps_amd.device import DeviceArray  # noqa: E402
from probe_explored import frames  # noqa: E402
from probe_morph2d import stats  # noqa: E402

H, W, GS, CS, VH, C, N_OBJ, N_VOXELS = 720, 1080, 1000, 0.05, 30, 40, 60, 2_000_000
PARAMS = dict(stride=1, min_depth=0.1, max_depth=6.0)
K = np.array([[540.0, 0, 540.0], [0, 540.0, 360.0], [0, 0, 1.0]])


def semantic_frames(n, seed=1):
    rng = np.random.default_rng(seed)
    patches = rng.integers(-1, N_OBJ + 1, (n, H // 24, W // 24)).astype(np.int32)        # -1 and N_OBJ: pixels without an object of the table
    return np.ascontiguousarray(np.repeat(np.repeat(patches, 24, axis=1), 24, axis=2))


def frame_cells(depth, T):
    """(flat index into (GS, GS, VH), valid) of every pixel of a frame: plain products and sums where the kernel has fma"""
    Kinv = np.linalg.inv(K)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dirs = Kinv @ np.stack([u.ravel() + 0.5, v.ravel() + 0.5, np.ones(u.size)])
    p = dirs * depth.reshape(-1).astype(np.float64)
    ok = (p[2] > PARAMS["min_depth"]) & (p[2] < PARAMS["max_depth"])
    with np.errstate(all="ignore"):
        g = T[:3, :3] @ p + T[:3, 3][:, None]
        g = np.where(ok, g, 0.0)
        row = (GS / 2 - np.trunc(g[0] / CS)).astype(np.int64)
        col = (GS / 2 - np.trunc(g[1] / CS)).astype(np.int64)
        h = np.trunc(g[2] / CS).astype(np.int64)
    ok &= (row >= 0) & (row < GS) & (col >= 0) & (col < GS) & (h >= 0) & (h < VH)
    return np.where(ok, (row * GS + col) * VH + h, 0), ok


def numpy_vote(votes, counts, depth, semantic, T, table, occupied_flat):
    cell, ok = frame_cells(depth, T)
    counts[0] += int((~ok).sum())
    o = semantic.reshape(-1)
    has = ok & (o >= 0) & (o < len(table))
    c = np.where(has, table[np.clip(o, 0, len(table) - 1)], -1)
    has &= (c >= 0) & (c < C)
    counts[1] += int((ok & ~has).sum())
    r = np.where(has, occupied_flat[cell], -1)
    cast = has & (r >= 0)
    counts[2] += int((has & ~cast).sum())
    counts[3] += int(cast.sum())
    np.add.at(votes, (r[cast], c[cast]), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    depth, Ts = frames(64)
    Ts[:, 2, 3] = 0.75                                                           # a camera inside the map's 1.5 m of height
    semantic = semantic_frames(64)
    rng = np.random.default_rng(2)
    table = rng.integers(0, C, N_OBJ).astype(np.int32)
    table[::13] = -1
    # the index: 70 % of the cells the first 16 frames reach (every 7th pixel), filled up to N_VOXELS with cells drawn at random
    reached = np.unique(np.concatenate([(lambda cell, ok: cell[ok][::7])(*frame_cells(depth[f], Ts[f])) for f in range(16)]))
    reached = reached[rng.random(reached.size) < 0.7][:N_VOXELS]
    others = np.setdiff1d(rng.choice(GS * GS * VH, N_VOXELS + reached.size, replace=False), reached)[:N_VOXELS - reached.size]
    cells = rng.permutation(np.concatenate([reached, others]))
    occupied = np.full(GS * GS * VH, -1, np.int32)
    occupied[cells] = np.arange(cells.size, dtype=np.int32)
    N = int(cells.size)
    res = {"frame": [H, W], "gs": GS, "cs": CS, "vh": VH, "classes": C, "voxels": N, "votes_attempted_per_frame": H * W,
           "library": os.environ.get("AVLMAPS_HIP_LIB") or "stock", "method": "host clock around synchronised calls, median of reps",
           "cases": {}}
    docc, dtable = DeviceArray.from_numpy(occupied.reshape(GS, GS, VH)), DeviceArray.from_numpy(table)
    dvotes, dstats, flag = DeviceArray((N, C), np.uint32), DeviceArray((4,), np.uint64), DeviceArray((1,), np.int32).zero_()
    want_votes, want_counts, host_ms = np.zeros((N, C), np.uint32), np.zeros(4, np.int64), []
    for f in range(min(a.host_frames, 64)):
        reps = a.host_reps if f == 0 else 1
        t0 = time.perf_counter()
        for k in range(reps):
            if k:
                want_votes[:], want_counts[:] = 0, 0
            numpy_vote(want_votes, want_counts, depth[f], semantic[f], Ts[f], table, occupied)
        host_ms.append((time.perf_counter() - t0) * 1e3 / reps)
        if f + 1 in (1, 16, 64):
            res["cases"][f"frames_{f + 1}"] = {"numpy_vote": {"total_ms": float(np.sum(host_ms)), "frames": f + 1},
                                               "_want": (want_votes.copy(), want_counts.copy())}
    for F in (1, 16, 64):
        d, s, T = depth[:F], semantic[:F], Ts[:F]
        ddepth, dsem = DeviceArray.from_numpy(d), DeviceArray.from_numpy(s)
        kw = dict(obj2cls=dtable, stats=dstats, err_flag=flag, device=True, **PARAMS)

        def vote_resident():
            ops.gt_vote(dvotes, ddepth, dsem, K, T, docc, N, C, CS, **kw)

        def vote_upload():
            ops.gt_vote(dvotes, DeviceArray.from_numpy(d), DeviceArray.from_numpy(s), K, T, docc, N, C, CS, **kw)
        dvotes.zero_()
        dstats.zero_()
        vote_resident()
        got_votes, got_counts = dvotes.numpy(), dstats.numpy()
        case = res["cases"].setdefault(f"frames_{F}", {})
        case.update(votes_cast=int(got_counts[3]), counts=[int(x) for x in got_counts], voxels_voted=int((got_votes.sum(axis=1) > 0).sum()))
        if "_want" in case:
            wv, wc = case.pop("_want")
            case.update(entries_differing=int((got_votes != wv).sum()), counts_numpy=[int(x) for x in wc],
                        same=bool(np.array_equal(got_votes, wv) and np.array_equal(got_counts.astype(np.int64), wc)))
        case["vote_resident"] = stats(lib, vote_resident, a.reps, a.warmup)
        case["vote_upload"] = stats(lib, vote_upload, a.reps, a.warmup)
        ops.check_label_flag(flag, "probe_gtmap")
        if F == 64:
            dvotes.zero_()
            vote_resident()
            votes = dvotes.numpy()

            def labels_numpy():
                label = np.argmax(votes, axis=1).astype(np.int32)
                label[votes.max(axis=1) == 0] = -1
                return label, votes.sum(axis=1, dtype=np.uint32)
            dlabel, dsupport = ops.gt_labels(dvotes, device=True)
            label, support = labels_numpy()
            res["cases"]["labels_2M_x_40"] = {
                "labelled": int((label >= 0).sum()), "same": bool(np.array_equal(dlabel.numpy(), label) and np.array_equal(dsupport.numpy(), support)),
                "labels_device": stats(lib, lambda: ops.gt_labels(dvotes, device=True), a.reps, a.warmup),
                "labels_numpy": stats(lib, labels_numpy, a.host_reps, 0)}
            gt = rng.integers(-1, C, N).astype(np.int32)
            pred = rng.integers(0, C + 1, N).astype(np.int32)
            dgt, dpred = DeviceArray.from_numpy(gt), DeviceArray.from_numpy(pred)
            dconf, dskip = DeviceArray((C, C + 1), np.uint64).zero_(), DeviceArray((2,), np.uint64).zero_()

            def confusion_numpy():
                keep = gt >= 0
                return np.bincount(gt[keep].astype(np.int64) * (C + 1) + pred[keep], minlength=C * (C + 1)).reshape(C, C + 1)
            conf, _ = ops.label_confusion(dgt, dpred, C, C + 1)
            res["cases"]["confusion_2M_40x41"] = {
                "same": bool(np.array_equal(conf, confusion_numpy())),
                "confusion_device": stats(lib, lambda: ops.label_confusion(dgt, dpred, C, C + 1, conf=dconf, skipped=dskip, err_flag=flag, device=True),
                                          a.reps, a.warmup),
                "confusion_numpy": stats(lib, confusion_numpy, a.host_reps, 0)}
            occ3 = occupied.reshape(GS, GS, VH)

            def pool_numpy():
                out = np.full((GS, GS), -1, np.int32)
                for h in range(VH):                                              # bottom up: a higher labelled voxel overwrites
                    ids = occ3[:, :, h]
                    lab = np.where(ids >= 0, label[np.maximum(ids, 0)], -1)
                    out = np.where(lab >= 0, lab, out)
                return out
            pooled = ops.pool_labels_2d(dlabel, docc)
            res["cases"]["pool_1000x1000"] = {
                "cells_labelled": int((pooled >= 0).sum()), "same": bool(np.array_equal(pooled, pool_numpy())),
                "pool_device": stats(lib, lambda: ops.pool_labels_2d(dlabel, docc, err_flag=flag, device=True), a.reps, a.warmup),
                "pool_numpy": stats(lib, pool_numpy, a.host_reps, 0)}
    for case in res["cases"].values():
        case.pop("_want", None)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
