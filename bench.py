#!/usr/bin/env python3
"""Benchmark of the AVLMaps hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload index|build] [--dump-outputs DIR]

Default workload = BASELINE.json configs[1]: landmark indexing of a 2M-voxel x 512-D map with 64 text
queries on one GPU (voxel rows shard across GPUs for N > 1, no data-path collective -> weak scaling).
One step = one pass of the index hot path: scores = feat @ queries.T fused with the row argmax
(VLMap.index_map, vlmap.py:104-125); the feature map is resident in HBM when the timed region starts.
`--workload build` times map creation instead (configs[2]/[3]): one step = fusing one 720x1080 RGB-D
frame (7 776 sampled pixels, 512-D channels-last features) into the voxel map.  STRONG scaling: the K frames
of one sequence shard across the GPUs, and the merge (one sparse RCCL sum-reduce + chained colour replay) and
the finalisation on rank 0 are INSIDE the timed region.  Feature extraction (LSeg) is not included.

Prints ONE JSON line on rank 0; `ms_per_step` is the wall time of one timed step.  --dump-outputs DIR writes what the
timed path computed in its last step as .npy files (see --help), so that two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)


def event_timer(lib):
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.avl_event_create(C.byref(e0))
    lib.avl_event_create(C.byref(e1))

    def elapsed_ms(fn, stream=None):
        lib.avl_event_record(e0, stream)
        fn()
        lib.avl_event_record(e1, stream)
        lib.avl_event_sync(e1)
        ms = C.c_float()
        lib.avl_event_elapsed_ms(e0, e1, C.byref(ms))
        return ms.value

    return elapsed_ms


def sustained_ms(lib, fn, launches=100, warm=60, stream=None):
    """mean duration of `launches` back-to-back calls after `warm` untimed ones (one event pair): the rate at the package's
    settled power operating point - the first ~30 launches of an MFMA-heavy kernel after an idle gap run 10-25 % slower
    while the power controller converges (profiles/HISTORY.md 4.1, power-management transient)"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.avl_event_create(C.byref(e0))
    lib.avl_event_create(C.byref(e1))
    for _ in range(warm):
        fn()
    lib.avl_event_record(e0, stream)
    for _ in range(launches):
        fn()
    lib.avl_event_record(e1, stream)
    lib.avl_event_sync(e1)
    ms = C.c_float()
    lib.avl_event_elapsed_ms(e0, e1, C.byref(ms))
    lib.avl_event_destroy(e0)
    lib.avl_event_destroy(e1)
    return ms.value / launches


def barrier_sync(torch, dist, ws):
    torch.cuda.synchronize()
    if ws > 1:
        dist.barrier()
    torch.cuda.synchronize()


def max_over_ranks(torch, dist, ws, x):
    if ws == 1:
        return x
    t = torch.tensor([x], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(torch, dist, ws, x):
    if ws == 1:
        return x
    t = torch.tensor([x], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


# ---------------------------------------------------------------------------------------- index workload
def make_index_inputs(torch, N, D, Q, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    feat = torch.randn((N, D), device="cuda", generator=g)
    # LSeg rows: weighted means of logit_scale * unit vectors -> norms <= 14.29 (lseg_net.py:268,321)
    feat *= (14.2857 * (0.05 + 0.95 * torch.rand((N, 1), device="cuda", generator=g))) / feat.norm(dim=1, keepdim=True)
    # queries: mean of 63 unit template embeddings each, not re-normalised (clip_utils.py:218-225)
    base = torch.randn((Q, 1, D), device="cuda", generator=g)
    t = base + 0.7 * torch.randn((Q, 63, D), device="cuda", generator=g)
    t /= t.norm(dim=2, keepdim=True)
    qm = t.mean(dim=1).contiguous()
    if D == 1536:
        # config 5 (fused visual | audio map): the first half of the queries are text queries living in the 512 visual
        # columns, the second half audio queries living in the 1024 AudioCLIP columns
        qm[: Q // 2, 512:] = 0
        qm[Q // 2:, :512] = 0
    return feat, qm


def index_map_api_probe(feat_h, D, reps=30):
    """wall-clock of VLMap.index_map through the reference-shaped API on a host map already loaded (grid_feat resident in HBM
    after the first call)"""
    from avlmaps_amd.apps.common import HashClip
    from avlmaps_amd.map.vlmap import VLMap

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    cfg = Cfg(map_type="vlmap", grid_size=1000, cell_size=0.05, depth_sample_rate=100, cam_calib_mat=[540, 0, 540, 0, 540, 360, 0, 0, 1],
              pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                            base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0]))
    vm = VLMap(cfg)
    vm.grid_feat, vm.clip_feat_dim, vm.clip_model = feat_h, D, HashClip(D)
    t0 = time.perf_counter()
    m0 = vm.index_map("sofa", with_init_cat=False)                 # upload + conversion to the compact resident copy, once per map
    first = time.perf_counter() - t0
    for _ in range(8):
        vm.index_map("sofa", with_init_cat=False)
    cached, fresh = [], []
    for i in range(reps):
        t0 = time.perf_counter()
        m = vm.index_map("sofa", with_init_cat=False)
        cached.append(time.perf_counter() - t0)
    for i in range(reps):
        t0 = time.perf_counter()
        vm.index_map(f"chair number {i}", with_init_cat=False)
        fresh.append(time.perf_counter() - t0)
    assert m.dtype == np.bool_ and m.shape == (len(feat_h),) and np.array_equal(m, m0)
    out = dict(voxels=len(feat_h), first_call_s=first, cached_query_ms=float(np.median(cached)) * 1e3, new_query_ms=float(np.median(fresh)) * 1e3,
               mask_true=int(m.sum()), what="VLMap.index_map(name, with_init_cat=False): (N,) bool on the host; text tower = hash stand-in")
    # AVLMap.index_object (avlmap.py:67-76): query -> argmax -> mask -> nearest-target decay heat, (N,) float32 back on the host
    try:
        from avlmaps_amd.map.avlmap import AVLMap
        N = len(feat_h)
        rng = np.random.default_rng(3)
        side = int(round((N / 0.07) ** (1 / 3))) + 1
        lin = rng.choice(side ** 3, size=N, replace=False)
        am = AVLMap(Cfg(map_config=cfg, params=Cfg(cs=0.05, gs=1000)))
        am.vlmap = vm
        vm.grid_pos = np.stack([lin // (side * side), (lin // side) % side, lin % side], 1).astype(np.int32)
        for _ in range(3):
            am.index_object("sofa", decay_rate=0.01)
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            heat = am.index_object("sofa", decay_rate=0.01)
            ts.append(time.perf_counter() - t0)
        out["index_object_cached_query_ms"] = float(np.median(ts)) * 1e3
        assert heat.shape == (N,) and heat.dtype == np.float32 and float(heat.max()) == 1.0
    except Exception as e:
        out["index_object_error"] = repr(e)
    return out


def cpu_index_baseline(feat_h, q_h, repeats=3):
    """the reference's own op on the host cores: map_feats @ text_feats.T then argmax(axis=1)"""
    try:
        from threadpoolctl import threadpool_info
        threads = max([p.get("num_threads", 1) for p in threadpool_info() if p.get("user_api") == "blas"] or [1])
    except Exception:
        threads = os.cpu_count() or 1
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        sc = feat_h @ q_h.T
        am = np.argmax(sc, axis=1)
        best = min(best, time.perf_counter() - t0)
    return best, threads, am


def run_index(args, torch, dist, lib, rank, ws):
    from avlmaps_amd import _lib
    N, D, Q = args.voxels, args.feat_dim, args.queries
    feat, q = make_index_inputs(torch, N, D, Q, seed=1234 + rank)
    am = torch.empty((N,), dtype=torch.int32, device="cuda")
    best = torch.empty((N,), dtype=torch.float32, device="cuda")
    wsb = C.c_size_t()
    lib.avl_sim_workspace_bytes_n(N, D, Q, C.byref(wsb))      # query image + one range-guard word per 32 rows: no allocation per call
    wsbuf = torch.empty((max(wsb.value, 64),), dtype=torch.uint8, device="cuda")

    # block-structured query sets (config 5: text queries live in the 512 visual columns, audio queries in the 1024 audio
    # columns): the non-zero column window of every query is known on the host (the queries come from there) and the library
    # scores each group against its own columns only -- the map is still read once per step
    from avlmaps_amd.ops import query_col_support
    cb, ce = query_col_support(q.cpu().numpy())
    use_blocks = (not args.dense) and len(set(zip((cb // 128).tolist(), ((ce + 127) // 128).tolist()))) > 1

    # --resident: the form of the map the timed steps read.  raw = the float32 map as the reference holds it (the headline);
    # prepared / compact = the resident copies VLMap keeps for a map that is queried many times (avl_sim_prepare_map: same 4 B
    # per element as fp16 hi | lo; avl_sim_prepare_map24: 3 B per element, VLMap's default)
    resident = getattr(args, "resident", "raw")
    res_map = res_scale = None
    if resident == "prepared":
        res_map = feat.clone()
        res_scale = torch.empty((N,), dtype=torch.float32, device="cuda")
        _lib.check(lib.avl_sim_prepare_map(res_map.data_ptr(), N, D, D, res_scale.data_ptr(), None), "avl_sim_prepare_map")
    elif resident == "compact":
        res_map = torch.empty((N, 3 * D), dtype=torch.uint8, device="cuda")
        res_scale = torch.empty((N,), dtype=torch.float32, device="cuda")
        _lib.check(lib.avl_sim_prepare_map24(feat.data_ptr(), N, D, D, res_map.data_ptr(), res_scale.data_ptr(), None), "avl_sim_prepare_map24")
    res_prec = {"prepared": _lib.SIM_PREPARED, "compact": _lib.SIM_PREPARED24}.get(resident)

    def step(scores_ptr=None):
        # what VLMap.index_map asks for: the row argmax only (the best score is an optional extra output of the kernel)
        if res_map is not None:
            if use_blocks:
                rc = lib.avl_sim_scores_blocks(res_map.data_ptr(), res_scale.data_ptr(), N, D, D, q.data_ptr(), Q, D, cb.ctypes.data,
                                               ce.ctypes.data, scores_ptr, am.data_ptr(), None, res_prec, wsbuf.data_ptr(), wsb.value, None)
            elif resident == "prepared":
                rc = lib.avl_sim_scores_prepared(res_map.data_ptr(), res_scale.data_ptr(), N, D, D, q.data_ptr(), Q, D, scores_ptr,
                                                 am.data_ptr(), None, wsbuf.data_ptr(), wsb.value, None)
            else:
                rc = lib.avl_sim_scores_prepared24(res_map.data_ptr(), res_scale.data_ptr(), N, D, q.data_ptr(), Q, D, scores_ptr, am.data_ptr(),
                                                   None, wsbuf.data_ptr(), wsb.value, None)
        elif use_blocks:
            rc = lib.avl_sim_scores_blocks(feat.data_ptr(), None, N, D, D, q.data_ptr(), Q, D, cb.ctypes.data, ce.ctypes.data, scores_ptr,
                                           am.data_ptr(), None, _lib.SIM_AUTO, wsbuf.data_ptr(), wsb.value, None)
        else:
            rc = lib.avl_sim_scores_ws(feat.data_ptr(), N, D, D, q.data_ptr(), Q, D, scores_ptr, am.data_ptr(), None,
                                       _lib.SIM_AUTO, wsbuf.data_ptr(), wsb.value, None)
        _lib.check(rc, "avl_sim_scores")

    # untimed settle phase before the W warm-up steps: after an idle gap the first ~30 launches run 10-25 % slower while
    # the package power controller converges on its operating point (the kernel sits at the 1.4 kW cap);
    # the figure reported is the settled rate whatever W the caller picks
    for _ in range(args.settle_steps):
        step()
    for _ in range(args.warmup):
        step()
    # HIP events on the launch stream: one pair around the K timed steps (default; an event record between launches
    # costs a few % on a 0.7 ms kernel because its release fence drains the queue), or --event-mode each = K + 1 records
    n_ev = args.steps + 1 if args.event_mode == "each" else 2
    evs = []
    for _ in range(n_ev):
        e = C.c_void_p()
        lib.avl_event_create(C.byref(e))
        evs.append(e)
    barrier_sync(torch, dist, ws)
    t0 = time.perf_counter()
    if args.event_mode == "each":
        for i in range(args.steps):
            lib.avl_event_record(evs[i], None)
            step()
    else:
        lib.avl_event_record(evs[0], None)
        for i in range(args.steps):
            step()
    lib.avl_event_record(evs[-1], None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dt = max_over_ranks(torch, dist, ws, dt)
    if ws > 1:
        dist.barrier()
    # --dump-outputs: what the last timed step returned -- the row argmax (query index per voxel) of this rank's rows; the
    # variants below launch the same kernel into `am` again
    last = dict(argmax=am.cpu().numpy().astype(np.float32)) if args.dump_outputs and rank == 0 else None
    ms = C.c_float()
    per_step = []
    for i in range(n_ev - 1):
        lib.avl_event_elapsed_ms(evs[i], evs[i + 1], C.byref(ms))
        per_step.append(ms.value)
    for e in evs:
        lib.avl_event_destroy(e)
    # per-launch duration of the dominant kernel (+ the ~5 us query prep launch)
    ev_ms = float(np.mean(per_step)) if args.event_mode == "each" else per_step[0] / args.steps
    timer = event_timer(lib)
    map_bytes = N * D * 3 + N * 4 if resident == "compact" else (N * D * 4 + N * 4 if resident == "prepared" else N * D * 4)
    alg_bytes = map_bytes + Q * D * 4 + N * 4            # feature stream (+ row scales) + queries + argmax out
    achieved = alg_bytes / (ev_ms * 1e-3) / 1e9

    out = dict(
        metric="voxel_query_similarities_per_sec", value=ws * N * Q * args.steps / dt, unit="similarities/s",
        n_gpus=ws, steps=args.steps, warmup=args.warmup, ms_per_step=dt / args.steps * 1e3, higher_is_better=True,
        scaling="weak", scaling_note=("voxel rows are sharded over the ranks, no data-path collective: N x by construction; the strong-scaling "
                                      "answer for map creation is the top-level `build` block" if ws > 1 else None),
        vs_baseline=None, dtype="f32", data="synthetic",
        config=dict(workload=f"index_map: {N} voxels x {D}-D float32 map per GPU, {Q} text queries, "
                             "scores fused with row argmax (no scores_mat write)"
                             + ("" if resident == "raw" else f"; the kernel reads the map's {resident} resident copy "
                                + ("(fp16 hi | lo, 4 B per element)" if resident == "prepared" else
                                   "(fp16 hi + residual byte, 3 B per element: VLMap's default; roofline on the bytes it reads)")),
                    resident_form=resident,
                    voxels_per_gpu=N, feat_dim=D, queries=Q, parallelism=f"voxel-row shards x{ws}; NO data-path collective (weak scaling by construction: only a barrier and the "
                                                                         "timing all-reduce cross ranks; the exchange-bearing numbers are extra.map_build_strong*)",
                    settle_steps=args.settle_steps,
                    kernel=("column-block launches (avl_sim_scores_blocks): sim_split_f16_kernel on the 512 visual columns + "
                            "sim_kswap_f16_kernel on the audio columns, each for its own queries" if use_blocks else
                            "sim_split_f16_kernel (fp16 hi/lo split MFMA, fp32 accumulate, query image resident in LDS)"
                            if D <= 512 and Q <= 78 else
                            "sim_kswap_f16_kernel (fp16 hi/lo split MFMA, fp32 accumulate, half the query image resident, swapped per 3 voxel tiles)"
                            if D <= 1024 and Q <= 64 else
                            "sim_stream_f16_kernel (fp16 hi/lo split MFMA, fp32 accumulate, query image streamed through LDS)")),
    )
    if last is not None:
        out["dumped_outputs"] = write_outputs(args.dump_outputs, last)
    out["roofline"] = dict(bound="hbm", achieved=achieved, peak=HBM_PEAK_GBS, unit="GB/s", frac=achieved / HBM_PEAK_GBS,
                           kernel_ms=ev_ms, algorithmic_bytes=alg_bytes,
                           **pmc_lookup("index", dict(N=N, D=D, Q=Q, resident=resident)))
    if resident != "raw":
        # the same pass priced on the float32 map's bytes, for comparison with the headline (the work it replaces)
        out["roofline"]["float32_equivalent_speed_frac"] = (N * D * 4 + Q * D * 4 + N * 4) / (ev_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
    if rank == 0:
        # what a kernel that ONLY reads the same 4.1 GB gets on this box (spec peak is 8 TB/s; boxes differ by ~15 %)
        g0, g1 = C.c_float(), C.c_float()
        lib.avl_hbm_read_probe(feat.data_ptr(), N, D, 0, 5, C.byref(g0), None)
        lib.avl_hbm_read_probe(feat.data_ptr(), N, D, 1, 5, C.byref(g1), None)
        ceiling = max(g0.value, g1.value)
        # the same read, `steps` launches back to back like the timed loop above: a pure 6 TB/s read already draws
        # ~1.1 kW of the 1.4 kW package cap (tools/power_probe.py), so the sustained rate sits below the burst rate
        g2 = C.c_float()
        lib.avl_hbm_read_probe(feat.data_ptr(), N, D, 3, max(args.steps, 10), C.byref(g2), None)
        out["roofline"].update(measured_read_ceiling=dict(coalesced_gbs=g0.value, rowline_gbs=g1.value,
                                                          rowline_sustained_gbs=g2.value),
                               frac_of_measured_ceiling=achieved / ceiling if ceiling > 0 else None,
                               frac_of_sustained_read=achieved / g2.value if g2.value > 0 else None)
    if rank == 0 and not args.profile_run:
        # variant: also materialise scores_mat (VLMap.init_categories, vlmap.py:92-102)
        sc = torch.empty((N, Q), dtype=torch.float32, device="cuda")
        for _ in range(2):
            step(sc.data_ptr())
        ms_sc = sustained_ms(lib, lambda: step(sc.data_ptr()), launches=50, warm=40)
        # variant: the map kept in the library's prepared split-fp16 layout (what VLMap does with its private device copy;
        # avl_sim_prepare_map, same bytes per element, bit-identical scores, no per-query fp32->fp16 split)
        prep = feat.clone()
        rscale = torch.empty((N,), dtype=torch.float32, device="cuda")     # per-row 2^-s: how VLMap keeps its resident copy
        _lib.check(lib.avl_sim_prepare_map(prep.data_ptr(), N, D, D, rscale.data_ptr(), None), "avl_sim_prepare_map")
        am2 = torch.empty_like(am)

        def step_prepared():
            _lib.check(lib.avl_sim_scores_prepared(prep.data_ptr(), rscale.data_ptr(), N, D, D, q.data_ptr(), Q, D, None, am2.data_ptr(),
                                                   None, wsbuf.data_ptr(), wsb.value, None), "avl_sim_scores_prepared")
        for _ in range(3):
            step_prepared()
        ms_prep = sustained_ms(lib, step_prepared, launches=100, warm=60)
        same = float((am2 == am).double().mean())
        del prep, rscale
        # variant: the COMPACT resident copy (VLMap's default for D <= 512): 3 bytes per element, fp16 hi + one residual byte
        compact = None
        if D % 64 == 0 and D <= 512:              # the compact form runs on the resident-query kernel: one pass up to 78 queries at D <= 512
            m24 = torch.empty((N, 3 * D), dtype=torch.uint8, device="cuda")
            rs24 = torch.empty((N,), dtype=torch.float32, device="cuda")
            _lib.check(lib.avl_sim_prepare_map24(feat.data_ptr(), N, D, D, m24.data_ptr(), rs24.data_ptr(), None), "avl_sim_prepare_map24")
            sc24 = torch.empty((8192, Q), dtype=torch.float32, device="cuda")

            def step_compact():
                _lib.check(lib.avl_sim_scores_prepared24(m24.data_ptr(), rs24.data_ptr(), N, D, q.data_ptr(), Q, D, None, am2.data_ptr(),
                                                         None, wsbuf.data_ptr(), wsb.value, None), "avl_sim_scores_prepared24")
            for _ in range(3):
                step_compact()
            ms24 = sustained_ms(lib, step_compact, launches=100, warm=60)
            same24 = float((am2 == am).double().mean())
            _lib.check(lib.avl_sim_scores_prepared24(m24.data_ptr(), rs24.data_ptr(), 8192, D, q.data_ptr(), Q, D, sc24.data_ptr(), None,
                                                     None, wsbuf.data_ptr(), wsb.value, None), "avl_sim_scores_prepared24")
            err24 = float((sc24.double() - feat[:8192].double() @ q.double().T).abs().max())
            bytes24 = N * D * 3 + N * 4 + Q * D * 4 + N * 4
            compact = dict(ms=ms24, similarities_per_s=N * Q / (ms24 * 1e-3), bytes_per_pass=bytes24, gbs=bytes24 / (ms24 * 1e-3) / 1e9,
                           argmax_agreement_with_primary=same24, max_abs_err_vs_fp64_first_8192_rows=err24, tolerance=1e-4,
                           what="VLMap's resident copy for D <= 512: fp16 hi + residual byte in units of ulp(hi)/256 per element, per-row power-of-two scale")
            del m24, rs24, sc24
        # parity spot check against float64 on the device (north_star tolerance 1e-4)
        g = torch.Generator(device="cuda").manual_seed(7)
        idx = torch.randint(0, N, (8192,), device="cuda", generator=g)
        ref = feat[idx].double() @ q.double().T
        err = float((sc[idx].double() - ref).abs().max())
        am_ok = float((ref.argmax(dim=1) == am[idx].long()).double().mean())
        out["extra"] = dict(
            prepared_map_variant=dict(ms=ms_prep, similarities_per_s=N * Q / (ms_prep * 1e-3), gbs=alg_bytes / (ms_prep * 1e-3) / 1e9,
                                      argmax_agreement_with_primary=same, per_row_scale=True),
            scores_mat_variant=dict(ms=ms_sc, similarities_per_s=N * Q / (ms_sc * 1e-3),
                                    gbs=(alg_bytes + N * Q * 4) / (ms_sc * 1e-3) / 1e9),
            parity_sample=dict(rows=8192, max_abs_err_vs_fp64=err, argmax_agreement=am_ok, tolerance=1e-4))
        if compact is not None:
            out["extra"]["compact_prepared_map_variant"] = compact
        # a map of the size real scenes produce (a few hundred thousand voxels), "64 categories + other" as the reference's
        # init_categories scores them (65 columns), and the two-column query of index_map(with_init_cat=False)
        try:
            n3 = min(300_000, N)
            am3 = torch.empty((n3,), dtype=torch.int32, device="cuda")
            res3 = {}
            for q3n in (2, 65):
                q3 = torch.cat([q] * ((q3n + Q - 1) // Q))[:q3n].contiguous()
                fn3 = lambda: _lib.check(lib.avl_sim_scores_ws(feat.data_ptr(), n3, D, D, q3.data_ptr(), q3n, D, None, am3.data_ptr(),
                                                               None, _lib.SIM_AUTO, None, 0, None), "sim")
                ms3 = sustained_ms(lib, fn3, launches=200, warm=100)
                res3[f"q{q3n}"] = dict(us=ms3 * 1e3, gbs=n3 * D * 4 / (ms3 * 1e-3) / 1e9, similarities_per_s=n3 * q3n / (ms3 * 1e-3))
            out["extra"]["scene_sized_map_300k_voxels"] = res3
        except Exception as e:
            out["extra"]["scene_sized_map_300k_voxels"] = dict(error=str(e))
        # the reference's real query shape: "64 categories + other" = 65 columns (clip_utils.py:213-215), at the full map size.
        # The 65th row runs on v_mfma_f32_4x4x4_16b_f16 instead of a third, mostly padded 32-row tile
        try:
            if D == 512 and Q == 64:
                q65 = torch.cat([q, q[:1] * 0.5]).contiguous()
                w65 = C.c_size_t()
                lib.avl_sim_workspace_bytes_n(N, D, 65, C.byref(w65))
                ws65 = torch.empty((max(w65.value, 64),), dtype=torch.uint8, device="cuda")
                am65 = torch.empty_like(am)
                fn65 = lambda: _lib.check(lib.avl_sim_scores_ws(feat.data_ptr(), N, D, D, q65.data_ptr(), 65, D, None, am65.data_ptr(), None,
                                                                _lib.SIM_AUTO, ws65.data_ptr(), w65.value, None), "sim")
                ms65 = sustained_ms(lib, fn65, launches=200, warm=80)
                b65 = N * D * 4 + 65 * D * 4 + N * 4
                out["extra"]["q65_64_categories_plus_other"] = dict(
                    ms=ms65, similarities_per_s=N * 65 / (ms65 * 1e-3), gbs=b65 / (ms65 * 1e-3) / 1e9, frac_of_hbm_peak=b65 / (ms65 * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    argmax_agreement_with_64_query_run=float(((am65 == am) | (am65 == 64)).double().mean()),
                    kernel="sim_split_f16_kernel<2, 8, ..., XR>: two full MFMA tiles + the 65th row on 4x4x4 MFMAs, raw float32 map")
                del ws65, am65, q65
        except Exception as e:
            out["extra"]["q65_64_categories_plus_other"] = dict(error=str(e))
        # the step after the mask in AVLMap.index_object: nearest-target decay heat over the same 2M voxels
        # (visualize_utils.py:29-49 is an O(N_other * N_target) Python loop upstream: hours at this size)
        try:
            g = torch.Generator(device="cuda").manual_seed(11)
            side = int(round((N / 0.07) ** (1 / 3))) + 1      # ~7 % occupancy of a cube, unique voxel positions
            lin = torch.randperm(side ** 3, device="cuda", generator=g)[:N]
            pos = torch.stack([lin // (side * side), (lin // side) % side, lin % side], 1).to(torch.int32).contiguous()
            mask = (am == 0).to(torch.uint8)
            heat = torch.empty((N,), dtype=torch.float32, device="cuda")

            def heat_step():
                _lib.check(lib.avl_heatmap_from_mask(pos.data_ptr(), mask.data_ptr(), N, 0.05, 0.01, heat.data_ptr(), None))
            heat_step()
            torch.cuda.synchronize()
            ms_heat = float(np.median([timer(heat_step) for _ in range(5)]))
            out["extra"]["heatmap_from_mask"] = dict(ms=ms_heat, voxels=N, targets=int(mask.sum().item()), decay_rate=0.01,
                                                     nonzero_heat=int((heat > 0).sum().item()),
                                                     geometry=f"{side}^3 cube at 7 % occupancy, targets scattered uniformly (5 words per column)")
            # the reference's map shape: a 1000 x 1000 x 30 grid (one word per column); targets scattered uniformly -- every window
            # holds some -- and clustered into a few objects, the case index_object meets (most windows are empty: coarse pruning)
            lin = torch.randperm(1000 * 1000 * 30, device="cuda", generator=g)[:N]
            pos = torch.stack([lin // 30000, (lin // 30) % 1000, lin % 30], 1).to(torch.int32).contiguous()
            centres = pos[torch.randint(0, N, (6,), device="cuda", generator=g)]
            shaped = {}
            plan = C.c_void_p()                             # what AVLMap.index_object keeps per map: the voxels' cell order
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(lib.avl_heat_plan_create(C.byref(plan), pos.data_ptr(), N, None))
            shaped["plan_build_ms"] = (time.perf_counter() - t0) * 1e3

            def planned_step():
                _lib.check(lib.avl_heatmap_from_mask_planned(plan, mask.data_ptr(), 0.05, 0.01, heat.data_ptr(), None))
            for name, mk in (("uniform_targets", mask), ("clustered_targets",
                                                         ((pos[:, None, :] - centres[None]).abs().amax(dim=2) <= 12).any(dim=1).to(torch.uint8))):
                mask = mk
                heat_step()
                torch.cuda.synchronize()
                shaped[name] = dict(ms=float(np.median([timer(heat_step) for _ in range(5)])), targets=int(mk.sum().item()),
                                    nonzero_heat=int((heat > 0).sum().item()))
                want = heat.clone()
                planned_step()
                torch.cuda.synchronize()
                shaped[name]["planned_ms"] = float(np.median([timer(planned_step) for _ in range(5)]))
                shaped[name]["planned_same_bits"] = bool(torch.equal(want, heat))
            lib.avl_heat_plan_destroy(plan)
            out["extra"]["heatmap_from_mask"]["map_shaped_1000x1000x30"] = shaped
            del pos, mask, heat, lin
        except Exception as e:  # the extra must never break the benchmark line
            out["extra"]["heatmap_from_mask"] = dict(error=str(e))
        if ws == 1 and not args.no_cpu:
            feat_h, q_h = feat.cpu().numpy(), q.cpu().numpy()
            t_cpu, threads, am_cpu = cpu_index_baseline(feat_h, q_h)
            agree = float(np.mean(am_cpu == am.cpu().numpy()))
            out["cpu_baseline"] = dict(value=N * Q / t_cpu, unit="similarities/s", cores=threads, kind="reference",
                                       kind_note="the reference's OWN op on the host cores (NumPy / OpenBLAS sgemm + np.argmax), not a port",
                                       sample=f"full workload ({N}x{D} @ {D}x{Q} numpy/OpenBLAS sgemm + np.argmax, best of 3, "
                                              f"{t_cpu * 1e3:.0f} ms; the op at clip_utils.py:229 + vlmap.py:123)",
                                       argmax_agreement_with_gpu=agree)
            out["extra"]["speedup_vs_cpu"] = out["value"] / out["cpu_baseline"]["value"]
            # what a navigator gets: VLMap.index_map(name, with_init_cat=False) end to end at this map size (vlmap.py:104-125) --
            # text features (cached per string), the kernel on the compact resident copy, mask compared + bit-packed on the device,
            # N / 8 bytes to the host.  The text tower is a hash stand-in (no CLIP weights here); its cost is on the uncached line.
            try:
                out["extra"]["index_map_api"] = index_map_api_probe(feat_h, D)
            except Exception as e:
                out["extra"]["index_map_api"] = dict(error=repr(e))
            del feat_h
            if not args.no_build_extra and D == 512:
                del sc
                # BASELINE config 5 (fused multimodal index): 2M x (512 visual | 1024 audio) columns, 128 queries, one pass
                try:
                    del feat
                    torch.cuda.empty_cache()
                    D5, Q5 = 1536, 128
                    f5, q5 = make_index_inputs(torch, N, D5, Q5, seed=77)
                    w5 = C.c_size_t()
                    lib.avl_sim_workspace_bytes_n(N, D5, Q5, C.byref(w5))
                    ws5 = torch.empty((max(w5.value, 64),), dtype=torch.uint8, device="cuda")

                    cb5, ce5 = query_col_support(q5.cpu().numpy())

                    def step5_dense():
                        _lib.check(lib.avl_sim_scores_ws(f5.data_ptr(), N, D5, D5, q5.data_ptr(), Q5, D5, None, am.data_ptr(),
                                                         best.data_ptr(), _lib.SIM_AUTO, ws5.data_ptr(), w5.value, None), "sim")

                    def step5():
                        _lib.check(lib.avl_sim_scores_blocks(f5.data_ptr(), None, N, D5, D5, q5.data_ptr(), Q5, D5, cb5.ctypes.data,
                                                             ce5.ctypes.data, None, am.data_ptr(), best.data_ptr(), _lib.SIM_AUTO,
                                                             ws5.data_ptr(), w5.value, None), "sim")
                    ms5_dense = sustained_ms(lib, step5_dense, launches=40, warm=30)
                    ms5_raw = sustained_ms(lib, step5, launches=40, warm=30)
                    idx = torch.randint(0, N, (4096,), device="cuda")
                    ref5 = f5[idx].double() @ q5.double().T
                    ok5_raw = float((ref5.argmax(dim=1) == am[idx].long()).double().mean())
                    # VLMap's resident copy of a fused map: the compact 3-byte form through the same column-block launches
                    m5 = torch.empty((N, 3 * D5), dtype=torch.uint8, device="cuda")
                    rs5 = torch.empty((N,), dtype=torch.float32, device="cuda")
                    _lib.check(lib.avl_sim_prepare_map24(f5.data_ptr(), N, D5, D5, m5.data_ptr(), rs5.data_ptr(), None), "avl_sim_prepare_map24")

                    def step5_compact():
                        _lib.check(lib.avl_sim_scores_blocks(m5.data_ptr(), rs5.data_ptr(), N, D5, D5, q5.data_ptr(), Q5, D5, cb5.ctypes.data,
                                                             ce5.ctypes.data, None, am.data_ptr(), best.data_ptr(), _lib.SIM_PREPARED24,
                                                             ws5.data_ptr(), w5.value, None), "sim")
                    ms5 = sustained_ms(lib, step5_compact, launches=40, warm=30)
                    ok5 = float((ref5.argmax(dim=1) == am[idx].long()).double().mean())
                    err5 = float((best[idx].double() - ref5.max(dim=1).values).abs().max())
                    fp32_bytes, read_bytes = N * D5 * 4, N * D5 * 3 + N * 4
                    raw_bytes = N * D5 * 4 + N * 8
                    out["extra"]["fused_multimodal_config5"] = dict(
                        voxels=N, feat_dim=D5, queries=Q5,
                        # headline of this block = the RAW float32 map (the form BASELINE config 5 names): roofline on the bytes it reads
                        ms=ms5_raw, similarities_per_s=N * Q5 / (ms5_raw * 1e-3), map_form="raw float32 map (on-the-fly fp16 split, range guard)",
                        hbm_bytes_read=raw_bytes, gbs=raw_bytes / (ms5_raw * 1e-3) / 1e9,
                        frac_of_hbm_peak=raw_bytes / (ms5_raw * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        argmax_agreement_vs_fp64_sample=ok5_raw,
                        # VLMap's resident copy (3 B per element): frac_of_hbm_peak = the bytes THIS form reads over the time; the same
                        # time priced on the float32 map's bytes is a speed comparison, not a roofline fraction
                        compact_resident_copy=dict(
                            ms=ms5, similarities_per_s=N * Q5 / (ms5 * 1e-3),
                            map_form="fp16 hi + residual byte, 3 B per element, float32-class scores (VLMap's default resident copy)",
                            hbm_bytes_read=read_bytes, gbs=read_bytes / (ms5 * 1e-3) / 1e9,
                            frac_of_hbm_peak=read_bytes / (ms5 * 1e-3) / 1e9 / HBM_PEAK_GBS,
                            float32_equivalent_speed_frac=fp32_bytes / (ms5 * 1e-3) / 1e9 / HBM_PEAK_GBS,
                            float32_equivalent_speed_frac_is="the float32 map's bytes over this pass's time: how fast a float32 pass would have to "
                                                             "be to match it -- NOT a roofline fraction, the kernel does not read those bytes",
                            argmax_agreement_vs_fp64_sample=ok5, max_abs_err_best_vs_fp64_sample=err5, tolerance=1e-4),
                        dense_single_pass_ms=ms5_dense,
                        kernel="column-block launches: 64 text queries x 512 visual columns (resident kernel) + 64 audio queries x 1024 "
                               "audio columns (K-swap kernel: half the query image resident, swapped per 3 voxel tiles); the map is read once")
                    del m5, rs5
                    del f5, q5, ws5
                except Exception as e:
                    out["extra"]["fused_multimodal_config5"] = dict(error=str(e))
    return out


# ---------------------------------------------------------------------------------------- build workload
def make_build_inputs(torch, H, W, Hf, Wf, D, nbuf, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H, device="cuda"), torch.linspace(-1, 1, W, device="cuda"), indexing="ij")
    depths, rgbs, feats = [], [], []
    for i in range(nbuf):
        d = 2.6 + 1.6 * torch.sin(2.0 * xx + 0.37 * i) * torch.cos(1.5 * yy) + 0.7 * yy
        d = d + 0.02 * torch.randn((H, W), device="cuda", generator=g)
        depths.append(d.float().contiguous())
        rgbs.append(torch.randint(0, 256, (H, W, 3), device="cuda", generator=g, dtype=torch.uint8))
        f = torch.randn((Hf, Wf, D), device="cuda", generator=g)
        f = (f / f.norm(dim=2, keepdim=True) * 14.2857).half().float().contiguous()      # LSeg: fp16 then cast
        feats.append(f)
    return depths, rgbs, feats


def _json_default(o):
    """0-d tensors / NumPy scalars that slipped into a record"""
    if hasattr(o, "item"):
        return o.item()
    if hasattr(o, "tolist"):
        return o.tolist()
    return str(o)


# ---------------------------------------------------------------------------------------- --dump-outputs
DUMP_LIMIT_BYTES = 64 << 20


def sample_index(n, k, seed):
    """all of range(n) when n <= k, else k of them drawn by a generator of fixed seed, ascending"""
    if n <= k:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False)).astype(np.int64)


def build_outputs(torch, fin, max_rows=16384, occupied_samples=1 << 18):
    """the map the build's timed region ended with (finalize, or this rank's block of the merge) on the host: every row when
    there are at most max_rows, otherwise the same seeded sample of rows of every per-voxel array (row_index says which)"""
    rows = {k: fin[k] for k in ("grid_feat", "grid_pos", "weight", "grid_rgb") if fin.get(k) is not None}
    n = int(rows["grid_pos"].shape[0])
    idx = sample_index(n, max_rows, seed=0)
    out = dict(num_rows=np.array([n], np.float64), row_index=idx.astype(np.float64))
    for k, v in rows.items():
        t = torch.as_tensor(v)
        out[k] = t.index_select(0, torch.from_numpy(idx).to(t.device)).cpu().numpy().astype(np.float32)
    if fin.get("occupied_ids") is not None:
        t = torch.as_tensor(fin["occupied_ids"]).reshape(-1)
        j = sample_index(t.numel(), occupied_samples, seed=1)
        out["occupied_ids_index"] = j.astype(np.float64)
        out["occupied_ids"] = t.index_select(0, torch.from_numpy(j).to(t.device)).cpu().numpy().astype(np.float64)
    return out


def write_outputs(dirpath, arrays):
    """DIR/<name>.npy per array, float32 / float64 only, at most DUMP_LIMIT_BYTES in all -> {name: shape}"""
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {k: a.dtype for k, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, total
    d = Path(dirpath)
    d.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        np.save(d / f"{name}.npy", np.ascontiguousarray(a))
    return {name: list(a.shape) for name, a in arrays.items()}


def trajectory(n, kind="loop", radius=8.0):
    """synthetic base poses (x y z qx qy qz qw, dataset/README.md:93).  "loop": a 3 m circle walked every 1 571 frames while the
    camera turns once per 524 frames -- a 10 k-frame sequence revisits the same room six times, so EVERY contiguous frame shard
    sees nearly the whole map (the merge's worst case: almost every voxel is shared by all ranks).  "spiral": exploration -- a
    square spiral outwards from the start, rings 4 m apart, inside the +-25 m the 1000 x 0.05 m grid spans, camera along the
    direction of travel with a slow sweep: contiguous frame shards map mostly disjoint space and share their ring borders
    (radius 8 m: a 10 k-frame sequence maps about as many voxels as the loop, ~2.3 M; 18 m: ~12 M)."""
    from scipy.spatial.transform import Rotation as R
    i = np.arange(n)
    if kind == "loop":
        yaw = 0.012 * i
        p = np.stack([3.0 * np.sin(0.004 * i), np.zeros(n), -3.0 * (1 - np.cos(0.004 * i))], 1)
    elif kind == "spiral":
        pts, d, seg, pos = [np.zeros(2)], 0, 4.0, np.zeros(2)
        dirs = np.array([[1.0, 0.0], [0.0, -1.0], [-1.0, 0.0], [0.0, 1.0]])
        while np.abs(pos).max() < radius:
            for _ in range(2):
                pos = pos + dirs[d % 4] * seg
                pts.append(pos.copy())
                d += 1
            seg += 4.0
        pts = np.array(pts)
        cum = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(pts, axis=0), axis=1))])
        s = np.linspace(0.0, cum[-1], n)
        xz = np.stack([np.interp(s, cum, pts[:, 0]), np.interp(s, cum, pts[:, 1])], 1)
        k = np.clip(np.searchsorted(cum, s, side="right") - 1, 0, len(pts) - 2)
        head = np.arctan2(-(pts[k + 1, 0] - pts[k, 0]), -(pts[k + 1, 1] - pts[k, 1]))      # camera looks along -z of the base frame
        yaw = np.unwrap(head) + 0.6 * np.sin(0.01 * i)
        p = np.stack([xz[:, 0], np.zeros(n), xz[:, 1]], 1)
    else:
        raise ValueError(kind)
    q = R.from_euler("y", yaw).as_quat()
    return np.concatenate([p, q], 1)


def pc_transforms(poses):
    """host-side pose chain exactly as the product does it (avlmaps_amd.map.vlmap_builder)"""
    from avlmaps_amd.utils.mapping_utils import cvt_pose_vec2tf
    b2c = np.eye(4)
    b2c[:3, :3] = np.array([1, 0, 0, 0, -1, 0, 0, 0, -1.0]).reshape(3, 3)
    b2c[1, 3] = 1.5
    bt = np.eye(4)
    bt[0, :3], bt[1, :3], bt[2, :3] = [0, 0, -1], [-1, 0, 0], [0, 1, 0]
    inv_bt = np.linalg.inv(bt)
    init = bt @ cvt_pose_vec2tf(poses[0]) @ inv_bt
    inv_init = np.linalg.inv(init)
    return [inv_init @ (bt @ cvt_pose_vec2tf(p) @ inv_bt) @ bt @ b2c for p in poses]


def make_vit_standin(torch):
    """A random-weight ViT-L/16-shaped encoder (24 pre-norm layers, width 1024, 16 heads, MLP 4096) run in bf16 on the two
    480x480 crops (900 tokens each) upstream's sliding-window LSeg evaluation feeds per 720x1080 frame (lseg_utils.py:61-102).
    It is NOT LSeg -- no DPT decoder, no text head, no weights -- only a stand-in for the bulk of its per-frame cost, so that
    the build line can also be quoted with a feature-extraction-sized load in front of every frame."""
    layer = torch.nn.TransformerEncoderLayer(d_model=1024, nhead=16, dim_feedforward=4096, dropout=0.0, activation="gelu",
                                             batch_first=True, norm_first=True)
    enc = torch.nn.TransformerEncoder(layer, num_layers=24, enable_nested_tensor=False).cuda().to(torch.bfloat16).eval()
    x = torch.randn((2, 900, 1024), device="cuda", dtype=torch.bfloat16)

    def step():
        with torch.no_grad():
            return enc(x)
    return step


_MERGED_ONCE = []          # non-empty once this process has run a merge (the first one is the cold one)


def merge_ranks(parallel, acc, mode, exact_rgb, timings=None):
    """the multi-GPU merge of the build: row-sharded all_to_all of every rank's own voxel rows (default; the finished map stays
    row-sharded over the ranks' HBM, where the index kernels want it) or ONE dense sum-reduce to rank 0 (--merge-mode reduce)"""
    if mode == "reduce":
        return parallel.merge_accumulator(acc, dst=0, exact_rgb=exact_rgb, timings=timings)
    return parallel.merge_accumulator_sharded(acc, exact_rgb=exact_rgb, timings=timings)


def run_build_core(args, torch, dist, lib, rank, ws, total_frames, warmup=8, batch=1, exact_rgb=True, feature_standin=None,
                   deferred=False, solo=False, merge_mode=None, dump=None):
    """STRONG scaling of map creation: `total_frames` frames of one sequence are sharded contiguously over the ranks; the
    timed region is everything between the first fused frame and the finished map resident in HBM:
        fuse own shard (K1/K2/K3 per launch)  ->  [ws > 1: plan + scatter + ONE all_to_all of the ranks' own voxel rows to the
        owners of their final rows (or, --merge-mode reduce, one dense RCCL sum-reduce to rank 0) + chained colour replay]
        -> finalize (first-touch-key order, grid_feat / grid_pos / weight / grid_rgb): every rank its block of rows
    max over ranks.  Per-frame feature extraction (LSeg, 2 ViT-L crops per frame upstream) is NOT included: the pixel features
    are resident in HBM, as the kernel boundary takes them.  dump: a dict that receives the finished map on the host
    (build_outputs) once the timed region is over."""
    from avlmaps_amd import ops, parallel
    H, W, Hf, Wf, D, rate = 720, 1080, 347, 520, 512, 100
    nbuf = 4
    depths, rgbs, feats = make_build_inputs(torch, H, W, Hf, Wf, D, nbuf, seed=99 + rank)
    lo, hi = parallel.shard_frames(total_frames, rank, ws)
    Ts = pc_transforms(trajectory(total_frames, getattr(args, "trajectory", "loop"), getattr(args, "spiral_radius", 8.0)))
    calib = np.array([540, 0, 540, 0, 540, 360, 0, 0, 1.0])
    rs = np.random.RandomState(5 + rank)
    samples = []
    for _ in range(nbuf):
        m = np.arange(H * W)
        rs.shuffle(m)
        samples.append(torch.from_numpy(m[::rate].astype(np.int32)).cuda())
    P = int(samples[0].numel())
    nloc = hi - lo
    warmup = min(warmup, nloc)
    cap = args.capacity or max(1_500_000, 300_000 + 450 * nloc)
    # doubles on demand like the reference's arrays; deferred: one launch per frame (K1 + K2 of frame i next to K3 of frame i - 1)
    acc = ops.VoxelAccumulator(1000, 0.05, 30, D, capacity=cap, deferred_fuse=bool(deferred) and int(batch) <= 1)
    if exact_rgb:
        acc.enable_replay_log(max(1, (nloc + warmup) * P))
    BATCH = max(1, int(batch))
    plans = {}

    extract = make_vit_standin(torch) if feature_standin == "vit-l16" else None

    # frame-by-frame launches with the frames resident: the LOOP runs in C (avl_builder_integrate_frames, 64 frames per call; one
    # launch pair -- deferred: one launch -- per frame, no two frames share a launch; inside a call frame i + 1's map-independent half
    # of K1 rides in frame i's launch (PreGather), which per-frame integrate_frame calls cannot do).  VLMapBuilder issues the same
    # calls whenever staged frames are waiting (frame_loop_frames).  A Python call costs 12.4 us of host time, more than the
    # pipe_kernel it launches (tools/probe_frame_loop.py); --python-frame-loop keeps the loop in Python (one integrate_frame per frame)
    c_loop = BATCH == 1 and extract is None and not getattr(args, "python_frame_loop", False)
    SEQ = 64

    def fuse(i0, i1):
        if c_loop:
            for j0 in range(i0, i1, SEQ):
                j1 = min(i1, j0 + SEQ)
                idx = tuple(i % nbuf for i in range(j0, j1))
                plan = plans.get(idx)
                if plan is None:
                    plan = plans[idx] = acc.make_batch_plan([depths[b] for b in idx], [samples[b] for b in idx], [feats[b] for b in idx],
                                                            [rgbs[b] for b in idx])
                acc.integrate_frames(plan, calib, Ts[j0:j1], frame_idx0=j0)
            return
        if BATCH == 1:
            for i in range(i0, i1):
                b = i % nbuf
                if extract is not None:
                    extract()                                # same stream: the frame's fusion launches queue behind it
                acc.integrate_frame(depths[b], calib, Ts[i], samples[b], feats[b], rgbs[b], frame_idx=i)
            return
        for j0 in range(i0, i1, BATCH):
            j1 = min(i1, j0 + BATCH)
            if extract is not None:
                for _ in range(j0, j1):
                    extract()
            # the frame buffers form a ring of nbuf: the pointer table of a batch is resolved once per ring phase
            idx = tuple(i % nbuf for i in range(j0, j1))
            plan = plans.get(idx)
            if plan is None:
                plan = plans[idx] = acc.make_batch_plan([depths[b] for b in idx], [samples[b] for b in idx], [feats[b] for b in idx],
                                                        [rgbs[b] for b in idx])
            acc.integrate_batch(plan, calib, Ts[j0:j1], frame_idx0=j0)

    if warmup:
        fuse(lo, lo + warmup)           # untimed: code objects loaded, pools warm; then start from an empty map
    # the warm-up covers the tail of the path too: the first merge of a process pays for torch's sort / unique kernels, RCCL's
    # lazily created point-to-point communicators and the allocator's first large blocks (tens to hundreds of ms, once)
    mode = merge_mode or getattr(args, "merge_mode", "sharded")
    first_merge_s = None
    if ws > 1:
        # one untimed merge of the warm-up frames (every rank, also one without warm-up frames): RCCL's communicator, the first
        # launches of the merge's code objects.  If it is the FIRST merge of this process its wall time is reported
        # (merge_first_call_s); no other warm-up exists -- the gather-plan merge has nothing lazy to load (merge2.py), and the timed
        # merge below allocates its 10k-frame-sized buffers inside the timed region, as a production build does
        t_first = time.perf_counter()
        merge_ranks(parallel, acc, mode, exact_rgb)
        torch.cuda.synchronize()
        if not _MERGED_ONCE:
            first_merge_s = time.perf_counter() - t_first
        _MERGED_ONCE.append(1)
    elif warmup:
        acc.finalize(as_torch=True)
    if warmup or ws > 1:
        acc.num_voxels()
        acc.reset()
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.avl_event_create(C.byref(e0))
    lib.avl_event_create(C.byref(e1))
    tim = {}
    barrier_sync(torch, dist, ws)
    t0 = time.perf_counter()
    lib.avl_event_record(e0, None)
    fuse(lo, hi)
    acc.flush()                                                # deferred fuse: the last frame's K3 belongs to the fuse time
    lib.avl_event_record(e1, None)
    if ws == 1:
        fin = acc.finalize(as_torch=True)                      # sorts first-touch keys, emits the reference's arrays (device)
    else:
        fin = merge_ranks(parallel, acc, mode, exact_rgb, timings=tim)
    torch.cuda.synchronize()
    dt_local = time.perf_counter() - t0
    dt = max_over_ranks(torch, dist, ws, dt_local)
    ms = C.c_float()
    lib.avl_event_elapsed_ms(e0, e1, C.byref(ms))
    fuse_ms = ms.value
    fuse_s = max_over_ranks(torch, dist, ws, fuse_ms * 1e-3)
    lib.avl_event_destroy(e0)
    lib.avl_event_destroy(e1)
    if dump is not None and fin is not None:
        dump.update(build_outputs(torch, fin))
    nvox, npts, ngroups = acc.num_voxels(), acc.num_points(), acc.num_groups()
    n_final = None if fin is None else int(fin["M"]) if "M" in fin else int(fin["grid_pos"].shape[0])
    if ws > 1 and tim:
        # per-rank merge traffic next to the times (rank 0's own breakdown stays at the top level)
        keys = ("bytes_sent_per_rank", "payload_bytes_sent", "payload_bytes_fp64_form", "rows_sent", "local_voxels", "own_rows", "single_rank_voxels",
                "shared_voxels_local", "directory_entries", "compute_total_s", "in_collectives_total_s", "compute_s", "in_collectives_s", "wall_s",
                "shared_gpu_wait_s", "null_launch_us", "exchange_s", "scatter_reduce_s")
        per_rank = [None] * ws
        dist.all_gather_object(per_rank, {k: tim.get(k) for k in keys})
        tim["per_rank"] = per_rank
        tim["timed_merge_is"] = ("the first merge of this size in the process (after one small untimed merge of the warm-up frames): its send / "
                                 "receive / work buffers are allocated inside, as in a build that merges once")
    single_gpu_merge = None
    if ws == 1 and not solo:          # (solo: rank 0 of an N-rank run measuring the single-GPU reference while the others wait)
        # what the merge path itself costs on this GPU at this map size (plan = key sort, scatter into the send buffer, the
        # receiving side's row adds, chained replay, finalize): everything of the N-GPU merge except the transfer.  Untimed extra.
        del fin
        torch.cuda.empty_cache()
        single_gpu_merge = {}
        # the FIRST merge of the process, timed as it is (no warm-up of any kind before it: code objects, allocator blocks of the
        # map's size, the replay log's sort): what a build that merges ONCE pays -- then the same merge again, warm
        cold = {}
        if exact_rgb:
            acc.drop_replay_cache()
        torch.cuda.synchronize()
        t_cold = time.perf_counter()
        merge_ranks(parallel, acc, mode, exact_rgb, timings=cold)
        torch.cuda.synchronize()
        t_cold = time.perf_counter() - t_cold
        was_first = not _MERGED_ONCE
        _MERGED_ONCE.append(1)
        if exact_rgb:
            acc.drop_replay_cache()                            # (the timed merge sorts the replay log itself, as a merge that runs once does)
        merge_ranks(parallel, acc, mode, exact_rgb, timings=single_gpu_merge)
        single_gpu_merge["merge_cold_s" if was_first else "merge_after_empty_cache_s"] = t_cold
        single_gpu_merge["merge_cold_compute_s"] = cold.get("compute_s")
        single_gpu_merge["merge_cold_note"] = ("wall time of the FIRST merge of this process (no warm-up merge, no warm_up_merge; the accumulators' map of "
                                               f"{nvox} voxels; its {nvox * D * 4 / 1e9:.1f} GB block of finished rows is allocated inside)" if was_first else
                                               "an earlier build of this process had merged already: the allocator's blocks were released (empty_cache), the code was warm")
        if exact_rgb:
            acc.drop_replay_cache()                            # (the plain finalisation sorts the replay log itself, like the merges above)
        torch.cuda.synchronize()
        t_fin = time.perf_counter()
        acc.finalize(as_torch=True)
        torch.cuda.synchronize()
        single_gpu_merge["plain_finalize_s"] = time.perf_counter() - t_fin
    # algorithmic bytes per frame: every sample 4 B index + 4 B depth + 25 B record; every active sample 3 B rgb + D*4 B
    # feature gather + 25 B record re-read; every (frame, voxel) group one fp64 row store (D*8 B), plus a row load when
    # the voxel already existed, plus the first-touch feature row (D*4 B) when it is new
    nfr = max(1, nloc)
    pts_per_frame, groups, newv = npts / nfr, ngroups / nfr, nvox / nfr
    alg_frame = P * (4 + 4 + 25) + pts_per_frame * (3 + D * 4 + 25) + groups * D * 8 + (groups - newv) * D * 8 + newv * D * 4
    res = dict(total_frames=total_frames, frames_per_gpu=nloc, frames_per_launch=BATCH, deferred_fuse=bool(deferred) and BATCH == 1,
               host_loop=("C: avl_builder_integrate_frames, 64 frames per call -- one launch pair (deferred: one launch) per frame, no frames share a launch"
                          if c_loop else "Python: one integrate call per frame / batch"),
               frames_per_s=total_frames / dt,
               seconds=dt, fuse_seconds_max_rank=fuse_s, merge_finalize_seconds=dt - fuse_s, exact_rgb_replay=bool(exact_rgb),
               feature_standin=feature_standin, trajectory=getattr(args, "trajectory", "loop"),
               merge_mode=mode,
               timed_region=("fuse shard + merge (row-sharded all_to_all of the ranks' own voxel rows, chained replay) + finalize of every "
                             "rank's block of rows; " if mode != "reduce" else
                             "fuse shard + merge (one dense RCCL sum-reduce, chained replay) + finalize on rank 0; ")
                            + ("a random-weight ViT-L/16-shaped encoder (2 crops of 900 tokens, bf16) runs before every frame as a "
                               "stand-in for LSeg's cost" if feature_standin else "no feature extraction"),
               ms_per_frame_fuse=fuse_ms / nfr, sampled_px_per_frame=P, active_points_per_frame=pts_per_frame,
               voxel_groups_per_frame=groups, new_voxels_per_frame=newv, voxels_local=nvox, voxels_merged=n_final,
               merge_breakdown=tim or None, single_gpu_merge_path=single_gpu_merge, merge_first_call_s=first_merge_s,
               algorithmic_bytes_per_frame=alg_frame, fuse_achieved_gbs=alg_frame * nloc / (fuse_ms * 1e-3) / 1e9 if fuse_ms > 0 else None)
    acc.close()
    del acc
    torch.cuda.empty_cache()
    return res


def run_pipeline_probe(torch, frames=300):
    """The product's whole host + device pipeline (VLMapBuilder.create_mobile_base_map: frame queue, pixel sampling, host-to-device
    copies, the kernels, checkpoints every 100 frames through the incremental HDF5 writer) around a FREE feature extractor, single
    process: what the pipeline itself sustains.  Reference pixel sampling is one serial np.random.shuffle of H*W indices per frame."""
    import tempfile
    from pathlib import Path
    from avlmaps_amd.map.map import Map
    from avlmaps_amd.map.vlmap_builder import VLMapBuilder

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    H, W, Hf, Wf, D, nbuf = 720, 1080, 347, 520, 512, 4
    depths, rgbs, feats = make_build_inputs(torch, H, W, Hf, Wf, D, nbuf, seed=7)
    depths_h, rgbs_h = [d.cpu().numpy() for d in depths], [r.cpu().numpy() for r in rgbs]
    cfg = Cfg(map_type="vlmap", grid_size=1000, cell_size=0.05, depth_sample_rate=100, cam_calib_mat=[540, 0, 540, 0, 540, 360, 0, 0, 1],
              pose_info=Cfg(pose_type="mobile_base", camera_height=1.5, base2cam_rot=[1, 0, 0, 0, -1, 0, 0, 0, -1],
                            base_forward_axis=[0, 0, -1], base_left_axis=[-1, 0, 0], base_up_axis=[0, 1, 0]))
    res = {}
    # the first build of a PROCESS pays for things a running service has long paid for (the HDF5 library, the writer / sampler /
    # stager threads' first page-locked buffers, the first multi-hundred-MB host arrays): it runs first, in full, and is reported
    # on its own line (`cold_first_build`); the two legs after it are the pipeline's sustained rate
    for sampling in ("cold", "reference", "uniform"):
        cold = sampling == "cold"
        if cold:
            sampling = "reference"
        with tempfile.TemporaryDirectory() as tmp:
            tmp = Path(tmp)
            m = Map(cfg)
            np.savetxt(tmp / "poses.txt", trajectory(frames))
            k = [0]

            def extractor(rgb):
                k[0] += 1
                return feats[k[0] % nbuf]
            b = VLMapBuilder(tmp, cfg, tmp / "poses.txt", [None] * frames, [None] * frames, m.base2cam_tf, m.base_transform,
                             feat_extractor=extractor)
            b.load_frame = lambda i: (rgbs_h[i % nbuf], depths_h[i % nbuf])
            b.pixel_sampling = sampling
            np.random.seed(0)
            import contextlib
            import io
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):          # "Temporarily saving ..." lines of the checkpoints
                b.create_mobile_base_map()
            dt = time.perf_counter() - t0
            bt = dict(b.build_times)
            res["cold_first_build" if cold else f"{sampling}_pixel_sampling"] = dict(frames_per_s=frames / dt, ms_per_frame=1e3 * dt / frames,
                                                     **(dict(what="the FIRST create_mobile_base_map of this process (reference pixel sampling): includes the one-off "
                                                                  "costs of a cold process; the legs below ran after it") if cold else {}),
                                                     checkpoint_log=[(k, round(v, 4)) for k, v in bt.get("checkpoint_log", [])],
                                                     voxels=int(len(b.last_map["grid_pos"])), checkpoints=len(b._map_writer.stats),
                                                     # the frame loop alone (decode queue, sampling, pinned staging, kernels, the periodic
                                                     # checkpoints' share of the fusing thread) and the final save of the whole map
                                                     frame_loop_frames_per_s=frames / bt["frame_loop_s"], final_save_s=bt["final_save_s"],
                                                     final_save_parts={k: (round(v, 4) if isinstance(v, float) else v)
                                                                       for k, v in (bt.get("final_save_parts") or {}).items()},
                                                     checkpoints_skipped_writer_busy=bt.get("checkpoints_skipped", 0),
                                                     slow_steps_over_50ms=bt.get("slow_steps", []),
                                                     host_threads={k: bt.get(k) for k in ("sampler_busy_s", "sampler_workers", "sampler_workers_busy_s",
                                                                                          "stager_busy_s", "fuse_thread_wait_s",
                                                                                          "checkpoints_on_fusing_thread_s")})
    res["what"] = (f"VLMapBuilder.create_mobile_base_map over {frames} in-memory 720x1080 frames, free feature extractor, checkpoints every "
                   "100 frames, one process; reference sampling = the permutation np.random.shuffle(arange(H*W)) draws per frame from the global RNG "
                   "(its DRAWS are serial: the sampler thread moves the RNG on with the library's host C code, worker threads compute the lists from "
                   "snapshots of the state -- NumPy's samples and RNG state)")
    return res


def run_build(args, torch, dist, lib, rank, ws):
    last = {} if args.dump_outputs and rank == 0 else None
    r = run_build_core(args, torch, dist, lib, rank, ws, total_frames=args.steps, warmup=args.warmup, batch=args.build_batch,
                       exact_rgb=not args.no_exact_rgb, feature_standin=args.feature_standin, deferred=args.deferred_fuse, dump=last)
    out = dict(metric="map_build_frames_per_sec", value=r["frames_per_s"], unit="frames/s", n_gpus=ws, steps=args.steps,
               warmup=args.warmup, ms_per_step=r["seconds"] / max(1, args.steps) * 1e3, higher_is_better=True, scaling="strong",
               vs_baseline=None, dtype="f64", data="synthetic",
               config=dict(workload=f"create_map: {args.steps} RGB-D frames 720x1080 of one sequence -> 7776 sampled px each -> "
                                    "back-project + voxelise + fp64 feature fusion of 512-D channels-last pixel features resident in HBM "
                                    + ("(a random-weight ViT-L/16-shaped encoder, 2 x 900 tokens bf16, runs before every frame as a stand-in "
                                       "for LSeg's cost -- not LSeg)" if args.feature_standin else "(feature extraction / LSeg NOT included)")
                                    + ", then merge + finalize INSIDE the timed region",
                           feature_standin=args.feature_standin,
                           total_frames=args.steps, frames_per_launch=r["frames_per_launch"],
                           parallelism=f"contiguous frame shards x{ws}; merge = {args.merge_mode} ("
                                       + ("one all_to_all of every rank's own voxel rows to the owners of their final rows"
                                          if args.merge_mode != "reduce" else "one dense RCCL sum-reduce to rank 0")
                                       + ") + chained colour replay + finalize, all timed"))
    out["roofline"] = dict(bound="hbm", achieved=r["fuse_achieved_gbs"], peak=HBM_PEAK_GBS, unit="GB/s",
                           frac=(r["fuse_achieved_gbs"] or 0) / HBM_PEAK_GBS, kernel="K1+K2 voxelize_link + K3 fuse (per launch pair; deferred fuse: one pipe_kernel)",
                           algorithmic_bytes=r["algorithmic_bytes_per_frame"] * max(1, r["frames_per_launch"]),
                           **pmc_lookup("build", dict(frames_per_launch=r["frames_per_launch"])))
    out["extra"] = r
    if last is not None:
        out["dumped_outputs"] = write_outputs(args.dump_outputs, last)
    if rank == 0 and ws == 1 and not args.no_cpu:
        out["cpu_baseline"] = cpu_build_baseline()
    return out


def cpu_build_baseline(frames=64):
    """sequential C port of the reference loop (oracle) on one core; the reference itself is a Python loop (~5 frames/s)"""
    from oracle import avl_oracle as O
    H, W, Hf, Wf, D, rate = 720, 1080, 347, 520, 512, 100
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    depth = (2.6 + 1.6 * np.sin(2 * xx) * np.cos(1.5 * yy) + 0.7 * yy).astype(np.float32)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    feat = rng.standard_normal((D, Hf, Wf), dtype=np.float32)
    Ts = pc_transforms(trajectory(frames))
    calib = np.array([540, 0, 540, 0, 540, 360, 0, 0, 1.0])
    rs = np.random.RandomState(1)
    samples = [O.sample_indices(rs, H * W, rate) for _ in range(frames)]
    m = O.OracleMap(1000, 0.05, 1.5, D)
    t0 = time.perf_counter()
    for i in range(frames):
        m.integrate(depth, calib, Ts[i], samples[i], feat, rgb)
    dt = time.perf_counter() - t0
    return dict(value=frames / dt, unit="frames/s", cores=1, kind="port",
                sample=f"{frames} frames 720x1080, 7776 sampled px each, sequential C restatement of vlmap_builder.py:129-178 "
                       "(the reference's own Python loop measured ~5.2 frames/s, SURVEY.md section 6)")


def pmc_lookup(which, shape):
    """HBM bytes per launch (and, where collected, the matrix-pipe busy fraction) of the dominant kernel from the committed PMC
    passes: profiles/pmc_traffic.json holds one entry per (workload, shape) that tools/publish_profiles.py derived from separate
    `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` / SQ-counter runs of this same command.  Only an entry whose shape matches
    this run exactly is reported; otherwise traffic is null (never another shape's number)."""
    out = dict(traffic=None, traffic_source=None, mfma_busy_frac=None)
    try:
        entries = json.loads((ROOT / "profiles" / "pmc_traffic.json").read_text())["entries"]
    except Exception:
        return out
    for e in entries:
        if e.get("workload") == which and all(e.get("shape", {}).get(k) == v for k, v in shape.items()):
            out.update(traffic=e.get("total_bytes"), traffic_source=e.get("source"), mfma_busy_frac=e.get("mfma_busy_frac"),
                       traffic_kernel=e.get("kernel"))
            break
    return out


def measure_traffic_in_run(argv_shape, kernels=("sim_",), timeout=120):
    """HBM bytes per step of THIS run's kernels on THIS box: bench.py re-executes itself under `rocprofv3 --pmc FETCH_SIZE` and,
    in a second pass, `--pmc WRITE_SIZE` (counter-only runs, no tracing flags; the two do not fit one pass:
    /opt/skills/guides/MI355X_MICROARCH.md, rocprofv3 PMC slots) for a few profile-run steps of the same shape, and sums the
    per-launch means of the step's kernels.  gfx950: FETCH_SIZE is in KB and reports half of a wide coalesced read stream (same
    guide, HBM section) -> x 1024 x 2; WRITE_SIZE (KB) is taken as reported (uncalibrated there).  Returns None when rocprofv3 is
    missing or a pass fails -- the caller falls back to the committed profiles/pmc_traffic.json."""
    import csv
    import shutil
    import subprocess
    import tempfile
    from collections import defaultdict
    rocprof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if Path("/opt/rocm/bin/rocprofv3").exists() else None)
    if rocprof is None or os.environ.get("AVL_BENCH_PMC_CHILD") == "1":
        return None
    if any(k.startswith(("ROCPROF", "ROCP_", "ROCPROFILER")) for k in os.environ):
        return None            # this process is itself being profiled: no nested counter passes
    env = dict(os.environ, AVL_BENCH_PMC_CHILD="1", TMPDIR="/tmp", PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tot, names, launches = {}, set(), None
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        with tempfile.TemporaryDirectory(dir="/tmp") as td:
            cmd = [rocprof, "--pmc", counter, "--output-format", "csv", "-d", td, "-o", "pmc", "--", sys.executable, str(ROOT / "bench.py"),
                   "--profile-run", "--steps", "5", "--warmup", "1", "--settle-steps", "2", "--no-cpu", "--no-build-extra"] + argv_shape
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd="/tmp")
            except Exception:
                return None
            files = list(Path(td).rglob("*counter_collection.csv"))
            if r.returncode != 0 or not files:
                return None
            agg = defaultdict(list)
            for f in files:
                for row in csv.DictReader(open(f)):
                    k = row.get("Kernel_Name") or row.get("Kernel Name") or ""
                    if row.get("Counter_Name") == counter and any(m in k for m in kernels) and "prepare_map" not in k:
                        agg[k].append(float(row["Counter_Value"]))
            if not agg:
                return None
            # every kernel of a step is launched once per step: the step's bytes = sum of the per-launch means
            tot[counter] = sum(sum(v) / len(v) for v in agg.values()) * 1024.0
            names |= set(agg)
            launches = max(len(v) for v in agg.values())
    read_b, write_b = 2.0 * tot["FETCH_SIZE"], tot["WRITE_SIZE"]
    # third pass: how busy the matrix pipe is (SQ_VALU_MFMA_BUSY_CYCLES summed over the 1024 SIMDs against GRBM_GUI_ACTIVE, which
    # counts per XCD: x 1024 / 8), for the step's dominant kernel; optional -- a failure leaves the committed figure in place
    busy = None
    try:
        with tempfile.TemporaryDirectory(dir="/tmp") as td:
            cmd = [rocprof, "--pmc", "SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE", "--output-format", "csv", "-d", td, "-o", "pmc", "--",
                   sys.executable, str(ROOT / "bench.py"), "--profile-run", "--steps", "5", "--warmup", "1", "--settle-steps", "2", "--no-cpu",
                   "--no-build-extra"] + argv_shape
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd="/tmp")
            agg = defaultdict(lambda: defaultdict(list))
            for f in Path(td).rglob("*counter_collection.csv"):
                for row in csv.DictReader(open(f)):
                    k = row.get("Kernel_Name") or row.get("Kernel Name") or ""
                    if ("sim_split" in k or "sim_stream" in k or "sim_kswap" in k) and "prepare_map" not in k:
                        agg[k][row.get("Counter_Name")].append(float(row["Counter_Value"]))
            if r.returncode == 0 and agg:
                busy = {}
                for k, c in agg.items():
                    if c.get("SQ_VALU_MFMA_BUSY_CYCLES") and c.get("GRBM_GUI_ACTIVE"):
                        b = (sum(c["SQ_VALU_MFMA_BUSY_CYCLES"]) / len(c["SQ_VALU_MFMA_BUSY_CYCLES"])) / (
                            1024.0 * (sum(c["GRBM_GUI_ACTIVE"]) / len(c["GRBM_GUI_ACTIVE"])) / 8.0)
                        busy[pretty_kernel(k)] = b
                busy = (list(busy.values())[0] if len(busy) == 1 else busy) or None
    except Exception:
        busy = None
    extra_busy = dict(mfma_busy_frac=busy, mfma_busy_source="in-run: rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE") if busy else {}
    return dict(**extra_busy, traffic=read_b + write_b, traffic_source="in-run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE passes of this command on this box",
                traffic_read_bytes=read_b, traffic_write_bytes=write_b, traffic_launches_sampled=launches,
                traffic_kernels=sorted(pretty_kernel(n) for n in names),
                traffic_note="FETCH_SIZE KB x 1024 x 2 (gfx950 wide-read correction) + WRITE_SIZE KB x 1024, per step")


def pretty_kernel(name):
    import re
    m = re.match(r"_ZN3avl\d+([A-Za-z0-9_]+?)I((?:L[ib]\d+E)+)E", name)
    if m:
        return m.group(1) + "<" + ",".join(re.findall(r"L[ib](\d+)E", m.group(2))) + ">"
    return name.split("(")[0].replace("avl::", "").replace("void ", "")


def rehearsal_per_rank_merge():
    """per-rank compute of the merge in the committed eight-rank rehearsal (8 processes taking turns on ONE MI355X, gloo; the only
    8-rank evidence a 1-GPU box can give): profiles/r06_merge_rehearsal_8ranks.json, written by tools/summarize_merge.py --json"""
    f = Path(__file__).resolve().parent / "profiles" / "r06_merge_rehearsal_8ranks.json"
    if not f.exists():
        return None
    try:
        return json.loads(f.read_text())
    except Exception:
        return None


def make_summary(out):
    """The secondary numbers of this run in <= 1.5 kB at the END of the JSON line: ms / us and fraction of the 8 TB/s
    HBM peak of the bytes each kernel reads; build rates per frame; the merge path warm and cold; the product pipeline."""
    r3 = lambda v: None if v is None else round(float(v), 4)
    ex = out.get("extra", {}) or {}
    if "single_gpu_merge_path" in ex:          # --workload build: the record itself is the build
        ex = {"map_build_strong_deferred_fuse" if ex.get("deferred_fuse") else ("map_build_strong_batched64" if ex.get("frames_per_launch", 1) > 1
                                                                                else "map_build_strong"): ex}
    sm = {}
    c5 = ex.get("fused_multimodal_config5") or {}
    if "ms" in c5:
        cc = c5.get("compact_resident_copy") or {}
        sm["config5"] = dict(raw_ms=r3(c5["ms"]), raw_frac=r3(c5.get("frac_of_hbm_peak")), compact_ms=r3(cc.get("ms")), compact_frac=r3(cc.get("frac_of_hbm_peak")))
    cp = ex.get("compact_prepared_map_variant") or {}
    if "ms" in cp:
        sm["compact_config2"] = dict(ms=r3(cp["ms"]), frac=r3(cp["gbs"] / HBM_PEAK_GBS))
    q65 = ex.get("q65_64_categories_plus_other") or {}
    if "ms" in q65:
        sm["q65"] = dict(ms=r3(q65["ms"]), frac=r3(q65.get("frac_of_hbm_peak")))
    builds = {}
    for key, name in (("map_build_strong", "two_launch"), ("map_build_strong_deferred_fuse", "one_launch"), ("map_build_strong_batched64", "b64")):
        b = ex.get(key) or {}
        if b.get("ms_per_frame_fuse") is not None:
            builds[name] = dict(us_per_frame=r3(1e3 * b["ms_per_frame_fuse"]), frac=r3((b.get("fuse_achieved_gbs") or 0) / HBM_PEAK_GBS),
                                frames_per_s=round(b["frames_per_s"]))
    if builds:
        sm["build"] = builds
    b1 = ex.get("map_build_strong_deferred_fuse") or ex.get("map_build_strong") or {}
    mp = (ex.get("map_build_strong") or {}).get("single_gpu_merge_path") or b1.get("single_gpu_merge_path") or {}
    mpd = (ex.get("map_build_strong_deferred_fuse") or {}).get("single_gpu_merge_path") or {}
    if mp:
        sm["merge_path"] = dict(compute_total_ms=r3(1e3 * min(x for x in (mp.get("compute_total_s"), mpd.get("compute_total_s")) if x is not None)),
                                merge_cold_ms=r3(1e3 * mp["merge_cold_s"]) if mp.get("merge_cold_s") is not None else None,
                                plain_finalize_ms=r3(1e3 * mp.get("plain_finalize_s", 0)), voxels=mp.get("merged_voxels"))
    reh = rehearsal_per_rank_merge()
    if reh and b1.get("seconds"):
        t1, fuse1 = b1["seconds"], b1["fuse_seconds_max_rank"]
        m8 = max(reh["per_rank_compute_ms"]) * 1e-3
        sm["projected_speedup_8gpu"] = dict(value=r3(t1 / (fuse1 / 8 + m8)), t1_ms=r3(1e3 * t1), fuse1_ms=r3(1e3 * fuse1), per_rank_merge_ms=r3(1e3 * m8),
                                            note="PROJECTION, not a measurement: T1 / (T1_fuse / 8 + slowest rank's merge compute in the committed 8-rank "
                                                 "rehearsal on one GPU); the collectives' time on xGMI is NOT in it (no 8-GPU node)")
    pp = ex.get("vlmapbuilder_pipeline") or {}
    if pp and "error" not in pp:
        sm["pipeline_frames_per_s"] = {k.split("_")[0]: dict(total=round(v["frames_per_s"]), frame_loop=round(v["frame_loop_frames_per_s"]),
                                                               final_save_s=r3(v["final_save_s"]))
                                       for k, v in pp.items() if isinstance(v, dict) and "frames_per_s" in v}
    return sm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", choices=["index", "build"], default="index")
    ap.add_argument("--voxels", type=int, default=2_000_000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--feat-dim", type=int, default=512, help="feature width of the index workload (config 5: 1536 with --queries 128)")
    ap.add_argument("--capacity", type=int, default=None,
                    help="voxel capacity of the builder (default: 1.5 M, grown with the frame count: config 3's 5 000 frames "
                         "create 2.1 M voxels)")
    ap.add_argument("--build-frames", type=int, default=10_000,
                    help="index workload: total frames of the map-creation strong-scaling extra (north_star: a 10k-frame sequence)")
    ap.add_argument("--trajectory", choices=["loop", "spiral"], default="loop",
                    help="build workload: 'loop' = the same room revisited six times per 10 k frames (every frame shard sees nearly the "
                         "whole map); 'spiral' = exploration, contiguous frame shards map mostly disjoint space")
    ap.add_argument("--spiral-radius", type=float, default=8.0, help="extent of the spiral trajectory in metres (rings 4 m apart)")
    ap.add_argument("--feature-standin", choices=["vit-l16"], default=None,
                    help="build workload: run a random-weight ViT-L/16-shaped encoder (2 crops, bf16) before every frame as a "
                         "stand-in for LSeg's per-frame cost (no weights exist here; it is NOT LSeg)")
    ap.add_argument("--no-exact-rgb", action="store_true", help="build without the per-sample replay log (no exact weight / colour)")
    ap.add_argument("--merge-mode", choices=["sharded", "reduce"], default="sharded",
                    help="multi-GPU merge of the build: row-sharded all_to_all of the ranks' own voxel rows (default) or one dense sum-reduce")
    ap.add_argument("--standin-frames", type=int, default=2048,
                    help="frames of the N > 1 extra that runs the build behind a ViT-L/16-shaped stand-in for LSeg's cost")
    ap.add_argument("--build-batch", type=int, default=1, help="frames fused per launch pair (avl_builder_integrate_batch)")
    ap.add_argument("--deferred-fuse", action="store_true",
                    help="frame-by-frame build with one launch per frame (avl_builder_set_deferred_fuse); ignored with --build-batch > 1")
    ap.add_argument("--event-mode", choices=["pair", "each"], default="pair",
                    help="HIP events around the whole timed region (pair) or between every step (each)")
    ap.add_argument("--settle-steps", type=int, default=80,
                    help="untimed launches before the warm-up so that the power controller has converged (index workload)")
    ap.add_argument("--dense", action="store_true", help="index workload: ignore the block structure of the queries (one dense pass)")
    ap.add_argument("--resident", choices=["raw", "prepared", "compact"], default="raw",
                    help="index workload: the form of the map the timed steps read (raw float32 = headline; prepared / compact = VLMap's resident copies)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="do not re-run a few steps under rocprofv3 --pmc to measure HBM traffic in the run")
    ap.add_argument("--no-build-extra", action="store_true")
    ap.add_argument("--python-frame-loop", action="store_true",
                    help="build workload, one frame per launch: call integrate_frame from Python per frame (12.4 us of host time per call) "
                         "instead of running the frame loop in C (avl_builder_integrate_frames)")
    ap.add_argument("--profile-run", action="store_true",
                    help="only the timed kernel launches (no scores_mat variant, CPU baseline or build extra): used under rocprofv3 "
                         "so that the trace's per-kernel average is the benchmarked launch")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the timed path computed in its last step (rank 0) as DIR/<name>.npy, "
                         "float32 / float64, at most 64 MB: index = the row argmax; build = the finished map, a fixed seeded "
                         "sample of rows when it has more than 16384 voxels. The inputs are seeded: the same arguments give the same inputs")
    args = ap.parse_args()
    if args.profile_run:
        args.no_cpu = args.no_build_extra = True
    if args.steps is None:
        args.steps = 500 if args.workload == "index" else 10_000     # build: north_star's 10k-frame sequence (config 4: --steps 40000)
    if args.warmup is None:
        args.warmup = 20

    import torch
    import torch.distributed as dist
    from avlmaps_amd import _lib, parallel
    rank, ws, local = parallel.init_distributed()
    if ws != args.gpus and rank == 0:
        print(f"[bench] note: WORLD_SIZE={ws} but --gpus {args.gpus}; using WORLD_SIZE", file=sys.stderr)
    torch.cuda.set_device(local)
    lib = _lib.load()
    _lib.require_gpu()
    _lib.check(lib.avl_set_device(local), "avl_set_device")

    out = run_index(args, torch, dist, lib, rank, ws) if args.workload == "index" else run_build(args, torch, dist, lib, rank, ws)
    if args.workload == "index" and not args.no_build_extra:
        # map creation next to the index line, at every N (all ranks take part: the merge is a collective): STRONG scaling of a
        # fixed `--build-frames` sequence with merge + finalize inside the timed region (see run_build_core)
        torch.cuda.empty_cache()
        try:
            r1 = run_build_core(args, torch, dist, lib, rank, ws, total_frames=args.build_frames, batch=1)
            r1d = run_build_core(args, torch, dist, lib, rank, ws, total_frames=args.build_frames, batch=1, deferred=True)
            r64 = run_build_core(args, torch, dist, lib, rank, ws, total_frames=args.build_frames, batch=64)
            if rank == 0:
                out.setdefault("extra", {})["map_build_strong"] = r1
                out["extra"]["map_build_strong_deferred_fuse"] = r1d      # frame by frame, ONE launch per frame
                out["extra"]["map_build_strong_batched64"] = r64
                if ws == 1:
                    out["extra"]["vlmapbuilder_pipeline"] = run_pipeline_probe(torch)
            if ws > 1:
                # the regime north_star's ">= 6x at 8 GPUs for map creation" is about: a per-frame extraction cost in front of the
                # fusion.  NOT LSeg (no weights here): a random-weight ViT-L/16-shaped encoder, 2 crops x 900 tokens, bf16
                nst = max(args.standin_frames, 2 * ws)
                rv = run_build_core(args, torch, dist, lib, rank, ws, total_frames=nst, batch=1, feature_standin="vit-l16")
                # north_star's wording is "a single RCCL reduce over xGMI": the same frames once more with the OTHER merge mode
                # (dense (M, D + 4) float64 sum-reduce to rank 0 when the default is the row-sharded all_to_all, and vice versa),
                # so that one --gpus N run exercises both collectives on the hardware
                other = "reduce" if getattr(args, "merge_mode", "sharded") != "reduce" else "sharded"
                ro = run_build_core(args, torch, dist, lib, rank, ws, total_frames=args.build_frames, batch=1, merge_mode=other)
                # the single-GPU reference of the SAME sequences, measured in this run by rank 0 alone while the others wait:
                # the top-level `build` block then answers north_star's strong-scaling question without a second command
                s1 = sv = None
                if rank == 0:
                    s1 = run_build_core(args, torch, dist, lib, 0, 1, total_frames=args.build_frames, batch=1, solo=True)
                    sv = run_build_core(args, torch, dist, lib, 0, 1, total_frames=nst, batch=1, feature_standin="vit-l16", solo=True)
                barrier_sync(torch, dist, ws)
                if rank == 0:
                    rv["note"] = "feature extraction is a random-weight ViT-L/16-shaped stand-in for LSeg's cost, NOT LSeg"
                    out["extra"]["map_build_strong_vit_standin"] = rv
                    out["extra"]["merge_breakdown"] = r1.get("merge_breakdown")
                    mb = r1.get("merge_breakdown") or {}
                    out["build"] = dict(
                        what=f"map creation, STRONG scaling: {args.build_frames} frames of one sequence sharded contiguously over {ws} ranks, "
                             "features resident in HBM (no extractor), merge + finalize inside the timed region",
                        metric="map_build_frames_per_sec", n_gpus=ws, frames=args.build_frames, frames_per_s=r1["frames_per_s"],
                        seconds=r1["seconds"], single_gpu_frames_per_s=s1["frames_per_s"], single_gpu_seconds=s1["seconds"],
                        speedup_vs_single_gpu=r1["frames_per_s"] / s1["frames_per_s"],
                        single_gpu_reference="the same frames fused by rank 0 alone in this run (one process, no collectives)",
                        fuse_seconds_max_rank=r1["fuse_seconds_max_rank"], merge_finalize_seconds=r1["merge_finalize_seconds"],
                        merge_breakdown={k: mb.get(k) for k in ("plan", "wall_s", "in_collectives_s", "compute_s", "compute_total_s",
                                                                "in_collectives_total_s", "merged_voxels", "local_voxels", "single_rank_voxels",
                                                                "shared_voxels_local", "payload_bytes_sent", "payload_bytes_fp64_form",
                                                                "bytes_sent_per_rank", "world_size", "backend", "exchange_chunks", "exchange_chunk_rows",
                                                                "exchange_buffer_bytes")},
                        other_merge_mode=dict(merge_mode=ro["merge_mode"], frames_per_s=ro["frames_per_s"], seconds=ro["seconds"],
                                              merge_finalize_seconds=ro["merge_finalize_seconds"], voxels_merged=ro["voxels_merged"],
                                              speedup_vs_single_gpu=ro["frames_per_s"] / s1["frames_per_s"],
                                              breakdown={k: (ro.get("merge_breakdown") or {}).get(k) for k in
                                                         ("mode", "plan_s", "scatter_s", "reduce_s", "exchange_s", "replay_chain_s", "accumulate_s",
                                                          "finalize_s", "dense_reduce_payload_bytes", "bytes_sent_per_rank")}),
                        with_extractor_standin=dict(
                            note="a random-weight ViT-L/16-shaped encoder (2 crops x 900 tokens, bf16) runs before every frame: a stand-in "
                                 "for LSeg's per-frame cost, NOT LSeg -- the regime north_star's >= 6x at 8 GPUs is about",
                            frames=nst, frames_per_s=rv["frames_per_s"], single_gpu_frames_per_s=sv["frames_per_s"],
                            speedup_vs_single_gpu=rv["frames_per_s"] / sv["frames_per_s"]),
                        pixel_sampling="per-frame sample lists are inputs of the kernel boundary here (no RNG fast-forward in the timed region); "
                                       "VLMapBuilder's pixel-faithful mode fast-forwards the global RNG first, see INTEGRATION.md (multi-GPU)")
        except Exception as e:   # the extra must never break the benchmark line
            if rank == 0:
                out.setdefault("extra", {})["map_build_strong"] = dict(error=repr(e))
    if ws > 1 or os.environ.get("AVLMAPS_FORCE_COLLECTIVES") == "1":
        # what actually carried the collectives of this run
        devs = [None] * ws
        dist.all_gather_object(devs, dict(rank=rank, local_rank=local, device=int(torch.cuda.current_device()),
                                          device_name=torch.cuda.get_device_name(), pid=os.getpid()))
        if rank == 0:
            out.setdefault("extra", {})["collectives"] = dict(backend=dist.get_backend(), world_size=dist.get_world_size(), ranks=devs,
                                                               note="backend nccl = RCCL over xGMI; gloo only when several ranks "
                                                                    "share one GPU in the tests (AVLMAPS_DIST_BACKEND)")
    if rank == 0 and ws == 1 and args.workload == "index" and not args.profile_run and not args.no_pmc:
        # HBM traffic of the headline kernels measured in THIS run, the committed file only as a fallback
        try:
            shape_argv = ["--voxels", str(args.voxels), "--queries", str(args.queries), "--feat-dim", str(args.feat_dim), "--resident", args.resident]
            shape_argv += ["--dense"] if args.dense else []
            torch.cuda.empty_cache()
            m = measure_traffic_in_run(shape_argv)
            if m is not None:
                out["roofline"].update(m)
                out["roofline"]["traffic_over_algorithmic"] = m["traffic"] / out["roofline"]["algorithmic_bytes"]
        except Exception as e:
            out["roofline"]["traffic_in_run_error"] = repr(e)
    if rank == 0:
        try:
            out["summary"] = make_summary(out)          # LAST key of the line: the driver keeps the tail of a long line
        except Exception as e:
            out["summary"] = dict(error=repr(e))
        print(json.dumps(out, default=_json_default))
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
