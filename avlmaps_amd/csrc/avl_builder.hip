// Map builder for gfx950: depth back-projection + voxelisation + distance-weighted feature fusion.
//
// Replaces the per-frame body of the upstream reference's builder loop (path:line, upstream repo root):
//   avlmaps/map/vlmap_builder.py:129-178          per-point Python loop
//   avlmaps/utils/mapping_utils.py:226-251        depth2pc            (only for the sampled pixels)
//   avlmaps/utils/mapping_utils.py:305-315        transform_pc
//   avlmaps/utils/mapping_utils.py:345-349        base_pos2grid_id_3d (fp64 divide, trunc toward zero)
//   avlmaps/utils/mapping_utils.py:599-605        project_point       (rgb pixel, LSeg pixel)
//
// This file is compiled with -ffp-contract=off: the ONLY fused multiply-adds in the index math are the
// explicit fma() calls that mirror the reference's BLAS dgemm / dgemv summation (see oracle/avl_oracle.c).
//
// Device state (all in HBM, sized for a 288 GB part -- dense tables instead of a probing hash):
//   cell_slot  int32 [gs*gs*vh]   cell -> slot (-1 empty)
//   slot_cell  int32 [cap]        slot -> linear cell
//   slot_key   uint64[cap]        first-touch key (frame << 32 | position in the frame's sample list), ~0 until known
//   sum_feat   f64   [cap, D]     sum_i alpha_i * f_i
//   sum_w4     f64   [cap, 4]     sum alpha, sum alpha*(r,g,b)
//   first_feat f32   [cap, D]     feature of the first-touch point, first_alpha f64 [cap]
//   head       int32 [cap]        per-frame list head of the samples that hit the voxel (-1 between frames)
// The reference's order-dependent result has the closed form
//   grid_feat = (sum_feat - a1*(1-a1)*first_feat) / sum_alpha,  weight = sum_alpha
// so the accumulation itself is commutative; only the first-touch point (smallest key) is special.
//
// Per launch (one frame, or the B frames of a batch) two kernels on the caller's stream, none of them serial:
//   voxelize_link_kernel, thread per sampled pixel:
//     K1 bp_voxelize  fp64 geometry; an empty cell is created by the CAS winner (slot = atomicAdd on the voxel counter)
//     K2 link         push the sample on its voxel's list (atomicExch on head); the first pusher becomes the voxel's owner
//                     for this launch.  A sample whose cell is being created by another workgroup polls for the slot
//                     (bounded; the creator needs one atomic and one store) -- K1 and K2 used to be two launches
//   fuse_kernel:
//   K3 fuse         wave per sampled pixel, owners only: walk the list, gather each member's channels-last
//                   feature row (2 KB contiguous at D=512), accumulate alpha*f in fp64 REGISTERS, then ONE plain
//                   read-modify-write of the voxel row (store-only for a voxel born this frame).  No floating-point
//                   atomics: an earlier version used 512 fp64 atomics per point and was bound by the L2 atomic rate
//                   (36 us/frame, 47 MB of write traffic for 11 MB of algorithmic RMW).  The owner also finds the
//                   voxel's first-touch sample (smallest position) when the voxel is new.
// Deferred fuse (avl_builder_set_deferred_fuse): pipe_kernel = voxelize_link of frame i + fuse of frame i - 1 in one launch.
// The frame loop in C (avl_builder_integrate_frames) additionally runs the map-independent half of K1 for frame i + 1 -- everything
// in front of the cell_slot lookup -- in workgroups of its own at the front of frame i's launch (struct PreGather,
// voxelize_link_next_kernel / pipe_kernel), so that a frame's dependent chain starts at the voxel-hash lookup.
// K1 and K3 are written as STRAIGHT-LINE code around their loads (flags and selects, full-width rows): a load inside a branch makes
// the compiler wait for everything outstanding where the branches merge, and these kernels live on having several loads in flight.
// This file is the frame path only.  Finalisation and map I/O: avl_finalize.hip; the exact-colour replay: avl_replay.hip; the state
// all three share (struct avl_builder, the per-sample records): avl_builder_state.h.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "avl_builder_state.h"
#include "avl_pinhole.h"

namespace avl {

#ifdef AVL_PROBE_CHAIN
// tools/probe_chain.py: per-work-item timestamps (s_memrealtime, 100 MHz) of the dependent-load chains of K1 + K2 and K3, taken
// AFTER the loads before them have landed.  Never compiled into the shipped library (tools/build_variant.py -DAVL_PROBE_CHAIN).
__device__ unsigned long long* g_probe = nullptr;
constexpr int kProbeK12Row0 = 16384;
#define AVL_STAMP(var)                                                                                             \
    unsigned long long var;                                                                                        \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory")
#define AVL_STAMP_DECL(var) unsigned long long var = 0
#define AVL_RESTAMP(var) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory")
#else
#define AVL_STAMP(var)
#define AVL_STAMP_DECL(var)
#define AVL_RESTAMP(var)
#endif

#ifndef AVL_K3_THREADS
#define AVL_K3_THREADS 256      // wave-per-sample K3 launches (single frames): threads per workgroup
#endif
constexpr int kFuseWaves = 128;   // K3 waves per K2 workgroup of 256 samples (more owners than that: a wave takes several)

constexpr int kEmpty = -1, kPending = -2;
constexpr int kAggregateSamples = 32768;   // launches at least this large allocate slots per workgroup instead of per wave
constexpr int kMaxPendingSpins = 1 << 18;   // link step of a deferred-fuse launch: polls of a cell that is being created

// The kernel-argument block of these kernels is 450-1 040 bytes (FrameParams alone: three 3 x 3 matrices and the pose), the
// compiler fetches it piecemeal, each piece where it is first needed and behind the branch that needs it, and every piece is a
// scalar-cache miss that goes to memory: several dependent misses at the head of every work item's chain.  Touch every line of the
// block at once, first thing in the kernels that read most of it (LINES x 64 bytes, LINES in {4, 8, 12, 16} and not beyond the segment): one miss time for all of them.
template <int LINES>
__device__ __forceinline__ void warm_kernel_arguments() {
#ifndef AVL_NO_KERNARG_WARMUP
    static_assert(LINES == 4 || LINES == 8 || LINES == 12 || LINES == 16, "four lines per step");
    const auto p = __builtin_amdgcn_kernarg_segment_ptr();     // (an address_space(4) pointer: two scalar registers)
    int t0, t1, t2, t3;
    if constexpr (LINES == 4)
        asm volatile("s_load_dword %0, %4, 0x0\n s_load_dword %1, %4, 0x40\n s_load_dword %2, %4, 0x80\n s_load_dword %3, %4, 0xc0\n"
                     "s_waitcnt lgkmcnt(0)" : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3) : "s"(p));
    if constexpr (LINES == 8)
        asm volatile("s_load_dword %0, %4, 0x0\n s_load_dword %1, %4, 0x40\n s_load_dword %2, %4, 0x80\n s_load_dword %3, %4, 0xc0\n"
                     "s_load_dword %0, %4, 0x100\n s_load_dword %1, %4, 0x140\n s_load_dword %2, %4, 0x180\n s_load_dword %3, %4, 0x1c0\n"
                     "s_waitcnt lgkmcnt(0)" : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3) : "s"(p));
    if constexpr (LINES == 12)
        asm volatile("s_load_dword %0, %4, 0x0\n s_load_dword %1, %4, 0x40\n s_load_dword %2, %4, 0x80\n s_load_dword %3, %4, 0xc0\n"
                     "s_load_dword %0, %4, 0x100\n s_load_dword %1, %4, 0x140\n s_load_dword %2, %4, 0x180\n s_load_dword %3, %4, 0x1c0\n"
                     "s_load_dword %0, %4, 0x200\n s_load_dword %1, %4, 0x240\n s_load_dword %2, %4, 0x280\n s_load_dword %3, %4, 0x2c0\n"
                     "s_waitcnt lgkmcnt(0)" : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3) : "s"(p));
    if constexpr (LINES == 16)
        asm volatile("s_load_dword %0, %4, 0x0\n s_load_dword %1, %4, 0x40\n s_load_dword %2, %4, 0x80\n s_load_dword %3, %4, 0xc0\n"
                     "s_load_dword %0, %4, 0x100\n s_load_dword %1, %4, 0x140\n s_load_dword %2, %4, 0x180\n s_load_dword %3, %4, 0x1c0\n"
                     "s_load_dword %0, %4, 0x200\n s_load_dword %1, %4, 0x240\n s_load_dword %2, %4, 0x280\n s_load_dword %3, %4, 0x2c0\n"
                     "s_load_dword %0, %4, 0x300\n s_load_dword %1, %4, 0x340\n s_load_dword %2, %4, 0x380\n s_load_dword %3, %4, 0x3c0\n"
                     "s_waitcnt lgkmcnt(0)" : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3) : "s"(p));
    (void)t0; (void)t1; (void)t2; (void)t3;
    __builtin_amdgcn_sched_barrier(0);     // (nothing of the kernel is scheduled in front of the touches)
#endif
}

// (py_int, bp_backproject and bp_transform: avl_pinhole.h, shared with the bounding-box pass and the free-space carver)
__device__ __forceinline__ double gemv3(const double* a, double x0, double x1, double x2) {
    // numpy (3,3)@(3,1) -> OpenBLAS dgemv tail:  fma(a2,x2, fma(a0,x0, a1*x1))   (oracle/avl_oracle.c)
    return fma(a[2], x2, fma(a[0], x0, a[1] * x1));
}

// what K1 leaves in registers for a fused K2 (deferred-fuse launches run both in one kernel)
struct SampleRec {
    double alpha;
    int32_t cell, fpix;
    uint32_t rgbv;
    int32_t slot;   // >= 0: the voxel's slot is already known (cell seen occupied, or created by this sample); else -1
};

// K1 body: block `blk` of a launch over fp.P samples.  Slots are published with agent-scope atomic stores so that a
// K2 running in the SAME kernel (other workgroups, other XCDs) can wait for them.
// (THREADS = the workgroup size, a compile-time constant: blockDim.x is a hidden kernel argument on a cache line of its own,
// i.e. one more scalar miss at the head of every chain)
// MODE 0: all of K1.  MODE 2: its stateless half only, for the NEXT frame, result to pre_out (PreGather).  MODE 1: the stateful half,
// starting from what a MODE-2 workgroup of the previous launch left in fp.pre.
template <int THREADS, int MODE = 0>
__device__ __forceinline__ SampleRec bp_voxelize_body(int blk, const FrameParams& fp, const float* depth,
                                                      const int32_t* __restrict__ sample_idx, const uint8_t* rgb,
                                                      int32_t* __restrict__ cell_slot, int32_t* __restrict__ slot_cell, const Recs& recs,
                                                      unsigned long long* __restrict__ counters, int* __restrict__ err_flags,
                                                      PreRec* __restrict__ pre_out = nullptr) {
    // slots are allocated per workgroup: creators are counted in LDS and ONE device atomic per 256 samples reserves the
    // block's range (a single hot device word only sustains ~90 atomics/us)
    __shared__ unsigned blk_new;
    __shared__ unsigned long long blk_base;
    if constexpr (MODE != 2) {
        if (threadIdx.x == 0) blk_new = 0;
        __syncthreads();
    }
    const int s = blk * THREADS + threadIdx.x;   // global sample index: frame-major within a batch
    const bool valid = s < fp.P;
    AVL_STAMP(pt0);
    AVL_STAMP_DECL(pt1);
    AVL_STAMP_DECL(pt2);
    AVL_STAMP_DECL(pt3);
    double alpha = 0.0;
    int32_t cell = -1, fpix = 0;
    uint32_t rgbv = 0;
    int32_t seen = kEmpty;
    bool ok = false, err_box = false, err_img = false;
    uint8_t c0 = 0, c1 = 0, c2 = 0;
    if constexpr (MODE == 1) {
        // 24 bytes per sample from the previous launch, then straight to the cell's slot
        const PreRec r = valid ? fp.pre[s] : PreRec{0.0, -1, 0, 0u, 0u};
        alpha = r.alpha;
        cell = r.cell;
        fpix = r.fpix;
        rgbv = r.rgbv;
        ok = cell >= 0;
        err_box = (r.flags & 1u) != 0;
        err_img = (r.flags & 2u) != 0;
        AVL_RESTAMP(pt1);
        seen = cell_slot[ok ? cell : 0];
        AVL_RESTAMP(pt2);
        AVL_RESTAMP(pt3);
    } else {

    // (kernel-uniform null test: a single-frame launch reads its pose from the kernel arguments, i.e. scalar registers -- selecting
    // per lane between be->t and fp.t made twelve vector loads behind twelve branches, issued only after the depth had arrived:
    // one more memory round trip on every sample's chain)
    const BatchEntry* be = fp.batch ? fp.batch + (valid ? s / fp.P_frame : 0) : nullptr;
    double T[12];
    if (be) {
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = be->t[k];
        depth = be->depth;
        rgb = be->rgb;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = fp.t[k];
    }
    const int pix = !valid ? -1 : (be ? be->samples[s % fp.P_frame] : sample_idx[s]);
    const bool ok0 = pix >= 0 && pix < fp.H * fp.W;
    AVL_RESTAMP(pt1);
    // From here to the CAS the code is STRAIGHT-LINE (flags and selects, no branch around a load): the sample's chain is depth ->
    // cell -> cell_slot, and the cell's slot is requested as soon as the cell is known; the two pinhole projections (four of the
    // seven fp64 divides), the colour gather and the weight's exp() are computed while that load is in flight.  They used to sit
    // in `if (ok)` blocks in FRONT of it: ~1.4-1.7 us of dependent fp64 arithmetic on every sample's chain (one wave per SIMD in
    // these workgroups: nothing hides it).  A sample that dropped out keeps computing on harmless values and reads element 0.
    // The arithmetic of a surviving sample is unchanged, operation for operation.
    // depth2pc: p_2d = (u + 0.5, v + 0.5, 1); pc = Kinv @ p_2d (dgemm: FMA chain over k); pc *= z
    const int pixc = ok0 ? pix : 0;
    const float* dsrc = ok0 ? depth : reinterpret_cast<const float*>(cell_slot);   // (batched launches carry no frame-level pointers)
    const double x = (double)(pixc % fp.W) + 0.5, y = (double)(pixc / fp.W) + 0.5;
    const double z = fp.depth_u16 ? (double)reinterpret_cast<const uint16_t*>(dsrc)[pixc] / fp.depth_div : (double)dsrc[pixc];
    double pl0, pl1, pl2;
    bp_backproject(fp.kinv, x, y, z, pl0, pl1, pl2);
    const bool ok1 = ok0 && (pl2 > fp.min_depth) && (pl2 < fp.max_depth);  // strict on both sides, NaN fails
    AVL_RESTAMP(pt2);
    // transform_pc: pose @ [pc; 1]  (dgemm FMA chain k = 0..3)
    double g0, g1, g2;
    bp_transform(T, pl0, pl1, pl2, g0, g1, g2);
    int row, col, h;         // (32-bit from here on: saturated values fail the range tests, in-range ones are small)
    if (fp.mode == 0) {       // (kernel-uniform)
        // base_pos2grid_id_3d: int(gs/2 - int(x/cs)) with a true fp64 divide
        row = py_int(fp.half_gs - (double)py_int(g0 / fp.cs));
        col = py_int(fp.half_gs - (double)py_int(g1 / fp.cs));
        h = py_int(g2 / fp.cs);
    } else {
        // row, height, col = np.round((p - pcd_min) / cs).astype(int)   (vlmap_builder_multi_floor.py:146; half-to-even)
        row = py_int(rint((g0 - fp.pcd_min[0]) / fp.cs));
        h = py_int(rint((g1 - fp.pcd_min[1]) / fp.cs));
        col = py_int(rint((g2 - fp.pcd_min[2]) / fp.cs));
    }
    const bool in_grid = !(col >= fp.n1 || row >= fp.n0 || h >= fp.n2 || col < 0 || row < 0 || h < 0);
    const bool ok2 = ok1 && in_grid;
    // global mode: the reference only tests the upper row/col bounds and otherwise wraps or raises; a point outside
    // the pass-1 bounding box is dropped here and reported
    err_box = ok1 && !in_grid && fp.mode == 1;
    const int32_t cell_try = ok2 ? (int32_t)(((unsigned)row * (unsigned)fp.n1 + (unsigned)col) * (unsigned)fp.n2 + (unsigned)h) : 0;
    // cell states only move forward (empty -> pending -> slot), so a slot read here is final even if the line is old
    if constexpr (MODE == 0) seen = cell_slot[cell_try];
    __builtin_amdgcn_sched_barrier(0);      // (the scheduler otherwise sinks the request below the arithmetic that follows)
    // project_point(calib, p_local) -> rgb[py, px] with numpy's negative-index wrap
    double q0 = gemv3(fp.k + 0, pl0, pl1, pl2), q1 = gemv3(fp.k + 3, pl0, pl1, pl2), q2 = gemv3(fp.k + 6, pl0, pl1, pl2);
    int px = py_int(q0 / q2 - 0.5), py = py_int(q1 / q2 - 0.5);
    px += px < 0 ? fp.W : 0;
    py += py < 0 ? fp.H : 0;
    const bool in_img = !(px < 0 || px >= fp.W || py < 0 || py >= fp.H);
    err_img = ok2 && !in_img;    // the reference raises IndexError here; we drop the point and flag it
    const bool ok3 = ok2 && in_img;
    const size_t rgb_off = ok3 ? ((size_t)py * fp.W + px) * 3 : 0;
    // the colour gather (a sample that dropped out reads element 0 of cell_slot: batched launches carry no frame-level rgb pointer)
    // (global address space stated: a FLAT load -- batched launches read the pointer from memory -- may return out of order with the
    // cell_slot load, so the wait before the CAS would have to be for both)
    using gbyte_ptr = const __attribute__((address_space(1))) uint8_t*;
    const gbyte_ptr c = (gbyte_ptr)(ok3 ? rgb + rgb_off : reinterpret_cast<const uint8_t*>(cell_slot));
    c0 = c[0];
    c1 = c[1];
    c2 = c[2];
    __builtin_amdgcn_sched_barrier(0);
    // project_point(get_sim_cam_mat(Hf, Wf), p_local) -> feature pixel, bounds-checked (vlmap_builder.py:161)
    q0 = gemv3(fp.kf + 0, pl0, pl1, pl2);
    q1 = gemv3(fp.kf + 3, pl0, pl1, pl2);
    q2 = gemv3(fp.kf + 6, pl0, pl1, pl2);
    px = py_int(q0 / q2 - 0.5);
    py = py_int(q1 / q2 - 0.5);
    ok = ok3 && !(px < 0 || py < 0 || px >= fp.Wf || py >= fp.Hf);
    if (ok2) fpix = (int32_t)((unsigned)py * (unsigned)fp.Wf + (unsigned)px);
    const double radial = (pl0 * pl0 + pl1 * pl1) + pl2 * pl2;  // np.sum(np.square(p_local))
    const double alpha_try = exp(-radial / fp.two_sigma_sq);
    if (ok) {
        alpha = alpha_try;
        cell = cell_try;
    }
    AVL_RESTAMP(pt3);
    }   // (MODE != 1)
    if constexpr (MODE == 2) {
        if (valid)
            pre_out[s] = PreRec{alpha, cell, fpix, ok ? ((uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16)) : 0u,
                                (err_box ? 1u : 0u) | (err_img ? 2u : 0u)};
        return SampleRec{};
    }
    // create the voxel if the cell is empty: the CAS winner takes the next slot.  One counter atomic per wave:
    // winners are ranked with a ballot (a single hot word only sustains ~90 atomics/us).
    int32_t known = -1;
    bool creator = false;
    if (ok) {
        if (seen == kEmpty) creator = atomicCAS(&cell_slot[cell], kEmpty, kPending) == kEmpty;
        else if (seen >= 0) known = seen;
    }
    AVL_STAMP(pt4);
    const unsigned long long cmask = __ballot(creator);
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
#ifndef AVL_K1_AGG_MIN
#define AVL_K1_AGG_MIN kAggregateSamples
#endif
    if (fp.P >= AVL_K1_AGG_MIN) {   // kernel-uniform: batched launches take the two barriers, single frames do not
        unsigned woff = 0;
        if (cmask) {
            const int leader = __ffsll((long long)cmask) - 1;
            if (lane == leader) woff = atomicAdd(&blk_new, (unsigned)__popcll(cmask));   // LDS: the wave's offset in the block
            woff = __shfl(woff, leader, 64);
        }
        __syncthreads();
        if (threadIdx.x == 0 && blk_new) blk_base = atomicAdd(&counters[0], (unsigned long long)blk_new);
        __syncthreads();
        base = blk_base + woff;
    } else if (cmask) {
        const int leader = __ffsll((long long)cmask) - 1;
        if (lane == leader) base = atomicAdd(&counters[0], (unsigned long long)__popcll(cmask));
        base = __shfl(base, leader, 64);
    }
    if (creator) {
        const unsigned long long slot = base + __popcll(cmask & ((1ull << lane) - 1ull));
        if ((long long)slot >= fp.capacity) {
            atomicOr(err_flags, 1);
            // give the cell back; its samples are dropped in K2
            __hip_atomic_store(&cell_slot[cell], kEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            slot_cell[slot] = cell;
            __hip_atomic_store(&cell_slot[cell], (int32_t)slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            known = (int32_t)slot;
        }
    }
    // (the colour bytes are first looked at HERE: the CAS above only waits for the cell's slot, the gather is still in flight then)
    if (MODE == 0 && ok) rgbv = (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16);
    if (valid) {
        recs.alpha[s] = alpha;
        recs.fpix[s] = fpix;
        recs.rgb[s] = rgbv;
    }
    if (err_box) atomicOr(err_flags, 8);
    if (err_img) atomicOr(err_flags, 2);
#ifdef AVL_PROBE_CHAIN
    {
        AVL_STAMP(pt5);
        if (g_probe && valid && fp.P < kProbeK12Row0) {
            unsigned long long* q = g_probe + (size_t)(kProbeK12Row0 + s) * 8;
            q[0] = pt0; q[1] = pt1; q[2] = pt2; q[3] = pt3; q[4] = pt4; q[5] = pt5;
        }
    }
#endif
    return SampleRec{alpha, cell, fpix, rgbv, known};
}

// K2 body.  Runs right behind K1 in the same kernel: the sample comes in registers, and a cell another workgroup is still
// creating (kPending) is waited for.  That cannot deadlock: a creator publishes its slot without waiting for anybody but
// its own workgroup's barrier (batched launches), which every wave of the workgroup reaches before it spins.
template <bool MAY_COMPACT = true, int THREADS = 256>
__device__ __forceinline__ void link_body(int blk, int P, const int32_t* __restrict__ cell_slot, int32_t* __restrict__ head,
                                          const Recs& recs, unsigned long long* __restrict__ counters, const ReplayLog& log,
                                          long long log_base, unsigned long long frame_key, const BatchEntry* __restrict__ batch,
                                          int P_frame, const SampleRec& in, int* __restrict__ err_flags, const OwnerList& ol = OwnerList{}) {
    // statistics counters are aggregated per workgroup in LDS: a single hot device word sustains only ~90 atomics/us,
    // which at one atomic per wave was most of this kernel's time in batched launches
    __shared__ unsigned blk_cnt[2];
    __shared__ unsigned sh_own[4];
    if (threadIdx.x < 2) blk_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int s = blk * THREADS + threadIdx.x;
    const bool valid = s < P;
    int32_t slot = -1, next = -1;
    uint8_t owner = 0;
    if (valid) {
        const int32_t cell = in.cell;
        if (cell >= 0) {
            {
                // most samples hit a voxel of an earlier frame: K1 has read its slot already
                slot = in.slot >= 0 ? in.slot : __hip_atomic_load(&cell_slot[cell], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // the creator needs one counter atomic and one store (~1-2 us); the cap (~0.2 s) turns a wait that should be
                // impossible into AVL_ERR_STATE at the next flag check instead of a hung device
                for (int spins = 0; slot == kPending; ++spins) {
                    if (spins >= kMaxPendingSpins) {
                        atomicOr(err_flags, 16);
                        slot = -1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                    slot = __hip_atomic_load(&cell_slot[cell], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (slot >= 0) {
                next = atomicExch(&head[slot], s);  // LIFO push; whoever finds the list empty owns it this launch
                owner = next == -1;
            }
        }
    }
    const unsigned long long amask = __ballot(slot >= 0);
    const unsigned long long omask = __ballot(owner != 0);
    if (amask && (threadIdx.x & 63) == __ffsll((long long)amask) - 1) {
        atomicAdd(&blk_cnt[0], (unsigned)__popcll(amask));
        if (omask) atomicAdd(&blk_cnt[1], (unsigned)__popcll(omask));
    }
    if (MAY_COMPACT && (threadIdx.x & 63) == 0) sh_own[threadIdx.x >> 6] = (unsigned)__popcll(omask);
    if (valid) {
        recs.slot[s] = slot;
        recs.next[s] = next;
        recs.owner[s] = owner;
        if (log.slot) {
            const long long i = log_base + s;
            log.slot[i] = slot >= 0 ? (uint32_t)slot : 0xFFFFFFFFu;
#ifdef AVL_ABL_NOLOGREC   // timing ablation only (WRONG replay): what the record store costs a frame
            if (false) {
#elif defined(AVL_LOG_UNCOND)
            {
#else
            if (slot >= 0) {     // (the replay only ever reads the records of samples that updated a voxel)
#endif
                const unsigned long long k = batch ? (batch[s / P_frame].frame_key | (unsigned)(s % P_frame)) : (frame_key | (unsigned)s);
                using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;
                u64x2* r = reinterpret_cast<u64x2*>(log.rec + i);
                r[0] = u64x2{(unsigned long long)__double_as_longlong(in.alpha), k};
                r[1] = u64x2{(unsigned long long)in.rgbv, 0ull};
            }
        }
    }
#ifdef AVL_PROBE_CHAIN
    {
        AVL_STAMP(pt7);
        if (g_probe && valid && P < kProbeK12Row0) g_probe[(size_t)(kProbeK12Row0 + s) * 8 + 7] = pt7 | ((unsigned long long)(slot >= 0) << 63);
    }
#endif
    __syncthreads();
    if (MAY_COMPACT && owner && P >= kAggregateSamples) {   // (kernel-uniform: only batched launches fuse from the compacted owners, see fuse_body)
        unsigned pos = (unsigned)__popcll(omask & ((1ull << (threadIdx.x & 63)) - 1ull));
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pos += sh_own[w];
        const size_t o = (size_t)blk * 256 + pos;
        ol.o_s[o] = s;
        ol.o_slot[o] = slot;
        ol.o_alpha[o] = in.alpha;
        ol.o_fpix[o] = in.fpix;
        ol.o_rgb[o] = in.rgbv;
    }
    if (MAY_COMPACT && P >= kAggregateSamples && threadIdx.x == 0) ol.ocnt[blk] = (int32_t)(sh_own[0] + sh_own[1] + sh_own[2] + sh_own[3]);
    if (threadIdx.x < 2 && blk_cnt[threadIdx.x]) atomicAdd(&counters[1 + threadIdx.x], (unsigned long long)blk_cnt[threadIdx.x]);
}

// K1 + K2 of one launch (a frame, or the B frames of a batch) in ONE kernel: the record stays in registers between the two
// steps, and a sample whose cell is being created by another workgroup waits for the slot instead of for a kernel boundary
__global__ __launch_bounds__(256) void voxelize_link_kernel(FrameParams fp, const float* depth, const int32_t* __restrict__ sample_idx,
                                                            const uint8_t* rgb, int32_t* __restrict__ cell_slot,
                                                            int32_t* __restrict__ slot_cell, Recs recs, int32_t* __restrict__ head,
                                                            unsigned long long* __restrict__ counters, int* __restrict__ err_flags,
                                                            ReplayLog log, long long log_base, unsigned long long frame_key, OwnerList ol) {
    warm_kernel_arguments<12>();       // (944 bytes with the hidden arguments)
    const SampleRec r = bp_voxelize_body<256>(blockIdx.x, fp, depth, sample_idx, rgb, cell_slot, slot_cell, recs, counters, err_flags);
    link_body<true, 256>(blockIdx.x, fp.P, cell_slot, head, recs, counters, log, log_base, frame_key, fp.batch, fp.P_frame, r, err_flags, ol);
}

// The same for one frame of the C frame loop (avl_builder_integrate_frames): gb workgroups in FRONT run the stateless half of K1 for
// the NEXT frame (fpn / next, see PreGather), and this frame's K1 starts from what the previous launch prepared when fp.pre is set.
__global__ __launch_bounds__(256) void voxelize_link_next_kernel(FrameParams fp, const float* depth, const int32_t* __restrict__ sample_idx,
                                                                 const uint8_t* rgb, int32_t* __restrict__ cell_slot,
                                                                 int32_t* __restrict__ slot_cell, Recs recs, int32_t* __restrict__ head,
                                                                 unsigned long long* __restrict__ counters, int* __restrict__ err_flags,
                                                                 ReplayLog log, long long log_base, unsigned long long frame_key,
                                                                 FrameParams fpn, PreGather next, int gb) {
    if ((int)blockIdx.x < gb) {
        bp_voxelize_body<256, 2>((int)blockIdx.x, fpn, next.depth, next.samples, next.rgb, cell_slot, slot_cell, recs, counters, err_flags, next.out);
        return;
    }
    const int blk = (int)blockIdx.x - gb;
    warm_kernel_arguments<12>();
    SampleRec r;
    if (fp.pre) r = bp_voxelize_body<256, 1>(blk, fp, depth, sample_idx, rgb, cell_slot, slot_cell, recs, counters, err_flags);
    else r = bp_voxelize_body<256, 0>(blk, fp, depth, sample_idx, rgb, cell_slot, slot_cell, recs, counters, err_flags);
    link_body<false, 256>(blk, fp.P, cell_slot, head, recs, counters, log, log_base, frame_key, nullptr, fp.P_frame, r, err_flags);
}

// wave per sampled point; only owners work.  CH = number of 256-float chunks kept in registers (D <= 256*CH).
// The owner sample s0 is the wave's own index and the TAIL of the LIFO list, so its record is fetched (scalar loads, the
// index is wave-uniform) together with the owner flag, and its feature row, the list head and the accumulator row go out in
// the next round trip; the rest of the list (1.3 samples per group on average) is walked from the head down to s0.
// FULL: D == 256 CH exactly (D = 512 at CH = 2, the LSeg width): every row access is an unconditional 16-byte vector access.
// With a run-time width the per-lane "does my piece of the row exist" tests are branches around the loads, and the compiler's
// s_waitcnt bookkeeping falls back to vmcnt(0) where they merge: the accumulator row, the owner's feature row and every
// member's row then arrive one after the other instead of together.
template <int CH, bool FULL>
__device__ __forceinline__ void fuse_group_impl(int s0, int32_t slot, double alpha0, int32_t fpix0, uint32_t rgb0, int P, int D_rt, unsigned long long frame_key, const BatchEntry* __restrict__ batch,
                                                int P_frame, const Recs& recs, int32_t* __restrict__ head, const float* __restrict__ feat,
                                                double* __restrict__ sum_feat, double* __restrict__ sum_w4,
                                                float* __restrict__ first_feat, double* __restrict__ first_alpha,
                                                unsigned long long* __restrict__ slot_key, uint8_t* __restrict__ dirty) {
    const int D = FULL ? 256 * CH : D_rt;
    const int lane = threadIdx.x & 63;
    AVL_STAMP(pt0);
    AVL_STAMP(pt1);
    const bool is_new = slot_key[slot] == kNoKey;  // born in this launch: accumulators hold nothing yet
    const int h0 = head[slot];
    double* sf = sum_feat + (size_t)slot * D;
    AVL_STAMP(pt2);
#ifdef AVL_PROBE_CHAIN
    int probe_n = 1;
    unsigned long long pt3 = 0, pt4 = 0;
#endif

    double acc[CH][4], old[CH][4];
    float f1[CH][4];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) { acc[c][e] = 0.0; f1[c][e] = 0.f; old[c][e] = 0.0; }
    double w4 = 0.0, a1 = 0.0, w4_old = 0.0;
    int min_s = INT_MAX;
    // the voxel's accumulator row is requested NOW, together with the first feature row, instead of after the list walk: one
    // memory round trip less on the wave's dependent chain (owner flag -> slot -> head / rows -> write).  Requesting it
    // before slot_key is known (reading the row of a new voxel too, discarding it) was measured slower: 12.5 vs 12.1 us per
    // frame, 260 vs 236 us per 64-frame launch -- the scalar loads of slot_key / head are not what the wave waits for.
    if (!is_new) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int d = c * 256 + lane * 4;
            if (FULL || (d + 3 < D && (D & 1) == 0)) {   // 16-byte aligned rows
                const double2 q0 = *reinterpret_cast<const double2*>(sf + d), q1 = *reinterpret_cast<const double2*>(sf + d + 2);
                old[c][0] = q0.x; old[c][1] = q0.y; old[c][2] = q1.x; old[c][3] = q1.y;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (d + e < D) old[c][e] = sf[d + e];
            }
        }
    }
    if (lane < 4) w4_old = is_new ? 0.0 : sum_w4[(size_t)slot * 4 + lane];

    auto row_of = [&](int cur, int32_t fpix) { return (batch ? batch[cur / P_frame].feat : feat) + (size_t)fpix * D; };
    auto load_row = [&](float (&v)[CH][4], const float* f) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int d = c * 256 + lane * 4;
            if (FULL || (d + 3 < D && (D & 3) == 0)) {
                const float4 q = *reinterpret_cast<const float4*>(f + d);
                v[c][0] = q.x; v[c][1] = q.y; v[c][2] = q.z; v[c][3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[c][e] = d + e < D ? f[d + e] : 0.f;
            }
        }
    };
    auto add = [&](int cur, double alpha, uint32_t rgbv, const float (&v)[CH][4]) {
        // The first-touch sample of a voxel BORN in this launch is kept OUT of the sum: sum_feat = sum over all OTHER samples of
        // alpha f, and the finalisation adds a1^2 f1 (the reference stores feat * alpha with weight alpha for a new voxel and
        // treats it as a mean afterwards, vlmap_builder.py:166-174).  The earlier form sum(alpha f) - a1 (1 - a1) f1 cancels
        // catastrophically for a voxel touched once from far away (alpha = exp(-r^2 / 1.2) < 1e-13 beyond ~6 m: 1 - a1 rounds to
        // 1 and the row came out as ZERO instead of a1 f1).  Members arrive in ascending sample order (up to 64 per launch), so
        // `first` normally fires once; if a smaller sample index turns up later the previous candidate rejoins the sum.
        const bool first = cur < min_s;  // wave-uniform
        const bool hold = first && is_new;
        const bool rejoin = hold && min_s != INT_MAX;
        const double a_prev = a1;
        if (first) { min_s = cur; a1 = alpha; }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (FULL || c * 256 + lane * 4 < D) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (rejoin) acc[c][e] += a_prev * (double)f1[c][e];
                    if (!hold) acc[c][e] += alpha * (double)v[c][e];
                    if (first) f1[c][e] = v[c][e];
                }
            }
        }
        if (lane < 4) w4 += lane == 0 ? alpha : alpha * (double)((rgbv >> (8 * (lane - 1))) & 0xffu);
    };
    const float* feat0 = row_of(s0, fpix0);
#ifdef AVL_ABL_K3_SINGLE      // timing ablation only (WRONG maps): every group treated as a single-sample group -- what the long groups cost
    if (true) {
#else
    if (h0 == s0) {
#endif
        float v[CH][4];
        load_row(v, feat0);
        add(s0, alpha0, rgb0, v);   // one sample for this voxel in this launch: 70 % of the groups of a single frame
#ifdef AVL_PROBE_CHAIN
        { AVL_STAMP(ptx); pt3 = pt4 = ptx; }
#endif
    } else {
        // Several samples: sum them in ASCENDING SAMPLE ORDER (the reference's order), not in the order in which their atomics
        // happened to arrive -- fp64 addition is not associative, and with the arrival order two runs of the same build could
        // differ in the last bit of a feature (seen in 1 map of 10 000).  Lane i keeps the i-th member met on the walk (the
        // owner, the tail, is member 0) and fetches its record; ranks come from n wave-wide compares; up to 64 members are
        // ordered, what is beyond (all-pixel sampling into coarse cells) is added in list order.
        // The range test and the step caps never fire: a list is a simple chain of at most P samples; they only make sure
        // that no corrupted list can keep a wave (and with it the device) busy forever.
        int my = lane == 0 ? s0 : INT_MAX;
        int n = 1, cur = h0;
        while (cur != s0 && n < 64 && (unsigned)cur < (unsigned)P) {
            if (lane == n) my = cur;
            ++n;
            cur = recs.next[cur];
        }
#ifdef AVL_PROBE_CHAIN
        { AVL_STAMP(ptx); pt3 = ptx; probe_n = n; }
#endif
        double a_l = 0.0;
        int32_t fp_l = 0;
        uint32_t rgb_l = 0;
        if (lane < n) {
            a_l = recs.alpha[my];
            fp_l = recs.fpix[my];
            rgb_l = recs.rgb[my];
        }
#ifdef AVL_PROBE_CHAIN
        { AVL_STAMP(ptx); pt4 = ptx; }
#endif
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += __builtin_amdgcn_readlane(my, j) < my ? 1 : 0;
        const int a_lo = __double2loint(a_l), a_hi = __double2hiint(a_l);
        // The rows of MR members (ranks k0 .. k0 + MR - 1) are requested TOGETHER, and unconditionally: until round 5 every member's
        // row was loaded inside its add -- one HBM round trip (1.3-1.7 us) per member -- and a load inside a branch would not do
        // either: the compiler's s_waitcnt bookkeeping falls back to vmcnt(0) where the branches merge.  Ranks beyond the group
        // re-read the owner's row (a cache hit) and are not added.  Two at a time: 73 % of the multi-sample groups of a frame are
        // pairs, and four in flight cost 16 more registers and 5-9 % in 16- / 64-frame launches, where most groups are large
        // (profiles/r05_ab_builder_k3.txt).
#ifndef AVL_K3_MR
#define AVL_K3_MR 2
#endif
        constexpr int MR = CH <= 4 ? AVL_K3_MR : 1;   // (CH = 6: 219 VGPRs already)
        for (int k0 = 0; k0 < n; k0 += MR) {
            float v[MR][CH][4];
            int cj[MR], lj[MR];
#pragma unroll
            for (int j = 0; j < MR; ++j) {
                const unsigned long long m = __ballot(lane < n && rank == k0 + j);
                lj[j] = m ? __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1) : 0;
                cj[j] = m ? __builtin_amdgcn_readlane(my, lj[j]) : -1;
                load_row(v[j], cj[j] >= 0 ? row_of(cj[j], __builtin_amdgcn_readlane(fp_l, lj[j])) : feat0);
            }
#pragma unroll
            for (int j = 0; j < MR; ++j) {
                if (cj[j] >= 0) {
                    const double al = __hiloint2double(__builtin_amdgcn_readlane(a_hi, lj[j]), __builtin_amdgcn_readlane(a_lo, lj[j]));
                    add(cj[j], al, (uint32_t)__builtin_amdgcn_readlane((int)rgb_l, lj[j]), v[j]);
                }
            }
        }
        for (int steps = 0; cur != s0 && (unsigned)cur < (unsigned)P && steps < P; ++steps) {   // members beyond the 64th
            const int nxt = recs.next[cur];
            float v[CH][4];
            load_row(v, row_of(cur, recs.fpix[cur]));
            add(cur, recs.alpha[cur], recs.rgb[cur], v);
            cur = nxt;
        }
    }

    AVL_STAMP(pt5);
    float* ff = first_feat + (size_t)slot * D;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int d = c * 256 + lane * 4;
        double r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = is_new ? acc[c][e] : old[c][e] + acc[c][e];
        if constexpr (FULL) {
            *reinterpret_cast<double2*>(sf + d) = double2{r[0], r[1]};
            *reinterpret_cast<double2*>(sf + d + 2) = double2{r[2], r[3]};
            if (is_new) *reinterpret_cast<float4*>(ff + d) = float4{f1[c][0], f1[c][1], f1[c][2], f1[c][3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (d + e < D) {
                    sf[d + e] = r[e];
                    if (is_new) ff[d + e] = f1[c][e];
                }
        }
    }
    if (lane < 4) sum_w4[(size_t)slot * 4 + lane] = w4_old + w4;
    if (is_new) {
        if (lane == 0) {
            first_alpha[slot] = a1;
            slot_key[slot] = batch ? (batch[min_s / P_frame].frame_key | (unsigned)(min_s % P_frame)) : (frame_key | (unsigned)min_s);
        }
    }
    if (lane == 0) {
        head[slot] = -1;  // ready for the next launch
        dirty[slot] = 1;  // changed since the last checkpoint (avl_builder_finalize_ex)
    }
#ifdef AVL_PROBE_CHAIN
    {
        AVL_STAMP(pt6);
        if (g_probe && lane == 0 && P < kProbeK12Row0) {
            unsigned long long* q = g_probe + (size_t)s0 * 8;
            q[0] = pt0; q[1] = pt1; q[2] = pt2; q[3] = pt3; q[4] = pt4; q[5] = pt5; q[6] = pt6;
            q[7] = (unsigned long long)probe_n | (is_new ? 1ull << 32 : 0ull);
        }
    }
#endif
}

template <int CH, bool COMPACT = false>
__device__ __forceinline__ void fuse_body(int blk, int P, int D, unsigned long long frame_key, const BatchEntry* __restrict__ batch,
                                          int P_frame, const Recs& recs, int32_t* __restrict__ head, const float* __restrict__ feat,
                                          double* __restrict__ sum_feat, double* __restrict__ sum_w4,
                                          float* __restrict__ first_feat, double* __restrict__ first_alpha,
                                          unsigned long long* __restrict__ slot_key, uint8_t* __restrict__ dirty,
                                          const OwnerList& ol = OwnerList{}) {
    auto group = [&](int s0, int32_t slot, double alpha0, int32_t fpix0, uint32_t rgb0) {
        if (D == 256 * CH)
            fuse_group_impl<CH, true>(s0, slot, alpha0, fpix0, rgb0, P, D, frame_key, batch, P_frame, recs, head, feat, sum_feat, sum_w4, first_feat,
                                      first_alpha, slot_key, dirty);
        else
            fuse_group_impl<CH, false>(s0, slot, alpha0, fpix0, rgb0, P, D, frame_key, batch, P_frame, recs, head, feat, sum_feat, sum_w4, first_feat,
                                       first_alpha, slot_key, dirty);
    };
    if constexpr (!COMPACT) {
        // a single frame (and every launch below kAggregateSamples samples): wave per SAMPLE, the owner flag fetched with the record (72 % of the waves leave here).  The compacted
        // form below measured slower at this size -- pipe_kernel 11.2 -> 12.0 us, fuse_kernel 10.35 -> 10.7 (profiles/r05_ab_builder_k3.txt s27)
        const int s0 = __builtin_amdgcn_readfirstlane((int)((blk * AVL_K3_THREADS + threadIdx.x) >> 6));   // (not blockDim.x: see bp_voxelize_body)
        if (s0 >= P) return;
        const uint8_t own = recs.owner[s0];
        const int32_t slot = recs.slot[s0];
        const double alpha0 = recs.alpha[s0];
        const int32_t fpix0 = recs.fpix[s0];
        const uint32_t rgb0 = recs.rgb[s0];
        if (!own) return;
        group(s0, slot, alpha0, fpix0, rgb0);
        return;
    } else {
    // Batched launches (a kernel of their own, so that the single-frame kernels keep their 80 registers): K3 runs over the owners K2 compacted -- half the workgroups, and +7 % at 64 frames per launch.  Wave i of
    // workgroup j takes owner entry t = i * nblk + j of the launch's nb * kFuseWaves entries (K2 workgroup t / kFuseWaves, its owner
    // t % kFuseWaves): the owners of a K2 workgroup are a PREFIX of its entries and consecutive entries go to different workgroups,
    // so every workgroup -- every CU -- gets the same mix of live and idle waves.
    const int nb = (P + 255) / 256;
    const int nblk = nb * (kFuseWaves / 4);
    const int t = (int)(threadIdx.x >> 6) * nblk + blk;
    const int b = __builtin_amdgcn_readfirstlane(t / kFuseWaves);
    if (b >= nb) return;
    const int n_own = __builtin_amdgcn_readfirstlane(ol.ocnt[b]);
    for (int k = t % kFuseWaves; k < n_own; k += kFuseWaves) {
        const int oi = __builtin_amdgcn_readfirstlane(b * 256 + k);
        // (oi is wave-uniform: scalar registers whatever kind of load the compiler picks)
        const double a0 = ol.o_alpha[oi];
        group(__builtin_amdgcn_readfirstlane(ol.o_s[oi]), __builtin_amdgcn_readfirstlane(ol.o_slot[oi]),
              __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(a0)), __builtin_amdgcn_readfirstlane(__double2loint(a0))),
              __builtin_amdgcn_readfirstlane(ol.o_fpix[oi]), (uint32_t)__builtin_amdgcn_readfirstlane((int)ol.o_rgb[oi]));
    }
    }
}

#ifndef AVL_K3_WPE
#define AVL_K3_WPE 0
#endif
#if AVL_K3_WPE
#define AVL_K3_OCC(CH) __attribute__((amdgpu_waves_per_eu((CH) <= 2 ? AVL_K3_WPE : 1)))
#else
#define AVL_K3_OCC(CH)
#endif

template <int CH, bool COMPACT>
__global__ __launch_bounds__(COMPACT ? 256 : AVL_K3_THREADS) AVL_K3_OCC(CH) void fuse_kernel(int P, int D, unsigned long long frame_key, const BatchEntry* __restrict__ batch,
                                                   int P_frame, Recs recs, int32_t* __restrict__ head, const float* __restrict__ feat,
                                                   double* __restrict__ sum_feat, double* __restrict__ sum_w4,
                                                   float* __restrict__ first_feat, double* __restrict__ first_alpha,
                                                   unsigned long long* __restrict__ slot_key, uint8_t* __restrict__ dirty, OwnerList ol) {
    fuse_body<CH, COMPACT>(blockIdx.x, P, D, frame_key, batch, P_frame, recs, head, feat, sum_feat, sum_w4, first_feat, first_alpha, slot_key, dirty, ol);
}

// Deferred-fuse launch (avl_builder_set_deferred_fuse): ONE kernel per frame.  Workgroups [0, pb) run K1 + K2 of the NEW frame
// (records into recs / lists into head), the others run K3 of the PREVIOUS frame (prev_recs / prev_head, the other halves of
// the double buffers).  The two touch disjoint state: K1/K2 use cell_slot, slot_cell, the slot counter and the new frame's
// buffers; K3 uses the accumulators, slot_key, dirty and the previous frame's buffers.
struct FusePrev {
    int P;                       // 0: nothing pending
    unsigned long long frame_key;
    Recs recs;
    int32_t* head;
    const float* feat;
};

template <int CH>
__global__ __launch_bounds__(AVL_K3_THREADS) AVL_K3_OCC(CH) void pipe_kernel(FrameParams fp, int pb, const float* depth, const int32_t* __restrict__ sample_idx,
                                                   const uint8_t* rgb, int32_t* __restrict__ cell_slot, int32_t* __restrict__ slot_cell,
                                                   Recs recs, int32_t* __restrict__ head, unsigned long long* __restrict__ counters,
                                                   int* __restrict__ err_flags, ReplayLog log, long long log_base,
                                                   unsigned long long frame_key, FusePrev prev, int D, double* __restrict__ sum_feat,
                                                   double* __restrict__ sum_w4, float* __restrict__ first_feat,
                                                   double* __restrict__ first_alpha, unsigned long long* __restrict__ slot_key,
                                                   uint8_t* __restrict__ dirty, FrameParams fpn, PreGather next, int gb) {
    if ((int)blockIdx.x < gb) {                   // (in front of K1 + K2's and K3's workgroups: the stateless half of the NEXT frame's K1)
        bp_voxelize_body<AVL_K3_THREADS, 2>((int)blockIdx.x, fpn, next.depth, next.samples, next.rgb, cell_slot, slot_cell, recs, counters, err_flags,
                                            next.out);
        return;
    }
    const int blk = (int)blockIdx.x - gb;
    if (blk < pb) {
        warm_kernel_arguments<12>();   // (K1 + K2 read FrameParams and a dozen pointers; a K3 wave needs two lines, and touching more
                                       // costs it: fuse_kernel 10.4-10.7 -> 10.9-11.1 us, 64 frames per launch 230 -> 255 us)
        SampleRec r;
        if (fp.pre) r = bp_voxelize_body<AVL_K3_THREADS, 1>(blk, fp, depth, sample_idx, rgb, cell_slot, slot_cell, recs, counters, err_flags);
        else r = bp_voxelize_body<AVL_K3_THREADS, 0>(blk, fp, depth, sample_idx, rgb, cell_slot, slot_cell, recs, counters, err_flags);
        link_body<false, AVL_K3_THREADS>(blk, fp.P, cell_slot, head, recs, counters, log, log_base, frame_key, nullptr, fp.P_frame, r, err_flags);
    } else {
        fuse_body<CH>(blk - pb, prev.P, D, prev.frame_key, nullptr, prev.P, prev.recs, prev.head, prev.feat, sum_feat, sum_w4,
                      first_feat, first_alpha, slot_key, dirty);
    }
}

// generic feature width (D > 1536).  A voxel's samples are summed in ASCENDING SAMPLE ORDER like fuse_group_impl does, so that two runs
// of a build give the same bits: the wave orders up to 64 members at a time (ranks from wave-wide compares, the order parked in LDS)
// and adds them 64 columns x kGenTile column groups at a time from registers; a list of more than 64 members is taken in ROUNDS -- every
// round re-walks it and keeps the 64 smallest sample indices above the previous round's largest -- whose partial sums are added to the
// row one after the other (a fixed association, whatever order the atomics of K2 arrived in).
constexpr int kGenTile = 8;
__global__ __launch_bounds__(256) void fuse_generic_kernel(int P, int D, unsigned long long frame_key,
                                                           const BatchEntry* __restrict__ batch, int P_frame, Recs recs,
                                                           int32_t* __restrict__ head, const float* __restrict__ feat,
                                                           double* __restrict__ sum_feat, double* __restrict__ sum_w4,
                                                           float* __restrict__ first_feat, double* __restrict__ first_alpha,
                                                           unsigned long long* __restrict__ slot_key, uint8_t* __restrict__ dirty) {
    __shared__ int ord_s[4][64];
    const int lane = threadIdx.x & 63;
    int* ord = ord_s[(threadIdx.x >> 6) & 3];
    const int s0 = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (s0 >= P) return;
    if (!recs.owner[s0]) return;
    const int32_t slot = recs.slot[s0];
    const bool is_new = slot_key[slot] == kNoKey;
    const int h0 = head[slot];
    auto wave_max = [&](int v) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
        return v;
    };
    // one walk: the size of the list, its smallest sample (the first touch) and -- all a short list needs -- its first 64 members
    int n_total = 0, min_s = INT_MAX, held = INT_MAX;
    for (int cur = h0; cur >= 0 && (unsigned)cur < (unsigned)P && n_total < P; cur = recs.next[cur]) {
        if (n_total < 64 && lane == n_total) held = cur;
        min_s = min(min_s, cur);
        ++n_total;
    }
    if (n_total == 0) return;      // (a corrupted list: never -- the owner is on its own list)
    const double a1 = recs.alpha[min_s];
    const float* row1 = (batch ? batch[min_s / P_frame].feat : feat) + (size_t)recs.fpix[min_s] * D;
    double* sf = sum_feat + (size_t)slot * D;
    float* ff = first_feat + (size_t)slot * D;
    if (is_new)
        for (int d = lane; d < D; d += 64) ff[d] = row1[d];
    double w4 = 0.0;
    int prev = -1;
    bool first_round = true;
    for (int done = 0; done < n_total;) {
        int m;
        if (n_total <= 64) {
            m = n_total;
        } else {
            // the 64 smallest sample indices above `prev`: lanes fill up, then a smaller newcomer replaces the largest one held
            held = INT_MAX;
            int cnt = 0, curmax = -1, steps = 0;
            for (int cur = h0; cur >= 0 && (unsigned)cur < (unsigned)P && steps < P; cur = recs.next[cur], ++steps) {
                if (cur <= prev) continue;
                if (cnt < 64) {
                    if (lane == cnt) held = cur;
                    if (++cnt == 64) curmax = wave_max(held);
                } else if (cur < curmax) {
                    const unsigned long long at = __ballot(held == curmax);
                    if (lane == __ffsll((long long)at) - 1) held = cur;
                    curmax = wave_max(held);
                }
            }
            m = cnt;
            if (m == 0) break;     // (a corrupted list: never)
        }
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += __builtin_amdgcn_readlane(held, j) < held ? 1 : 0;
        if (lane < m) ord[rank] = held;
        __builtin_amdgcn_wave_barrier();
        prev = ord[m - 1];
        for (int k = 0; k < m; ++k) {
            const int cur = ord[k];
            const double alpha = recs.alpha[cur];
            const uint32_t rgbv = recs.rgb[cur];
            if (lane < 4) w4 += lane == 0 ? alpha : alpha * (double)((rgbv >> (8 * (lane - 1))) & 0xffu);
        }
        for (int d0 = 0; d0 < D; d0 += 64 * kGenTile) {
            double acc[kGenTile];
#pragma unroll
            for (int t = 0; t < kGenTile; ++t) acc[t] = 0.0;
            for (int k = 0; k < m; ++k) {
                const int cur = ord[k];
                if (is_new && cur == min_s) continue;            // the first touch of a new voxel stays out of the sum (fuse_group_impl)
                const double alpha = recs.alpha[cur];
                const float* row = (batch ? batch[cur / P_frame].feat : feat) + (size_t)recs.fpix[cur] * D;
#pragma unroll
                for (int t = 0; t < kGenTile; ++t) {
                    const int d = d0 + t * 64 + lane;
                    if (d < D) acc[t] += alpha * (double)row[d];
                }
            }
#pragma unroll
            for (int t = 0; t < kGenTile; ++t) {
                const int d = d0 + t * 64 + lane;
                if (d < D) sf[d] = (is_new && first_round) ? acc[t] : sf[d] + acc[t];
            }
        }
        __builtin_amdgcn_wave_barrier();
        done += m;
        first_round = false;
    }
    if (lane < 4) {
        double* w = sum_w4 + (size_t)slot * 4 + lane;
        *w = is_new ? w4 : *w + w4;
    }
    if (lane == 0) {
        if (is_new) {
            first_alpha[slot] = a1;
            slot_key[slot] = batch ? (batch[min_s / P_frame].frame_key | (unsigned)(min_s % P_frame)) : (frame_key | (unsigned)min_s);
        }
        head[slot] = -1;
        dirty[slot] = 1;
    }
}

}  // namespace avl

using namespace avl;

// the parameters the stateless half of K1 reads (everything of FrameParams up to the grid shape, the mode; not pre / capacity / batch)
static bool same_geometry(const FrameParams& a, const FrameParams& b) {
    return std::memcmp(&a, &b, offsetof(FrameParams, batch)) == 0 && a.P_frame == b.P_frame && a.mode == b.mode && a.depth_u16 == b.depth_u16;
}

static int builder_check_flags(avl_builder* b, hipStream_t st) {
    int flags = 0;
    AVL_HIP_CHECK(hipMemcpyAsync(&flags, b->err_flags, sizeof(int), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    if (flags & 1) {
        set_error("voxel capacity %lld exhausted: create the builder with a larger capacity", (long long)b->capacity);
        return AVL_ERR_CAPACITY;
    }
    if (flags & 2) {
        set_error("a sampled point projected outside the RGB image (the reference raises IndexError here)");
        return AVL_ERR_INVALID;
    }
    if (flags & 16) {
        set_error("internal error: a voxel under creation was never published to the samples waiting for it (deferred fuse)");
        return AVL_ERR_STATE;
    }
    return AVL_OK;   // bit 8 (global mode: samples outside the pass-1 bounding box were dropped) is informational
}

static int read_counter(avl_builder* b, int which, int64_t* h_n, hipStream_t st) {
    unsigned long long v = 0;
    AVL_HIP_CHECK(hipMemcpyAsync(&v, b->counters + which, sizeof(v), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    *h_n = (int64_t)v;
    return AVL_OK;
}

static int ensure_recs(avl_builder* b, int P, hipStream_t st) {
    if (P <= b->recs_cap) return AVL_OK;
    int rc = flush_pending(b, st);   // the pending frame's records live in the buffers about to be freed
    if (rc != AVL_OK) return rc;
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    if (b->recs_mem) AVL_HIP_CHECK(hipFree(b->recs_mem));
    b->recs_mem = nullptr;
    const size_t cap = ((size_t)P + P / 4 + 1024 + 255) / 256 * 256;
    const size_t one = (cap * (8 + 4 * 4 + 1) + 255) / 256 * 256;
    const size_t own = (cap * (8 + 4 * 4) + (cap / 256 + 1) * 4 + 255) / 256 * 256;
    const size_t pre = (cap * sizeof(PreRec) + 255) / 256 * 256;
    AVL_HIP_CHECK(hipMalloc((void**)&b->recs_mem, 2 * one + own + 2 * pre));
    auto carve = [&](Recs& r, char* p) {
        r.alpha = reinterpret_cast<double*>(p); p += cap * 8;
        r.slot = reinterpret_cast<int32_t*>(p); p += cap * 4;
        r.fpix = reinterpret_cast<int32_t*>(p); p += cap * 4;
        r.rgb = reinterpret_cast<uint32_t*>(p); p += cap * 4;
        r.next = reinterpret_cast<int32_t*>(p); p += cap * 4;
        r.owner = reinterpret_cast<uint8_t*>(p);
    };
    carve(b->recs, b->recs_mem);
    carve(b->recs_alt, b->recs_mem + one);
    {
        char* p = b->recs_mem + 2 * one;
        OwnerList& o = b->owners;
        o.o_alpha = reinterpret_cast<double*>(p); p += cap * 8;
        o.o_s = reinterpret_cast<int32_t*>(p); p += cap * 4;
        o.o_slot = reinterpret_cast<int32_t*>(p); p += cap * 4;
        o.o_fpix = reinterpret_cast<int32_t*>(p); p += cap * 4;
        o.o_rgb = reinterpret_cast<uint32_t*>(p); p += cap * 4;
        o.ocnt = reinterpret_cast<int32_t*>(p);
    }
    b->pre_buf[0] = reinterpret_cast<PreRec*>(b->recs_mem + 2 * one + own);
    b->pre_buf[1] = reinterpret_cast<PreRec*>(b->recs_mem + 2 * one + own + pre);
    b->pre_held.valid = false;
    b->recs_cap = (int)cap;
    return AVL_OK;
}

// The reference doubles its arrays when max_id reaches their length (_reserve_map_space, vlmap_builder.py:286-311).  Here the
// per-slot arrays are reallocated at (at least) twice the size and copied device-to-device; cell_slot is indexed by cell and
// does not change.  Called between launches only (stream drained first).
int avl::grow_builder(avl_builder* b, int64_t want, hipStream_t st) {
    // `want` is a worst-case bound (every sample of the next launch creates a voxel): grow as far as allowed; if the map
    // really outgrows max_capacity the kernel's own overflow flag reports it (AVL_ERR_CAPACITY at the next counter read)
    int64_t cap = b->capacity;
    while (cap < want) cap *= 2;
    if (cap > b->max_capacity) cap = b->max_capacity;
    if (cap <= b->capacity) return AVL_OK;
    int rcf = flush_pending(b, st);
    if (rcf != AVL_OK) return rcf;
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    const size_t oc = (size_t)b->capacity, nc = (size_t)cap, D = (size_t)b->D;
    auto regrow = [&](void** p, size_t elem, int fill) -> hipError_t {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, nc * elem);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(q, *p, oc * elem, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && fill >= 0) e = hipMemsetAsync(static_cast<char*>(q) + oc * elem, fill, (nc - oc) * elem, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(q); return e; }
        (void)hipFree(*p);
        *p = q;
        return hipSuccess;
    };
    hipError_t e = regrow((void**)&b->slot_cell, sizeof(int32_t), 0xFF);
    if (e == hipSuccess) e = regrow((void**)&b->slot_key, sizeof(unsigned long long), 0xFF);
    if (e == hipSuccess) e = regrow((void**)&b->head, sizeof(int32_t), 0xFF);
    if (e == hipSuccess) e = regrow((void**)&b->head_alt, sizeof(int32_t), 0xFF);
    if (e == hipSuccess) e = regrow((void**)&b->dirty, 1, 0);
    if (e == hipSuccess) e = regrow((void**)&b->sum_feat, D * sizeof(double), -1);
    if (e == hipSuccess) e = regrow((void**)&b->sum_w4, 4 * sizeof(double), -1);
    if (e == hipSuccess) e = regrow((void**)&b->first_feat, D * sizeof(float), -1);
    if (e == hipSuccess) e = regrow((void**)&b->first_alpha, sizeof(double), -1);
    if (e != hipSuccess) {
        set_error("growing the voxel accumulators from %lld to %lld voxels failed: %s", (long long)b->capacity, (long long)cap,
                  hipGetErrorString(e));
        return AVL_ERR_HIP;   // arrays already regrown keep their new size; the handle stays usable at the old capacity
    }
    b->capacity = cap;
    return AVL_OK;
}

// K3 over one launch's records (CH = 256-float register chunks of a feature row)
// `owners_compacted`: the K2 that produced `recs` was voxelize_link_kernel with b->owners (it compacts iff P >= kAggregateSamples);
// pipe_kernel's and voxelize_link_next_kernel's K2 never write the OwnerList, so their K3 is always wave-per-sample
static int launch_fuse(avl_builder* b, int P, unsigned long long frame_key, const BatchEntry* batch, int P_frame, const Recs& recs,
                       int32_t* head, const float* d_feat, hipStream_t st, bool owners_compacted) {
    // batched launches run over the owners K2 compacted; single frames and the generic kernel: wave per sample
    const bool compact = owners_compacted && b->D <= 1536 && P >= kAggregateSamples;
    constexpr int kWaves = AVL_K3_THREADS / 64;
    const unsigned wb = compact ? (unsigned)((P + 255) / 256) * (kFuseWaves / 4) : (unsigned)((P + kWaves - 1) / kWaves);
    const unsigned wb_generic = (unsigned)((P + 256 / 64 - 1) / (256 / 64));     // (fuse_generic_kernel has 256 threads whatever AVL_K3_THREADS is)
#define AVL_FUSE_LAUNCH(CH)                                                                                                              \
    do {                                                                                                                                 \
        if (compact)                                                                                                                     \
            hipLaunchKernelGGL((fuse_kernel<CH, true>), dim3(wb), dim3(256), 0, st, P, b->D, frame_key, batch, P_frame, recs, head, d_feat,  \
                               b->sum_feat, b->sum_w4, b->first_feat, b->first_alpha, b->slot_key, b->dirty, b->owners);                 \
        else                                                                                                                             \
            hipLaunchKernelGGL((fuse_kernel<CH, false>), dim3(wb), dim3(AVL_K3_THREADS), 0, st, P, b->D, frame_key, batch, P_frame, recs, head, d_feat, \
                               b->sum_feat, b->sum_w4, b->first_feat, b->first_alpha, b->slot_key, b->dirty, OwnerList{});               \
    } while (0)
    if (b->D <= 256) AVL_FUSE_LAUNCH(1);
    else if (b->D <= 512) AVL_FUSE_LAUNCH(2);
    else if (b->D == 768) AVL_FUSE_LAUNCH(3);      // CLIP ViT-L: three full chunks (the full-width path: unconditional row accesses)
    else if (b->D <= 1024) AVL_FUSE_LAUNCH(4);
    else if (b->D <= 1536) AVL_FUSE_LAUNCH(6);     // a fused visual | audio map (512 + 1024 columns, BASELINE config 5)
    else
        hipLaunchKernelGGL(fuse_generic_kernel, dim3(wb_generic), dim3(256), 0, st, P, b->D, frame_key, batch, P_frame, recs, head, d_feat,
                           b->sum_feat, b->sum_w4, b->first_feat, b->first_alpha, b->slot_key, b->dirty);
#undef AVL_FUSE_LAUNCH
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

// deferred fuse: run the K3 that is still owed (on `st`, which must be the stream the frame was integrated on)
int avl::flush_pending(avl_builder* b, hipStream_t st) {
    if (b->pend.P == 0) return AVL_OK;
    const int P = b->pend.P;
    b->pend.P = 0;
    return launch_fuse(b, P, b->pend.frame_key, nullptr, P, b->recs_alt, b->head_alt, b->pend.feat, st, /*owners_compacted=*/false);
}

template <int CH>
static void launch_pipe(avl_builder* b, const FrameParams& fp, unsigned pb, const void* d_depth, const int32_t* d_sample_idx,
                        const uint8_t* d_rgb, unsigned long long frame_key, const FusePrev& prev, hipStream_t st, const FrameParams& fpn,
                        const PreGather& next) {
    constexpr int kWaves = AVL_K3_THREADS / 64;
    const unsigned wb = prev.P ? (unsigned)((prev.P + kWaves - 1) / kWaves) : 0u;
    const unsigned gb = next.out ? (unsigned)((fpn.P + AVL_K3_THREADS - 1) / AVL_K3_THREADS) : 0u;
    hipLaunchKernelGGL(pipe_kernel<CH>, dim3(pb + wb + gb), dim3(AVL_K3_THREADS), 0, st, fp, (int)pb, reinterpret_cast<const float*>(d_depth), d_sample_idx,
                       d_rgb, b->cell_slot, b->slot_cell, b->recs, b->head, b->counters, b->err_flags, b->log, b->log_used, frame_key, prev,
                       b->D, b->sum_feat, b->sum_w4, b->first_feat, b->first_alpha, b->slot_key, b->dirty, fpn, next, (int)gb);
}

extern "C" {

#ifdef AVL_PROBE_CHAIN
__attribute__((visibility("default"))) int avl_debug_set_probe(void* d_buf) {
    AVL_HIP_CHECK(hipDeviceSynchronize());
    unsigned long long* p = reinterpret_cast<unsigned long long*>(d_buf);
    AVL_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(avl::g_probe), &p, sizeof(p)));
    return AVL_OK;
}
#endif

int avl_builder_reset(avl_builder* b, void* stream) {
    AVL_REQUIRE(b, "avl_builder_reset: null handle");
    hipStream_t st = as_stream(stream);
    // sum_feat / sum_w4 / first_* need no clearing: a voxel's first fuse is store-only
    AVL_HIP_CHECK(hipMemsetAsync(b->cell_slot, 0xFF, b->ncell * sizeof(int32_t), st));
    AVL_HIP_CHECK(hipMemsetAsync(b->head, 0xFF, (size_t)b->capacity * sizeof(int32_t), st));
    AVL_HIP_CHECK(hipMemsetAsync(b->head_alt, 0xFF, (size_t)b->capacity * sizeof(int32_t), st));
    b->pend = avl_builder::Pending{};   // a pending frame is dropped with the rest of the map
    b->pre_held.valid = false;
    AVL_HIP_CHECK(hipMemsetAsync(b->dirty, 0, (size_t)b->capacity, st));
    AVL_HIP_CHECK(hipMemsetAsync(b->slot_cell, 0xFF, (size_t)b->capacity * sizeof(int32_t), st));
    AVL_HIP_CHECK(hipMemsetAsync(b->slot_key, 0xFF, (size_t)b->capacity * sizeof(unsigned long long), st));
    AVL_HIP_CHECK(hipMemsetAsync(b->counters, 0, 4 * sizeof(unsigned long long), st));
    AVL_HIP_CHECK(hipMemsetAsync(b->err_flags, 0, sizeof(int), st));
    b->key_bias = 0;
    b->log_used = 0;
    b->vox_bound = 0;
    drop_log_segments(b, st);
    return AVL_OK;
}

int avl_builder_destroy(avl_builder* b) {
    if (!b) return AVL_OK;
    drop_log_segments(b, nullptr);
    (void)hipFree(b->cell_slot); (void)hipFree(b->slot_cell); (void)hipFree(b->slot_key); (void)hipFree(b->sum_feat);
    (void)hipFree(b->sum_w4); (void)hipFree(b->first_feat); (void)hipFree(b->first_alpha); (void)hipFree(b->head);
    (void)hipFree(b->head_alt);
    (void)hipFree(b->dirty);
    (void)hipFree(b->counters); (void)hipFree(b->err_flags); (void)hipFree(b->recs_mem);
    (void)hipFree(b->log.slot); (void)hipFree(b->log.rec);
    (void)hipFree(b->rs_mem);
    (void)hipFree(b->d_table);
    delete b;
    return AVL_OK;
}

int avl_builder_create_grid(avl_builder** h_out, int n0, int gs, int vh, double cs, int D, int64_t capacity) {
    AVL_REQUIRE(h_out, "avl_builder_create: null output");
    *h_out = nullptr;
    avl::keep_mempool_once();
    avl_merge2_load();      // (the merge's kernels live in another code object: loaded with the builder, not inside the first merge)
    AVL_REQUIRE(n0 > 0 && gs > 0 && vh > 0 && D > 0 && cs > 0 && capacity > 0, "avl_builder_create: bad parameters");
    const double ncell_d = (double)n0 * gs * vh;
    AVL_REQUIRE(ncell_d < 2.0e9, "avl_builder_create: gs*gs*vh = %.0f cells exceeds the int32 cell index", ncell_d);
    AVL_REQUIRE(capacity < (1ll << 31), "avl_builder_create: capacity must fit int32 voxel ids");
    avl_builder* b = new avl_builder();
    b->n0 = n0; b->gs = gs; b->vh = vh; b->D = D; b->cs = cs; b->capacity = capacity;
    b->ncell = (size_t)n0 * gs * vh;
    hipError_t e = hipSuccess;
    auto alloc = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    alloc((void**)&b->cell_slot, b->ncell * sizeof(int32_t));
    alloc((void**)&b->slot_cell, (size_t)capacity * sizeof(int32_t));
    alloc((void**)&b->slot_key, (size_t)capacity * sizeof(unsigned long long));
    alloc((void**)&b->sum_feat, (size_t)capacity * D * sizeof(double));
    alloc((void**)&b->sum_w4, (size_t)capacity * 4 * sizeof(double));
    alloc((void**)&b->first_feat, (size_t)capacity * D * sizeof(float));
    alloc((void**)&b->first_alpha, (size_t)capacity * sizeof(double));
    alloc((void**)&b->head, (size_t)capacity * sizeof(int32_t));
    alloc((void**)&b->head_alt, (size_t)capacity * sizeof(int32_t));
    alloc((void**)&b->dirty, (size_t)capacity);
    alloc((void**)&b->counters, 4 * sizeof(unsigned long long));
    alloc((void**)&b->err_flags, sizeof(int));
    if (e != hipSuccess) {
        set_error("avl_builder_create: hipMalloc failed: %s (capacity %lld x D %d)", hipGetErrorString(e), (long long)capacity, D);
        avl_builder_destroy(b);
        return AVL_ERR_HIP;
    }
    int rc = avl_builder_reset(b, nullptr);
    if (rc == AVL_OK && hipDeviceSynchronize() != hipSuccess) rc = AVL_ERR_HIP;
    if (rc != AVL_OK) {
        avl_builder_destroy(b);
        return rc;
    }
    *h_out = b;
    return AVL_OK;
}

int avl_builder_enable_replay_log(avl_builder* b, int64_t max_samples) {
    AVL_REQUIRE(b && max_samples > 0, "avl_builder_enable_replay_log: bad arguments");
    AVL_REQUIRE(max_samples < (1ll << 31), "avl_builder_enable_replay_log: at most 2^31 - 1 samples");
    AVL_HIP_CHECK(hipDeviceSynchronize());
    if (b->log_used != 0) {
        set_error("avl_builder_enable_replay_log: frames were already fused; enable the log on a fresh or reset builder");
        return AVL_ERR_STATE;
    }
    (void)hipFree(b->log.slot); (void)hipFree(b->log.rec);
    b->log = ReplayLog{};
    b->log_cap = 0;
    hipError_t e = hipMalloc((void**)&b->log.slot, (size_t)max_samples * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&b->log.rec, (size_t)max_samples * sizeof(LogRec));
    if (e != hipSuccess) {
        (void)hipFree(b->log.slot); (void)hipFree(b->log.rec);
        b->log = ReplayLog{};
        set_error("avl_builder_enable_replay_log: hipMalloc failed: %s", hipGetErrorString(e));
        return AVL_ERR_HIP;
    }
    b->log_cap = max_samples;
    // the log's slot-sorted form (LogSegments: two words per sample + two per ACTIVE sample + the radix sort's storage) lives next to
    // the log itself: allocated here, not inside the first finalisation / merge
    (void)hipFree(b->rs_mem);
    b->rs_mem = nullptr;
    b->rs_bytes = b->rs_tmp_bytes = 0;
    if (const size_t tb = replay_sort_tmp_bytes(max_samples)) {
        const size_t w = ((size_t)max_samples * 4 + 255) / 256 * 256;
        const size_t total = 4 * w + (tb + 255) / 256 * 256 + 256;
        if (hipMalloc((void**)&b->rs_mem, total) == hipSuccess) {
            b->rs_bytes = total;
            b->rs_tmp_bytes = (tb + 255) / 256 * 256;
        } else {
            b->rs_mem = nullptr;      // (not fatal: LogSegments falls back to the stream-ordered pool)
            (void)hipGetLastError();
        }
    }
    return AVL_OK;
}

int avl_builder_set_max_capacity(avl_builder* b, int64_t max_capacity) {
    AVL_REQUIRE(b, "avl_builder_set_max_capacity: null handle");
    AVL_REQUIRE(max_capacity == 0 || (max_capacity >= b->capacity && max_capacity < (1ll << 31)),
                "avl_builder_set_max_capacity: must be 0 (fixed) or in [capacity, 2^31)");
    b->max_capacity = max_capacity;
    return AVL_OK;
}

int avl_builder_capacity(avl_builder* b, int64_t* h_capacity) {
    AVL_REQUIRE(b && h_capacity, "avl_builder_capacity: null argument");
    *h_capacity = b->capacity;
    return AVL_OK;
}

int avl_builder_create(avl_builder** h_out, int gs, double cs, int vh, int D, int64_t capacity) {
    return avl_builder_create_grid(h_out, gs, gs, vh, cs, D, capacity);
}

// B == 0: one frame, pointers passed directly.  B > 0: h_*_ptrs[B] give the per-frame device buffers, h_pc_transform holds B 4x4s,
// frames frame_idx .. frame_idx + B - 1 are fused by ONE K1/K2/K3 triple (samples of a voxel from different frames share one list).
static int integrate_impl(avl_builder* b, const void* d_depth, int depth_u16, double depth_div, int H, int W, const double* h_calib,
                          const double* h_calib_inv, const double* h_pc_transform, const int32_t* d_sample_idx, int P,
                          const float* d_feat, int Hf, int Wf, const uint8_t* d_rgb, int64_t frame_idx, double min_depth,
                          double max_depth, double sigma_sq, const double* h_pcd_min, void* stream, int B = 0,
                          const void* const* h_depth_ptrs = nullptr, const int32_t* const* h_sample_ptrs = nullptr,
                          const float* const* h_feat_ptrs = nullptr, const uint8_t* const* h_rgb_ptrs = nullptr) {
    AVL_REQUIRE(b, "avl_builder_integrate_frame: null handle");
    // the records a previous launch prepared are good for THIS call only: whatever path leaves this function (errors included),
    // a later call must not find them (the ring slot they were read from may hold another frame by then)
    const auto held = b->pre_held;
    b->pre_held.valid = false;
    AVL_REQUIRE(H > 0 && W > 0 && Hf > 0 && Wf > 0 && P >= 0, "avl_builder_integrate_frame: bad shape");
    AVL_REQUIRE(P < (1 << 30), "avl_builder_integrate_frame: at most 2^30 samples per frame");
    AVL_REQUIRE(B >= 0 && (int64_t)(B > 0 ? B : 1) * P < (1ll << 30), "avl_builder_integrate_batch: at most 2^30 samples per launch");
    AVL_REQUIRE(frame_idx >= 0 && frame_idx + B < (1ll << 30), "avl_builder_integrate_frame: bad frame_idx");
    AVL_REQUIRE(sigma_sq > 0, "avl_builder_integrate_frame: sigma_sq must be positive");
    if (P == 0) return AVL_OK;
    AVL_REQUIRE(h_calib && h_calib_inv && h_pc_transform, "avl_builder_integrate_frame: null pointer");
    if (B == 0) AVL_REQUIRE(d_depth && d_sample_idx && d_feat && d_rgb, "avl_builder_integrate_frame: null pointer");
    else AVL_REQUIRE(h_depth_ptrs && h_sample_ptrs && h_feat_ptrs && h_rgb_ptrs, "avl_builder_integrate_batch: null pointer table");
    hipStream_t st = as_stream(stream);
    const int P_frame = P;
    if (B > 0) P = B * P_frame;   // total samples of the launch
    int rc = ensure_recs(b, P, st);
    if (rc != AVL_OK) return rc;
    // worst case every sample of this launch creates a voxel: when the host-side bound reaches the capacity, read the real
    // counter (one sync, rare: the bound advances ~20x faster than the map) and double the accumulators if it is really close
    if (b->max_capacity > b->capacity && b->vox_bound + P > b->capacity) {
        int64_t have = 0;
        rc = read_counter(b, 0, &have, st);
        if (rc != AVL_OK) return rc;
        b->vox_bound = have;
        int64_t need = have + P;                       // a grid cannot hold more voxels than it has cells
        if (need > (int64_t)b->ncell) need = (int64_t)b->ncell;
        if (need > b->capacity) {
            rc = grow_builder(b, need, st);
            if (rc != AVL_OK) return rc;
        }
    }
    b->vox_bound += P;
    const unsigned long long key_bias = b->key_bias;
    if (B > 0) {
        if (B > b->table_cap) {
            AVL_HIP_CHECK(hipStreamSynchronize(st));
            if (b->d_table) AVL_HIP_CHECK(hipFree(b->d_table));
            b->d_table = nullptr;
            AVL_HIP_CHECK(hipMalloc((void**)&b->d_table, (size_t)(B + 16) * sizeof(BatchEntry)));
            b->table_cap = B + 16;
        }
        std::vector<BatchEntry> tab((size_t)B);
        for (int i = 0; i < B; ++i) {
            AVL_REQUIRE(h_depth_ptrs[i] && h_sample_ptrs[i] && h_feat_ptrs[i] && h_rgb_ptrs[i], "avl_builder_integrate_batch: null frame %d", i);
            memcpy(tab[i].t, h_pc_transform + 16 * i, 16 * sizeof(double));
            tab[i].depth = reinterpret_cast<const float*>(h_depth_ptrs[i]);
            tab[i].samples = h_sample_ptrs[i];
            tab[i].rgb = h_rgb_ptrs[i];
            tab[i].feat = h_feat_ptrs[i];
            tab[i].frame_key = key_bias | ((unsigned long long)(frame_idx + i) << 32);
        }
        // pageable source: the runtime stages the bytes before returning, so `tab` may go out of scope
        AVL_HIP_CHECK(hipMemcpyAsync(b->d_table, tab.data(), (size_t)B * sizeof(BatchEntry), hipMemcpyHostToDevice, st));
    }
    FrameParams fp;
    for (int i = 0; i < 9; ++i) { fp.kinv[i] = h_calib_inv[i]; fp.k[i] = h_calib[i]; fp.kf[i] = 0.0; }
    // get_sim_cam_mat(h, w): eye(3); [0,0] = [1,1] = w/2; [0,2] = w/2; [1,2] = h/2
    fp.kf[0] = fp.kf[4] = (double)Wf / 2.0;
    fp.kf[2] = (double)Wf / 2.0;
    fp.kf[5] = (double)Hf / 2.0;
    fp.kf[8] = 1.0;
    for (int i = 0; i < 16; ++i) fp.t[i] = h_pc_transform[i];
    fp.min_depth = min_depth; fp.max_depth = max_depth;
    fp.two_sigma_sq = 2 * sigma_sq;
    fp.cs = b->cs; fp.half_gs = (double)b->gs / 2.0;
    fp.H = H; fp.W = W; fp.Hf = Hf; fp.Wf = Wf; fp.n0 = b->n0; fp.n1 = b->gs; fp.n2 = b->vh; fp.P = P;
    fp.batch = B > 0 ? b->d_table : nullptr;
    fp.P_frame = P_frame;
    fp.mode = h_pcd_min ? 1 : 0;
    for (int i = 0; i < 3; ++i) fp.pcd_min[i] = h_pcd_min ? h_pcd_min[i] : 0.0;
    fp.depth_u16 = depth_u16;
    fp.depth_div = depth_div;
    fp.capacity = b->capacity;
    // PreGather: start from what the previous launch prepared for exactly this frame; let this launch prepare the frame the C loop
    // issues next (single float32 frames below the batched-launch size, the register-resident K3 kernels)
    fp.pre = nullptr;
    FrameParams fpn{};
    PreGather next{};
    const bool pre_ok = B == 0 && !depth_u16 && b->D <= 1536 && P < kAggregateSamples;
    if (pre_ok) {
        const auto& h = held;
        if (h.valid && h.samples == d_sample_idx && h.depth == d_depth && h.rgb == d_rgb && same_geometry(h.fp, fp)) fp.pre = b->pre_buf[h.buf];
        if (b->pre_next.samples) {
            fpn = fp;
            fpn.pre = nullptr;
            for (int i = 0; i < 16; ++i) fpn.t[i] = b->pre_next.h_pc_transform[i];
            next = PreGather{b->pre_buf[fp.pre ? 1 - h.buf : 0], b->pre_next.depth, b->pre_next.samples, b->pre_next.rgb};
        }
    }
    const int next_buf = next.out == b->pre_buf[1] ? 1 : 0;
    auto hold_next = [&]() {
        if (!next.out) return;
        b->pre_held.fp = fpn;
        b->pre_held.samples = next.samples;
        b->pre_held.depth = next.depth;
        b->pre_held.rgb = next.rgb;
        b->pre_held.buf = next_buf;
        b->pre_held.valid = true;
    };
    const unsigned long long frame_key = b->key_bias | ((unsigned long long)frame_idx << 32);

    if (b->ls_cache) drop_log_segments(b, st);   // the sorted log of the last merge is stale from here on
    if (b->log.slot && b->log_used + P > b->log_cap) {
        set_error("replay log full (%lld samples): enable it with a larger max_samples", b->log_cap);
        return AVL_ERR_CAPACITY;
    }
    const unsigned pb = (unsigned)((P + 255) / 256);
    if (b->deferred && B == 0 && b->D <= 1536) {
        // ONE launch: K1 + K2 of this frame next to K3 of the previous one; this frame's K3 rides in the next launch (or a flush)
        const FusePrev prev{b->pend.P, b->pend.frame_key, b->recs_alt, b->head_alt, b->pend.feat};
        const unsigned pb = (unsigned)((P + AVL_K3_THREADS - 1) / AVL_K3_THREADS);      // (its K1 + K2 workgroups have the kernel's size)
        if (b->D <= 256) launch_pipe<1>(b, fp, pb, d_depth, d_sample_idx, d_rgb, frame_key, prev, st, fpn, next);
        else if (b->D <= 512) launch_pipe<2>(b, fp, pb, d_depth, d_sample_idx, d_rgb, frame_key, prev, st, fpn, next);
        else if (b->D == 768) launch_pipe<3>(b, fp, pb, d_depth, d_sample_idx, d_rgb, frame_key, prev, st, fpn, next);
        else if (b->D <= 1024) launch_pipe<4>(b, fp, pb, d_depth, d_sample_idx, d_rgb, frame_key, prev, st, fpn, next);
        else launch_pipe<6>(b, fp, pb, d_depth, d_sample_idx, d_rgb, frame_key, prev, st, fpn, next);
        if (b->log.slot) b->log_used += P;
        b->pend.P = P;
        b->pend.frame_key = frame_key;
        b->pend.feat = d_feat;
        std::swap(b->recs, b->recs_alt);
        std::swap(b->head, b->head_alt);
        AVL_HIP_CHECK(hipGetLastError());
        hold_next();
        return AVL_OK;
    }
    rc = flush_pending(b, st);
    if (rc != AVL_OK) return rc;
    const bool k2_compacts = !(fp.pre || next.out);
    if (!k2_compacts) {     // a frame of the C loop: K1 from the prepared records and / or the next frame's stateless half in front
        const unsigned gb = next.out ? pb : 0u;
        hipLaunchKernelGGL(voxelize_link_next_kernel, dim3(gb + pb), dim3(256), 0, st, fp, reinterpret_cast<const float*>(d_depth), d_sample_idx,
                           d_rgb, b->cell_slot, b->slot_cell, b->recs, b->head, b->counters, b->err_flags, b->log, b->log_used, frame_key, fpn,
                           next, (int)gb);
    } else {
        hipLaunchKernelGGL(voxelize_link_kernel, dim3(pb), dim3(256), 0, st, fp, reinterpret_cast<const float*>(d_depth), d_sample_idx, d_rgb,
                           b->cell_slot, b->slot_cell, b->recs, b->head, b->counters, b->err_flags, b->log, b->log_used, frame_key, b->owners);
    }
    if (b->log.slot) b->log_used += P;
    rc = launch_fuse(b, P, frame_key, fp.batch, P_frame, b->recs, b->head, d_feat, st, k2_compacts);
    if (rc == AVL_OK) hold_next();
    return rc;
}

int avl_builder_set_deferred_fuse(avl_builder* b, int on, void* stream) {
    AVL_REQUIRE(b, "avl_builder_set_deferred_fuse: null handle");
    if (!on) {
        int rc = flush_pending(b, as_stream(stream));
        if (rc != AVL_OK) return rc;
    }
    b->deferred = on ? 1 : 0;
    return AVL_OK;
}

int avl_builder_flush(avl_builder* b, void* stream) {
    AVL_REQUIRE(b, "avl_builder_flush: null handle");
    return flush_pending(b, as_stream(stream));
}

int avl_builder_release_scratch(avl_builder* b, int64_t keep_bytes, void* stream) {
    AVL_REQUIRE(b, "avl_builder_release_scratch: null handle");
    AVL_REQUIRE(keep_bytes >= 0, "avl_builder_release_scratch: keep_bytes < 0");
    hipStream_t st = as_stream(stream);
    drop_log_segments(b, st);                       // the slot-sorted replay log cached between the two replay calls of a merge
    AVL_HIP_CHECK(hipStreamSynchronize(st));        // the pool only gives back what no stream still uses
    avl::trim_mempool((uint64_t)keep_bytes);
    return AVL_OK;
}

int avl_builder_integrate_frame(avl_builder* b, const float* d_depth, int H, int W, const double* h_calib,
                                const double* h_calib_inv, const double* h_pc_transform, const int32_t* d_sample_idx, int P,
                                const float* d_feat, int Hf, int Wf, const uint8_t* d_rgb, int64_t frame_idx,
                                double min_depth, double max_depth, double sigma_sq, void* stream) {
    return integrate_impl(b, d_depth, 0, 1.0, H, W, h_calib, h_calib_inv, h_pc_transform, d_sample_idx, P, d_feat, Hf, Wf, d_rgb,
                          frame_idx, min_depth, max_depth, sigma_sq, nullptr, stream);
}

int avl_builder_integrate_frame_global(avl_builder* b, const void* d_depth, int depth_is_u16, double depth_div, int H, int W,
                                       const double* h_calib, const double* h_calib_inv, const double* h_transform,
                                       const int32_t* d_sample_idx, int P, const float* d_feat, int Hf, int Wf,
                                       const uint8_t* d_rgb, int64_t frame_idx, double min_depth, double max_depth,
                                       double sigma_sq, const double* h_pcd_min, void* stream) {
    AVL_REQUIRE(h_pcd_min, "avl_builder_integrate_frame_global: pcd_min is required");
    AVL_REQUIRE(!depth_is_u16 || depth_div > 0, "avl_builder_integrate_frame_global: depth_div must be positive");
    return integrate_impl(b, d_depth, depth_is_u16 ? 1 : 0, depth_div, H, W, h_calib, h_calib_inv, h_transform, d_sample_idx, P, d_feat,
                          Hf, Wf, d_rgb, frame_idx, min_depth, max_depth, sigma_sq, h_pcd_min, stream);
}

int avl_builder_integrate_batch(avl_builder* b, int B, const float* const* h_depth_ptrs, int H, int W, const double* h_calib,
                                const double* h_calib_inv, const double* h_pc_transforms, const int32_t* const* h_sample_ptrs, int P,
                                const float* const* h_feat_ptrs, int Hf, int Wf, const uint8_t* const* h_rgb_ptrs, int64_t frame_idx0,
                                double min_depth, double max_depth, double sigma_sq, void* stream) {
    AVL_REQUIRE(B > 0, "avl_builder_integrate_batch: B must be positive");
    return integrate_impl(b, nullptr, 0, 1.0, H, W, h_calib, h_calib_inv, h_pc_transforms, nullptr, P, nullptr, Hf, Wf, nullptr, frame_idx0,
                          min_depth, max_depth, sigma_sq, nullptr, stream, B, reinterpret_cast<const void* const*>(h_depth_ptrs),
                          h_sample_ptrs, h_feat_ptrs, h_rgb_ptrs);
}

int avl_builder_integrate_frames(avl_builder* b, int n_frames, const float* const* h_depth_ptrs, int H, int W, const double* h_calib,
                                 const double* h_calib_inv, const double* h_pc_transforms, const int32_t* const* h_sample_ptrs, int P,
                                 const float* const* h_feat_ptrs, int Hf, int Wf, const uint8_t* const* h_rgb_ptrs, int64_t frame_idx0,
                                 double min_depth, double max_depth, double sigma_sq, void* stream) {
    AVL_REQUIRE(n_frames > 0, "avl_builder_integrate_frames: n_frames must be positive");
    AVL_REQUIRE(h_depth_ptrs && h_sample_ptrs && h_feat_ptrs && h_rgb_ptrs && h_pc_transforms, "avl_builder_integrate_frames: null pointer table");
    AVL_REQUIRE(b, "avl_builder_integrate_frames: null handle");
    for (int i = 0; i < n_frames; ++i) {
        // the frame after this one, for the gather workgroups of this frame's launch (PreGather); the last frame of a call has none:
        // what a later call brings is not known to be resident yet
        b->pre_next = {};
        if (i + 1 < n_frames && h_sample_ptrs[i + 1] && h_depth_ptrs[i + 1] && h_rgb_ptrs[i + 1])
            b->pre_next = {h_sample_ptrs[i + 1], h_depth_ptrs[i + 1], h_rgb_ptrs[i + 1], h_pc_transforms + 16 * (i + 1)};
        const int rc = integrate_impl(b, h_depth_ptrs[i], 0, 1.0, H, W, h_calib, h_calib_inv, h_pc_transforms + 16 * i, h_sample_ptrs[i], P,
                                      h_feat_ptrs[i], Hf, Wf, h_rgb_ptrs[i], frame_idx0 + i, min_depth, max_depth, sigma_sq, nullptr, stream);
        b->pre_next = {};
        if (rc != AVL_OK) return rc;
    }
    return AVL_OK;
}

int avl_builder_num_voxels(avl_builder* b, int64_t* h_n, void* stream) {
    AVL_REQUIRE(b && h_n, "avl_builder_num_voxels: null argument");
    int rc = flush_pending(b, as_stream(stream));
    if (rc != AVL_OK) return rc;
    rc = builder_check_flags(b, as_stream(stream));
    if (rc != AVL_OK) return rc;
    rc = read_counter(b, 0, h_n, as_stream(stream));
    if (rc == AVL_OK && *h_n > b->capacity) *h_n = b->capacity;
    return rc;
}

int avl_builder_num_points(avl_builder* b, int64_t* h_n, void* stream) {
    AVL_REQUIRE(b && h_n, "avl_builder_num_points: null argument");
    if (int rc = flush_pending(b, as_stream(stream)); rc != AVL_OK) return rc;
    return read_counter(b, 1, h_n, as_stream(stream));
}

int avl_builder_num_groups(avl_builder* b, int64_t* h_n, void* stream) {
    AVL_REQUIRE(b && h_n, "avl_builder_num_groups: null argument");
    if (int rc = flush_pending(b, as_stream(stream)); rc != AVL_OK) return rc;
    return read_counter(b, 2, h_n, as_stream(stream));
}

}  // extern "C"
