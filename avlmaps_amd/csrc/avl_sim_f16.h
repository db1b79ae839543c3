// Building blocks of the fp16 hi|lo similarity kernels of avl_sim.hip (split, kswap, stream, stream_tb), each once.  A kernel
// uses a block only where all its instantiations keep their ISA (tools/isa_diff.py, profiles/sim_blocks_isa.txt): the tables in
// all four; mfma_step and the two drivers in the resident kernel (its six extra-row variants keep their own step) and the K-swap
// one; voxel_load_step in the K-swap and the streamed kernels; the streamed-image blocks in the two streamed kernels.
// Included by avl_sim.hip alone, inside namespace avl, below the voxel-operand makers it builds on (compact_operands).
#pragma once
// ---- per-query tables of TQ rows, `rows` of them valid: qml[r] = the caller's query index of row r (QM: column blocks) ...
template <bool QM>
__device__ __forceinline__ void fill_query_map(int32_t* qml, int TQ, int rows, const int32_t* qmap, int q_base) {
    if constexpr (QM) {
        if (threadIdx.x < TQ) qml[threadIdx.x] = threadIdx.x < rows ? qmap[q_base + threadIdx.x] : INT_MAX;
    }
}
// ... and isc[r] = 2^-S of query row r
__device__ __forceinline__ void fill_inv_scale(float* isc, int TQ, int rows, const float* inv_scale, int q_base) {
    if (threadIdx.x < TQ) isc[threadIdx.x] = threadIdx.x < rows ? inv_scale[q_base + threadIdx.x] : 0.f;
}
// ---- the three-product MFMA step.  Ablation switches (variant libraries only, never shipped): they live in the shared step, so
// they act on every kernel that uses it -- the resident kernel (no longer its extra-row variants) and now the K-swap one too:
//   AVL_ABL_NOLDS   the query fragments are constants instead of LDS reads
//   AVL_ABL_NOMFMA  the products are not issued (their operands are kept alive)
//   AVL_ABL_HIONLY  hi*hi only: what ONE product per pair would cost (the argmax-only question)
__device__ __forceinline__ half8 query_fragment(const char* p, int lo) {
#ifdef AVL_ABL_NOLDS
    half8 a;
    for (int e = 0; e < 8; ++e) a[e] = (_Float16)(1 + lo);
    asm volatile("" : "+v"(a));
    return a;
#else
    return *reinterpret_cast<const half8*>(p);
#endif
}
__device__ __forceinline__ void mfma_f16(f32x16& acc, const half8& a, const half8& b) {
#ifdef AVL_ABL_NOMFMA
    asm volatile("" ::"v"(a), "v"(b));
#else
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
#endif
}
// Step s of a K chunk for one 32-voxel tile: per 8-column group m, operands(m, bh, bl) makes the voxel-side fragments and
// a_hi(t, off) is the address of query tile t's hi fragment at byte `off` of its row (its lo fragment lies lo_off bytes further).
// hi.hi, lo.hi, hi.lo in term-major, tile-minor issue order: consecutive MFMAs target different accumulators.
// NA independent accumulator sets per query tile (hi*hi | cross terms) so that back-to-back MFMAs never wait on each other's
// result: a dependent 32x32x16 MFMA cannot issue until its predecessor retires.
template <int QT, int NA, class Operands, class AHi>
__device__ __forceinline__ void mfma_step(f32x16 (&acc)[QT][NA], int s, int lo_off, Operands&& operands, AHi&& a_hi) {
    [[maybe_unused]] constexpr int X1 = NA > 1 ? 1 : 0, X2 = NA > 2 ? 2 : X1;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        half8 bh, bl;
        operands(m, bh, bl);
        const int off = (s * 64 + 8 * m) * 2;
        half8 ah[QT], al[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            ah[t] = query_fragment(a_hi(t, off), 0);
            al[t] = query_fragment(a_hi(t, off) + lo_off, 1);
        }
#pragma unroll
        for (int t = 0; t < QT; ++t) mfma_f16(acc[t][0], ah[t], bh);
#ifndef AVL_ABL_HIONLY
#pragma unroll
        for (int t = 0; t < QT; ++t) mfma_f16(acc[t][X1], al[t], bh);
#pragma unroll
        for (int t = 0; t < QT; ++t) mfma_f16(acc[t][X2], ah[t], bl);
#endif
    }
}
// ---- the step drivers of a resident K chunk with a compile-time trip count: load(buf, s) fetches step s of the lane's row into
// f32x4[8], compute(buf, s) contracts it, contract(operands, s) is compute with the operand maker given (mfma_step's `operands`)
// Compact map, window starting on a 128-column block (the launcher checks): the residual line of a block serves its two steps
// and is requested ONCE, with the even step -- 64 B per lane half into a buffer of its own (two, by block parity: the odd step
// still reads one while the next block's is in flight); hi: two buffers by step parity.  One step ahead, like the ring below.
// row = first byte of the map row, ld = columns of a full row, sa0 = index of the chunk's first step in the row
template <int NSTEPS, class Contract>
__device__ __forceinline__ void drive_compact_blocks(const char* row, int64_t ld, int kg, int sa0, Contract&& contract) {
    static_assert(NSTEPS % 2 == 0, "whole 128-column blocks");
    f32x4 hb[2][4], lb[2][4];
    auto load_hi = [&](int st) {
        const f32x4* g = reinterpret_cast<const f32x4*>(row + 128 * (sa0 + st) + 64 * kg);
#pragma unroll
        for (int t = 0; t < 4; ++t) hb[st & 1][t] = g[t];
    };
    auto load_lo = [&](int blk) {
        const f32x4* g = reinterpret_cast<const f32x4*>(row + 2 * ld + 128 * ((sa0 >> 1) + blk) + 64 * kg);
#pragma unroll
        for (int t = 0; t < 4; ++t) lb[blk & 1][t] = g[t];
    };
    load_hi(0);
    load_lo(0);
#pragma unroll
    for (int st = 0; st < NSTEPS; ++st) {
        if (st + 1 < NSTEPS) {
            load_hi(st + 1);
            if (((st + 1) & 1) == 0) load_lo((st + 1) >> 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        contract([&](int m, half8& bh, half8& bl) {
            compact_operands(hb[st & 1][m], lb[(st >> 1) & 1][2 * (st & 1) + (m >> 1)], m & 1, bh, bl);
        }, st);
    }
}
// ring of kRing register buffers: the loads of the next kRing - 1 steps fly while step s is computed, all waits counted vmcnt
template <int NSTEPS, int kRing, class Load, class Compute>
__device__ __forceinline__ void drive_ring(Load&& load, Compute&& compute) {
    f32x4 ring[kRing][8];
#pragma unroll
    for (int r = 0; r + 1 < kRing; ++r)
        if (r < NSTEPS) load(ring[r], r);
#pragma unroll
    for (int s = 0; s < NSTEPS; ++s) {
        if (s + kRing - 1 < NSTEPS) load(ring[(s + kRing - 1) % kRing], s + kRing - 1);
        __builtin_amdgcn_sched_barrier(0);   // keep the prefetch block ahead of the compute block
        compute(ring[s % kRing], s);
    }
}
// ---- one 64-column step of a lane's voxel row.  Byte geometry of the walk: float32 / prepared rows are 4 B per column and a lane
// owns 128 B of every step; the compact form (P24) is 3 B per column, 96 B per lane and step (hi[32] | residual bytes[32])
template <bool P24>
struct VoxelBytes {
    static constexpr int kElB = P24 ? 3 : 4, kLaneB = P24 ? 96 : 128, kStepB = 2 * kLaneB, kLoads = P24 ? 6 : 8;
};
// step sa0 + step of the row into b.  float32 / prepared: src = the lane's line of the window's first step (row + kLaneB * kg);
// compact: src = first byte of the map row, sa0 = index of the window's first step in the row, ld = columns of a full row
template <bool P24>
__device__ __forceinline__ void voxel_load_step(f32x4 (&b)[8], const char* src, int64_t ld, int kg, int sa0, int step) {
    if constexpr (P24) {
        compact_load_step(b, src, ld, kg, sa0 + step);
    } else {
        const f32x4* g = reinterpret_cast<const f32x4*>(src + VoxelBytes<P24>::kStepB * step);
#pragma unroll
        for (int t = 0; t < VoxelBytes<P24>::kLoads; ++t) b[t] = g[t];
    }
}
// ---- the streamed query image: K chunks of KS = 64 * SPC columns, [nch][Qtot][hi KS | lo KS | pad 8] fp16, double buffered in LDS;
// the next chunk is staged in SPC slices, one per k step (registers: 5 x 16 B at SPC = 2, 3 x 16 B at SPC = 4)
constexpr int kStreamFill = 9;   // 16-byte staging registers per thread: one LDS buffer <= 9 * 512 * 16 B = 72 KB
template <int SPC>
struct StreamLayout {
    static constexpr int KS = 64 * SPC;
    static constexpr int row_b = (2 * KS + kRowPadHalves) * 2;   // bytes per query row of one chunk: hi[KS] | lo[KS] | pad
    static constexpr int lo_b = 2 * KS;                          // byte offset of the lo half inside a row
    static constexpr int NSTG = kStreamFill - ((SPC - 1) * kStreamFill) / SPC;   // 16-byte staging registers per thread
};
// 16-byte pieces i0 .. i1 - 1 (of `units`) of chunk c: global -> registers, registers -> the LDS buffer at dst
template <int NT, int NSTG>
__device__ __forceinline__ void stage_load_slice(f32x4 (&stg)[NSTG], const _Float16* img, int c, int Qtot, int q_base, int row_b,
                                                 int units, int i0, int i1) {
    const f32x4* src = reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(img) + ((int64_t)c * Qtot + q_base) * row_b);
#pragma unroll
    for (int i = i0; i < i1; ++i) {
        const int u = threadIdx.x + i * NT;
        if (u < units) stg[i - i0] = src[u];
    }
}
template <int NT, int NSTG>
__device__ __forceinline__ void stage_store_slice(const f32x4 (&stg)[NSTG], char* buf, int units, int i0, int i1) {
    f32x4* dst = reinterpret_cast<f32x4*>(buf);
#pragma unroll
    for (int i = i0; i < i1; ++i) {
        const int u = threadIdx.x + i * NT;
        if (u < units) dst[u] = stg[i - i0];
    }
}
// publish the next chunk / retire this one: LDS traffic only (lgkmcnt, one raw s_barrier), the voxel prefetch stays in flight
__device__ __forceinline__ void stream_publish() {
#ifndef AVL_ABL_NOBARRIER
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#endif
}
// the lane's line of voxel tile `tile` (tile_rows rows per workgroup): row + kLaneB * kg, or the first byte of a compact row;
// rows past the map re-read row N - 1
template <bool P24>
__device__ __forceinline__ const char* stream_tile_ptr(const float* feat, int64_t tile, int tile_rows, int wave, int j, int kg,
                                                       int64_t N, int64_t ld) {
    const int64_t r = tile * tile_rows + wave * 32 + j;
    return reinterpret_cast<const char*>(feat) + (r < N ? r : N - 1) * (ld * VoxelBytes<P24>::kElB) + (P24 ? 0 : VoxelBytes<P24>::kLaneB * kg);
}
// byte offset in an image half / stream buffer of the query row lane (j, kg) reads for tile t; lanes past the last row read `last`
__device__ __forceinline__ int query_row_offset(int t, int j, int kg, int last, int row_b) {
    return min(t * 32 + j, last) * row_b + kg * 64;
}
