// Exact-colour replay of the voxel map builder: weight / grid_rgb as the reference's SEQUENTIAL running mean leaves them
// (vlmap_builder.py:164-178: float32 / uint8 stores at every update), which no commutative sum reproduces.  The frame path
// (avl_builder.hip, link_body) logs one record per sample in key order; here the log is compacted to the samples that updated a voxel,
// sorted by voxel (LogSegments) and replayed voxel by voxel -- at finalisation (replay_rgb) or as a chain over the ranks of a multi-GPU
// build (avl_builder_replay_chain, avl_replay_state_apply).
// Compiled with -ffp-contract=off: the replay's roundings are the reference's, step by step.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "avl_builder_state.h"
#include "avl_wave.h"

namespace avl {

// first / one-past-last position of every slot's run in the slot-sorted log
__global__ void log_segments_kernel(const uint32_t* __restrict__ sorted_slot, long long L, long long nslots,
                                    long long* __restrict__ seg_start, long long* __restrict__ seg_end) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (long long)gridDim.x * blockDim.x) {
        const uint32_t sl = sorted_slot[i];
        if (sl >= (uint32_t)nslots) continue;
        if (i == 0 || sorted_slot[i - 1] != sl) seg_start[sl] = i;
        if (i == L - 1 || sorted_slot[i + 1] != sl) seg_end[sl] = i + 1;
    }
}

// One update of the reference's running weight / colour with the reference's dtypes (vlmap_builder.py:164-178; NumPy >= 2
// promotion, see oracle/avl_oracle.c avlo_integrate_frame):
//   until the first capacity doubling (_reserve_map_space, :286-311) weight is float32 and grid_rgb uint8 (truncating
//   store at every update); afterwards weight is float64 and grid_rgb float32.  The doubling happens right after the
//   voxel with id gs*gs - 1 was created, i.e. for every update whose key is greater than that voxel's first-touch key
//   (`grown`).  c[] holds uint8 or float32 values exactly.
__device__ __forceinline__ void replay_step(double& w, double (&c)[3], bool& started, double alpha, uint32_t rgbv, bool grown) {
    const double v[3] = {(double)(rgbv & 0xffu), (double)((rgbv >> 8) & 0xffu), (double)((rgbv >> 16) & 0xffu)};
    if (!started) {
        started = true;
        for (int k = 0; k < 3; ++k) c[k] = v[k];
        const double ww = 0.0 + alpha;
        w = grown ? ww : (double)(float)ww;
    } else {
        const double denom = w + alpha;
        if (!grown) {
            const float wf = (float)w;
            for (int k = 0; k < 3; ++k) {
                const float prod = (float)c[k] * wf;
                const double q = ((double)prod + v[k] * alpha) / denom;
                c[k] = (double)(uint8_t)q;
            }
            w = (double)(float)denom;
        } else {
            for (int k = 0; k < 3; ++k) c[k] = (double)(float)((c[k] * w + v[k] * alpha) / denom);
            w = denom;
        }
    }
}

// The updates [i0, i1) of one voxel, in order.  The state is a serial chain, the loads are not: kReplayAhead entries' index ->
// {alpha, rgb, key} gathers are requested together (unconditionally: positions past the end re-read the last entry), so a long
// segment pays one memory round trip per kReplayAhead entries instead of two per entry.
#ifndef AVL_REPLAY_AHEAD
#define AVL_REPLAY_AHEAD 4
#endif
constexpr int kReplayAhead = AVL_REPLAY_AHEAD;
__device__ __forceinline__ void replay_walk(double& w, double (&c)[3], bool& started, long long i0, long long i1, const int32_t* __restrict__ order,
                                            const ReplayLog& log, unsigned long long gkey) {
    for (long long i = i0; i < i1; i += kReplayAhead) {
        int32_t e[kReplayAhead];
#pragma unroll
        for (int k = 0; k < kReplayAhead; ++k) e[k] = order[i + k < i1 ? i + k : i1 - 1];
        double a[kReplayAhead];
        uint32_t v[kReplayAhead];
        unsigned long long ky[kReplayAhead];
#pragma unroll
        for (int k = 0; k < kReplayAhead; ++k) {
            using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;
            const u64x2* r = reinterpret_cast<const u64x2*>(log.rec + e[k]);
            const u64x2 r0 = r[0];
            a[k] = __longlong_as_double((long long)r0.x);
            ky[k] = r0.y;
            v[k] = (uint32_t)r[1].x;
        }
#pragma unroll
        for (int k = 0; k < kReplayAhead; ++k)
            if (i + k < i1) replay_step(w, c, started, a[k], v[k], ky[k] > gkey);
    }
}

// Thread per output row: replay the voxel's updates in the reference's order (the log is in key order, `order` is its stable
// sort by slot).
__global__ __launch_bounds__(256) void replay_rgb_kernel(int64_t n, long long gs2, const int32_t* __restrict__ perm,
                                                         const unsigned long long* __restrict__ keys_sorted,
                                                         const int32_t* __restrict__ order, const long long* __restrict__ seg_start,
                                                         const long long* __restrict__ seg_end, ReplayLog log,
                                                         float* __restrict__ weight, uint8_t* __restrict__ grid_rgb) {
    const unsigned long long gkey = n >= gs2 ? keys_sorted[gs2 - 1] : kNoKey;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t sl = perm[r];
        double w = 0.0, c[3] = {0.0, 0.0, 0.0};
        bool started = false;
        replay_walk(w, c, started, seg_start[sl], seg_end[sl], order, log, gkey);
        if (started) {
            if (weight) weight[r] = (float)w;
            if (grid_rgb)
                for (int k = 0; k < 3; ++k) grid_rgb[r * 3 + k] = (uint8_t)fmin(fmax(c[k], 0.0), 255.0);
        }
    }
}

// Multi-GPU: the sequential replay is a CHAIN over ranks (frames are sharded contiguously, so every update of rank r comes
// before every update of rank r + 1): a rank receives the per-voxel state left by its predecessors, continues it with its own
// log and passes it on -- 24 bytes per voxel per hop instead of shipping the logs (avlmaps_amd/parallel.py).
__global__ __launch_bounds__(256) void replay_chain_kernel(int64_t n, unsigned long long gkey, const int64_t* __restrict__ row_of_slot,
                                                           const int32_t* __restrict__ order, const long long* __restrict__ seg_start,
                                                           const long long* __restrict__ seg_end, ReplayLog log,
                                                           ReplayState* __restrict__ state) {
    for (int64_t sl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; sl < n; sl += (int64_t)gridDim.x * blockDim.x) {
        const int64_t si = row_of_slot[sl];
        if (si < 0 || seg_start[sl] >= seg_end[sl]) continue;          // negative index: slot not part of this call
        ReplayState& st = state[si];
        double w = st.w, c[3] = {(double)st.c[0], (double)st.c[1], (double)st.c[2]};
        bool started = st.started != 0;
        replay_walk(w, c, started, seg_start[sl], seg_end[sl], order, log, gkey);
        st.w = w;
        for (int k = 0; k < 3; ++k) st.c[k] = (float)c[k];
        st.started = started ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void replay_apply_kernel(int64_t n, const ReplayState* __restrict__ state, float* __restrict__ weight,
                                                           uint8_t* __restrict__ grid_rgb) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const ReplayState st = state[r];
        if (!st.started) continue;
        if (weight) weight[r] = (float)st.w;
        if (grid_rgb)
            for (int k = 0; k < 3; ++k) grid_rgb[r * 3 + k] = (uint8_t)fminf(fmaxf(st.c[k], 0.f), 255.f);
    }
}

}  // namespace avl

using namespace avl;

// Compaction of the replay log to the entries that updated a voxel (slot != 0xFFFFFFFF), order kept: kLogParts contiguous parts,
// one workgroup each -- count, one-workgroup scan of the counts, then every part writes its survivors' log position and slot behind
// its offset (ballot ranks inside a wave, LDS across the four waves).  rocprim::select with a predicate over a counting iterator
// took 0.92 ms for 78 M entries (0.43 GB of traffic); these three kernels read the slots twice and write 2 x 4 B per survivor.
constexpr int kLogParts = 2048;

__global__ __launch_bounds__(256) void log_count_kernel(const uint32_t* __restrict__ slot, long long L, long long chunk, int* __restrict__ counts) {
    __shared__ int wsum[4];
    const long long lo = (long long)blockIdx.x * chunk, hi = lo + chunk < L ? lo + chunk : L;
    int c = 0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) c += slot[i] != 0xFFFFFFFFu;
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(1024) void log_offsets_kernel(const int* __restrict__ counts, long long* __restrict__ offsets, long long* __restrict__ total) {
    __shared__ long long part[1024];
    static_assert(kLogParts == 2048, "two parts per thread");
    const int t = threadIdx.x;
    const long long a = counts[2 * t], b = counts[2 * t + 1];
    part[t] = a + b;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long long v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const long long before = part[t] - (a + b);
    offsets[2 * t] = before;
    offsets[2 * t + 1] = before + a;
    if (t == 1023) *total = part[t];
}

__global__ __launch_bounds__(256) void log_compact_kernel(const uint32_t* __restrict__ slot, long long L, long long chunk,
                                                          const long long* __restrict__ offsets, int32_t* __restrict__ active,
                                                          uint32_t* __restrict__ active_slot) {
    __shared__ int wsum[4];
    const long long lo = (long long)blockIdx.x * chunk, hi = lo + chunk < L ? lo + chunk : L;
    long long base = offsets[blockIdx.x];
    for (long long i0 = lo; i0 < hi; i0 += 256) {                 // (chunk is a multiple of 256: a uniform trip count per workgroup)
        const long long i = i0 + threadIdx.x;
        const uint32_t sl = i < hi ? slot[i] : 0xFFFFFFFFu;
        const bool keep = sl != 0xFFFFFFFFu;
        int all;
        const int rank = block_compact_rank<4>(keep, wsum, &all);
        if (keep) {
            active[base + rank] = (int32_t)i;
            active_slot[base + rank] = sl;
        }
        base += all;
        __syncthreads();                                          // wsum is rewritten by the next round
    }
}

// The replay log sorted by voxel: `order` = the positions of the entries that updated a voxel, stably sorted by slot (the log is
// in key order, so every voxel's run is in the reference's update order), [seg_start[s], seg_end[s]) = the run of slot s.
// Only ~35 % of the sampled pixels update a voxel (depth mask, feature-image bounds): the log is first compacted to those
// entries, and the radix sort only looks at the bits a slot index can have -- a third of the entries and three of the four
// passes (sorting all 78 M entries of a 10 000-frame log instead: 0.58 ms per pass against 0.22).
struct LogSegments {
    uint32_t *active_slot = nullptr, *sorted_slot = nullptr;
    int32_t *active = nullptr, *order = nullptr;
    long long *seg_start = nullptr, *seg_end = nullptr, *d_count = nullptr;
    void* tmp = nullptr;
    char *block1 = nullptr, *block2 = nullptr;   // TWO pool allocations hold all of the above (a hipMallocAsync / hipFreeAsync pair costs
                                                 // ~90 us of host time: nine of them were most of a small rank's replay)
    int build(avl_builder* b, int64_t n, hipStream_t st) {
        const long long L = b->log_used;
        const long long chunk = ((L + kLogParts - 1) / kLogParts + 255) / 256 * 256;
        size_t tmp_bytes = 0;
        const size_t b_active = align256((size_t)L * sizeof(int32_t)), b_seg = align256((size_t)n * sizeof(long long));
        const size_t b_counts = align256(kLogParts * sizeof(int)), b_off = align256(kLogParts * sizeof(long long));
        // the two L-sized arrays (and, below, the two La-sized ones + the sort's storage) come from the scratch allocated with the log
        // when it is there and large enough; the small per-voxel arrays always from the pool
        const bool own = b->rs_mem && b->rs_bytes >= 4 * b_active + b->rs_tmp_bytes + 256;
        AVL_HIP_CHECK(hipMallocAsync((void**)&block1, (own ? 0 : 2 * b_active) + 256 + 2 * b_seg + b_counts + b_off, st));
        char* p1 = block1;
        if (own) {
            active = reinterpret_cast<int32_t*>(b->rs_mem);
            active_slot = reinterpret_cast<uint32_t*>(b->rs_mem + b_active);
        } else {
            active = reinterpret_cast<int32_t*>(p1);
            active_slot = reinterpret_cast<uint32_t*>(p1 + b_active);
            p1 += 2 * b_active;
        }
        d_count = reinterpret_cast<long long*>(p1);
        seg_start = reinterpret_cast<long long*>(p1 + 256);
        seg_end = reinterpret_cast<long long*>(p1 + 256 + b_seg);
        int* counts = reinterpret_cast<int*>(p1 + 256 + 2 * b_seg);
        long long* offsets = reinterpret_cast<long long*>(p1 + 256 + 2 * b_seg + b_counts);
        AVL_HIP_CHECK(hipMemsetAsync(seg_start, 0, 2 * b_seg, st));
        hipLaunchKernelGGL(log_count_kernel, dim3(kLogParts), dim3(256), 0, st, b->log.slot, L, chunk, counts);
        hipLaunchKernelGGL(log_offsets_kernel, dim3(1), dim3(1024), 0, st, counts, offsets, d_count);
        hipLaunchKernelGGL(log_compact_kernel, dim3(kLogParts), dim3(256), 0, st, b->log.slot, L, chunk, offsets, active, active_slot);
        long long La = 0;
        AVL_HIP_CHECK(hipMemcpyAsync(&La, d_count, sizeof(La), hipMemcpyDeviceToHost, st));
        AVL_HIP_CHECK(hipStreamSynchronize(st));
        const size_t Ls = (size_t)(La > 0 ? La : 1);
        int bits = 1;
        while (bits < 32 && (1ll << bits) <= (long long)n) ++bits;      // slots are < n
        if (La > 0)
            AVL_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                                                    (size_t)La, 0, bits, st));
        const size_t b_ls = align256(Ls * sizeof(uint32_t));
        if (own && tmp_bytes <= b->rs_tmp_bytes) {
            char* p2 = b->rs_mem + 2 * b_active;
            sorted_slot = reinterpret_cast<uint32_t*>(p2);
            order = reinterpret_cast<int32_t*>(p2 + b_ls);
            tmp = p2 + 2 * b_active;                   // (behind the four L-sized words: La <= L)
        } else {
            AVL_HIP_CHECK(hipMallocAsync((void**)&block2, 2 * b_ls + align256(tmp_bytes ? tmp_bytes : 16), st));
            sorted_slot = reinterpret_cast<uint32_t*>(block2);
            order = reinterpret_cast<int32_t*>(block2 + b_ls);
            tmp = block2 + 2 * b_ls;
        }
        if (La > 0) {
            AVL_HIP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, active_slot, sorted_slot, active, order, (size_t)La, 0, bits, st));
            hipLaunchKernelGGL(log_segments_kernel, dim3((unsigned)std::min<long long>((La + 255) / 256, 8192)), dim3(256), 0, st, sorted_slot,
                               La, (long long)n, seg_start, seg_end);
        }
        AVL_HIP_CHECK(hipGetLastError());
        return AVL_OK;
    }
    void release(hipStream_t st) {
        if (block2) (void)hipFreeAsync(block2, st);
        if (block1) (void)hipFreeAsync(block1, st);
        block1 = block2 = nullptr;
    }
};

void avl::drop_log_segments(avl_builder* b, hipStream_t st) {
    if (!b->ls_cache) return;
    b->ls_cache->release(st);
    delete b->ls_cache;
    b->ls_cache = nullptr;
    b->ls_log_used = -1;
    b->ls_n = -1;
}

// rocPRIM's storage for the (slot, log position) sort of a log of n samples, all 32 key bits: what avl_builder_enable_replay_log sets
// aside next to the log.  This file is the only one that instantiates that sort.
size_t avl::replay_sort_tmp_bytes(int64_t n) {
    size_t tb = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                                                   (size_t)n, 0, 32, nullptr);
    (void)hipGetLastError();
    return e == hipSuccess ? tb : 0;
}

// the log sorted by voxel (LogSegments), built if it is not there.  A finalisation and the first avl_builder_replay_chain call of a
// merge (phase A of merge2.py) build it on the spot -- the compaction, the sort and one host synchronisation in between, in front of
// the replay -- and the merge's second call (phase B) reuses it.  avl_builder_replay_prepare builds it ahead of time for a C caller
// with host work to hide it under; neither merge2.py nor parallel.py calls it.
static int ensure_log_segments(avl_builder* b, int64_t n, hipStream_t st) {
    if (b->ls_cache && b->ls_log_used == b->log_used && b->ls_n == n) return AVL_OK;
    drop_log_segments(b, st);
    b->ls_cache = new LogSegments();
    int rc = b->ls_cache->build(b, n, st);
    if (rc != AVL_OK) {
        drop_log_segments(b, st);
        return rc;
    }
    b->ls_log_used = b->log_used;
    b->ls_n = n;
    return AVL_OK;
}

// exact sequential weight / grid_rgb: stable sort of the key-ordered log by slot, then replay per voxel
// (the builder's ONE voxel-sorted form of the log, shared with the merge's replay: it lives in the scratch allocated with the log,
// so a private second build here would overwrite a cached one; it stays valid until the next frame is fused)
int avl::replay_rgb(avl_builder* b, int64_t n, const int32_t* perm, const unsigned long long* keys_sorted, float* d_weight,
                    uint8_t* d_grid_rgb, hipStream_t st) {
    int rc = ensure_log_segments(b, n, st);
    if (rc != AVL_OK) return rc;
    const LogSegments& ls = *b->ls_cache;
    hipLaunchKernelGGL(replay_rgb_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, st, n,
                       (long long)b->n0 * b->gs, perm, keys_sorted, ls.order, ls.seg_start, ls.seg_end, b->log, d_weight, d_grid_rgb);
    if (hipGetLastError() != hipSuccess) rc = AVL_ERR_HIP;
    return rc;
}

extern "C" {

int avl_builder_drop_replay_cache(avl_builder* b, void* stream) {
    AVL_REQUIRE(b, "avl_builder_drop_replay_cache: null handle");
    drop_log_segments(b, as_stream(stream));
    return AVL_OK;
}

int avl_builder_replay_prepare(avl_builder* b, int64_t n, void* stream) {
    AVL_REQUIRE(b, "avl_builder_replay_prepare: null handle");
    int64_t have = 0;
    int rc = avl_builder_num_voxels(b, &have, stream);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n == have, "avl_builder_replay_prepare: n=%lld but the map holds %lld voxels", (long long)n, (long long)have);
    if (!b->log.slot || b->key_bias != 0 || n == 0 || b->log_used == 0) return AVL_OK;      // (nothing to prepare: replay_chain reports a missing log)
    // (a build on a stream of the builder's own, overlapping the merge plan's host work, was measured in round 6: nothing in the 8-rank
    // rehearsal, +10 ms on the first merge of a process for the stream and its events -- the form is built on the caller's stream)
    return ensure_log_segments(b, n, as_stream(stream));
}

int avl_builder_replay_chain(avl_builder* b, int64_t n, const int64_t* d_row_of_slot, uint64_t grow_key, void* d_state,
                             void* stream) {
    AVL_REQUIRE(b, "avl_builder_replay_chain: null handle");
    hipStream_t st = as_stream(stream);
    int64_t have = 0;
    int rc = avl_builder_num_voxels(b, &have, stream);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n == have, "avl_builder_replay_chain: n=%lld but the map holds %lld voxels", (long long)n, (long long)have);
    if (!b->log.slot || b->key_bias != 0) {
        set_error("avl_builder_replay_chain: the builder has no replay log (avl_builder_enable_replay_log on a fresh builder)");
        return AVL_ERR_STATE;
    }
    if (n == 0 || b->log_used == 0) return AVL_OK;
    AVL_REQUIRE(d_row_of_slot && d_state, "avl_builder_replay_chain: null pointer");
    rc = ensure_log_segments(b, n, st);
    if (rc != AVL_OK) return rc;
    const LogSegments& ls = *b->ls_cache;
    hipLaunchKernelGGL(replay_chain_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, st, n,
                       (unsigned long long)grow_key, d_row_of_slot, ls.order, ls.seg_start, ls.seg_end, b->log,
                       reinterpret_cast<ReplayState*>(d_state));
    if (hipGetLastError() != hipSuccess) rc = AVL_ERR_HIP;
    return rc;
}

int avl_replay_state_apply(int64_t n, const void* d_state, float* d_weight, uint8_t* d_grid_rgb, void* stream) {
    AVL_REQUIRE(n >= 0, "avl_replay_state_apply: bad n");
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_state, "avl_replay_state_apply: null state");
    hipLaunchKernelGGL(replay_apply_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, as_stream(stream), n,
                       reinterpret_cast<const ReplayState*>(d_state), d_weight, d_grid_rgb);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
