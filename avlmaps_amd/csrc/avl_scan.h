// The steps between the launches of a count / scan / write pipeline, shared by the small kernels: the one-workgroup scan that turns
// per-block counts into exclusive offsets and a total, and the kernels that count or number the flagged items of a block.
// Template kernels: a source that launches one instantiates it for itself.
#pragma once
#include "avl_wave.h"

namespace avl {

// out[b] = op(id, in[0], .. in[b - 1]) for b < n, *total = the combination of all n (when total is given).  ONE workgroup of
// THREADS threads, in rounds of THREADS elements with the rounds before in a register.  in and out may be the same array: a
// thread reads its element before any thread of that round writes.  The element of the NEXT round is requested before this
// round's scan, so that a round does not begin with a memory round trip: a round only writes below its own end, and a thread
// without a next element reads in[b0] instead and drops the value.
template <int THREADS, typename In, typename Out, typename Op>
__global__ __launch_bounds__(THREADS) void scan_counts_kernel(const In* in, int64_t n, Out* out, Out* total, Op op, Out id) {
    __shared__ Out s_w[THREADS / kWave];
    Out carry = id;
    Out v = threadIdx.x < n ? (Out)in[threadIdx.x] : id;
    for (int64_t b0 = 0; b0 < n; b0 += THREADS) {
        const int64_t b = b0 + threadIdx.x;
        const In ahead = in[b + THREADS < n ? b + THREADS : b0];  // an unconditional load: nothing waits for it before the scan
        Out round;
        const Out ex = block_excl_scan<THREADS / kWave>(v, op, id, s_w, &round);
        if (b < n) out[b] = op(carry, ex);
        carry = op(carry, round);
        v = b + THREADS < n ? (Out)ahead : id;
        __syncthreads();                                          // s_w is written again in the next round
    }
    if (threadIdx.x == 0 && total) *total = carry;
}

// bit k: item i0 + k exists and pred holds for it
template <int PER, typename Pred>
__device__ __forceinline__ int flags_of(int64_t n, int64_t i0, Pred pred) {
    int f = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (i0 + k < n && pred(i0 + k)) f |= 1 << k;
    return f;
}

// Workgroup blockIdx.x owns THREADS * PER consecutive items, a thread PER consecutive ones from *i0 on.  Returns the thread's
// flags; *before = the flagged items of the workgroup before *i0, *total = all of them.  lds: THREADS / 64 ints (avl_wave.h's rule).
template <int THREADS, int PER, typename Pred>
__device__ __forceinline__ int block_flags(int64_t n, Pred pred, int* lds, int64_t* i0, int* before, int* total) {
    *i0 = (int64_t)blockIdx.x * (THREADS * PER) + threadIdx.x * PER;
    const int f = flags_of<PER>(n, *i0, pred);
    *before = block_excl_scan<THREADS / kWave>((int)__popc(f), OpSum{}, 0, lds, total);
    return f;
}

template <int THREADS, int PER, typename Pred>
__global__ __launch_bounds__(THREADS) void count_flagged_kernel(int64_t n, Pred pred, int* __restrict__ counts) {
    __shared__ int s_w[THREADS / kWave];
    int64_t i0;
    int before, total;
    block_flags<THREADS, PER>(n, pred, s_w, &i0, &before, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// out[i] = 1 + the number of flagged items before i, for every flagged i; offsets = the scanned counts of count_flagged_kernel
template <int THREADS, int PER, typename Pred>
__global__ __launch_bounds__(THREADS) void number_flagged_kernel(int64_t n, Pred pred, const int* __restrict__ offsets, int* __restrict__ out) {
    __shared__ int s_w[THREADS / kWave];
    const int base = offsets[blockIdx.x];
    int64_t i0;
    int before, total;
    const int f = block_flags<THREADS, PER>(n, pred, s_w, &i0, &before, &total);
    int rank = base + before;
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (f >> k & 1) out[i0 + k] = ++rank;
}

}  // namespace avl
