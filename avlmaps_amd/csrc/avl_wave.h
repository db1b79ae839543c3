// Wave and workgroup primitives shared by the small kernels (device side): reductions over the 64 lanes of a wave, the ordered
// compaction rank and the exclusive scan of a workgroup, and the block min/max that ends in two atomics.
//
// LDS rule of every workgroup helper here: the helper holds the ONE barrier between writing its LDS words and reading them, and
// returns with threads possibly still reading.  A caller that hands the same LDS to another call (a loop, a second scan) puts a
// __syncthreads() in between; a caller that uses it once needs none.
#pragma once
#include "avl_common.h"

namespace avl {

struct OpMin {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct OpMax {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};
struct OpSum {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// The one xor butterfly: distances 32, 16, .. 1, every lane ends with the result.  The order is fixed, so a float64 sum is the same
// bits on every run and on every lane (addition is commutative: both partners of a step compute the same value).
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
    for (int off = kWave / 2; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, kWave));
    return v;
}
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, OpMin{}); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, OpMax{}); }
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, OpSum{}); }

// Ordered stream compaction of a workgroup of WAVES waves: the number of threads before this one (in thread order) whose `keep`
// is set, and *total = the number of all of them.  Every thread calls it.  lds: WAVES ints (see the LDS rule above).
template <int WAVES>
__device__ __forceinline__ int block_compact_rank(bool keep, int* lds, int* total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) lds[wave] = __popcll(kept);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int x = lds[w];
        before += w < wave ? x : 0;
        all += x;
    }
    *total = all;
    return before + __popcll(kept & ((1ull << lane) - 1ull));
}

// Exclusive scan of one integer per thread over a workgroup of WAVES waves under `op` with identity `id` (a running maximum with
// id = -1, a sum with id = 0): the return value combines the threads before this one, *total all of them.  Shuffles inside a wave,
// one LDS step across the waves.  lds: WAVES values of T (see the LDS rule above).
template <int WAVES, typename T, typename Op>
__device__ __forceinline__ T block_excl_scan(T v, Op op, T id, T* lds, T* total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    T incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T o = __shfl_up(incl, d, kWave);
        if (lane >= d) incl = op(incl, o);
    }
    if (lane == kWave - 1) lds[wave] = incl;
    __syncthreads();
    T before = id, all = id;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const T x = lds[w];
        if (w < wave) before = op(before, x);
        all = op(all, x);
    }
    const T up = __shfl_up(incl, 1, kWave);
    *total = all;
    return lane ? op(before, up) : before;
}

// Minimum and maximum of a workgroup of THREADS threads, then atomicMin / atomicMax of their bit patterns into minmax[0] / [1].
// The values are >= +0 (or +-inf for a thread with nothing to offer): IEEE patterns of non-negative numbers order like the numbers,
// so unsigned integer atomics do.  U = unsigned long long keeps float64, U = unsigned int rounds to float32 first.  A workgroup with
// no value at all (mn = +inf > mx = -inf) leaves minmax alone.  red: 2 * THREADS / 64 doubles (see the LDS rule above).
template <int THREADS, typename U>
__device__ __forceinline__ void block_minmax_atomic(double mn, double mx, U* minmax, double* red) {
    mn = wave_min(mn);
    mx = wave_max(mx);
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red[2 * w] = mn;
        red[2 * w + 1] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < THREADS / kWave; ++k) {
            mn = fmin(mn, red[2 * k]);
            mx = fmax(mx, red[2 * k + 1]);
        }
        if (mn <= mx) {
            if constexpr (sizeof(U) == 8) {
                atomicMin(&minmax[0], (U)__double_as_longlong(mn));
                atomicMax(&minmax[1], (U)__double_as_longlong(mx));
            } else {
                atomicMin(&minmax[0], (U)__float_as_uint((float)mn));
                atomicMax(&minmax[1], (U)__float_as_uint((float)mx));
            }
        }
    }
}

}  // namespace avl
