// The decay of a 2-D distance map and its min-max normalisation, shared by the Euclidean maps (avl_edt2d.hip) and the travel maps
// (avl_travel.hip): one expression, one [min, max] pair kept by bit pattern, one normalisation kernel.  Both sources are compiled
// with -ffp-contract=off: every operation here rounds like NumPy's float64 expression.
#pragma once
#include <algorithm>

#include "avl_common.h"
#include "avl_wave.h"

namespace avl {

// NumPy: t = 1 - (d / cell_size) * decay_rate, t < 0 -> 0
__device__ __forceinline__ double decay_value(double d, double cell_size, double decay_rate) {
    const double t = 1.0 - __ddiv_rn(d, cell_size) * decay_rate;
    return t < 0.0 ? 0.0 : t;
}

// [min, max] of values >= +0 as block_minmax_atomic keeps them (IEEE patterns of non-negative numbers order like the numbers):
// the identity of the minimum is all ones, that of the maximum +0
static inline int decay_minmax_reset(double* minmax, hipStream_t st) {
    AVL_HIP_CHECK(hipMemsetAsync(minmax, 0xFF, sizeof(double), st));
    AVL_HIP_CHECK(hipMemsetAsync(minmax + 1, 0, sizeof(double), st));
    return AVL_OK;
}

// NumPy: (t - min) / (max - min), in place (field_normalize_kernel's expression on an (H, W) image); max == min divides by zero as
// NumPy does.  CONSTANT_FLAG: constant[0] = 1 when max > min does not hold, else 0, for a caller without [min, max] on the host.
template <bool CONSTANT_FLAG>
__global__ __launch_bounds__(256) void decay_normalize_kernel(double* __restrict__ t, const double* __restrict__ minmax, int64_t n,
                                                              int32_t* __restrict__ constant) {
    const double mn = minmax[0], span = minmax[1] - minmax[0];
    if (CONSTANT_FLAG && blockIdx.x == 0 && threadIdx.x == 0) constant[0] = minmax[1] > minmax[0] ? 0 : 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        t[i] = __ddiv_rn(t[i] - mn, span);
}

static inline int decay_normalize(double* t, const double* minmax, int64_t n, int32_t* constant, hipStream_t st) {
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)num_cus() * 8));
    if (constant)
        hipLaunchKernelGGL(decay_normalize_kernel<true>, dim3(blocks), dim3(256), 0, st, t, minmax, n, constant);
    else
        hipLaunchKernelGGL(decay_normalize_kernel<false>, dim3(blocks), dim3(256), 0, st, t, minmax, n, (int32_t*)nullptr);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // namespace avl
