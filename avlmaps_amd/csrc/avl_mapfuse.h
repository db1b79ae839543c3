// The small device helpers that the two resamplers of finished voxel maps share: avl_mapfuse.hip (the forward move, the join and the
// weighted mean) and avl_mappull.hip (the backward gather).  Both sources are built with
// -ffp-contract=off: every product and sum below rounds once.
#pragma once
#include "avl_cellindex.h"

namespace avl {

constexpr int kMfMaxDim = 8192;

struct MfTransform {
    double t[12];
};

// upstream's int(gs / 2 - int(q)) for q = x / cs with |q| < 2^31
__device__ __forceinline__ int64_t mf_index(double q, int gs) { return (int64_t)((double)gs / 2.0 - (double)(int64_t)q); }

__device__ __forceinline__ bool mf_weight_ok(float w) { return w > 0.0f && w < __builtin_inff(); }     // false for a NaN

__device__ __forceinline__ int mf_lin(const int32_t* __restrict__ cells, int64_t i, int gs, int vh) {
    return (int)ci_linear(cells[3 * i], cells[3 * i + 1], cells[3 * i + 2], gs, vh);                    // -1 outside; inside < 2^31
}

// every lane of the wave calls it
__device__ __forceinline__ void mf_count(bool p, int32_t* counter) {
    const int c = __popcll(__ballot(p));
    if ((threadIdx.x & (kWave - 1)) == 0 && c) atomicAdd(counter, c);
}

// the four elements d .. d + 3 of a row (d < D), zeros past D; `vec`: D % 4 == 0 and the row is 16-byte aligned
__device__ __forceinline__ float4 mf_load4(const float* __restrict__ row, int d, int D, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(row + d);
    float4 v;
    v.x = row[d];
    v.y = d + 1 < D ? row[d + 1] : 0.0f;
    v.z = d + 2 < D ? row[d + 2] : 0.0f;
    v.w = d + 3 < D ? row[d + 3] : 0.0f;
    return v;
}

struct MfAcc {
    double x, y, z, w;
    bool any;
    __device__ __forceinline__ void add(double wi, float4 f) {
        const double px = wi * (double)f.x, py = wi * (double)f.y, pz = wi * (double)f.z, pw = wi * (double)f.w;
        if (any) x = x + px, y = y + py, z = z + pz, w = w + pw;
        else x = px, y = py, z = pz, w = pw, any = true;
    }
};

}  // namespace avl
