// The pinhole back-projection and the pose product of K1 (bp_voxelize_body, avl_builder.hip), shared with the bounding-box pass
// (avl_finalize.hip) and the free-space carver (avl_explore.hip): one definition of the arithmetic every kernel that turns a depth
// pixel into a map point has to reproduce bit for bit (oracle/avl_oracle.c: avlo_depth2pc_pixel, avlo_transform_point).  The files
// that include it are compiled with -ffp-contract=off: the only fused multiply-adds are the explicit fma() below.
#pragma once
#include "avl_common.h"

namespace avl {

__device__ __forceinline__ int py_int(double v) {
    // Python int(): truncate toward zero.  Far-out values saturate at +-2e9 and NaN goes to -2e9 (all of them fail the range
    // tests that follow: grid, image and feature-image bounds are far below that), which lets the conversion be ONE instruction
    // (v_cvt_i32_f64) instead of the ~15 of a float64 -> int64 conversion -- five of those sat on every sample's chain in K1.
    return (int)fmin(fmax(v, -2.0e9), 2.0e9);
}

// depth2pc: p_2d = (x, y, 1) with x = u + 0.5, y = v + 0.5; pc = Kinv @ p_2d (dgemm: FMA chain over k); pc *= z
__device__ __forceinline__ void bp_backproject(const double* kinv, double x, double y, double z, double& p0, double& p1, double& p2) {
    p0 = fma(kinv[2], 1.0, fma(kinv[1], y, kinv[0] * x)) * z;
    p1 = fma(kinv[5], 1.0, fma(kinv[4], y, kinv[3] * x)) * z;
    p2 = fma(kinv[8], 1.0, fma(kinv[7], y, kinv[6] * x)) * z;
}

// transform_pc: pose @ [pc; 1]  (dgemm FMA chain k = 0..3); T: the first three rows of the 4 x 4 pose, row-major
__device__ __forceinline__ void bp_transform(const double* T, double p0, double p1, double p2, double& g0, double& g1, double& g2) {
    g0 = fma(T[3], 1.0, fma(T[2], p2, fma(T[1], p1, T[0] * p0)));
    g1 = fma(T[7], 1.0, fma(T[6], p2, fma(T[5], p1, T[4] * p0)));
    g2 = fma(T[11], 1.0, fma(T[10], p2, fma(T[9], p1, T[8] * p0)));
}

}  // namespace avl
