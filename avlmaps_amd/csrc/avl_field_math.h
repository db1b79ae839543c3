// Per-voxel arithmetic of the goal queries, shared by the stand-alone kernels (avl_field2d.hip) and the fused goal kernel
// (avl_goal.hip), so that a term of the fused product is the stand-alone query's value bit for bit.  Every translation unit that
// includes this file is compiled with -ffp-contract=off: each product, difference and quotient rounds where NumPy rounds it.
#pragma once
#include "avl_common.h"

namespace avl {

__device__ __forceinline__ double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

// avlmaps/map/avlmap.py:97,132 (min-max normalisation of the 2-D map) and the float32 store of :100-109 / :135-144
__device__ __forceinline__ float lift_norm(double v, double mn, double mx) { return (float)__ddiv_rn(v - mn, mx - mn); }
__device__ __forceinline__ float lift_norm(float v, float mn, float mx) { return __fdiv_rn(v - mn, mx - mn); }

// the voxel (r, c, h) lies inside the (gs, gs, vh) grid: the voxels the reference's loop over occupied_ids reaches
__device__ __forceinline__ bool in_grid(int r, int c, int h, int gs, int vh) {
    return r >= 0 && r < gs && c >= 0 && c < gs && h >= 0 && h < vh;
}

// avlmaps/map/avlmap.py:154-161 with peak = 1, robot/habitat_lang_robot.py:219-220 in cells: clip(peak - decay * ||(r, c) - (row, col)||, 0, 1).
// The differences of int32 coordinates and their squares are exact in float64 up to 2^53, far beyond any map, so the radicand is the
// integer squared distance and the one correctly rounded sqrt is NumPy's.
__device__ __forceinline__ double planar_cone(double peak, double decay, int r, int c, double row, double col) {
    const double dx = (double)r - row, dy = (double)c - col;
    return clip01(peak - decay * sqrt(dx * dx + dy * dy));
}

}  // namespace avl
