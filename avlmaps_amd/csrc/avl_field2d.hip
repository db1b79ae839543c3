// 2-D goal fields of AVLMap's area, sound and image queries for gfx950, and their lift to the voxels.
//
// Replaces, in avlmaps/map/avlmap.py (upstream reference):
//   * index_area_2d  (:78-98)   one full-grid scipy distance_transform_edt per frame pose, folded with a running maximum:
//                                D = max over poses i inside the grid of clip(s_i - decay * ||cell - cell_i||, 0, 1), D starts at 0
//   * index_sound_2d (:111-133) one full-grid EDT per sound segment, summed into a float32 grid in segment order:
//                                D = f32(D + max(p_i - (p_i * min_j ||cell - cell_ij||) * decay, 0))
//   * index_area / index_sound (:100-109, :135-144) the min-max normalisation of D and the Python loop over occupied_ids
//     that copies D[row, col] to every voxel of the column
//   * index_image    (:146-163) sim = clip(1 - decay * ||grid_pos[:, :2] - (row, col)||, 0, 1), float64
//
// Exactness.  Distances between integer cells are square roots of exact integers (EDT returns the distance to the NEAREST
// marked cell, so min over the marked cells of the squared distance, then sqrt, is its value); sqrt and the divisions are
// correctly rounded in fp64 (and __fdiv_rn in fp32), and the file is compiled with -ffp-contract=off, so every product and
// difference rounds exactly where NumPy rounds it.  Given the same peaks the fields are the reference's bits.
//
// Work.  A workgroup owns a 16 x 16 tile of cells, one cell per thread.  Only poses / segments that can change a cell of the
// tile are evaluated:
//   * area: poses are streamed through LDS in chunks of 256; a pose is dropped (exactly: it cannot raise any cell of the tile)
//     when it lies outside the grid, when its clipped peak does not exceed the smallest running maximum of the tile, or when its
//     cone s_i - decay * d has become negative at the tile's nearest point (squared integer distance against the squared radius,
//     with a two-cell margin; no sqrt).  Survivors are compacted into LDS and every thread folds them into its cell.
//   * sound: segments are visited in order (the float32 sum is order-dependent); a segment whose every location is beyond the
//     cone radius 1 / decay of the whole tile adds exactly +0 and is skipped by the whole workgroup.
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_common.h"
#include "avl_wave.h"
#include "avl_field_math.h"

namespace avl {

constexpr int kFieldTile = 16;                    // tile edge in cells; the workgroup is kFieldTile^2 = 256 threads
constexpr int kFieldThreads = kFieldTile * kFieldTile;

// squared distance from (r, c) to the nearest cell of the tile [r0, r1] x [c0, c1]
__device__ __forceinline__ long long tile_d2(int r, int c, int r0, int r1, int c0, int c1) {
    const long long dr = r < r0 ? (long long)r0 - r : (r > r1 ? (long long)r - r1 : 0);
    const long long dc = c < c0 ? (long long)c0 - c : (c > c1 ? (long long)c - c1 : 0);
    return dr * dr + dc * dc;
}

__global__ __launch_bounds__(kFieldThreads) void field_area_kernel(const int32_t* __restrict__ cells, const double* __restrict__ peaks,
                                                                  int64_t P, int gs, double decay, double decay2,
                                                                  double* __restrict__ field, unsigned long long* __restrict__ minmax) {
    __shared__ int s_r[kFieldThreads], s_c[kFieldThreads];
    __shared__ double s_s[kFieldThreads];
    __shared__ double s_red[2 * kFieldThreads / kWave];
    __shared__ int s_n;
    const int r0 = blockIdx.y * kFieldTile, c0 = blockIdx.x * kFieldTile;
    const int r1 = min(r0 + kFieldTile, gs) - 1, c1 = min(c0 + kFieldTile, gs) - 1;
    const int r = r0 + (int)(threadIdx.x / kFieldTile), c = c0 + (int)(threadIdx.x % kFieldTile);
    const bool inside = r < gs && c < gs;
    const int w = threadIdx.x / kWave;
    double best = 0.0;
    for (int64_t base = 0; base < P; base += kFieldThreads) {
        // smallest running maximum of the tile: a pose whose clipped peak is not above it cannot raise any cell
        const double m = wave_min(inside ? best : 2.0);
        if ((threadIdx.x & (kWave - 1)) == 0) s_red[w] = m;
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        double tmin = s_red[0];
        for (int k = 1; k < kFieldThreads / kWave; ++k) tmin = fmin(tmin, s_red[k]);
        const int64_t j = base + threadIdx.x;
        if (j < P) {
            const int pr = cells[2 * j], pc = cells[2 * j + 1];
            const double s = peaks[j];
            bool keep = pr >= 0 && pr < gs && pc >= 0 && pc < gs && fmin(s, 1.0) > tmin;
            if (keep) {
                // the cone is <= -2 * decay (< 0) at the tile's nearest cell: every value it gives the tile clips to 0
                const long long d2 = tile_d2(pr, pc, r0, r1, c0, c1);
                const double reach = s + 2.0 * decay;
                if (d2 > 0 && decay2 * (double)d2 >= reach * reach) keep = false;
            }
            if (keep) {
                const int k = atomicAdd(&s_n, 1);
                s_r[k] = pr;
                s_c[k] = pc;
                s_s[k] = s;
            }
        }
        __syncthreads();
        const int n = s_n;
        if (inside) {
            for (int k = 0; k < n; ++k) {
                const double s = s_s[k];
                if (fmin(s, 1.0) <= best) continue;                       // clip(s - x) <= clip(s) for x >= 0
                const long long dr = (long long)r - s_r[k], dc = (long long)c - s_c[k];
                const double v = clip01(s - decay * sqrt((double)(dr * dr + dc * dc)));
                if (v > best) best = v;
            }
        }
        __syncthreads();                                                   // LDS is refilled by the next chunk
    }
    if (inside) field[(size_t)r * gs + c] = best;
    // min / max of the tile into d_minmax (non-negative values: their bit patterns order like the values)
    block_minmax_atomic<kFieldThreads>(inside ? best : INFINITY, inside ? best : -INFINITY, minmax, s_red);
}

__global__ __launch_bounds__(kFieldThreads) void field_sound_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ cells,
                                                                   int64_t L, const float* __restrict__ peaks, int64_t S, int gs,
                                                                   double decay, double decay2, double reach2,
                                                                   float* __restrict__ field, unsigned int* __restrict__ minmax) {
    __shared__ double s_red[2 * kFieldThreads / kWave];
    const int r0 = blockIdx.y * kFieldTile, c0 = blockIdx.x * kFieldTile;
    const int r1 = min(r0 + kFieldTile, gs) - 1, c1 = min(c0 + kFieldTile, gs) - 1;
    const int r = r0 + (int)(threadIdx.x / kFieldTile), c = c0 + (int)(threadIdx.x % kFieldTile);
    const bool inside = r < gs && c < gs;
    float acc = 0.0f;
    for (int64_t i = 0; i < S; ++i) {
        const float p = peaks[i];
        if (p == 0.0f) continue;                                           // adds exactly +0 everywhere
        int64_t b = offsets[i], e = offsets[i + 1];                       // (clamped to [0, L]: never read past the cells)
        b = b < 0 ? 0 : (b > L ? L : b);
        e = e < b ? b : (e > L ? L : e);
        // does some location reach the tile?  (p * d) * decay >= p * (1 + 2 decay) beyond the radius: the term clips to 0
        int reach = 0;
        for (int64_t k = b + threadIdx.x; k < e; k += kFieldThreads) {
            const long long d2 = tile_d2(cells[2 * k], cells[2 * k + 1], r0, r1, c0, c1);
            reach |= !(d2 > 0 && decay2 * (double)d2 >= reach2);
        }
        if (!__syncthreads_or(reach)) continue;
        if (inside) {
            long long dmin = LLONG_MAX;
            for (int64_t k = b; k < e; ++k) {
                const long long dr = (long long)r - cells[2 * k], dc = (long long)c - cells[2 * k + 1];
                dmin = min(dmin, dr * dr + dc * dc);
            }
            const double pd = (double)p;
            double t = pd - (pd * sqrt((double)dmin)) * decay;
            if (t < 0.0) t = 0.0;
            acc = (float)((double)acc + t);
        }
    }
    if (inside) field[(size_t)r * gs + c] = acc;
    block_minmax_atomic<kFieldThreads>(inside ? (double)acc : INFINITY, inside ? (double)acc : -INFINITY, minmax, s_red);
}

// heat[i] = f32((D[row, col] - min) / (max - min)) for the voxel's column, 0 for a voxel outside the (gs, gs, vh) grid -- the
// voxels the reference's occupied_ids loop never reaches
template <bool F64>
__global__ __launch_bounds__(256) void field_lift_kernel(const void* __restrict__ field, const void* __restrict__ minmax, int gs, int vh,
                                                         const int32_t* __restrict__ pos, int64_t N, float* __restrict__ heat) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = pos[3 * i], c = pos[3 * i + 1], h = pos[3 * i + 2];
        float v = 0.0f;
        if (in_grid(r, c, h, gs, vh)) {
            const size_t cell = (size_t)r * gs + c;
            if (F64) {
                const double* mm = static_cast<const double*>(minmax);
                v = lift_norm(static_cast<const double*>(field)[cell], mm[0], mm[1]);
            } else {
                const float* mm = static_cast<const float*>(minmax);
                v = lift_norm(static_cast<const float*>(field)[cell], mm[0], mm[1]);
            }
        }
        heat[i] = v;
    }
}

template <bool F64>
__global__ __launch_bounds__(256) void field_normalize_kernel(const void* __restrict__ field, const void* __restrict__ minmax, int64_t n,
                                                              void* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (F64) {
            const double* mm = static_cast<const double*>(minmax);
            static_cast<double*>(out)[i] = __ddiv_rn(static_cast<const double*>(field)[i] - mm[0], mm[1] - mm[0]);
        } else {
            const float* mm = static_cast<const float*>(minmax);
            static_cast<float*>(out)[i] = __fdiv_rn(static_cast<const float*>(field)[i] - mm[0], mm[1] - mm[0]);
        }
    }
}

// NumPy: d = grid_pos - [row, col, h] in float64, sqrt(d0 * d0 + d1 * d1), clip(1 - decay * dist, 0, 1)
__global__ __launch_bounds__(256) void planar_decay_kernel(const int32_t* __restrict__ pos, int64_t N, double row, double col, double decay,
                                                           double* __restrict__ sim) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        sim[i] = planar_cone(1.0, decay, pos[3 * i], pos[3 * i + 1], row, col);
    }
}

static unsigned grid_stride_blocks(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)num_cus() * 8));
}

}  // namespace avl

using namespace avl;

extern "C" int avl_field_area(const int32_t* d_cells, const double* d_peaks, int64_t P, int gs, double decay_rate, double* d_field,
                              double* d_minmax, void* stream) {
    AVL_REQUIRE(P >= 0 && gs > 0 && gs <= 32768, "avl_field_area: bad sizes (P %lld, gs %d)", (long long)P, gs);
    AVL_REQUIRE(decay_rate >= 0.0 && std::isfinite(decay_rate), "avl_field_area: decay_rate must be finite and >= 0");
    AVL_REQUIRE(d_field && d_minmax && (P == 0 || (d_cells && d_peaks)), "avl_field_area: null pointer");
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(d_minmax, 0xFF, sizeof(double), st));      // min: all ones = above every non-negative value
    AVL_HIP_CHECK(hipMemsetAsync(d_minmax + 1, 0, sizeof(double), st));     // max: +0
    const unsigned nt = (unsigned)((gs + kFieldTile - 1) / kFieldTile);
    hipLaunchKernelGGL(field_area_kernel, dim3(nt, nt), dim3(kFieldThreads), 0, st, d_cells, d_peaks, P, gs, decay_rate,
                       decay_rate * decay_rate, d_field, reinterpret_cast<unsigned long long*>(d_minmax));
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

extern "C" int avl_field_sound(const int64_t* d_offsets, const int32_t* d_cells, int64_t L, const float* d_peaks, int64_t S, int gs,
                               double decay_rate, float* d_field, float* d_minmax, void* stream) {
    AVL_REQUIRE(S >= 0 && L >= 0 && gs > 0 && gs <= 32768, "avl_field_sound: bad sizes (S %lld, L %lld, gs %d)", (long long)S,
                (long long)L, gs);
    AVL_REQUIRE(decay_rate >= 0.0 && std::isfinite(decay_rate), "avl_field_sound: decay_rate must be finite and >= 0");
    AVL_REQUIRE(d_field && d_minmax && (S == 0 || (d_offsets && d_peaks)) && (L == 0 || d_cells), "avl_field_sound: null pointer");
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(d_minmax, 0xFF, sizeof(float), st));
    AVL_HIP_CHECK(hipMemsetAsync(d_minmax + 1, 0, sizeof(float), st));
    const double reach = 1.0 + 2.0 * decay_rate;
    const unsigned nt = (unsigned)((gs + kFieldTile - 1) / kFieldTile);
    hipLaunchKernelGGL(field_sound_kernel, dim3(nt, nt), dim3(kFieldThreads), 0, st, d_offsets, d_cells, L, d_peaks, S, gs, decay_rate,
                       decay_rate * decay_rate, reach * reach, d_field, reinterpret_cast<unsigned int*>(d_minmax));
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

extern "C" int avl_field_lift(const void* d_field, int is_f64, const void* d_minmax, int gs, int vh, const int32_t* d_grid_pos, int64_t N,
                              float* d_heat, void* stream) {
    AVL_REQUIRE(N >= 0 && gs > 0 && vh >= 0, "avl_field_lift: bad sizes");
    if (N == 0) return AVL_OK;
    AVL_REQUIRE(d_field && d_minmax && d_grid_pos && d_heat, "avl_field_lift: null pointer");
    hipStream_t st = as_stream(stream);
    if (is_f64)
        hipLaunchKernelGGL(field_lift_kernel<true>, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_field, d_minmax, gs, vh, d_grid_pos, N, d_heat);
    else
        hipLaunchKernelGGL(field_lift_kernel<false>, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_field, d_minmax, gs, vh, d_grid_pos, N, d_heat);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

extern "C" int avl_field_normalize(const void* d_field, int is_f64, const void* d_minmax, int gs, void* d_out, void* stream) {
    AVL_REQUIRE(gs > 0 && gs <= 32768, "avl_field_normalize: bad grid size %d", gs);
    AVL_REQUIRE(d_field && d_minmax && d_out, "avl_field_normalize: null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)gs * gs;
    if (is_f64)
        hipLaunchKernelGGL(field_normalize_kernel<true>, dim3(grid_stride_blocks(n)), dim3(256), 0, st, d_field, d_minmax, n, d_out);
    else
        hipLaunchKernelGGL(field_normalize_kernel<false>, dim3(grid_stride_blocks(n)), dim3(256), 0, st, d_field, d_minmax, n, d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

extern "C" int avl_planar_decay(const int32_t* d_grid_pos, int64_t N, int64_t row, int64_t col, double decay_rate, double* d_sim,
                                void* stream) {
    AVL_REQUIRE(N >= 0, "avl_planar_decay: bad size");
    if (N == 0) return AVL_OK;
    AVL_REQUIRE(d_grid_pos && d_sim, "avl_planar_decay: null pointer");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(planar_decay_kernel, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_grid_pos, N, (double)row, (double)col,
                       decay_rate, d_sim);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}
