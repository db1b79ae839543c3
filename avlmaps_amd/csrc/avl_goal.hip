// Cross-modal goals for gfx950: the float64 product of up to 8 per-voxel heats and its first maximum, in one pass over the voxels.
//
// Replaces, in avlmaps/robot/habitat_lang_robot.py (upstream reference), what generated robot code does with host arrays:
//   * get_map_3d(obj=..) * get_major_map_3d(sound=..) * ...  (:377-425)   one (N,) NumPy product per factor
//   * get_max_pos_3d (:427-430)                                          grid_pos[np.argmax(heat)]
//   * get_distribution_map_3d (:207-227)                                 max over points of clip(con - decay * dist, 0, 1), in cells
//
// Exactness.  Every term is the stand-alone query's value bit for bit: the arithmetic lives in avl_field_math.h, which
// avl_field2d.hip uses too, and this file is compiled with -ffp-contract=off.  float32 terms widen to float64 exactly and the
// product is taken left to right, one rounded float64 multiplication per term, as NumPy multiplies the arrays.
//
// Work.  A workgroup of 256 threads walks the voxels in a grid-stride loop, one voxel per thread and step: grid_pos is read once
// whatever K is, dense terms are one coalesced load, field terms one gather from the 2-D field (4-8 MB at gs = 1000: it stays in
// L2), cone points are staged through LDS 256 at a time.  Nothing of size N is written unless the caller asks for the product.
//
// Reduction.  The key is (product descending, index ascending): a total order on the non-NaN products, so taking its best is
// associative and commutative and the result does not depend on how the voxels are split over lanes, waves and workgroups.  Lanes
// keep their best, a wave folds with shuffles, a workgroup through LDS, and every workgroup stores one (value, index) partial.  A
// second launch of one wave folds the partials and writes (index, value, grid_pos[index]) for one 32-byte copy to the host.  The
// kernel boundary is the only inter-workgroup hand-off: no flag, no counter to reset, no floating-point atomic.
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_common.h"
#include "avl_field_math.h"

namespace avl {

constexpr int kGoalThreads = 256;
constexpr int kGoalWaves = kGoalThreads / kWave;

struct GoalTerms {
    avl_goal_term t[AVL_GOAL_MAX_TERMS];
    int K;
};

struct GoalResult {                                   // what comes back to the host, one copy
    long long index;
    double value;
    int32_t pos[3];
    int32_t pad;
};

__device__ __forceinline__ bool goal_better(double v, long long i, double bv, long long bi) {
    return v > bv || (v == bv && i < bi);
}

__device__ __forceinline__ void wave_best(double& bv, long long& bi) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off, kWave);
        const long long oi = __shfl_xor(bi, off, kWave);
        if (goal_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}

__global__ __launch_bounds__(kGoalThreads) void goal_fuse_kernel(const GoalTerms a, const int32_t* __restrict__ pos, int64_t N,
                                                                double* __restrict__ out, double* __restrict__ part_v,
                                                                long long* __restrict__ part_i) {
    __shared__ int s_r[kGoalThreads], s_c[kGoalThreads];
    __shared__ double s_p[kGoalThreads];
    __shared__ double s_bv[kGoalWaves];
    __shared__ long long s_bi[kGoalWaves];
    double bv = -INFINITY;                            // (-inf, LLONG_MAX): below every non-NaN product at every index
    long long bi = LLONG_MAX;
    const int64_t step = (int64_t)gridDim.x * kGoalThreads;
    for (int64_t base = (int64_t)blockIdx.x * kGoalThreads; base < N; base += step) {      // uniform over the workgroup
        const int64_t i = base + threadIdx.x;
        const bool active = i < N;
        int r = 0, c = 0, h = 0;
        if (active) { r = pos[3 * i]; c = pos[3 * i + 1]; h = pos[3 * i + 2]; }
        double acc = 0.0;
        for (int k = 0; k < a.K; ++k) {
            const avl_goal_term& t = a.t[k];
            double v = 0.0;
            switch (t.kind) {                         // uniform: the terms are kernel arguments
            case AVL_GOAL_DENSE_F32:
                if (active) v = (double)static_cast<const float*>(t.d_data)[i];
                break;
            case AVL_GOAL_DENSE_F64:
                if (active) v = static_cast<const double*>(t.d_data)[i];
                break;
            case AVL_GOAL_FIELD_F32:
                if (active && in_grid(r, c, h, t.gs, t.vh)) {
                    const float* mm = static_cast<const float*>(t.d_aux);
                    v = (double)lift_norm(static_cast<const float*>(t.d_data)[(size_t)r * t.gs + c], mm[0], mm[1]);
                }
                break;
            case AVL_GOAL_FIELD_F64:
                if (active && in_grid(r, c, h, t.gs, t.vh)) {
                    const double* mm = static_cast<const double*>(t.d_aux);
                    v = (double)lift_norm(static_cast<const double*>(t.d_data)[(size_t)r * t.gs + c], mm[0], mm[1]);
                }
                break;
            default: {                                // AVL_GOAL_CONES (the kinds are validated on the host)
                const int32_t* cells = static_cast<const int32_t*>(t.d_data);
                const double* peaks = static_cast<const double*>(t.d_aux);
                for (int64_t p0 = 0; p0 < t.n_points; p0 += kGoalThreads) {
                    const int n = (int)min((int64_t)kGoalThreads, t.n_points - p0);
                    __syncthreads();                  // the previous chunk (or term, or step) has been read
                    if ((int)threadIdx.x < n) {
                        const int64_t j = p0 + threadIdx.x;
                        s_r[threadIdx.x] = cells[2 * j];
                        s_c[threadIdx.x] = cells[2 * j + 1];
                        s_p[threadIdx.x] = peaks[j];
                    }
                    __syncthreads();
                    if (active) {
                        for (int j = 0; j < n; ++j) {
                            const double pk = s_p[j];
                            if (fmin(pk, 1.0) <= v) continue;                      // clip(pk - x) <= clip(pk) for x >= 0
                            const double w = planar_cone(pk, t.decay, r, c, (double)s_r[j], (double)s_c[j]);
                            if (w > v) v = w;
                        }
                    }
                }
            }
            }
            acc = k == 0 ? v : acc * v;
        }
        if (active) {
            if (out) out[i] = acc;
            if (goal_better(acc, i, bv, bi)) { bv = acc; bi = i; }
        }
    }
    wave_best(bv, bi);
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) { s_bv[w] = bv; s_bi[w] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kGoalWaves; ++k)
            if (goal_better(s_bv[k], s_bi[k], bv, bi)) { bv = s_bv[k]; bi = s_bi[k]; }
        part_v[blockIdx.x] = bv;
        part_i[blockIdx.x] = bi;
    }
}

// one wave: the best of the workgroups' partials, and grid_pos of that voxel
__global__ __launch_bounds__(kWave) void goal_finish_kernel(const double* __restrict__ part_v, const long long* __restrict__ part_i, int nb,
                                                           const int32_t* __restrict__ pos, GoalResult* __restrict__ res) {
    double bv = -INFINITY;
    long long bi = LLONG_MAX;
    for (int b = threadIdx.x; b < nb; b += kWave)
        if (goal_better(part_v[b], part_i[b], bv, bi)) { bv = part_v[b]; bi = part_i[b]; }
    wave_best(bv, bi);
    if (threadIdx.x == 0) {
        res->index = bi;
        res->value = bv;
        for (int k = 0; k < 3; ++k) res->pos[k] = (bi == LLONG_MAX || !pos) ? 0 : pos[3 * bi + k];   // (LLONG_MAX: every product is NaN)
        res->pad = 0;
    }
}

// ---------------------------------------------------------------------------------------------- 2-D windows
struct WindowTerms {
    avl_window_term t[AVL_GOAL_MAX_TERMS];
    int K;
};

// the product of K (h, w) windows, left to right in float64, and its first maximum in raster order: index = row * w + col
__global__ __launch_bounds__(kGoalThreads) void window_product_kernel(const WindowTerms a, int h, int w, double* __restrict__ out,
                                                                     double* __restrict__ part_v, long long* __restrict__ part_i) {
    __shared__ double s_bv[kGoalWaves];
    __shared__ long long s_bi[kGoalWaves];
    double bv = -INFINITY;
    long long bi = LLONG_MAX;
    const int64_t n = (int64_t)h * w;
    for (int64_t i = (int64_t)blockIdx.x * kGoalThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kGoalThreads) {
        const int64_t r = i / w, c = i - r * w;
        double acc = 0.0;
        for (int k = 0; k < a.K; ++k) {
            const avl_window_term& t = a.t[k];
            const int64_t at = r * t.ld + c;
            const double v = t.is_f64 ? static_cast<const double*>(t.d_data)[at] : (double)static_cast<const float*>(t.d_data)[at];
            acc = k == 0 ? v : acc * v;
        }
        if (out) out[i] = acc;
        if (goal_better(acc, i, bv, bi)) { bv = acc; bi = i; }
    }
    wave_best(bv, bi);
    const int wv = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) { s_bv[wv] = bv; s_bi[wv] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kGoalWaves; ++k)
            if (goal_better(s_bv[k], s_bi[k], bv, bi)) { bv = s_bv[k]; bi = s_bi[k]; }
        part_v[blockIdx.x] = bv;
        part_i[blockIdx.x] = bi;
    }
}

}  // namespace avl

using namespace avl;

extern "C" int avl_product_argmax_2d(const avl_window_term* h_terms, int K, int h, int w, double* d_out, int64_t* h_index, double* h_value,
                                     void* stream) {
    AVL_REQUIRE(h_terms, "avl_product_argmax_2d: null terms");
    AVL_REQUIRE(K >= 1 && K <= AVL_GOAL_MAX_TERMS, "avl_product_argmax_2d: K = %d terms, need 1 .. %d", K, AVL_GOAL_MAX_TERMS);
    AVL_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "avl_product_argmax_2d: bad window %d x %d", h, w);
    WindowTerms a;
    a.K = K;
    for (int k = 0; k < AVL_GOAL_MAX_TERMS; ++k) a.t[k] = avl_window_term{};
    for (int k = 0; k < K; ++k) {
        AVL_REQUIRE(h_terms[k].d_data, "avl_product_argmax_2d: term %d: null data pointer", k);
        AVL_REQUIRE(h_terms[k].ld >= w, "avl_product_argmax_2d: term %d: rows of %lld values cannot hold %d columns", k,
                    (long long)h_terms[k].ld, w);
        a.t[k] = h_terms[k];
    }
    AVL_REQUIRE(d_out || h_index || h_value, "avl_product_argmax_2d: no output requested");
    hipStream_t st = as_stream(stream);
    const int64_t n = (int64_t)h * w;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + kGoalThreads - 1) / kGoalThreads, (int64_t)num_cus() * 8));
    const size_t off_i = (size_t)nb * sizeof(double), off_res = off_i + (size_t)nb * sizeof(long long);
    char* sc = static_cast<char*>(avl::scratch(off_res + sizeof(GoalResult)));
    if (!sc) return AVL_ERR_HIP;
    double* d_pv = reinterpret_cast<double*>(sc);
    long long* d_pi = reinterpret_cast<long long*>(sc + off_i);
    GoalResult* d_res = reinterpret_cast<GoalResult*>(sc + off_res);
    hipLaunchKernelGGL(window_product_kernel, dim3((unsigned)nb), dim3(kGoalThreads), 0, st, a, h, w, d_out, d_pv, d_pi);
    AVL_HIP_CHECK(hipGetLastError());
    if (!h_index && !h_value) return AVL_OK;
    hipLaunchKernelGGL(goal_finish_kernel, dim3(1), dim3(kWave), 0, st, d_pv, d_pi, nb, (const int32_t*)nullptr, d_res);
    AVL_HIP_CHECK(hipGetLastError());
    GoalResult res;
    AVL_HIP_CHECK(hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    AVL_REQUIRE(res.index != LLONG_MAX, "avl_product_argmax_2d: every product is NaN");
    if (h_index) *h_index = res.index;
    if (h_value) *h_value = res.value;
    return AVL_OK;
}

extern "C" int avl_goal_fuse(const avl_goal_term* h_terms, int K, const int32_t* d_grid_pos, int64_t N, double* d_out, int64_t* h_index,
                             double* h_value, int32_t* h_pos3, void* stream) {
    AVL_REQUIRE(h_terms, "avl_goal_fuse: null terms");
    AVL_REQUIRE(K >= 1 && K <= AVL_GOAL_MAX_TERMS, "avl_goal_fuse: K = %d terms, need 1 .. %d", K, AVL_GOAL_MAX_TERMS);
    AVL_REQUIRE(N >= 0, "avl_goal_fuse: bad size (N %lld)", (long long)N);
    GoalTerms a;
    a.K = K;
    for (int k = 0; k < AVL_GOAL_MAX_TERMS; ++k) a.t[k] = avl_goal_term{};
    for (int k = 0; k < K; ++k) {
        const avl_goal_term& t = h_terms[k];
        switch (t.kind) {
        case AVL_GOAL_DENSE_F32:
        case AVL_GOAL_DENSE_F64:
            AVL_REQUIRE(t.d_data || N == 0, "avl_goal_fuse: term %d (dense): null data pointer", k);
            break;
        case AVL_GOAL_FIELD_F32:
        case AVL_GOAL_FIELD_F64:
            AVL_REQUIRE(t.gs >= 1 && t.gs <= 32768 && t.vh >= 0, "avl_goal_fuse: term %d (field): bad grid (gs %d, vh %d)", k, t.gs, t.vh);
            AVL_REQUIRE(t.d_data && t.d_aux, "avl_goal_fuse: term %d (field): null field or minmax pointer", k);
            break;
        case AVL_GOAL_CONES:
            AVL_REQUIRE(t.n_points >= 1, "avl_goal_fuse: term %d (cones): P = %lld points, need >= 1", k, (long long)t.n_points);
            AVL_REQUIRE(t.decay >= 0.0 && std::isfinite(t.decay), "avl_goal_fuse: term %d (cones): decay must be finite and >= 0", k);
            AVL_REQUIRE(t.d_data && t.d_aux, "avl_goal_fuse: term %d (cones): null cells or peaks pointer", k);
            break;
        default:
            AVL_REQUIRE(false, "avl_goal_fuse: term %d: unknown kind %d", k, (int)t.kind);
        }
        a.t[k] = t;
    }
    const bool want_host = h_index || h_value || h_pos3;
    AVL_REQUIRE(!(want_host && N == 0), "avl_goal_fuse: an empty map has no goal (N = 0)");
    if (N == 0) return AVL_OK;
    AVL_REQUIRE(d_grid_pos, "avl_goal_fuse: null grid_pos pointer");
    hipStream_t st = as_stream(stream);
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((N + kGoalThreads - 1) / kGoalThreads, (int64_t)num_cus() * 8));
    // partials and the result live in the library's per-thread scratch: no allocation per call
    const size_t off_i = (size_t)nb * sizeof(double), off_res = off_i + (size_t)nb * sizeof(long long);
    char* sc = static_cast<char*>(avl::scratch(off_res + sizeof(GoalResult)));
    if (!sc) return AVL_ERR_HIP;
    double* d_pv = reinterpret_cast<double*>(sc);
    long long* d_pi = reinterpret_cast<long long*>(sc + off_i);
    GoalResult* d_res = reinterpret_cast<GoalResult*>(sc + off_res);
    hipLaunchKernelGGL(goal_fuse_kernel, dim3((unsigned)nb), dim3(kGoalThreads), 0, st, a, d_grid_pos, N, d_out, d_pv, d_pi);
    AVL_HIP_CHECK(hipGetLastError());
    if (!want_host) return AVL_OK;
    hipLaunchKernelGGL(goal_finish_kernel, dim3(1), dim3(kWave), 0, st, d_pv, d_pi, nb, d_grid_pos, d_res);
    AVL_HIP_CHECK(hipGetLastError());
    GoalResult res;
    AVL_HIP_CHECK(hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    AVL_REQUIRE(res.index != LLONG_MAX, "avl_goal_fuse: every product is NaN");
    if (h_index) *h_index = res.index;
    if (h_value) *h_value = res.value;
    if (h_pos3)
        for (int k = 0; k < 3; ++k) h_pos3[k] = res.pos[k];
    return AVL_OK;
}
