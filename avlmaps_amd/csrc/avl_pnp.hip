// Image localization geometry for gfx950: depth lift of matched key points, P3P RANSAC, inlier scoring, pose refinement.
//
// Replaces (upstream reference, path:line):
//   avlmaps/utils/localization_utils.py:461-473   the depth2pc + fancy-index + mask of _get_relative_pose_with_depth
//   avlmaps/utils/mapping_utils.py:226-251        depth2pc, evaluated only at the matched pixels
//   avlmaps/utils/localization_utils.py:478-498   pycolmap.absolute_pose_estimation (SIMPLE_PINHOLE, max_error, fixed focal length)
// All arithmetic is float64 and lives in avl_pnp_math.h; this file is compiled with -ffp-contract=off.
//
// Sampling hash (restated on the host by ops.pnp_sample_indices):
//   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16            (uint32, wrapping)
//   word(seed, h, d) = mix(mix(mix(seed ^ 0x9e3779b9) + h) + d)
//   i0 = word(seed, h, 0) % m;   j = word(seed, h, 1) % (m - 1), i1 = j + (j >= i0);
//   k = word(seed, h, 2) % (m - 2), k += (k >= min(i0, i1)), k += (k >= max(i0, i1)), i2 = k
// No state and no atomics: hypothesis h is a function of (seed, h, m), whatever the launch shape.
//
// Shape of the RANSAC and scoring kernels: one wave per hypothesis (pose), four waves per block; the correspondences pass through
// LDS in stages of kStage = 1024 (five float64 planes, 40 KiB) that the four waves of a block share; each lane counts the
// correspondences lane, lane + 64, ... of a stage and the 64 integer counts are summed across the wave.  Integer sums only: the
// counts do not depend on the order.  The winner is picked by a second, single-block kernel on the key (count, -h).
#include "avl_common.h"
#include "avl_wave.h"
#include "avl_pnp_math.h"

namespace avl {

using namespace pnp;

constexpr int kStage = 1024;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int64_t kMaxM = 1ll << 24;

constexpr int kLiftErrPixel = 1;

struct Stage {
    double X[kStage], Y[kStage], Z[kStage], U[kStage], V[kStage];
};

struct Mat3 {
    double m[9];
};

__device__ __forceinline__ void load_stage(Stage& s, const double* __restrict__ pts, const double* __restrict__ pix, int64_t base, int n) {
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const int64_t g = base + i;
        s.X[i] = pts[3 * g];
        s.Y[i] = pts[3 * g + 1];
        s.Z[i] = pts[3 * g + 2];
        s.U[i] = pix[2 * g];
        s.V[i] = pix[2 * g + 1];
    }
}

// Counts the inliers of `np` (<= NP) poses held by this wave over all M correspondences; every wave of the block must call it
// (the stages are loaded by the whole block).  active = false: the wave only helps loading.  mask0: inlier mask of pose 0 or null.
template <int NP>
__device__ __forceinline__ void count_staged(Stage& st, const double* __restrict__ pts, const double* __restrict__ pix, int64_t M,
                                             const double* poses, int np, bool active, const Camera& cam, int* cnt, uint8_t* mask0) {
    const int lane = threadIdx.x & (kWave - 1);
    for (int s = 0; s < NP; ++s) cnt[s] = 0;
    for (int64_t base = 0; base < M; base += kStage) {
        const int n = (int)((M - base) < kStage ? (M - base) : kStage);
        __syncthreads();
        load_stage(st, pts, pix, base, n);
        __syncthreads();
        if (!active) continue;
        for (int i = lane; i < n; i += kWave) {
            const double X = st.X[i], Y = st.Y[i], Z = st.Z[i], U = st.U[i], V = st.V[i];
#pragma unroll
            for (int s = 0; s < NP; ++s) {
                if (s < np) {
                    const bool in = inlier(poses + 12 * s, cam, X, Y, Z, U, V);
                    cnt[s] += in ? 1 : 0;
                    if (s == 0 && mask0) mask0[base + i] = in ? 1 : 0;
                }
            }
        }
    }
    for (int s = 0; s < NP; ++s) cnt[s] = wave_sum(cnt[s]);
}

// ---- lift -----------------------------------------------------------------------------------------------------------------
// One block walks the M pairs in chunks of 256 in input order; kept pairs are compacted with a ballot prefix per wave and the
// four wave counts per chunk, so the output order is the input order.  counter[0] = M', counter[1] = error bits.
__global__ __launch_bounds__(kBlock) void loc_lift_kernel(const void* __restrict__ depth, int is_f64, int H, int W, Mat3 Kinv,
                                                          const double* __restrict__ kp_ref, const double* __restrict__ kp_query, int64_t M,
                                                          double* __restrict__ out_pts, double* __restrict__ out_pix, int* __restrict__ counter) {
    __shared__ int wcount[kWavesPerBlock];
    int64_t run = 0;
    for (int64_t base = 0; base < M; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        bool keep = false;
        double px = 0.0, py = 0.0, pz = 0.0;
        if (i < M) {
            const double x = kp_ref[2 * i], y = kp_ref[2 * i + 1];
            if (!(fabs(x) < 2147483648.0) || !(fabs(y) < 2147483648.0)) {
                atomicOr(&counter[1], kLiftErrPixel);
            } else {
                const int xi = (int)x, yi = (int)y;      // astype(np.int32): toward zero
                if (xi < 0 || xi >= W || yi < 0 || yi >= H) {
                    atomicOr(&counter[1], kLiftErrPixel);
                } else {
                    const int64_t o = (int64_t)yi * W + xi;
                    const double z = is_f64 ? ((const double*)depth)[o] : (double)((const float*)depth)[o];
                    const double u = (double)xi + 0.5, v = (double)yi + 0.5;
                    px = ((Kinv.m[0] * u + Kinv.m[1] * v) + Kinv.m[2]) * z;
                    py = ((Kinv.m[3] * u + Kinv.m[4] * v) + Kinv.m[5]) * z;
                    pz = ((Kinv.m[6] * u + Kinv.m[7] * v) + Kinv.m[8]) * z;
                    keep = pz > 0.1 && pz < 10.0;
                }
            }
        }
        int total;
        const int64_t o = run + block_compact_rank<kWavesPerBlock>(keep, wcount, &total);
        if (keep) {
            out_pts[3 * o] = px;
            out_pts[3 * o + 1] = py;
            out_pts[3 * o + 2] = pz;
            out_pix[2 * o] = kp_query[2 * i];
            out_pix[2 * o + 1] = kp_query[2 * i + 1];
        }
        run += total;
        __syncthreads();                                 // wcount is rewritten by the next chunk
    }
    if (threadIdx.x == 0) counter[0] = (int)run;
}

// ---- RANSAC ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pnp_ransac_kernel(const double* __restrict__ pts, const double* __restrict__ pix, int64_t M,
                                                            Camera cam, uint32_t seed, int n_hyp, int32_t* __restrict__ triples,
                                                            int32_t* __restrict__ hyp_counts, double* __restrict__ hyp_poses) {
    __shared__ Stage st;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int h = blockIdx.x * kWavesPerBlock + wave;
    const bool active = h < n_hyp;
    double poses[48];
    int ns = 0;
    int32_t idx[3] = {0, 0, 0};
    if (active) {
        sample_triple(seed, (uint32_t)h, (uint32_t)M, idx);
        double X[9], px[6];
        for (int k = 0; k < 3; ++k) {
            const int64_t g = idx[k];
            X[3 * k] = pts[3 * g];
            X[3 * k + 1] = pts[3 * g + 1];
            X[3 * k + 2] = pts[3 * g + 2];
            px[2 * k] = pix[2 * g];
            px[2 * k + 1] = pix[2 * g + 1];
        }
        ns = p3p(X, px, cam, poses);
    }
    int cnt[4];
    count_staged<4>(st, pts, pix, M, poses, ns, active, cam, cnt, nullptr);
    if (!active) return;
    int best = -1, best_cnt = 0;
    for (int s = 0; s < 4; ++s)
        if (s < ns && (best < 0 || cnt[s] > best_cnt)) {      // ties: the smallest solution index
            best = s;
            best_cnt = cnt[s];
        }
    if (lane < 12) {
        double v = (lane % 5 == 0) ? 1.0 : 0.0;      // [I|0] for a hypothesis without a solution
        for (int s = 0; s < 4; ++s)
            if (s == best) v = poses[12 * s + lane];
        hyp_poses[(int64_t)h * 12 + lane] = v;
    }
    if (lane == 12) hyp_counts[h] = best_cnt;
    if (triples && lane >= 13 && lane < 16) triples[(int64_t)h * 3 + (lane - 13)] = idx[lane - 13];
}

// winner = the largest (count, -h): one block, an integer key per hypothesis, a fixed LDS tree
__global__ __launch_bounds__(kBlock) void pnp_select_kernel(const int32_t* __restrict__ hyp_counts, const double* __restrict__ hyp_poses,
                                                            int n_hyp, double* __restrict__ out_pose, int32_t* __restrict__ out_count) {
    __shared__ unsigned long long keys[kBlock];
    unsigned long long best = 0ull;
    for (int h = threadIdx.x; h < n_hyp; h += kBlock) {
        const unsigned long long key = ((unsigned long long)(uint32_t)hyp_counts[h] << 32) | (unsigned long long)(0x7fffffffu - (uint32_t)h);
        best = key > best ? key : best;
    }
    keys[threadIdx.x] = best;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) keys[threadIdx.x] = keys[threadIdx.x + o] > keys[threadIdx.x] ? keys[threadIdx.x + o] : keys[threadIdx.x];
        __syncthreads();
    }
    const unsigned long long k = keys[0];
    const int h = (int)(0x7fffffffu - (uint32_t)(k & 0xffffffffull));
    if (threadIdx.x < 12) out_pose[threadIdx.x] = hyp_poses[(int64_t)h * 12 + threadIdx.x];
    if (threadIdx.x == 12) out_count[0] = (int32_t)(k >> 32);
}

// ---- scoring --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pnp_score_kernel(const double* __restrict__ pts, const double* __restrict__ pix, int64_t M,
                                                           const double* __restrict__ d_poses, int P, Camera cam, int32_t* __restrict__ counts,
                                                           uint8_t* __restrict__ mask0) {
    __shared__ Stage st;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int p = blockIdx.x * kWavesPerBlock + wave;
    const bool active = p < P;
    double pose[12];
    for (int k = 0; k < 12; ++k) pose[k] = active ? d_poses[(int64_t)p * 12 + k] : 0.0;
    int cnt[1];
    count_staged<1>(st, pts, pix, M, pose, 1, active, cam, cnt, (active && p == 0) ? mask0 : nullptr);
    if (active && lane == 0) counts[p] = cnt[0];
}

// ---- refinement -----------------------------------------------------------------------------------------------------------
// Levenberg-Marquardt in ONE launch of one block.  Every pass over the correspondences gives thread t the terms of t, t + 256, ...
// in that order; the 28 sums are then added across each wave by a fixed xor butterfly and across the four waves in wave order by
// thread 0, which also solves the 6 x 6 system and decides.  Nothing depends on scheduling.
struct RefineShared {
    double wave_acc[kWavesPerBlock][kNormal];
    int wave_bad[kWavesPerBlock];
    double cur[12], cand[12], acc[kNormal];
    int done, n_used, count;
};

__device__ __forceinline__ void refine_pass(RefineShared& sh, const double* pose_sh, const double* __restrict__ pts,
                                            const double* __restrict__ pix, int64_t M, const uint8_t* __restrict__ used, const Camera& cam,
                                            double* total, int* bad_out) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    double P[12], acc[kNormal];
    for (int k = 0; k < 12; ++k) P[k] = pose_sh[k];
    for (int k = 0; k < kNormal; ++k) acc[k] = 0.0;
    int bad = 0;
    for (int64_t i = threadIdx.x; i < M; i += kBlock) {
        if (!used[i]) continue;
        if (!normal_terms(P, cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], pix[2 * i], pix[2 * i + 1], acc)) bad = 1;
    }
    for (int k = 0; k < kNormal; ++k) acc[k] = wave_sum(acc[k]);
    bad = wave_sum(bad);
    if (lane == 0) {
        for (int k = 0; k < kNormal; ++k) sh.wave_acc[wave][k] = acc[k];
        sh.wave_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int b = 0;
        for (int k = 0; k < kNormal; ++k) {
            double s = sh.wave_acc[0][k];
            for (int w = 1; w < kWavesPerBlock; ++w) s += sh.wave_acc[w][k];
            total[k] = s;
        }
        for (int w = 0; w < kWavesPerBlock; ++w) b += sh.wave_bad[w];
        *bad_out = b;
    }
    __syncthreads();
}

// out_f64: 12 pose + cost; out_i32: iterations, inlier count of the refined pose, correspondences refined on
__global__ __launch_bounds__(kBlock) void pnp_refine_kernel(const double* __restrict__ pts, const double* __restrict__ pix, int64_t M,
                                                            const double* __restrict__ pose_in, Camera cam, int max_iter, double step_tol,
                                                            double* __restrict__ out_f64, int32_t* __restrict__ out_i32,
                                                            uint8_t* __restrict__ mask) {
    __shared__ RefineShared sh;
    if (threadIdx.x < 12) sh.cur[threadIdx.x] = pose_in[threadIdx.x];
    if (threadIdx.x == 0) {
        sh.done = 0;
        sh.n_used = 0;
        sh.count = 0;
    }
    __syncthreads();
    {
        double P[12];
        for (int k = 0; k < 12; ++k) P[k] = sh.cur[k];
        int mine = 0;
        for (int64_t i = threadIdx.x; i < M; i += kBlock) {      // thread t reads back only what it wrote: t, t + 256, ...
            const bool in = inlier(P, cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], pix[2 * i], pix[2 * i + 1]);
            mask[i] = in ? 1 : 0;
            mine += in ? 1 : 0;
        }
        atomicAdd(&sh.n_used, mine);
    }
    __syncthreads();
    __shared__ double cand_acc[kNormal];
    __shared__ int bad, iters;
    __shared__ double lambda;
    refine_pass(sh, sh.cur, pts, pix, M, mask, cam, sh.acc, &bad);
    if (threadIdx.x == 0) {
        iters = 0;
        lambda = 1e-4;
        if (sh.n_used < 3 || bad || max_iter <= 0) sh.done = 1;      // nothing to refine on: the pose stays
    }
    for (;;) {
        __syncthreads();
        const int stop = sh.done;      // read between two barriers: thread 0 writes it again below
        __syncthreads();
        if (stop) break;
        if (threadIdx.x == 0) {
            double d[6];
            if (!solve_step(sh.acc, lambda, d)) {
                sh.done = 1;
            } else {
                apply_step(sh.cur, d, sh.cand);
            }
        }
        __syncthreads();
        if (sh.done) break;
        refine_pass(sh, sh.cand, pts, pix, M, mask, cam, cand_acc, &bad);
        if (threadIdx.x == 0) {
            double d[6];
            solve_step(sh.acc, lambda, d);      // the step just tried (cheap to redo; keeps it out of shared memory)
            const double norm = sqrt(((((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]) + d[4] * d[4]) + d[5] * d[5]);
            ++iters;
            // a cost that rises by less than 1e-12 of itself is the rounding of the sum, not ascent
            if (!bad && cand_acc[27] <= sh.acc[27] * (1.0 + 1e-12)) {
                for (int k = 0; k < 12; ++k) sh.cur[k] = sh.cand[k];
                for (int k = 0; k < kNormal; ++k) sh.acc[k] = cand_acc[k];
                lambda = fmax(lambda * 0.1, 1e-12);
            } else {
                lambda *= 10.0;
                if (lambda > 1e12) sh.done = 1;
            }
            if (norm < step_tol || iters >= max_iter) sh.done = 1;
        }
        __syncthreads();
    }
    {
        double P[12];
        for (int k = 0; k < 12; ++k) P[k] = sh.cur[k];
        int mine = 0;
        for (int64_t i = threadIdx.x; i < M; i += kBlock) {
            const bool in = inlier(P, cam, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], pix[2 * i], pix[2 * i + 1]);
            mask[i] = in ? 1 : 0;
            mine += in ? 1 : 0;
        }
        atomicAdd(&sh.count, mine);
    }
    __syncthreads();
    if (threadIdx.x < 12) out_f64[threadIdx.x] = sh.cur[threadIdx.x];
    if (threadIdx.x == 12) out_f64[12] = sh.acc[27];
    if (threadIdx.x == 13) out_i32[0] = iters;
    if (threadIdx.x == 14) out_i32[1] = sh.count;
    if (threadIdx.x == 15) out_i32[2] = sh.n_used;
}

static bool camera_ok(double f, double cx, double cy, double max_error) {
    return f > 0.0 && f < 1e300 && fabs(cx) < 1e300 && fabs(cy) < 1e300 && max_error >= 0.0 && max_error < 1e150;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_pnp_lds_stage(void) { return kStage; }

int avl_loc_lift(const void* d_depth, int depth_is_f64, int H, int W, const double* h_Kinv9, const double* d_kp_ref,
                 const double* d_kp_query, int64_t M, double* d_points, double* d_pixels, int32_t* d_counter2, int64_t* h_count,
                 void* stream) {
    AVL_REQUIRE(h_count && h_Kinv9, "avl_loc_lift: null host argument");
    AVL_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && (depth_is_f64 == 0 || depth_is_f64 == 1), "avl_loc_lift: bad image (%d, %d)", H, W);
    AVL_REQUIRE(M >= 0 && M <= kMaxM, "avl_loc_lift: %lld matches, at most %lld", (long long)M, (long long)kMaxM);
    *h_count = 0;
    if (M == 0) return AVL_OK;
    AVL_REQUIRE(d_depth && d_kp_ref && d_kp_query && d_points && d_pixels && d_counter2, "avl_loc_lift: null device argument");
    hipStream_t st = as_stream(stream);
    Mat3 K;
    for (int k = 0; k < 9; ++k) K.m[k] = h_Kinv9[k];
    AVL_HIP_CHECK(hipMemsetAsync(d_counter2, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(loc_lift_kernel, dim3(1), dim3(kBlock), 0, st, d_depth, depth_is_f64, H, W, K, d_kp_ref, d_kp_query, M, d_points, d_pixels,
                       (int*)d_counter2);
    AVL_HIP_CHECK(hipGetLastError());
    int32_t h[2] = {0, 0};
    AVL_HIP_CHECK(hipMemcpyAsync(h, d_counter2, sizeof(h), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    if (h[1] & kLiftErrPixel) {
        set_error("avl_loc_lift: a key point truncates to a pixel outside the (%d, %d) image (the reference raises IndexError here)", H, W);
        return AVL_ERR_INVALID;
    }
    *h_count = h[0];
    return AVL_OK;
}

int avl_pnp_ransac_work_bytes(int n_hyp, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_pnp_ransac_work_bytes: null output");
    AVL_REQUIRE(n_hyp >= 1 && n_hyp <= (1 << 24), "avl_pnp_ransac_work_bytes: n_hyp %d is not in [1, 2^24]", n_hyp);
    *bytes = (size_t)n_hyp * 12 * sizeof(double);
    return AVL_OK;
}

int avl_pnp_ransac(const double* d_points, const double* d_pixels, int64_t M, double f, double cx, double cy, double max_error,
                   uint32_t seed, int n_hyp, int32_t* d_triples, int32_t* d_hyp_counts, double* d_pose12, int32_t* d_count, void* ws,
                   size_t ws_bytes, void* stream) {
    size_t need = 0;
    int rc = avl_pnp_ransac_work_bytes(n_hyp, &need);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(M >= 3 && M <= kMaxM, "avl_pnp_ransac: %lld correspondences, need 3 .. %lld", (long long)M, (long long)kMaxM);
    AVL_REQUIRE(camera_ok(f, cx, cy, max_error), "avl_pnp_ransac: bad camera or max_error");
    AVL_REQUIRE(d_points && d_pixels && d_hyp_counts && d_pose12 && d_count, "avl_pnp_ransac: null argument");
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_pnp_ransac: workspace of %zu bytes, need %zu", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const Camera cam{f, cx, cy, max_error * max_error};
    const unsigned grid = (unsigned)((n_hyp + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(pnp_ransac_kernel, dim3(grid), dim3(kBlock), 0, st, d_points, d_pixels, M, cam, seed, n_hyp, d_triples, d_hyp_counts,
                       (double*)ws);
    hipLaunchKernelGGL(pnp_select_kernel, dim3(1), dim3(kBlock), 0, st, d_hyp_counts, (const double*)ws, n_hyp, d_pose12, d_count);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_pnp_score(const double* d_points, const double* d_pixels, int64_t M, const double* d_poses, int P, double f, double cx, double cy,
                  double max_error, int32_t* d_counts, uint8_t* d_mask0, void* stream) {
    AVL_REQUIRE(M >= 0 && M <= kMaxM && P >= 1 && P <= (1 << 24), "avl_pnp_score: bad sizes (M %lld, P %d)", (long long)M, P);
    AVL_REQUIRE(camera_ok(f, cx, cy, max_error), "avl_pnp_score: bad camera or max_error");
    AVL_REQUIRE(d_poses && d_counts && (M == 0 || (d_points && d_pixels)), "avl_pnp_score: null argument");
    hipStream_t st = as_stream(stream);
    const Camera cam{f, cx, cy, max_error * max_error};
    const unsigned grid = (unsigned)((P + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(pnp_score_kernel, dim3(grid), dim3(kBlock), 0, st, d_points, d_pixels, M, d_poses, P, cam, d_counts, d_mask0);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_pnp_refine(const double* d_points, const double* d_pixels, int64_t M, const double* d_pose12, double f, double cx, double cy,
                   double max_error, int max_iter, double step_tol, double* d_out13, int32_t* d_out3, uint8_t* d_mask, void* stream) {
    AVL_REQUIRE(M >= 1 && M <= kMaxM, "avl_pnp_refine: %lld correspondences, need 1 .. %lld", (long long)M, (long long)kMaxM);
    AVL_REQUIRE(camera_ok(f, cx, cy, max_error), "avl_pnp_refine: bad camera or max_error");
    AVL_REQUIRE(max_iter >= 0 && max_iter <= 10000 && step_tol >= 0.0, "avl_pnp_refine: bad stopping rule");
    AVL_REQUIRE(d_points && d_pixels && d_pose12 && d_out13 && d_out3 && d_mask, "avl_pnp_refine: null argument");
    hipStream_t st = as_stream(stream);
    const Camera cam{f, cx, cy, max_error * max_error};
    hipLaunchKernelGGL(pnp_refine_kernel, dim3(1), dim3(kBlock), 0, st, d_points, d_pixels, M, d_pose12, cam, max_iter, step_tol, d_out13, d_out3,
                       d_mask);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
