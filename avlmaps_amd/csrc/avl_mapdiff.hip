// Comparing two voxel maps of one place: the join of two voxel lists by cell, the three dot products of every
// joined pair of feature rows, and the status of every voxel.  Upstream has no counterpart: its maps are static.
//
// THE JOIN.  A voxel of map A at cell (row, col, h), moved by the integer shift, looks into map B's cell index (avl_cellindex.h) at
// the cells within Chebyshev radius r <= 2 of it: at most 125 probes.  Of the occupied ones the winner has the smallest pair
// (squared cell distance, linear cell), compared in that order -- integers only, so the answer has one value.  A cell outside the grid
// is empty: the bounds are tested here, ci_linear's -1 never reaches ci_probe.  The centre is probed first: a hit there has d2 = 0,
// which no other cell can have, and ends the search -- in two maps of one place that is nearly every voxel.
//
// THE SUMS.  One wave per pair (i, m = match[i]).  Lane l owns the elements d with (d / 4) % 64 == l and adds their products in
// ascending d into one float64 accumulator per sum (a.b, a.a, b.b); the 64 lane values are combined by avl_wave.h's xor butterfly
// (32, 16, .. 1).  A product of two float32 values is exact in float64, every addition rounds once, and NOTHING IS CONTRACTED INTO AN
// FMA: this file is built with -ffp-contract=off (avlmaps_amd/build.py), and the products and sums below are plain * and +.  The
// order is fixed by d alone, so the bytes are the same on every run, for every D and on either load path: a lane loads its four
// elements of a 256-element chunk as one 16-byte load where D % 4 == 0 and the matrix is 16-byte aligned, and as up to four scalar
// loads otherwise (the choice is made per matrix and is wave-uniform).  An element past D is not added, which equals adding the
// +0.0 product of a zero-padded row: an accumulator that starts at +0.0 is never -0.0.  Rows of A are read once in order; rows of B
// are gathered as whole contiguous rows, several waves per CU keeping a few KB each in flight.
//
// THE STATUS.  Element-wise, in float64 with the grouping written in the kernel; the four counts go wave -> LDS -> one atomic per
// block and non-zero count, as the ground-truth vote pass does.
#include "avl_cellindex.h"
#include "avl_wave.h"

namespace avl {

constexpr int kMdMaxRadius = 2;
constexpr int kMdMaxDim = 8192;
constexpr int kMdChunk = 4 * kWave;             // elements of a row that one wave-wide 16-byte load covers

__global__ __launch_bounds__(256) void md_match_kernel(const int32_t* __restrict__ cells, int64_t n_a, int sr, int sc, int sh, int radius, int gs, int vh,
                                                       const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                                       const int32_t* __restrict__ perm, int32_t* __restrict__ match, int32_t* __restrict__ d2_out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_a; i += (int64_t)gridDim.x * 256) {
        const int64_t r0 = (int64_t)cells[3 * i] + sr, c0 = (int64_t)cells[3 * i + 1] + sc, h0 = (int64_t)cells[3 * i + 2] + sh;
        int best = -1, best_d2 = -1;
        if (r0 >= 0 && r0 < gs && c0 >= 0 && c0 < gs && h0 >= 0 && h0 < vh) {
            const int r = (int)r0, c = (int)c0, h = (int)h0;
            best = ci_probe(bits, prefix, perm, (r * gs + c) * vh + h);         // inside the grid: < 2^31 (checked by the entry point)
            if (best >= 0) {
                best_d2 = 0;
            } else if (radius > 0) {
                int best_lin = 0;
                for (int dr = -radius; dr <= radius; ++dr) {
                    const int rr = r + dr;
                    if (rr < 0 || rr >= gs) continue;
                    for (int dc = -radius; dc <= radius; ++dc) {
                        const int cc = c + dc;
                        if (cc < 0 || cc >= gs) continue;
                        for (int dh = -radius; dh <= radius; ++dh) {
                            const int hh = h + dh;
                            if (hh < 0 || hh >= vh) continue;
                            const int d2 = dr * dr + dc * dc + dh * dh, lin = (rr * gs + cc) * vh + hh;
                            if (best >= 0 && (d2 > best_d2 || (d2 == best_d2 && lin > best_lin))) continue;     // cannot win: no probe
                            const int row = ci_probe(bits, prefix, perm, lin);
                            if (row >= 0) best = row, best_d2 = d2, best_lin = lin;
                        }
                    }
                }
            }
        }
        match[i] = best;
        d2_out[i] = best_d2;
    }
}

// the four elements d .. d + 3 of a row (d < D), zeros past D; `vec`: D % 4 == 0 and the row is 16-byte aligned
__device__ __forceinline__ float4 md_load4(const float* __restrict__ row, int d, int D, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(row + d);
    float4 v;
    v.x = row[d];
    v.y = d + 1 < D ? row[d + 1] : 0.0f;
    v.z = d + 2 < D ? row[d + 2] : 0.0f;
    v.w = d + 3 < D ? row[d + 3] : 0.0f;
    return v;
}

__global__ __launch_bounds__(256) void md_row_dots_kernel(const float* __restrict__ feat_a, int64_t n_a, const float* __restrict__ feat_b, int64_t n_b,
                                                          int D, bool vec_a, bool vec_b, const int32_t* __restrict__ match,
                                                          double* __restrict__ sums) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * (256 / kWave);
    for (int64_t i = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave; i < n_a; i += waves) {
        const int m = match[i];                                                 // wave-uniform
        double ab = 0.0, aa = 0.0, bb = 0.0;
        if (m >= 0 && m < n_b) {
            const float* __restrict__ ra = feat_a + (size_t)i * D;
            const float* __restrict__ rb = feat_b + (size_t)m * D;
#pragma unroll 4
            for (int d = 4 * lane; d < D; d += kMdChunk) {
                const float4 a = md_load4(ra, d, D, vec_a), b = md_load4(rb, d, D, vec_b);
                const int left = D - d;                                         // >= 1; the elements of this lane's four that exist
                const double ax = a.x, bx = b.x;
                ab = ab + ax * bx, aa = aa + ax * ax, bb = bb + bx * bx;
                if (left > 1) {
                    const double ay = a.y, by = b.y;
                    ab = ab + ay * by, aa = aa + ay * ay, bb = bb + by * by;
                }
                if (left > 2) {
                    const double az = a.z, bz = b.z;
                    ab = ab + az * bz, aa = aa + az * az, bb = bb + bz * bz;
                }
                if (left > 3) {
                    const double aw = a.w, bw = b.w;
                    ab = ab + aw * bw, aa = aa + aw * aw, bb = bb + bw * bw;
                }
            }
            ab = wave_sum(ab);
            aa = wave_sum(aa);
            bb = wave_sum(bb);
        }
        if (lane < 3) sums[3 * i + lane] = lane == 0 ? ab : lane == 1 ? aa : bb;
    }
}

__global__ __launch_bounds__(256) void md_status_kernel(const int32_t* __restrict__ match, const double* __restrict__ sums, int64_t n, double t2,
                                                        const int32_t* __restrict__ through, int min_rays, uint8_t* __restrict__ status,
                                                        int32_t* __restrict__ counts) {
    __shared__ int block_counts[4];
    if (threadIdx.x < 4) block_counts[threadIdx.x] = 0;
    __syncthreads();
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    const int64_t rounds = (n + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);     // every lane takes part in every ballot
    for (int64_t k = 0; k < rounds; ++k) {
        const int64_t i = (k * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        int s = -1;
        if (i < n) {
            if (match[i] < 0) {
                s = through && through[i] < min_rays ? 3 : 2;
            } else {
                const double ab = sums[3 * i], aa = sums[3 * i + 1], bb = sums[3 * i + 2];
                s = aa > 0.0 && bb > 0.0 && ab > 0.0 && ab * ab >= t2 * (aa * bb) ? 0 : 1;
            }
            status[i] = (uint8_t)s;
        }
        n0 += __popcll(__ballot(s == 0));
        n1 += __popcll(__ballot(s == 1));
        n2 += __popcll(__ballot(s == 2));
        n3 += __popcll(__ballot(s == 3));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (n0) atomicAdd(block_counts + 0, n0);
        if (n1) atomicAdd(block_counts + 1, n1);
        if (n2) atomicAdd(block_counts + 2, n2);
        if (n3) atomicAdd(block_counts + 3, n3);
    }
    __syncthreads();
    if (threadIdx.x < 4 && block_counts[threadIdx.x]) atomicAdd(counts + threadIdx.x, block_counts[threadIdx.x]);
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_map_match_cells(const void* d_index, size_t index_bytes, int64_t N_b, int gs, int vh, const int32_t* d_cells, int64_t n_a,
                        const int32_t* h_shift, int radius, int32_t* d_match, int32_t* d_d2, void* stream) {
    const int rc = ci_check_grid("avl_map_match_cells", N_b, gs, vh);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n_a >= 0 && n_a < INT_MAX, "avl_map_match_cells: %lld cells (0 .. 2^31 - 2)", (long long)n_a);
    AVL_REQUIRE(radius >= 0 && radius <= kMdMaxRadius, "avl_map_match_cells: radius %d (0 .. %d)", radius, kMdMaxRadius);
    AVL_REQUIRE(d_index, "avl_map_match_cells: null index");
    const CellIndexView v = ci_layout(const_cast<void*>(d_index), N_b, gs, vh);
    AVL_REQUIRE(index_bytes >= v.total, "avl_map_match_cells: the index buffer has %zu bytes, needs %zu", index_bytes, v.total);
    if (n_a == 0) return AVL_OK;
    AVL_REQUIRE(d_cells && d_match && d_d2, "avl_map_match_cells: null pointer");
    const int sr = h_shift ? h_shift[0] : 0, sc = h_shift ? h_shift[1] : 0, sh = h_shift ? h_shift[2] : 0;
    hipLaunchKernelGGL(md_match_kernel, dim3(stride_blocks(n_a)), dim3(256), 0, as_stream(stream), d_cells, n_a, sr, sc, sh, radius, gs, vh,
                       (const uint32_t*)v.bits, (const int32_t*)v.prefix, (const int32_t*)v.perm, d_match, d_d2);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_row_dots_f32(const float* d_feat_a, int64_t n_a, const float* d_feat_b, int64_t N_b, int D, const int32_t* d_match, double* d_sums,
                     void* stream) {
    AVL_REQUIRE(n_a >= 0 && n_a < INT_MAX && N_b >= 0 && N_b < INT_MAX, "avl_row_dots_f32: %lld and %lld rows (0 .. 2^31 - 2)", (long long)n_a,
                (long long)N_b);
    AVL_REQUIRE(D >= 1 && D <= kMdMaxDim, "avl_row_dots_f32: D = %d (1 .. %d)", D, kMdMaxDim);
    if (n_a == 0) return AVL_OK;
    AVL_REQUIRE(d_feat_a && d_match && d_sums && (d_feat_b || N_b == 0), "avl_row_dots_f32: null pointer");
    const bool vec_a = D % 4 == 0 && reinterpret_cast<uintptr_t>(d_feat_a) % 16 == 0;
    const bool vec_b = D % 4 == 0 && reinterpret_cast<uintptr_t>(d_feat_b) % 16 == 0;
    hipLaunchKernelGGL(md_row_dots_kernel, dim3(stride_blocks(n_a * kWave)), dim3(256), 0, as_stream(stream), d_feat_a, n_a, d_feat_b, N_b, D, vec_a,
                       vec_b, d_match, d_sums);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_map_diff_status(const int32_t* d_match, const double* d_sums, int64_t n, double t2, const int32_t* d_through, int min_rays,
                        uint8_t* d_status, int32_t* d_counts, void* stream) {
    AVL_REQUIRE(n >= 0 && n < INT_MAX, "avl_map_diff_status: %lld voxels (0 .. 2^31 - 2)", (long long)n);
    AVL_REQUIRE(t2 > 0.0 && t2 <= 1.0, "avl_map_diff_status: t2 = %g (the square of a threshold in (0, 1])", t2);
    AVL_REQUIRE(d_counts, "avl_map_diff_status: null counts");
    AVL_HIP_CHECK(hipMemsetAsync(d_counts, 0, 4 * sizeof(int32_t), as_stream(stream)));
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_match && d_sums && d_status, "avl_map_diff_status: null pointer");
    hipLaunchKernelGGL(md_status_kernel, dim3(stride_blocks(n)), dim3(256), 0, as_stream(stream), d_match, d_sums, n, t2, d_through, min_rays,
                       d_status, d_counts);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
