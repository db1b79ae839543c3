// Finalisation and map I/O of the voxel map builder (avl_builder.hip holds the frame path, avl_builder_state.h the state): the
// accumulators become the reference's arrays (grid_feat, grid_pos, weight, grid_rgb, occupied_ids), leave as rows or partial sums for
// the multi-GPU merges (avlmaps_amd/parallel.py, merge2.py), or are rebuilt from a finalised map (resume); and pass 1 of the global
// (multi-floor) builder, the bounding box of a frame's points.
// Slots are handed out in arrival order, so finalisation sorts the first-touch keys (rocPRIM radix sort) to emit
// rows in the reference's voxel-id order; the sort is a once-per-save cost.
// Compiled with -ffp-contract=off like the frame path: the rows are the reference's float64 expressions, operation for operation.
#include <algorithm>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "avl_builder_state.h"
#include "avl_pinhole.h"

namespace avl {

// wave per output row r; the accumulators of row r live in slot perm[r] (perm == nullptr: identity).  sum_feat rows have
// stride ld_sf, the [sum alpha, sum alpha*rgb] quadruple of a row sits at sum_w4 + row * ld_w4.  first_feat == nullptr: the
// first-touch correction has already been folded into sum_feat (merged accumulators, scatter_merge_kernel).  Output row r
// is voxel id row0 + r (row0 != 0: one rank finalises one block of a reduce-scattered map).
__global__ __launch_bounds__(256) void finalize_kernel(int64_t n, int D, int gs, int vh, int64_t row0, const int32_t* __restrict__ perm,
                                                       const int32_t* __restrict__ cell, const double* __restrict__ sum_feat,
                                                       int64_t ld_sf, const double* __restrict__ sum_w4, int64_t ld_w4,
                                                       const float* __restrict__ first_feat, const double* __restrict__ first_alpha,
                                                       float* __restrict__ grid_feat, int32_t* __restrict__ grid_pos,
                                                       float* __restrict__ weight, uint8_t* __restrict__ grid_rgb,
                                                       int32_t* __restrict__ occupied) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave0; r < n; r += nwaves) {
        const int64_t sl = perm ? perm[r] : r;
        const double w = sum_w4[sl * ld_w4];
        if (grid_feat) {
            const double* s = sum_feat + sl * ld_sf;
            float* o = grid_feat + r * D;
            if (first_feat) {
                // reference closed form (a1^2 f1 + sum_{i >= 2} alpha_i f_i) / sum alpha; sum_feat excludes the first touch
                const double a1 = first_alpha[sl];
                const double a1sq = a1 * a1;
                const float* f1 = first_feat + sl * D;
                for (int c = lane; c < D; c += 64) o[c] = (float)((a1sq * (double)f1[c] + s[c]) / w);
            } else {
                for (int c = lane; c < D; c += 64) o[c] = (float)(s[c] / w);
            }
        }
        if (lane == 0) {
            const int32_t cl = cell[sl];
            if (grid_pos) {
                grid_pos[r * 3 + 0] = cl / (gs * vh);
                grid_pos[r * 3 + 1] = (cl / vh) % gs;
                grid_pos[r * 3 + 2] = cl % vh;
            }
            if (weight) weight[r] = (float)w;
            if (occupied) occupied[cl] = (int32_t)(row0 + r);
        }
        if (grid_rgb && lane < 3) {
            // running mean stored into a uint8 array (truncating cast); we truncate the exact weighted mean.  (sum alpha c) / (sum
            // alpha) of samples that all have the colour c is c or c - 1 ulp: the 1e-9 keeps that from truncating to c - 1 (a voxel
            // touched once stores its pixel's colour exactly, vlmap_builder.py:167)
            double m = sum_w4[sl * ld_w4 + 1 + lane] / w + 1e-9;
            m = fmin(fmax(m, 0.0), 255.0);
            grid_rgb[r * 3 + lane] = (uint8_t)m;
        }
    }
}

// Multi-GPU merge, step "scatter" (avlmaps_amd/parallel.py): wave per local slot s.  The slot's accumulators go to row
// row_of_slot[s] of the dense (M, D + 4) float64 buffer every rank reduces -- straight from the builder's own arrays, no
// export copy.  The rank that OWNS the voxel's global first touch (its slot_key equals the all-reduced MIN key) subtracts the
// first touch with the reference's weight a1^2 (every other rank: a1; vlmap_builder.py:166-174 closed form), so that the
// reduced rows only need dividing by sum alpha: ONE sum-reduce carries the whole merge.
__global__ __launch_bounds__(256) void scatter_merge_kernel(int64_t n, int D, const int64_t* __restrict__ row_of_slot,
                                                            const unsigned long long* __restrict__ global_key,
                                                            const unsigned long long* __restrict__ slot_key,
                                                            const double* __restrict__ sum_feat, const double* __restrict__ sum_w4,
                                                            const float* __restrict__ first_feat, const double* __restrict__ first_alpha,
                                                            double* __restrict__ acc, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t s = wave0; s < n; s += nwaves) {
        const int64_t row = row_of_slot[s];
        const bool owner = slot_key[s] == global_key[row];
        // sum_feat leaves the slot's LOCAL first touch out (fuse_body): the rank that holds the GLOBAL first touch contributes it
        // with the reference's a1^2, every other rank with its plain weight a1
        const double a1 = first_alpha[s];
        const double wf = owner ? a1 * a1 : a1;
        const double* sf = sum_feat + s * D;
        const float* f1 = first_feat + s * D;
        double* o = acc + row * ld;
        for (int c = lane; c < D; c += 64) o[c] = wf * (double)f1[c] + sf[c];
        if (lane < 4) o[D + lane] = sum_w4[s * 4 + lane];
    }
}

// Row-sharded merge with the mixed payload (avlmaps_amd/parallel.py, round 4).  A voxel that only ONE rank ever touched needs no
// float64 exchange: its finished float32 feature row (a1^2 f1 + sum) / sum alpha is computed where the accumulators live --
// the same float64 expression finalize_kernel evaluates, so the row is bit-identical to the single-process map -- and travels as
// 4 B per element.  Only voxels that several ranks touched ship float64 partial sums (own != 0: this rank holds the global first
// touch and folds the reference's first-touch term in).  Wave per listed slot; output row i belongs to slot slots[i].
__global__ __launch_bounds__(256) void export_rows_f32_kernel(int64_t k, int D, const int32_t* __restrict__ slots,
                                                              const double* __restrict__ sum_feat, const double* __restrict__ sum_w4,
                                                              const float* __restrict__ first_feat, const double* __restrict__ first_alpha,
                                                              float* __restrict__ out, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave0; i < k; i += nwaves) {
        const int64_t sl = slots[i];
        const double w = sum_w4[sl * 4];
        const double a1 = first_alpha[sl];
        const double a1sq = a1 * a1;
        const double* s = sum_feat + sl * D;
        const float* f1 = first_feat + sl * D;
        float* o = out + i * ld;
        for (int c = lane; c < D; c += 64) o[c] = (float)((a1sq * (double)f1[c] + s[c]) / w);   // finalize_kernel's expression
    }
}

__global__ __launch_bounds__(256) void export_rows_f64_kernel(int64_t k, int D, const int32_t* __restrict__ slots,
                                                              const uint8_t* __restrict__ own, const double* __restrict__ sum_feat,
                                                              const float* __restrict__ first_feat, const double* __restrict__ first_alpha,
                                                              double* __restrict__ out, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave0; i < k; i += nwaves) {
        const int64_t sl = slots[i];
        const double a1 = first_alpha[sl];
        const double wf = own[i] ? a1 * a1 : a1;   // global first touch: a1^2 f1 (reference closed form); else the sample's plain weight
        const double* s = sum_feat + sl * D;
        const float* f1 = first_feat + sl * D;
        double* o = out + i * ld;
        for (int c = lane; c < D; c += 64) o[c] = wf * (double)f1[c] + s[c];
    }
}

// Sender side of the gather-plan merge (avl_merge2.hip, avlmaps_amd/merge2.py): the rank's voxels in final-row order, straight from
// the accumulators into the send buffer of the ONE payload all_to_all.  Destination q's segment = [side records | finished float32
// rows | float64 partial rows].  Wave per voxel i: its 64-byte side record [row - first row of q's block | index in q's done / part
// list << 32 | flags, sum_w4 (4 x f64), 3 words of replay state (avl_merge2_side_state fills them after the replay)], and its
// feature row: export_rows_f32_kernel's expression for a voxel of this rank alone (straight into this rank's own block when it owns
// the row), export_rows_f64_kernel's for a voxel several ranks touched.
struct M2PackSeg {
    long long cum[65];        // cum[q] = voxels of this call for ranks < q (cum[ws] = all of them): wave w serves rank q with cum[q] <= w < cum[q + 1]
    long long lo[64];         // ... and is voxel lo[q] + (w - cum[q]) of the rank's final-row order
    long long dlo[64];        // single-rank voxels of that order before lo[q]
    long long row0[64];       // first final row this call covers at rank q (a chunk of q's block): side records carry row - row0[q]
    long long side_off[64], done_off[64], part_off[64];   // word (8 B) offsets of q's three lists in the send buffer
};

__global__ __launch_bounds__(256) void m2_pack_kernel(long long n, int ws, int rank, int D, long long own_r0, M2PackSeg sg,
                                                      const int32_t* __restrict__ order, const int32_t* __restrict__ row_s,
                                                      const int32_t* __restrict__ prev_s, const int32_t* __restrict__ next_s,
                                                      const int32_t* __restrict__ sidx, const double* __restrict__ sum_feat,
                                                      const double* __restrict__ sum_w4, const float* __restrict__ first_feat,
                                                      const double* __restrict__ first_alpha, long long* __restrict__ send,
                                                      float* __restrict__ own_feat) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long ldf = (D + 1) / 2 * 2;
    for (long long w = wave0; w < n; w += nwaves) {
        int q = 0;
        while (q + 1 < ws && w >= sg.cum[q + 1]) ++q;
        const long long j = w - sg.cum[q];
        const long long i = sg.lo[q] + j;
        const long long sl = order[i];
        const bool is_new = prev_s[sl] < 0, single = is_new && next_s[sl] < 0;
        const long long didx = (long long)sidx[i] - sg.dlo[q], pidx = j - didx;
        const bool direct = single && q == rank && own_feat != nullptr;
        const long long row = row_s[sl];
        const long long row_rel = row - sg.row0[q];
        const double a1 = first_alpha[sl];
        const double* s = sum_feat + sl * D;
        const float* f1 = first_feat + sl * D;
        if (single) {
            const double wsum = sum_w4[sl * 4];
            const double a1sq = a1 * a1;
            float* o = direct ? own_feat + (row - own_r0) * D : reinterpret_cast<float*>(send + sg.done_off[q]) + didx * ldf;
            for (int c = lane; c < D; c += 64) o[c] = (float)((a1sq * (double)f1[c] + s[c]) / wsum);     // finalize_kernel's expression
        } else {
            const double wf = is_new ? a1 * a1 : a1;   // global first touch: a1^2 f1 (reference closed form); else the sample's plain weight
            double* o = reinterpret_cast<double*>(send + sg.part_off[q]) + pidx * D;
            for (int c = lane; c < D; c += 64) o[c] = wf * (double)f1[c] + s[c];
        }
        long long* rec = send + sg.side_off[q] + 8 * j;
        if (lane == 0)
            rec[0] = (long long)((unsigned long long)row_rel | ((unsigned long long)(single ? didx : pidx) << 32) |
                                 (single ? (1ull << 63) : 0ull) | (direct ? (1ull << 62) : 0ull));
        else if (lane < 5)
            rec[lane] = __double_as_longlong(sum_w4[sl * 4 + lane - 1]);
        else if (lane < 8)
            rec[lane] = 0;
    }
}

// grid_pos / weight / grid_rgb / occupied_ids of n merged rows from their cells and [sum alpha, sum alpha rgb] quadruples alone
// (the feature rows of the mixed payload are finished elsewhere); same arithmetic as finalize_kernel's lane-0 part
__global__ __launch_bounds__(256) void finalize_side_kernel(int64_t n, int gs, int vh, int64_t row0, const int32_t* __restrict__ cell,
                                                            const double* __restrict__ w4, int32_t* __restrict__ grid_pos,
                                                            float* __restrict__ weight, uint8_t* __restrict__ grid_rgb,
                                                            int32_t* __restrict__ occupied) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t cl = cell[r];
        const double w = w4[r * 4];
        if (grid_pos) {
            grid_pos[r * 3 + 0] = cl / (gs * vh);
            grid_pos[r * 3 + 1] = (cl / vh) % gs;
            grid_pos[r * 3 + 2] = cl % vh;
        }
        if (weight) weight[r] = (float)w;
        if (occupied) occupied[cl] = (int32_t)(row0 + r);
        if (grid_rgb)
            for (int k = 0; k < 3; ++k) {
                double m = w4[r * 4 + 1 + k] / w + 1e-9;   // as finalize_kernel
                m = fmin(fmax(m, 0.0), 255.0);
                grid_rgb[r * 3 + k] = (uint8_t)m;
            }
    }
}

// row_dirty[r] = the voxel in output row r was fused since the flags were last cleared
__global__ void row_dirty_kernel(int64_t n, const int32_t* __restrict__ perm, uint8_t* __restrict__ dirty, uint8_t* __restrict__ row_dirty,
                                 int clear) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t sl = perm[r];
        row_dirty[r] = dirty[sl];
        if (clear) dirty[sl] = 0;
    }
}

__global__ void iota_kernel(int32_t* __restrict__ v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = (int32_t)i;
}

// wave per imported voxel row: rebuild accumulators from a finalised map (resume, vlmap_builder.py:212-222)
__global__ __launch_bounds__(256) void import_map_kernel(int64_t n, int D, int n0, int gs, int vh, const float* __restrict__ grid_feat,
                                                         const int32_t* __restrict__ grid_pos, const float* __restrict__ weight,
                                                         const uint8_t* __restrict__ grid_rgb, int32_t* __restrict__ cell_slot,
                                                         int32_t* __restrict__ slot_cell, unsigned long long* __restrict__ slot_key,
                                                         double* __restrict__ sum_feat, double* __restrict__ sum_w4,
                                                         float* __restrict__ first_feat, double* __restrict__ first_alpha,
                                                         int* __restrict__ err_flags) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave0; r < n; r += nwaves) {
        const double w = (double)weight[r];
        for (int c = lane; c < D; c += 64) {
            sum_feat[r * D + c] = (double)grid_feat[r * D + c] * w;   // first-touch weighting is already baked in
            first_feat[r * D + c] = 0.f;
        }
        if (lane == 0) {
            const int row = grid_pos[r * 3], col = grid_pos[r * 3 + 1], h = grid_pos[r * 3 + 2];
            if (row < 0 || row >= n0 || col < 0 || col >= gs || h < 0 || h >= vh) {
                atomicOr(err_flags, 4);
            } else {
                const int32_t cell = (row * gs + col) * vh + h;
                cell_slot[cell] = (int32_t)r;
                slot_cell[r] = cell;
            }
            slot_key[r] = (unsigned long long)r;                        // imported voxels order before any new one
            first_alpha[r] = 0.0;                                       // no first-touch term: it is baked into the imported row
            sum_w4[r * 4] = w;
            for (int c = 0; c < 3; ++c) sum_w4[r * 4 + 1 + c] = (grid_rgb ? (double)grid_rgb[r * 3 + c] : 0.0) * w;
        }
    }
}

// pass 1 of the global (multi-floor) builder: bounding box of the transformed sampled points
// (vlmap_builder_multi_floor.py:97-118).  minmax = [min xyz, max xyz] as order-preserving uint64 keys of the doubles.
__device__ __forceinline__ unsigned long long f64_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void bbox_kernel(FrameParams fp, const float* __restrict__ depth,
                                                   const int32_t* __restrict__ sample_idx, unsigned long long* __restrict__ minmax) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= fp.P) return;
    const int pix = sample_idx[s];
    if (pix < 0 || pix >= fp.H * fp.W) return;
    const double x = (double)(pix % fp.W) + 0.5, y = (double)(pix / fp.W) + 0.5;
    const double z = fp.depth_u16 ? (double)reinterpret_cast<const uint16_t*>(depth)[pix] / fp.depth_div : (double)depth[pix];
    double pl0, pl1, pl2;
    bp_backproject(fp.kinv, x, y, z, pl0, pl1, pl2);
    if (!((pl2 > fp.min_depth) && (pl2 < fp.max_depth))) return;
    double g[3];
    bp_transform(fp.t, pl0, pl1, pl2, g[0], g[1], g[2]);
    for (int c = 0; c < 3; ++c) {
        const unsigned long long k = f64_key(g[c]);
        atomicMin(&minmax[c], k);
        atomicMax(&minmax[3 + c], k);
    }
}

}  // namespace avl

using namespace avl;

extern "C" {

static int launch_finalize(int64_t n, int D, int gs, int vh, int64_t row0, const int32_t* perm, const int32_t* d_cell,
                           const double* d_sum_feat, int64_t ld_sf, const double* d_sum_w4, int64_t ld_w4, const float* d_first_feat,
                           const double* d_first_alpha, float* d_grid_feat, int32_t* d_grid_pos, float* d_weight,
                           uint8_t* d_grid_rgb, int32_t* d_occupied_ids, hipStream_t st) {
    int64_t blocks = (n + 3) / 4;
    const int64_t maxb = (int64_t)num_cus() * 16;
    if (blocks > maxb) blocks = maxb;
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, D, gs, vh, row0, perm, d_cell, d_sum_feat, ld_sf,
                       d_sum_w4, ld_w4, d_first_feat, d_first_alpha, d_grid_feat, d_grid_pos, d_weight, d_grid_rgb, d_occupied_ids);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_finalize_raw(int64_t n, int D, int gs, int vh, const int32_t* d_cell, const double* d_sum_feat,
                     const double* d_sum_w4, const float* d_first_feat, const double* d_first_alpha, float* d_grid_feat,
                     int32_t* d_grid_pos, float* d_weight, uint8_t* d_grid_rgb, int32_t* d_occupied_ids, void* stream) {
    AVL_REQUIRE(n >= 0 && D > 0 && gs > 0 && vh > 0, "avl_finalize_raw: bad shape");
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_cell && d_sum_w4 && d_first_alpha, "avl_finalize_raw: null input");
    AVL_REQUIRE(!d_grid_feat || (d_sum_feat && d_first_feat), "avl_finalize_raw: grid_feat needs sum_feat and first_feat");
    return launch_finalize(n, D, gs, vh, 0, nullptr, d_cell, d_sum_feat, D, d_sum_w4, 4, d_first_feat, d_first_alpha, d_grid_feat,
                           d_grid_pos, d_weight, d_grid_rgb, d_occupied_ids, as_stream(stream));
}

int avl_finalize_merged(int64_t n, int64_t row0, int D, int gs, int vh, const int32_t* d_cell, const double* d_acc,
                        int64_t ld_acc, float* d_grid_feat, int32_t* d_grid_pos, float* d_weight, uint8_t* d_grid_rgb,
                        int32_t* d_occupied_ids, void* stream) {
    AVL_REQUIRE(n >= 0 && row0 >= 0 && D > 0 && gs > 0 && vh > 0 && ld_acc >= D + 4, "avl_finalize_merged: bad shape");
    AVL_REQUIRE(row0 + n < (1ll << 31), "avl_finalize_merged: voxel ids must fit int32");
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_cell && d_acc, "avl_finalize_merged: null input");
    return launch_finalize(n, D, gs, vh, row0, nullptr, d_cell, d_acc, ld_acc, d_acc + D, ld_acc, nullptr, nullptr, d_grid_feat,
                           d_grid_pos, d_weight, d_grid_rgb, d_occupied_ids, as_stream(stream));
}

int avl_builder_scatter_merge(avl_builder* b, int64_t n, const int64_t* d_row_of_slot, const uint64_t* d_global_key,
                              double* d_acc, int64_t ld_acc, void* stream) {
    AVL_REQUIRE(b, "avl_builder_scatter_merge: null handle");
    hipStream_t st = as_stream(stream);
    int64_t have = 0;
    int rc = avl_builder_num_voxels(b, &have, stream);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n == have, "avl_builder_scatter_merge: n=%lld but the map holds %lld voxels", (long long)n, (long long)have);
    AVL_REQUIRE(ld_acc >= b->D + 4, "avl_builder_scatter_merge: ld_acc must be >= D + 4");
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_row_of_slot && d_global_key && d_acc, "avl_builder_scatter_merge: null pointer");
    int64_t blocks = (n + 3) / 4;
    const int64_t maxb = (int64_t)num_cus() * 16;
    if (blocks > maxb) blocks = maxb;
    hipLaunchKernelGGL(scatter_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, b->D, d_row_of_slot,
                       reinterpret_cast<const unsigned long long*>(d_global_key), b->slot_key, b->sum_feat, b->sum_w4, b->first_feat,
                       b->first_alpha, d_acc, ld_acc);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

static int check_slot_list(avl_builder* b, int64_t k, const void* slots, const void* out, int64_t ld, const char* who, void* stream) {
    AVL_REQUIRE(b, "%s: null handle", who);
    AVL_REQUIRE(k >= 0 && ld >= b->D, "%s: bad shape", who);
    int64_t have = 0;
    int rc = avl_builder_num_voxels(b, &have, stream);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(k <= have, "%s: %lld slots listed but the map holds %lld voxels", who, (long long)k, (long long)have);
    AVL_REQUIRE(k == 0 || (slots && out), "%s: null pointer", who);
    return AVL_OK;
}

int avl_builder_export_rows_f32(avl_builder* b, int64_t k, const int32_t* d_slots, float* d_out, int64_t ld, void* stream) {
    int rc = check_slot_list(b, k, d_slots, d_out, ld, "avl_builder_export_rows_f32", stream);
    if (rc != AVL_OK || k == 0) return rc;
    const int64_t blocks = std::min<int64_t>((k + 3) / 4, (int64_t)num_cus() * 16);
    hipLaunchKernelGGL(export_rows_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), k, b->D, d_slots, b->sum_feat,
                       b->sum_w4, b->first_feat, b->first_alpha, d_out, ld);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_builder_export_rows_f64(avl_builder* b, int64_t k, const int32_t* d_slots, const uint8_t* d_own, double* d_out, int64_t ld,
                                void* stream) {
    int rc = check_slot_list(b, k, d_slots, d_out, ld, "avl_builder_export_rows_f64", stream);
    if (rc != AVL_OK || k == 0) return rc;
    AVL_REQUIRE(d_own, "avl_builder_export_rows_f64: null ownership flags");
    const int64_t blocks = std::min<int64_t>((k + 3) / 4, (int64_t)num_cus() * 16);
    hipLaunchKernelGGL(export_rows_f64_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), k, b->D, d_slots, d_own, b->sum_feat,
                       b->first_feat, b->first_alpha, d_out, ld);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_builder_m2_pack(avl_builder* b, int64_t n, int ws, int rank, int64_t own_r0, const int64_t* h_cum, const int64_t* h_lo,
                        const int64_t* h_dlo, const int64_t* h_row0, const int64_t* h_side_off, const int64_t* h_done_off,
                        const int64_t* h_part_off, const int32_t* d_order, const int32_t* d_row, const int32_t* d_prev, const int32_t* d_next,
                        const int32_t* d_sidx, int64_t* d_send, float* d_own_feat, void* stream) {
    AVL_REQUIRE(b, "avl_builder_m2_pack: null handle");
    AVL_REQUIRE(n >= 0 && ws >= 1 && ws <= 64 && rank >= 0 && rank < ws && own_r0 >= 0, "avl_builder_m2_pack: bad arguments");
    hipStream_t st = as_stream(stream);
    int rc = flush_pending(b, st);
    if (rc != AVL_OK) return rc;
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(n <= b->capacity, "avl_builder_m2_pack: n=%lld exceeds the capacity %lld", (long long)n, (long long)b->capacity);
    AVL_REQUIRE(h_cum && h_lo && h_dlo && h_row0 && h_side_off && h_done_off && h_part_off && d_order && d_row && d_prev && d_next && d_sidx && d_send,
                "avl_builder_m2_pack: null pointer");
    M2PackSeg sg{};
    for (int q = 0; q <= 64; ++q) sg.cum[q] = h_cum[q < ws ? q : ws];
    for (int q = 0; q < ws; ++q) {
        sg.lo[q] = h_lo[q];
        sg.dlo[q] = h_dlo[q];
        sg.row0[q] = h_row0[q];
        sg.side_off[q] = h_side_off[q];
        sg.done_off[q] = h_done_off[q];
        sg.part_off[q] = h_part_off[q];
    }
    AVL_REQUIRE(sg.cum[0] == 0 && sg.cum[ws] == n, "avl_builder_m2_pack: the destination ranges cover %lld voxels, n = %lld", sg.cum[ws], (long long)n);
    int64_t blocks = (n + 3) / 4;
    const int64_t maxb = (int64_t)num_cus() * 16;
    if (blocks > maxb) blocks = maxb;
    hipLaunchKernelGGL(m2_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (long long)n, ws, rank, b->D, (long long)own_r0, sg, d_order, d_row,
                       d_prev, d_next, d_sidx, b->sum_feat, b->sum_w4, b->first_feat, b->first_alpha, reinterpret_cast<long long*>(d_send),
                       d_own_feat);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_finalize_side(int64_t n, int64_t row0, int gs, int vh, const int32_t* d_cell, const double* d_w4, int32_t* d_grid_pos,
                      float* d_weight, uint8_t* d_grid_rgb, int32_t* d_occupied_ids, void* stream) {
    AVL_REQUIRE(n >= 0 && row0 >= 0 && gs > 0 && vh > 0, "avl_finalize_side: bad shape");
    AVL_REQUIRE(row0 + n < (1ll << 31), "avl_finalize_side: voxel ids must fit int32");
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_cell && d_w4, "avl_finalize_side: null input");
    hipLaunchKernelGGL(finalize_side_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, as_stream(stream), n, gs,
                       vh, row0, d_cell, d_w4, d_grid_pos, d_weight, d_grid_rgb, d_occupied_ids);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_builder_finalize(avl_builder* b, int64_t n, float* d_grid_feat, int32_t* d_grid_pos, float* d_weight,
                         uint8_t* d_grid_rgb, int32_t* d_occupied_ids, void* stream) {
    return avl_builder_finalize_ex(b, n, d_grid_feat, d_grid_pos, d_weight, d_grid_rgb, d_occupied_ids, nullptr, 0, stream);
}

int avl_builder_finalize_ex(avl_builder* b, int64_t n, float* d_grid_feat, int32_t* d_grid_pos, float* d_weight,
                            uint8_t* d_grid_rgb, int32_t* d_occupied_ids, uint8_t* d_row_dirty, int clear_dirty, void* stream) {
    AVL_REQUIRE(b, "avl_builder_finalize: null handle");
    hipStream_t st = as_stream(stream);
    int64_t have = 0;
    int rc = avl_builder_num_voxels(b, &have, stream);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n == have, "avl_builder_finalize: n=%lld but the map holds %lld voxels", (long long)n, (long long)have);
    if (d_occupied_ids) AVL_HIP_CHECK(hipMemsetAsync(d_occupied_ids, 0xFF, b->ncell * sizeof(int32_t), st));
    if (n == 0) {
        AVL_HIP_CHECK(hipStreamSynchronize(st));
        return AVL_OK;
    }
    // rows in the reference's voxel-id order = slots sorted by first-touch key
    unsigned long long* keys_out = nullptr;
    int32_t *iota = nullptr, *perm = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    // one pool allocation for the four temporaries (each hipMallocAsync / hipFreeAsync pair is ~90 us of host time)
    AVL_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, b->slot_key, keys_out, iota, perm, (size_t)n, 0, 64, st));
    const size_t b_keys = ((size_t)n * sizeof(unsigned long long) + 255) / 256 * 256, b_idx = ((size_t)n * sizeof(int32_t) + 255) / 256 * 256;
    char* block = nullptr;
    AVL_HIP_CHECK(hipMallocAsync((void**)&block, b_keys + 2 * b_idx + (tmp_bytes ? tmp_bytes : 16), st));
    keys_out = reinterpret_cast<unsigned long long*>(block);
    iota = reinterpret_cast<int32_t*>(block + b_keys);
    perm = reinterpret_cast<int32_t*>(block + b_keys + b_idx);
    tmp = block + b_keys + 2 * b_idx;
    hipLaunchKernelGGL(iota_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, iota, n);
    AVL_HIP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, b->slot_key, keys_out, iota, perm, (size_t)n, 0, 64, st));
    rc = launch_finalize(n, b->D, b->gs, b->vh, 0, perm, b->slot_cell, b->sum_feat, b->D, b->sum_w4, 4, b->first_feat, b->first_alpha,
                         d_grid_feat, d_grid_pos, d_weight, d_grid_rgb, d_occupied_ids, st);
    // exact sequential weight / grid_rgb from the replay log (avl_replay.hip)
    if (rc == AVL_OK && b->log.slot && b->key_bias == 0 && b->log_used > 0 && (d_weight || d_grid_rgb))
        rc = replay_rgb(b, n, perm, keys_out, d_weight, d_grid_rgb, st);
    if (rc == AVL_OK && d_row_dirty) {
        hipLaunchKernelGGL(row_dirty_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, st, n, perm, b->dirty,
                           d_row_dirty, clear_dirty);
        if (hipGetLastError() != hipSuccess) rc = AVL_ERR_HIP;
    }
    (void)hipFreeAsync(block, st);
    if (rc != AVL_OK) return rc;
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    return AVL_OK;
}

int avl_builder_import_map(avl_builder* b, int64_t n, const float* d_grid_feat, const int32_t* d_grid_pos,
                           const float* d_weight, const uint8_t* d_grid_rgb, void* stream) {
    AVL_REQUIRE(b, "avl_builder_import_map: null handle");
    AVL_REQUIRE(n >= 0, "avl_builder_import_map: bad n");
    hipStream_t st = as_stream(stream);
    // a map that grew past the initial capacity (the reference doubles its arrays, _reserve_map_space vlmap_builder.py:286-311,
    // and resumes such a map): grow like a frame launch would, if the handle is allowed to
    if (n > b->capacity && b->max_capacity > b->capacity) {
        const int rcg = grow_builder(b, n, st);
        if (rcg != AVL_OK) return rcg;
    }
    AVL_REQUIRE(n <= b->capacity, "avl_builder_import_map: %lld voxels exceed the capacity %lld (avl_builder_set_max_capacity lets it grow)",
                (long long)n, (long long)b->capacity);
    int64_t have = 0;
    int rc = avl_builder_num_voxels(b, &have, stream);
    if (rc != AVL_OK) return rc;
    if (have != 0) {
        set_error("avl_builder_import_map: the map already holds %lld voxels (import into an empty builder)", (long long)have);
        return AVL_ERR_STATE;
    }
    if (n == 0) {
        b->key_bias = 1ull << 62;   // continuing a map: the voxels of new frames order after every imported one (none here: the
        return AVL_OK;              // other ranks of a resumed multi-GPU build import nothing but must use the same key space)
    }
    AVL_REQUIRE(d_grid_feat && d_grid_pos && d_weight, "avl_builder_import_map: null input");
    int64_t blocks = (n + 3) / 4;
    const int64_t maxb = (int64_t)num_cus() * 16;
    if (blocks > maxb) blocks = maxb;
    hipLaunchKernelGGL(import_map_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, b->D, b->n0, b->gs, b->vh, d_grid_feat, d_grid_pos,
                       d_weight, d_grid_rgb, b->cell_slot, b->slot_cell, b->slot_key, b->sum_feat, b->sum_w4, b->first_feat,
                       b->first_alpha, b->err_flags);
    const unsigned long long nn = (unsigned long long)n;
    AVL_HIP_CHECK(hipMemcpyAsync(b->counters, &nn, sizeof(nn), hipMemcpyHostToDevice, st));
    int flags = 0;
    AVL_HIP_CHECK(hipMemcpyAsync(&flags, b->err_flags, sizeof(int), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    if (flags & 4) {
        set_error("avl_builder_import_map: a grid_pos row lies outside the (gs, gs, vh) grid");
        return AVL_ERR_INVALID;
    }
    b->key_bias = 1ull << 62;
    b->vox_bound = n;
    return AVL_OK;
}

int avl_builder_export_raw(avl_builder* b, int64_t n, int32_t* d_cell, uint64_t* d_first_key, double* d_sum_feat,
                           double* d_sum_w4, float* d_first_feat, double* d_first_alpha, void* stream) {
    AVL_REQUIRE(b, "avl_builder_export_raw: null handle");
    hipStream_t st = as_stream(stream);
    int64_t have = 0;
    int rc = avl_builder_num_voxels(b, &have, stream);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n >= 0 && n <= have, "avl_builder_export_raw: n=%lld but the map holds %lld voxels", (long long)n, (long long)have);
    if (n == 0) return AVL_OK;
    const size_t D = (size_t)b->D;
    auto cp = [&](void* dst, const void* src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
    };
    AVL_HIP_CHECK(cp(d_cell, b->slot_cell, (size_t)n * sizeof(int32_t)));
    AVL_HIP_CHECK(cp(d_first_key, b->slot_key, (size_t)n * sizeof(uint64_t)));
    AVL_HIP_CHECK(cp(d_sum_feat, b->sum_feat, (size_t)n * D * sizeof(double)));
    AVL_HIP_CHECK(cp(d_sum_w4, b->sum_w4, (size_t)n * 4 * sizeof(double)));
    AVL_HIP_CHECK(cp(d_first_feat, b->first_feat, (size_t)n * D * sizeof(float)));
    AVL_HIP_CHECK(cp(d_first_alpha, b->first_alpha, (size_t)n * sizeof(double)));
    return AVL_OK;
}

int avl_points_bbox(const void* d_depth, int depth_is_u16, double depth_div, int H, int W, const double* h_calib_inv,
                    const double* h_transform, const int32_t* d_sample_idx, int P, double min_depth, double max_depth,
                    double* h_minmax, void* stream) {
    AVL_REQUIRE(H > 0 && W > 0 && P >= 0 && h_calib_inv && h_transform && h_minmax, "avl_points_bbox: bad arguments");
    if (P == 0) return AVL_OK;
    AVL_REQUIRE(d_depth && d_sample_idx, "avl_points_bbox: null pointer");
    hipStream_t st = as_stream(stream);
    auto key = [](double v) {
        unsigned long long u;
        memcpy(&u, &v, 8);
        return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
    };
    auto unkey = [](unsigned long long k) {
        unsigned long long u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
        double v;
        memcpy(&v, &u, 8);
        return v;
    };
    unsigned long long h_keys[6];
    for (int i = 0; i < 6; ++i) h_keys[i] = key(h_minmax[i]);
    unsigned long long* d_keys = nullptr;
    AVL_HIP_CHECK(hipMallocAsync((void**)&d_keys, sizeof(h_keys), st));
    AVL_HIP_CHECK(hipMemcpyAsync(d_keys, h_keys, sizeof(h_keys), hipMemcpyHostToDevice, st));
    FrameParams fp{};
    for (int i = 0; i < 9; ++i) fp.kinv[i] = h_calib_inv[i];
    for (int i = 0; i < 16; ++i) fp.t[i] = h_transform[i];
    fp.min_depth = min_depth; fp.max_depth = max_depth;
    fp.H = H; fp.W = W; fp.P = P;
    fp.depth_u16 = depth_is_u16 ? 1 : 0;
    fp.depth_div = depth_div;
    hipLaunchKernelGGL(bbox_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, fp, reinterpret_cast<const float*>(d_depth),
                       d_sample_idx, d_keys);
    AVL_HIP_CHECK(hipMemcpyAsync(h_keys, d_keys, sizeof(h_keys), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    (void)hipFreeAsync(d_keys, st);
    for (int i = 0; i < 6; ++i) h_minmax[i] = unkey(h_keys[i]);
    return AVL_OK;
}

}  // extern "C"
