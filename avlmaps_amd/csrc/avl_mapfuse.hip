// Fusing a revisit into the map: the cells of map B moved into map A's grid, the join of both voxel lists by
// cell, and the weighted mean of the joined rows.  Upstream has no counterpart for finished maps; the arithmetic is its builder's
// running mean (vlmap_builder.py:172-178) in closed form, sum(w_i f_i) / sum(w_i).
//
// THE MOVE.  One thread per cell.  A cell is the centre of the interval of base coordinates that base_pos2grid_id_3d maps to it
// (the cell k = 0 is two cells wide upstream and has the centre 0); the point goes through the 4 x 4 transform in float64, every
// product and sum rounded once (this file is built with -ffp-contract=off), and back through upstream's expression: a true float64
// divide and two truncations.  The whole-cell shift is added to the indices.  Without a transform nothing floats.
//
// THE PLAN.  Integers only.  The selected rows of A are numbered in row order (avl_scan.h's count / scan / number) and entered into
// the cell index (avl_cellindex.h) through a copy of the cells in which every other row is (-1, -1, -1): the index ignores those.  A
// selected row whose own cell names another row shares its cell: an error.  Every selected row of B probes that index; a hit gives
// its output voxel.  The rows that miss go into a SECOND index over the list in reverse order, in the same buffer: the index keeps
// the largest row of a cell, which in reverse order is the smallest row of B.  Those first rows are numbered in row order behind A's
// voxels, the other rows of a cell take their first row's number.  A stable argsort of the B rows by output voxel (avl_argsort_bits,
// unselected rows under a key above every voxel) is the CSR's row list, ascending within a voxel; b_start[v] is the lower bound of v
// in the sorted keys.  The counts are integer sums through atomics: the order does not matter.
//
// THE ROWS.  The hot kernel: about 2 KB read per member and 2 KB written per voxel at D = 512, no reuse -- bandwidth.  A group of L
// lanes owns an output voxel, L = 64 (one wave per voxel) for D > 128 and the power of two that covers D / 4 below, so that at a
// small D a wave serves several voxels with all lanes loading.  A lane owns the elements 4 * (lane % L) + 4 * L * k .. + 3: one 16-byte
// load per member and one 16-byte store where D % 4 == 0 and the matrix is 16-byte aligned, scalars otherwise; the elements do not
// depend on each other, so both paths give the same bytes.  Member indices and weights are the same addresses for all lanes of a
// group and are read again per chunk from cache (two chunks at D = 512).  Four float64 accumulators per lane, no LDS, no cross-lane
// step.  Rows of B are gathered as whole contiguous rows; the grid keeps every CU at 16 workgroups.
#include "avl_mapfuse.h"
#include "avl_scan.h"

namespace avl {

constexpr int kMfScanThreads = 256, kMfScanPer = 4;
constexpr int kMfErrOutside = 1, kMfErrShared = 2;

__global__ __launch_bounds__(256) void mf_move_kernel(const int32_t* __restrict__ cells, int64_t n, MfTransform T, bool moving, int sr, int sc, int sh,
                                                      int gs, double cs, int vh, int32_t* __restrict__ out, uint8_t* __restrict__ inside) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int64_t r = cells[3 * i], c = cells[3 * i + 1], h = cells[3 * i + 2];
        bool ok = true;
        if (moving) {
            const int64_t kr = gs / 2 - r, kc = gs / 2 - c;
            const double x = ((double)kr + (kr > 0 ? 0.5 : kr < 0 ? -0.5 : 0.0)) * cs;
            const double y = ((double)kc + (kc > 0 ? 0.5 : kc < 0 ? -0.5 : 0.0)) * cs;
            const double z = ((double)h + 0.5) * cs;
            const double x1 = ((T.t[0] * x + T.t[1] * y) + T.t[2] * z) + T.t[3];
            const double y1 = ((T.t[4] * x + T.t[5] * y) + T.t[6] * z) + T.t[7];
            const double z1 = ((T.t[8] * x + T.t[9] * y) + T.t[10] * z) + T.t[11];
            const double qx = x1 / cs, qy = y1 / cs, qz = z1 / cs;
            ok = fabs(qx) < 2147483648.0 && fabs(qy) < 2147483648.0 && fabs(qz) < 2147483648.0;     // false for a NaN
            if (ok) r = mf_index(qx, gs), c = mf_index(qy, gs), h = (int64_t)qz;
        }
        r += sr, c += sc, h += sh;
        ok = ok && r >= 0 && r < gs && c >= 0 && c < gs && h >= 0 && h < vh;
        out[3 * i] = ok ? (int32_t)r : -1;
        out[3 * i + 1] = ok ? (int32_t)c : -1;
        out[3 * i + 2] = ok ? (int32_t)h : -1;
        inside[i] = ok ? 1 : 0;
    }
}

// flag[i] = row i of A is selected and inside; masked = its cell, (-1, -1, -1) for every other row
__global__ __launch_bounds__(256) void mf_select_a_kernel(const int32_t* __restrict__ cells, const uint8_t* __restrict__ use, const float* __restrict__ w,
                                                          int64_t n, int gs, int vh, int32_t* __restrict__ masked, int32_t* __restrict__ flag,
                                                          int32_t* __restrict__ out_of_a, int32_t* __restrict__ head) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const bool sel = (!use || use[i]) && mf_weight_ok(w[i]);
        const bool in = mf_lin(cells, i, gs, vh) >= 0;
        if (sel && !in) atomicOr(head + 3, kMfErrOutside);
        const bool take = sel && in;
        masked[3 * i] = take ? cells[3 * i] : -1;
        masked[3 * i + 1] = take ? cells[3 * i + 1] : -1;
        masked[3 * i + 2] = take ? cells[3 * i + 2] : -1;
        flag[i] = take;
        out_of_a[i] = 0;                                // number_flagged_kernel writes 1 + rank into the flagged ones
    }
}

struct MfFlagged {
    const int32_t* flag;
    __device__ __forceinline__ bool operator()(int64_t i) const { return flag[i] != 0; }
};

// out_of_a: 1 + rank -> rank, 0 -> -1; a_row of the voxel; a selected row that does not own its cell shares it
__global__ __launch_bounds__(256) void mf_finish_a_kernel(const int32_t* __restrict__ cells, int64_t n, int gs, int vh, const uint32_t* __restrict__ bits,
                                                          const int32_t* __restrict__ prefix, const int32_t* __restrict__ perm,
                                                          int32_t* __restrict__ out_of_a, int32_t* __restrict__ a_row, int32_t* __restrict__ head,
                                                          int32_t* __restrict__ counts) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int v = out_of_a[i] - 1;
        out_of_a[i] = v;
        if (v >= 0) {
            a_row[v] = (int32_t)i;
            if (ci_probe(bits, prefix, perm, mf_lin(cells, i, gs, vh)) != i) atomicOr(head + 3, kMfErrShared);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[0] = (int32_t)n - head[1];
}

constexpr int kMfPending = -2;                          // out_of_b of a selected row of B that no row of A meets, until it is numbered

__global__ __launch_bounds__(256) void mf_select_b_kernel(const int32_t* __restrict__ cells, const uint8_t* __restrict__ inside,
                                                          const uint8_t* __restrict__ use, const float* __restrict__ w, int64_t n, int gs, int vh,
                                                          const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                                          const int32_t* __restrict__ perm, const int32_t* __restrict__ out_of_a,
                                                          int32_t* __restrict__ masked_rev, int32_t* __restrict__ out_of_b, int32_t* __restrict__ counts) {
    const int64_t rounds = (n + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);     // every lane takes part in every ballot
    for (int64_t k = 0; k < rounds; ++k) {
        const int64_t j = (k * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        bool unsel = false, outside = false, merged = false;
        if (j < n) {
            const bool sel = (!use || use[j]) && mf_weight_ok(w[j]);
            const int lin = (!inside || inside[j]) ? mf_lin(cells, j, gs, vh) : -1;
            unsel = !sel;
            outside = sel && lin < 0;
            int out = -1;
            bool fresh = false;
            if (sel && lin >= 0) {
                const int a = ci_probe(bits, prefix, perm, lin);
                merged = a >= 0;
                fresh = !merged;
                out = merged ? out_of_a[a] : kMfPending;
            }
            out_of_b[j] = out;
            const int64_t m = n - 1 - j;
            masked_rev[3 * m] = fresh ? cells[3 * j] : -1;
            masked_rev[3 * m + 1] = fresh ? cells[3 * j + 1] : -1;
            masked_rev[3 * m + 2] = fresh ? cells[3 * j + 2] : -1;
        }
        mf_count(unsel, counts + 1);
        mf_count(outside, counts + 2);
        mf_count(merged, counts + 3);
    }
}

// flag[j] = row j is the first row of B in its new cell
__global__ __launch_bounds__(256) void mf_first_b_kernel(const int32_t* __restrict__ cells, int64_t n, int gs, int vh, const uint32_t* __restrict__ bits,
                                                         const int32_t* __restrict__ prefix, const int32_t* __restrict__ perm,
                                                         const int32_t* __restrict__ out_of_b, int32_t* __restrict__ flag, int32_t* __restrict__ num) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        bool first = false;
        if (out_of_b[j] == kMfPending) first = n - 1 - ci_probe(bits, prefix, perm, mf_lin(cells, j, gs, vh)) == j;
        flag[j] = first;
        num[j] = 0;
    }
}

// head[2] = the new cells on entry; num[j] = 1 + rank of a first row
__global__ __launch_bounds__(256) void mf_number_b_kernel(const int32_t* __restrict__ cells, int64_t n_a, int64_t n, int gs, int vh,
                                                          const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                                          const int32_t* __restrict__ perm, const int32_t* __restrict__ num,
                                                          int32_t* __restrict__ out_of_b, int32_t* __restrict__ a_row, int32_t* __restrict__ keys,
                                                          const int32_t* __restrict__ head, int32_t* __restrict__ counts) {
    const int n_sel_a = head[1];
    const int64_t rounds = (n + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);
    for (int64_t k = 0; k < rounds; ++k) {
        const int64_t j = (k * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        bool later = false;
        if (j < n) {
            int out = out_of_b[j];
            if (out == kMfPending) {
                const int64_t first = n - 1 - ci_probe(bits, prefix, perm, mf_lin(cells, j, gs, vh));
                out = n_sel_a + num[first] - 1;
                later = first != j;
                if (!later) a_row[out] = -1;
                out_of_b[j] = out;
            }
            keys[j] = out >= 0 ? out : (int32_t)(n_a + n);      // above every voxel: an unselected row sorts to the end
        }
        mf_count(later, counts + 5);
    }
}

// after the scan of the first rows: head[0] = n_out, head[2] = the selected rows of B, counts[4] = the new cells (head[2] held them)
__global__ void mf_head_kernel(int64_t n_b, int32_t* __restrict__ head, int32_t* __restrict__ counts) {
    const int fresh = head[2];
    counts[4] = fresh;
    head[0] = head[1] + fresh;
    head[2] = (int32_t)n_b - counts[1] - counts[2];
}

// b_rows from the sorted order; b_start[v] = the first sorted position whose key is >= v
__global__ __launch_bounds__(256) void mf_csr_kernel(const int64_t* __restrict__ order, const int32_t* __restrict__ keys, int64_t n_b, int64_t n_v,
                                                     const int32_t* __restrict__ head, int32_t* __restrict__ b_start, int32_t* __restrict__ b_rows) {
    const int n_sel = head[2];
    const int64_t items = n_b > n_v ? n_b : n_v;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        if (i < n_b) b_rows[i] = i < n_sel ? (int32_t)order[i] : -1;
        if (i < n_v) {
            int64_t lo = 0, hi = n_b;                   // the first position p in [0, n_b] with keys[order[p]] >= i
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (keys[order[mid]] < i) lo = mid + 1; else hi = mid;
            }
            b_start[i] = (int32_t)(lo < n_sel ? lo : n_sel);
        }
    }
}

template <int L>
__global__ __launch_bounds__(256) void mf_rows_kernel(int64_t n_out, const int32_t* __restrict__ a_row, const int32_t* __restrict__ b_start,
                                                      const int32_t* __restrict__ b_rows, const float* __restrict__ feat_a, const float* __restrict__ w_a,
                                                      const uint8_t* __restrict__ rgb_a, const int32_t* __restrict__ cells_a, int64_t n_a,
                                                      const float* __restrict__ feat_b, const float* __restrict__ w_b, const uint8_t* __restrict__ rgb_b,
                                                      const int32_t* __restrict__ cells_b, int64_t n_b, int D, double g_a, double g_b, bool vec_a,
                                                      bool vec_b, bool vec_o, int gs, int vh, float* __restrict__ feat_out,
                                                      float* __restrict__ weight_out, uint8_t* __restrict__ rgb_out, int32_t* __restrict__ pos_out,
                                                      int32_t* __restrict__ occupied) {
    constexpr int kPerBlock = 256 / L;
    const int sub = threadIdx.x % L;
    const int64_t step = (int64_t)gridDim.x * kPerBlock;
    for (int64_t v = (int64_t)blockIdx.x * kPerBlock + threadIdx.x / L; v < n_out; v += step) {
        int a = a_row[v];
        if (a >= n_a) a = -1;
        int64_t p0 = b_start[v], p1 = b_start[v + 1];
        if (p0 < 0) p0 = 0;
        if (p1 > n_b) p1 = n_b;
        // the sum of the weights, in member order
        double W = 0.0;
        bool any = false;
        if (a >= 0) W = (double)w_a[a] * g_a, any = true;
        for (int64_t p = p0; p < p1; ++p) {
            const int b = b_rows[p];
            if (b < 0 || b >= n_b) continue;
            const double wi = (double)w_b[b] * g_b;
            W = any ? W + wi : wi;
            any = true;
        }
        float* __restrict__ ro = feat_out + (size_t)v * D;
        for (int d = 4 * sub; d < D; d += 4 * L) {
            MfAcc acc{0.0, 0.0, 0.0, 0.0, false};
            if (a >= 0) acc.add((double)w_a[a] * g_a, mf_load4(feat_a + (size_t)a * D, d, D, vec_a));
            for (int64_t p = p0; p < p1; ++p) {
                const int b = b_rows[p];
                if (b < 0 || b >= n_b) continue;
                acc.add((double)w_b[b] * g_b, mf_load4(feat_b + (size_t)b * D, d, D, vec_b));
            }
            float4 o;
            o.x = any ? (float)(acc.x / W) : 0.0f;
            o.y = any ? (float)(acc.y / W) : 0.0f;
            o.z = any ? (float)(acc.z / W) : 0.0f;
            o.w = any ? (float)(acc.w / W) : 0.0f;
            if (vec_o) {
                *reinterpret_cast<float4*>(ro + d) = o;
            } else {
                ro[d] = o.x;
                if (d + 1 < D) ro[d + 1] = o.y;
                if (d + 2 < D) ro[d + 2] = o.z;
                if (d + 3 < D) ro[d + 3] = o.w;
            }
        }
        if (sub == 0) {
            MfAcc acc{0.0, 0.0, 0.0, 0.0, false};
            const int32_t* cell = nullptr;
            if (a >= 0) {
                acc.add((double)w_a[a] * g_a, make_float4((float)rgb_a[3 * (size_t)a], (float)rgb_a[3 * (size_t)a + 1], (float)rgb_a[3 * (size_t)a + 2], 0.0f));
                cell = cells_a + 3 * (size_t)a;
            }
            for (int64_t p = p0; p < p1; ++p) {
                const int b = b_rows[p];
                if (b < 0 || b >= n_b) continue;
                acc.add((double)w_b[b] * g_b, make_float4((float)rgb_b[3 * (size_t)b], (float)rgb_b[3 * (size_t)b + 1], (float)rgb_b[3 * (size_t)b + 2], 0.0f));
                if (!cell) cell = cells_b + 3 * (size_t)b;
            }
            weight_out[v] = any ? (float)W : 0.0f;
            rgb_out[3 * v] = any ? (uint8_t)(int)(acc.x / W) : 0;
            rgb_out[3 * v + 1] = any ? (uint8_t)(int)(acc.y / W) : 0;
            rgb_out[3 * v + 2] = any ? (uint8_t)(int)(acc.z / W) : 0;
            const int r = cell ? cell[0] : -1, c = cell ? cell[1] : -1, h = cell ? cell[2] : -1;
            pos_out[3 * v] = r, pos_out[3 * v + 1] = c, pos_out[3 * v + 2] = h;
            if (occupied) {
                const int64_t lin = ci_linear(r, c, h, gs, vh);
                if (lin >= 0) occupied[lin] = (int32_t)v;
            }
        }
    }
}

static int mf_bit_length(int64_t x) {
    int b = 0;
    while (x > 0) ++b, x >>= 1;
    return b < 1 ? 1 : b;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_map_move_cells(const int32_t* d_cells, int64_t n, const double* h_T, const int32_t* h_shift, int gs, double cs, int vh, int32_t* d_out,
                       uint8_t* d_inside, void* stream) {
    const int rc = ci_check_grid("avl_map_move_cells", n, gs, vh);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(cs > 0.0 && cs < __builtin_inf(), "avl_map_move_cells: cs = %g (> 0 and finite)", cs);
    MfTransform T{};
    if (h_T) {
        for (int k = 0; k < 16; ++k) AVL_REQUIRE(h_T[k] - h_T[k] == 0.0, "avl_map_move_cells: the transform is not finite (element %d)", k);
        AVL_REQUIRE(h_T[12] == 0.0 && h_T[13] == 0.0 && h_T[14] == 0.0 && h_T[15] == 1.0, "avl_map_move_cells: the bottom row of the transform is not 0 0 0 1");
        for (int k = 0; k < 12; ++k) T.t[k] = h_T[k];
    }
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_cells && d_out && d_inside, "avl_map_move_cells: null pointer");
    const int sr = h_shift ? h_shift[0] : 0, sc = h_shift ? h_shift[1] : 0, sh = h_shift ? h_shift[2] : 0;
    hipLaunchKernelGGL(mf_move_kernel, dim3(stride_blocks(n)), dim3(256), 0, as_stream(stream), d_cells, n, T, h_T != nullptr, sr, sc, sh, gs, cs, vh,
                       d_out, d_inside);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_map_fuse_plan(const int32_t* d_cells_a, const uint8_t* d_use_a, const float* d_w_a, int64_t n_a, const int32_t* d_cells_b,
                      const uint8_t* d_inside_b, const uint8_t* d_use_b, const float* d_w_b, int64_t n_b, int gs, int vh, void* d_index,
                      size_t index_bytes, void* d_sort_work, size_t sort_work_bytes, int32_t* d_scratch, int64_t scratch_i32, int32_t* d_head,
                      int32_t* d_a_row, int32_t* d_b_start, int32_t* d_b_rows, int32_t* d_out_of_a, int32_t* d_out_of_b, int32_t* d_counts,
                      void* stream) {
    AVL_REQUIRE(n_a >= 0 && n_b >= 0 && n_a < INT_MAX && n_b < INT_MAX && n_a + n_b < INT_MAX, "avl_map_fuse_plan: %lld and %lld rows (together 0 .. 2^31 - 2)",
                (long long)n_a, (long long)n_b);
    const int64_t m = std::max(n_a, n_b);
    int rc = ci_check_grid("avl_map_fuse_plan", m, gs, vh);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_index && d_scratch && d_head && d_a_row && d_b_start && d_b_rows && d_counts, "avl_map_fuse_plan: null pointer");
    AVL_REQUIRE((d_cells_a && d_w_a && d_out_of_a) || n_a == 0, "avl_map_fuse_plan: null pointer for map A");
    AVL_REQUIRE((d_cells_b && d_w_b && d_out_of_b && d_sort_work) || n_b == 0, "avl_map_fuse_plan: null pointer for map B");
    AVL_REQUIRE(reinterpret_cast<uintptr_t>(d_scratch) % 8 == 0, "avl_map_fuse_plan: the scratch array is not 8-byte aligned");
    AVL_REQUIRE(scratch_i32 >= 9 * m + 1024, "avl_map_fuse_plan: the scratch array has %lld int32, needs %lld", (long long)scratch_i32,
                (long long)(9 * m + 1024));
    const size_t index_need = ci_layout(d_index, m, gs, vh).total;
    AVL_REQUIRE(index_bytes >= index_need, "avl_map_fuse_plan: the index buffer has %zu bytes, needs %zu", index_bytes, index_need);
    const int bits = mf_bit_length(n_a + n_b);
    size_t sort_need = 0;
    rc = avl_argsort_bits_work_bytes(n_b, 4, bits, &sort_need);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n_b == 0 || sort_work_bytes >= sort_need, "avl_map_fuse_plan: the sort workspace has %zu bytes, needs %zu", sort_work_bytes, sort_need);

    // the one layout of the scratch array, in int32: 8 m + m / 1024 + 1 + five roundings to 64 <= 9 m + 1024
    const int64_t nblocks = (m + kMfScanThreads * kMfScanPer - 1) / (kMfScanThreads * kMfScanPer);
    int64_t at = 0;
    const auto piece = [&](int64_t count) {
        int32_t* p = d_scratch + at;
        at += (count + 63) / 64 * 64;
        return p;
    };
    int64_t* order = reinterpret_cast<int64_t*>(piece(2 * n_b));
    int32_t* masked = piece(3 * m);
    int32_t* flag = piece(m);
    int32_t* num = piece(m);
    int32_t* keys = piece(n_b);
    int32_t* block_counts = piece(nblocks + 1);

    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(d_head, 0, 4 * sizeof(int32_t), st));
    AVL_HIP_CHECK(hipMemsetAsync(d_counts, 0, 6 * sizeof(int32_t), st));
    const dim3 scan_t(kMfScanThreads);
    const MfFlagged flagged{flag};

    // map A: select, index, number in row order
    if (n_a) hipLaunchKernelGGL(mf_select_a_kernel, dim3(stride_blocks(n_a)), dim3(256), 0, st, d_cells_a, d_use_a, d_w_a, n_a, gs, vh, masked, flag, d_out_of_a, d_head);
    rc = avl_cell_index_build(masked, n_a, gs, vh, d_index, index_bytes, stream);
    if (rc != AVL_OK) return rc;
    CellIndexView ix = ci_layout(d_index, n_a, gs, vh);
    if (n_a) {
        const int64_t nb = (n_a + kMfScanThreads * kMfScanPer - 1) / (kMfScanThreads * kMfScanPer);
        hipLaunchKernelGGL((count_flagged_kernel<kMfScanThreads, kMfScanPer, MfFlagged>), dim3((unsigned)nb), scan_t, 0, st, n_a, flagged, block_counts);
        hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)block_counts, nb, block_counts, d_head + 1,
                           OpSum{}, 0);
        hipLaunchKernelGGL((number_flagged_kernel<kMfScanThreads, kMfScanPer, MfFlagged>), dim3((unsigned)nb), scan_t, 0, st, n_a, flagged,
                           (const int*)block_counts, d_out_of_a);
        hipLaunchKernelGGL(mf_finish_a_kernel, dim3(stride_blocks(n_a)), dim3(256), 0, st, d_cells_a, n_a, gs, vh, (const uint32_t*)ix.bits,
                           (const int32_t*)ix.prefix, (const int32_t*)ix.perm, d_out_of_a, d_a_row, d_head, d_counts);
    }
    // map B: probe A's index, then the index of the rows that missed, in reverse order
    if (n_b) {
        hipLaunchKernelGGL(mf_select_b_kernel, dim3(stride_blocks(n_b)), dim3(256), 0, st, d_cells_b, d_inside_b, d_use_b, d_w_b, n_b, gs, vh,
                           (const uint32_t*)ix.bits, (const int32_t*)ix.prefix, (const int32_t*)ix.perm, (const int32_t*)d_out_of_a, masked, d_out_of_b,
                           d_counts);
        rc = avl_cell_index_build(masked, n_b, gs, vh, d_index, index_bytes, stream);
        if (rc != AVL_OK) return rc;
        ix = ci_layout(d_index, n_b, gs, vh);
        const int64_t nb = (n_b + kMfScanThreads * kMfScanPer - 1) / (kMfScanThreads * kMfScanPer);
        hipLaunchKernelGGL(mf_first_b_kernel, dim3(stride_blocks(n_b)), dim3(256), 0, st, d_cells_b, n_b, gs, vh, (const uint32_t*)ix.bits,
                           (const int32_t*)ix.prefix, (const int32_t*)ix.perm, (const int32_t*)d_out_of_b, flag, num);
        hipLaunchKernelGGL((count_flagged_kernel<kMfScanThreads, kMfScanPer, MfFlagged>), dim3((unsigned)nb), scan_t, 0, st, n_b, flagged, block_counts);
        hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)block_counts, nb, block_counts, d_head + 2,
                           OpSum{}, 0);
        hipLaunchKernelGGL((number_flagged_kernel<kMfScanThreads, kMfScanPer, MfFlagged>), dim3((unsigned)nb), scan_t, 0, st, n_b, flagged,
                           (const int*)block_counts, num);
        hipLaunchKernelGGL(mf_number_b_kernel, dim3(stride_blocks(n_b)), dim3(256), 0, st, d_cells_b, n_a, n_b, gs, vh, (const uint32_t*)ix.bits,
                           (const int32_t*)ix.prefix, (const int32_t*)ix.perm, (const int32_t*)num, d_out_of_b, d_a_row, keys, (const int32_t*)d_head,
                           d_counts);
    }
    hipLaunchKernelGGL(mf_head_kernel, dim3(1), dim3(1), 0, st, n_b, d_head, d_counts);
    AVL_HIP_CHECK(hipGetLastError());
    rc = avl_argsort_bits(n_b, keys, 4, bits, order, d_sort_work, sort_work_bytes, stream);
    if (rc != AVL_OK) return rc;
    hipLaunchKernelGGL(mf_csr_kernel, dim3(stride_blocks(n_a + n_b + 1)), dim3(256), 0, st, (const int64_t*)order, (const int32_t*)keys, n_b, n_a + n_b + 1,
                       (const int32_t*)d_head, d_b_start, d_b_rows);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_map_fuse_rows(int64_t n_out, const int32_t* d_a_row, const int32_t* d_b_start, const int32_t* d_b_rows, const float* d_feat_a,
                      const float* d_w_a, const uint8_t* d_rgb_a, const int32_t* d_cells_a, int64_t n_a, const float* d_feat_b, const float* d_w_b,
                      const uint8_t* d_rgb_b, const int32_t* d_cells_b, int64_t n_b, int D, double g_a, double g_b, int gs, int vh, float* d_feat_out,
                      float* d_weight_out, uint8_t* d_rgb_out, int32_t* d_grid_pos_out, int32_t* d_occupied, void* stream) {
    AVL_REQUIRE(n_a >= 0 && n_b >= 0 && n_a + n_b < INT_MAX && n_out >= 0 && n_out <= n_a + n_b,
                "avl_map_fuse_rows: %lld output voxels of %lld and %lld rows (n_out <= n_a + n_b < 2^31 - 1)", (long long)n_out, (long long)n_a, (long long)n_b);
    const int rc = ci_check_grid("avl_map_fuse_rows", n_out, gs, vh);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(D >= 1 && D <= kMfMaxDim, "avl_map_fuse_rows: D = %d (1 .. %d)", D, kMfMaxDim);
    AVL_REQUIRE(g_a > 0.0 && g_a < __builtin_inf() && g_b > 0.0 && g_b < __builtin_inf(), "avl_map_fuse_rows: gains %g and %g (> 0 and finite)", g_a, g_b);
    AVL_REQUIRE(n_out == 0 || (d_a_row && d_b_start && d_feat_out && d_weight_out && d_rgb_out && d_grid_pos_out), "avl_map_fuse_rows: null pointer");
    AVL_REQUIRE(n_out == 0 || n_a == 0 || (d_feat_a && d_w_a && d_rgb_a && d_cells_a), "avl_map_fuse_rows: null pointer for map A");
    AVL_REQUIRE(n_out == 0 || n_b == 0 || (d_b_rows && d_feat_b && d_w_b && d_rgb_b && d_cells_b), "avl_map_fuse_rows: null pointer for map B");
    hipStream_t st = as_stream(stream);
    if (d_occupied) AVL_HIP_CHECK(hipMemsetAsync(d_occupied, 0xFF, (size_t)gs * gs * vh * sizeof(int32_t), st));
    if (n_out == 0) return AVL_OK;
    const bool quad = D % 4 == 0;
    const bool vec_a = quad && reinterpret_cast<uintptr_t>(d_feat_a) % 16 == 0, vec_b = quad && reinterpret_cast<uintptr_t>(d_feat_b) % 16 == 0;
    const bool vec_o = quad && reinterpret_cast<uintptr_t>(d_feat_out) % 16 == 0;
    const int quads = (D + 3) / 4;
#define AVL_MF_LAUNCH(L)                                                                                                                            \
    hipLaunchKernelGGL(mf_rows_kernel<L>, dim3(stride_blocks(n_out* L)), dim3(256), 0, st, n_out, d_a_row, d_b_start, d_b_rows, d_feat_a, d_w_a, d_rgb_a, \
                       d_cells_a, n_a, d_feat_b, d_w_b, d_rgb_b, d_cells_b, n_b, D, g_a, g_b, vec_a, vec_b, vec_o, gs, vh, d_feat_out, d_weight_out,      \
                       d_rgb_out, d_grid_pos_out, d_occupied)
    if (quads > 32) AVL_MF_LAUNCH(64);
    else if (quads > 16) AVL_MF_LAUNCH(32);
    else if (quads > 8) AVL_MF_LAUNCH(16);
    else if (quads > 4) AVL_MF_LAUNCH(8);
    else if (quads > 2) AVL_MF_LAUNCH(4);
    else if (quads > 1) AVL_MF_LAUNCH(2);
    else AVL_MF_LAUNCH(1);
#undef AVL_MF_LAUNCH
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
