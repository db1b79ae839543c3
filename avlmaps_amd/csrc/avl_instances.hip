// Object instances in 3-D for gfx950: the connected components of the masked voxels of a SPARSE voxel list, and their table.
//
// Upstream has no counterpart.  Its nearest lines stop at the category mask: avlmaps/map/map.py:146-151 (the mask of a category)
// and avlmaps/map/vlmap_3d.py:75-100 (the 3-D index of a category); a user would scatter grid_pos into a dense
// 1000 x 1000 x 30 array on the host and call scipy.ndimage.label on it.  This labels the map's own voxel list instead, with the
// union-find and the numbering that avl_islands.hip uses on a dense image.
//
// What is pinned.  Two masked voxels are adjacent when their cells (row, col, height) differ by at most 1 on every axis and the
// number of differing axes is <= 1 / 2 / 3 for connectivity 6 / 18 / 26; voxels that share a cell belong together; unmasked voxels
// take part in nothing; instances are numbered 1 .. n in lexicographic (row, col, height) order of their first cell.  That is
// scipy.ndimage.label(dense, generate_binary_structure(3, k)) with dense[row, col, height] and k = 1, 2, 3, read back at the voxels.
// Every output follows uniquely from these definitions and is a minimum, a maximum or a sum of integers: the bytes do not depend
// on the order in which the atomics land.
//
// Labelling.  avl_voxel_label.h's labeller under its mask policy (VlMask): the pipeline is described there.
//
// Table.  avl_voxel_instance_table reads pos, labels and scores in voxel order, three passes: (1) count, box, coordinate sums and
// the largest score key; (2) among the voxels of an instance's first row the smallest (col, height), and among the voxels with the
// largest score the smallest index; (3) among the voxels of the first cell the smallest index.  Voxel order is insertion order, so
// the voxels of an object are spread over all waves: pass 1 collects a workgroup's voxels per label in LDS and sends each row to the
// table once (with one atomic per voxel and column a category of a few large objects spent 10 of its 11 ms on a few hundred hot
// words).  Minima and maxima are compared with a plain load first, so that most of them issue no atomic at all.
#include <algorithm>
#include <climits>

#include "avl_common.h"
#include "avl_voxel_label.h"

namespace avl {

constexpr int kVxTableCols = 12;                // count, rmin, rmax, cmin, cmax, hmin, hmax, sum_row, sum_col, sum_height, first, best
constexpr int kVxSlots = 256;                   // labels a workgroup of the table's first pass keeps in LDS (a power of two)
constexpr int kVxProbe = 8;
constexpr int kVxTablePer = 8192;               // voxels per workgroup of that pass, at least

// ---------------------------------------------------------------------------------------------------------------- the table
__device__ __forceinline__ long long vx_load64(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vx_min64(long long* p, long long v) {
    if (v < vx_load64(p)) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void vx_max64(long long* p, long long v) {
    if (v > vx_load64(p)) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void vx_add64(long long* p, long long v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// order-preserving unsigned image of a score: +0 and -0 coincide (np.argmax holds them equal), a NaN is below everything
__device__ __forceinline__ uint32_t vx_score_key(float v) {
    if (v != v) return 0u;
    if (v == 0.f) v = 0.f;
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void vx_table_init_kernel(long long* __restrict__ table, unsigned long long* __restrict__ first_cell,
                                                            uint32_t* __restrict__ score_key, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    long long* t = table + (int64_t)k * kVxTableCols;
    t[0] = 0;
    t[1] = t[3] = t[5] = LLONG_MAX;
    t[2] = t[4] = t[6] = LLONG_MIN;
    t[7] = t[8] = t[9] = 0;
    t[10] = t[11] = LLONG_MAX;
    first_cell[k] = ~0ull;
    score_key[k] = 0u;
}

// a row of partial results, in the table's column order: count, (min, max) of row, col and height, the three sums
constexpr int kVxRowVals = 10;

__device__ __forceinline__ void vx_row_commit(long long* t, uint32_t* score_key, const long long* v, uint32_t key, bool scored) {
    vx_add64(t + 0, v[0]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        vx_min64(t + 1 + 2 * c, v[1 + 2 * c]);
        vx_max64(t + 2 + 2 * c, v[2 + 2 * c]);
        vx_add64(t + 7 + c, v[7 + c]);
    }
    if (scored && key > __hip_atomic_load(score_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(score_key, key);
}

// pass 1.  A workgroup keeps up to kVxSlots labels in LDS (open addressing, kVxProbe probes) and adds its kVxTablePer or more voxels
// there; its rows go to the table once, at the end.  A voxel whose label finds no slot goes to the table directly: that happens when
// a workgroup meets more labels than slots, and then the table's rows are many and an atomic seldom meets another
__global__ __launch_bounds__(256) void vx_table_pass1_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ labels,
                                                             const float* __restrict__ scores, int64_t N, int n, long long* __restrict__ table,
                                                             uint32_t* __restrict__ score_key) {
    __shared__ int s_label[kVxSlots];
    __shared__ uint32_t s_key[kVxSlots];
    __shared__ long long s_v[kVxSlots][kVxRowVals];
    for (int s = threadIdx.x; s < kVxSlots; s += blockDim.x) {
        s_label[s] = 0;
        s_key[s] = 0u;
        s_v[s][0] = s_v[s][7] = s_v[s][8] = s_v[s][9] = 0;
        s_v[s][1] = s_v[s][3] = s_v[s][5] = LLONG_MAX;
        s_v[s][2] = s_v[s][4] = s_v[s][6] = LLONG_MIN;
    }
    __syncthreads();
    const bool scored = scores != nullptr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int lab = labels[i];
        if (lab <= 0 || lab > n) continue;
        const long long p[3] = {pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]};
        const uint32_t key = scored ? vx_score_key(scores[i]) : 0u;
        int slot = -1;
        unsigned s = ((unsigned)lab * 2654435761u) >> 24 & (kVxSlots - 1);
        for (int t = 0; t < kVxProbe; ++t, s = (s + 1) & (kVxSlots - 1)) {
            const int old = atomicCAS(&s_label[s], 0, lab);
            if (old == 0 || old == lab) {
                slot = (int)s;
                break;
            }
        }
        if (slot < 0) {
            const long long v[kVxRowVals] = {1, p[0], p[0], p[1], p[1], p[2], p[2], p[0], p[1], p[2]};
            vx_row_commit(table + (int64_t)(lab - 1) * kVxTableCols, score_key + (lab - 1), v, key, scored);
            continue;
        }
        long long* v = s_v[slot];
        __hip_atomic_fetch_add(v + 0, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            __hip_atomic_fetch_min(v + 1 + 2 * c, p[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(v + 2 + 2 * c, p[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(v + 7 + c, p[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (scored) atomicMax(&s_key[slot], key);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kVxSlots; s += blockDim.x) {
        const int lab = s_label[s];
        if (lab > 0) vx_row_commit(table + (int64_t)(lab - 1) * kVxTableCols, score_key + (lab - 1), s_v[s], s_key[s], scored);
    }
}

// (col - cmin, height - hmin) of a voxel of the instance's first row, 32 bits each, the column on top: ordered like (col, height).
// Both differences are >= 0 and below 2^20 for labels of avl_label_voxels; the value is compared, never used as an index
__device__ __forceinline__ unsigned long long vx_cell_in_row(const long long* t, int c, int h) {
    const unsigned long long dc = (unsigned long long)((long long)c - t[3]), dh = (unsigned long long)((long long)h - t[5]);
    return (dc << 32) | (dh & 0xffffffffull);
}

// pass 2: the first cell of the instance = the smallest (col, height) of its first row; the smallest index among its best scores
__global__ __launch_bounds__(256) void vx_table_pass2_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ labels,
                                                             const float* __restrict__ scores, int64_t N, int n, long long* __restrict__ table,
                                                             unsigned long long* __restrict__ first_cell, const uint32_t* __restrict__ score_key) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int lab = labels[i];
        if (lab <= 0 || lab > n) continue;
        long long* t = table + (int64_t)(lab - 1) * kVxTableCols;
        if (pos[i * 3] == t[1]) {
            const unsigned long long cell = vx_cell_in_row(t, pos[i * 3 + 1], pos[i * 3 + 2]);
            if (cell < __hip_atomic_load(first_cell + (lab - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(first_cell + (lab - 1), cell);
        }
        if (scores && vx_score_key(scores[i]) == score_key[lab - 1]) vx_min64(t + 11, (long long)i);
    }
}

// pass 3: the smallest voxel index at the first cell
__global__ __launch_bounds__(256) void vx_table_pass3_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ labels, int64_t N, int n,
                                                             long long* __restrict__ table, const unsigned long long* __restrict__ first_cell) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int lab = labels[i];
        if (lab <= 0 || lab > n) continue;
        long long* t = table + (int64_t)(lab - 1) * kVxTableCols;
        if (pos[i * 3] == t[1] && vx_cell_in_row(t, pos[i * 3 + 1], pos[i * 3 + 2]) == first_cell[lab - 1]) vx_min64(t + 10, (long long)i);
    }
}

// a label without a voxel (a table asked for more instances than the labels hold) gets first = best = -1 and an empty box
__global__ __launch_bounds__(256) void vx_table_finish_kernel(const float* __restrict__ scores, int64_t N, int n, long long* __restrict__ table,
                                                              float* __restrict__ best_score) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    long long* t = table + (int64_t)k * kVxTableCols;
    if (t[10] == LLONG_MAX) t[10] = -1;
    if (t[11] == LLONG_MAX) t[11] = -1;
    const long long b = t[11];
    best_score[k] = scores && b >= 0 && b < N ? scores[b] : 0.f;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_label_voxels_work_bytes(int64_t N, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_label_voxels_work_bytes: null output");
    int rc = vl_check_n("avl_label_voxels_work_bytes", N);
    if (rc != AVL_OK) return rc;
    *bytes = vl_work(N, nullptr).total;
    return AVL_OK;
}

int avl_label_voxels(const int32_t* d_grid_pos, const uint8_t* d_mask, int64_t N, int connectivity, int32_t* d_labels, int32_t* d_n, void* ws,
                     size_t ws_bytes, void* stream) {
    int rc = vl_check_n("avl_label_voxels", N);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "avl_label_voxels: connectivity %d (6, 18 or 26)", connectivity);
    AVL_REQUIRE(d_grid_pos, "avl_label_voxels: null d_grid_pos");
    AVL_REQUIRE(d_mask, "avl_label_voxels: null d_mask");
    AVL_REQUIRE(d_labels, "avl_label_voxels: null d_labels");
    AVL_REQUIRE(d_n, "avl_label_voxels: null d_n");
    return label_sparse_voxels("avl_label_voxels", "masked", VlMask{d_mask}, d_grid_pos, N, connectivity, d_labels, d_n, ws, ws_bytes, stream);
}

int avl_voxel_instance_table(const int32_t* d_grid_pos, const int32_t* d_labels, const float* d_scores, int64_t N, int32_t n, int64_t* d_table,
                             float* d_best_score, void* stream) {
    int rc = vl_check_n("avl_voxel_instance_table", N);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n >= 0 && (int64_t)n <= N, "avl_voxel_instance_table: n = %d instances among %lld voxels", n, (long long)N);
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_grid_pos, "avl_voxel_instance_table: null d_grid_pos");
    AVL_REQUIRE(d_labels, "avl_voxel_instance_table: null d_labels");
    AVL_REQUIRE(d_table, "avl_voxel_instance_table: null d_table");
    AVL_REQUIRE(d_best_score, "avl_voxel_instance_table: null d_best_score");
    hipStream_t st = as_stream(stream);
    keep_mempool_once();
    unsigned long long* first_cell = nullptr;                        // n first cells, then n score keys
    AVL_HIP_CHECK(hipMallocAsync((void**)&first_cell, (size_t)n * (sizeof(uint64_t) + sizeof(uint32_t)), st));
    uint32_t* score_key = reinterpret_cast<uint32_t*>(first_cell + n);
    long long* table = reinterpret_cast<long long*>(d_table);
    const dim3 rows((unsigned)((n + 255) / 256)), sb(stride_blocks(N));
    hipLaunchKernelGGL(vx_table_init_kernel, rows, dim3(256), 0, st, table, first_cell, score_key, n);
    const dim3 pass1((unsigned)std::max<int64_t>(1, std::min<int64_t>((N + kVxTablePer - 1) / kVxTablePer, (int64_t)num_cus() * 4)));
    hipLaunchKernelGGL(vx_table_pass1_kernel, pass1, dim3(256), 0, st, d_grid_pos, d_labels, d_scores, N, n, table, score_key);
    hipLaunchKernelGGL(vx_table_pass2_kernel, sb, dim3(256), 0, st, d_grid_pos, d_labels, d_scores, N, n, table, first_cell, (const uint32_t*)score_key);
    hipLaunchKernelGGL(vx_table_pass3_kernel, sb, dim3(256), 0, st, d_grid_pos, d_labels, N, n, table, (const unsigned long long*)first_cell);
    hipLaunchKernelGGL(vx_table_finish_kernel, rows, dim3(256), 0, st, d_scores, N, n, table, d_best_score);
    (void)hipFreeAsync(first_cell, st);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
