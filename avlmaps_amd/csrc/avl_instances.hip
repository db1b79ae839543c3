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
// Labelling.  The work is done on the masked voxels in CELL order, on their ranks t = 0 .. M - 1:
//   box      bounding box and number M of the masked voxels (one pass, read back: the sort needs M, the key the box).  A side
//            beyond 2^20 cells is refused here: three sides of 20 bits make a key of at most 60 bits
//   compact  the masked voxels in index order (avl_scan.h: count_flagged_kernel per 1024 voxels, scan_counts_kernel, then one
//            write): key = ((row - rmin) * ny + (col - cmin)) * nz + (height - hmin) as uint64, value = the voxel index
//   sort     rocPRIM's stable radix sort over the key's bits: equal cells keep index order, so the smallest rank of a cell is its
//            smallest voxel index
//   merge    union-find on one int32 parent per rank (uf_unite; avl_unionfind.h states the invariant, an element being a rank).
//            A voxel looks at the 13 cells that precede it in raster order: the height neighbour and a second voxel of its own
//            cell are the previous rank; the three cells of each of the four preceding columns (row - 1, col - 1 .. col + 1) and
//            (row, col - 1) are consecutive ranks, found by ONE binary search per column among the ranks before t
//   flatten  parent = root (uf_flatten_kernel)
//   number   the roots counted per 1024 ranks, scanned, every root receives 1 + the number of roots before it (count_flagged_kernel,
//            scan_counts_kernel, number_flagged_kernel).  Roots are first cells and ranks are in cell order, which is the
//            lexicographic order of (row, col, height)
//   scatter  labels[voxel of rank t] = label of t's root; the unmasked voxels keep the 0 of the memset
// The workspace is 28 bytes per voxel of the list whatever the box (no grid over the box is kept, not even one of bits).
//
// Table.  avl_voxel_instance_table reads pos, labels and scores in voxel order, three passes: (1) count, box, coordinate sums and
// the largest score key; (2) among the voxels of an instance's first row the smallest (col, height), and among the voxels with the
// largest score the smallest index; (3) among the voxels of the first cell the smallest index.  Voxel order is insertion order, so
// the voxels of an object are spread over all waves: pass 1 collects a workgroup's voxels per label in LDS and sends each row to the
// table once (with one atomic per voxel and column a category of a few large objects spent 10 of its 11 ms on a few hundred hot
// words).  Minima and maxima are compared with a plain load first, so that most of them issue no atomic at all.
#include <algorithm>
#include <climits>

#include <rocprim/device/device_radix_sort.hpp>

#include "avl_common.h"
#include "avl_scan.h"
#include "avl_unionfind.h"

namespace avl {

constexpr int kVxMaxSide = 1 << 20;
constexpr int64_t kVxMaxVoxels = ((int64_t)1 << 31) - 1;
constexpr int kVxTableCols = 12;                // count, rmin, rmax, cmin, cmax, hmin, hmax, sum_row, sum_col, sum_height, first, best
constexpr int kVxScanThreads = 256;
constexpr int kVxScanPer = 4;
constexpr int kVxScanBlock = kVxScanThreads * kVxScanPer;
constexpr int kVxSlots = 256;                   // labels a workgroup of the table's first pass keeps in LDS (a power of two)
constexpr int kVxProbe = 8;
constexpr int kVxTablePer = 8192;               // voxels per workgroup of that pass, at least

struct VxHeader {
    int mn[3], mx[3];
    int count;                                  // masked voxels
    int pad;
};

// the masked voxels, for avl_scan.h's counting kernel and the compaction
struct VxMasked {
    const uint8_t* mask;
    __device__ __forceinline__ bool operator()(int64_t i) const { return mask[i] != 0; }
};

__global__ void vx_header_init_kernel(VxHeader* __restrict__ h) {
    if (threadIdx.x < 3) {
        h->mn[threadIdx.x] = INT_MAX;
        h->mx[threadIdx.x] = INT_MIN;
    }
    if (threadIdx.x == 3) h->count = h->pad = 0;
}

__global__ __launch_bounds__(256) void vx_box_kernel(const int32_t* __restrict__ pos, const uint8_t* __restrict__ mask, int64_t N,
                                                     VxHeader* __restrict__ h) {
    __shared__ int red[7][4];
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN}, cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        if (!mask[i]) continue;
        ++cnt;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int v = pos[i * 3 + c];
            mn[c] = min(mn[c], v);
            mx[c] = max(mx[c], v);
        }
    }
    const int w = threadIdx.x / kWave;
    cnt = wave_sum(cnt);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mn[c] = wave_min(mn[c]);
        mx[c] = wave_max(mx[c]);
        if ((threadIdx.x & (kWave - 1)) == 0) {
            red[c][w] = mn[c];
            red[3 + c][w] = mx[c];
        }
    }
    if ((threadIdx.x & (kWave - 1)) == 0) red[6][w] = cnt;
    __syncthreads();
    if (threadIdx.x < 7) {
        const int c = threadIdx.x;
        int v = red[c][0];
        for (int k = 1; k < 4; ++k) v = c < 3 ? min(v, red[c][k]) : (c < 6 ? max(v, red[c][k]) : v + red[c][k]);
        if (c == 6) {
            if (v) atomicAdd(&h->count, v);
        } else if (red[6][0] + red[6][1] + red[6][2] + red[6][3]) {         // a workgroup without a masked voxel offers nothing
            if (c < 3) atomicMin(&h->mn[c], v);
            else atomicMax(&h->mx[c - 3], v);
        }
    }
}

// the masked voxels in index order: key, voxel index and the rank's own parent.  M is the count of the box pass: nothing is
// written at or past it, whatever the mask holds by now
__global__ __launch_bounds__(kVxScanThreads) void vx_compact_kernel(const int32_t* __restrict__ pos, const uint8_t* __restrict__ mask, int64_t N,
                                                                    const int* __restrict__ offsets, int ox, int oy, int oz, int ny, int nz,
                                                                    int64_t M, unsigned long long* __restrict__ keys, int* __restrict__ idx,
                                                                    int* __restrict__ parent) {
    __shared__ int s_w[kVxScanThreads / kWave];
    const int64_t base = offsets[blockIdx.x];
    int64_t i0;
    int before, total;
    const int f = block_flags<kVxScanThreads, kVxScanPer>(N, VxMasked{mask}, s_w, &i0, &before, &total);
    int64_t t = base + before;
#pragma unroll
    for (int k = 0; k < kVxScanPer; ++k) {
        if (!(f >> k & 1) || t >= M) continue;
        const int64_t i = i0 + k;
        const unsigned long long x = (unsigned)(pos[i * 3] - ox), y = (unsigned)(pos[i * 3 + 1] - oy), z = (unsigned)(pos[i * 3 + 2] - oz);
        keys[t] = (x * (unsigned long long)ny + y) * (unsigned long long)nz + z;
        idx[t] = (int)i;
        parent[t] = (int)t;
        ++t;
    }
}

// the first rank in [0, hi) whose key is >= k
__device__ __forceinline__ int vx_lower_bound(const unsigned long long* __restrict__ keys, int hi, unsigned long long k) {
    int lo = 0;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// axes: 1, 2 or 3 = the number of axes on which adjacent cells may differ
__global__ __launch_bounds__(256) void vx_merge_kernel(const unsigned long long* __restrict__ keys, int M, int ny, int nz, int axes,
                                                       int* __restrict__ parent) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < M; t += gridDim.x * blockDim.x) {
        if (t == 0) continue;
        const unsigned long long key = keys[t], prev = keys[t - 1];
        if (prev == key) {                                            // a second voxel of the cell: the cell's first one does the rest
            uf_unite(parent, t, t - 1);
            continue;
        }
        const int z = (int)(key % (unsigned long long)nz);
        const unsigned long long col = key / (unsigned long long)nz;
        const int y = (int)(col % (unsigned long long)ny), x = (int)(col / (unsigned long long)ny);
        if (z > 0 && prev == key - 1) uf_unite(parent, t, t - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dx = k < 3 ? -1 : 0, dy = k < 3 ? k - 1 : -1;   // (-1, -1) (-1, 0) (-1, +1) (0, -1)
            const int dz = min(axes - (dy != 0) - (dx != 0), 1);      // the height may differ by dz (0 or 1); < 0: no such neighbour
            const int a = x + dx, b = y + dy;
            if (dz < 0 || a < 0 || b < 0 || b >= ny) continue;
            const unsigned long long base = ((unsigned long long)a * (unsigned long long)ny + (unsigned long long)b) * (unsigned long long)nz;
            const unsigned long long lo = base + (unsigned long long)max(z - dz, 0), hi = base + (unsigned long long)min(z + dz, nz - 1);
            unsigned long long last = ~0ull;                          // no key: a key has at most 60 bits
            for (int s = vx_lower_bound(keys, t, lo); s < t; ++s) {
                const unsigned long long ks = keys[s];
                if (ks > hi) break;
                if (ks != last) uf_unite(parent, t, s);               // the first voxel of each neighbouring cell
                last = ks;
            }
        }
    }
}

// idx[t] < N by construction (vx_compact_kernel wrote it); the comparison only keeps a foreign workspace from writing out of bounds
__global__ __launch_bounds__(256) void vx_scatter_labels_kernel(const int* __restrict__ parent, const int* __restrict__ rank_label,
                                                                const int* __restrict__ idx, int M, int64_t N, int* __restrict__ labels) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < M; t += gridDim.x * blockDim.x) {
        const int p = parent[t], i = idx[t];
        if (p >= 0 && p < M && i >= 0 && i < N) labels[i] = rank_label[p];
    }
}

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

static int vx_check_n(const char* what, int64_t N) {
    AVL_REQUIRE(N >= 0 && N <= kVxMaxVoxels, "%s: N = %lld voxels (0 .. %lld)", what, (long long)N, (long long)kVxMaxVoxels);
    return AVL_OK;
}

// workspace of avl_label_voxels: header | keys, sorted keys | voxel indices, sorted | parents | one count per scan block.  After the
// sort the unsorted indices are dead: their piece takes the labels of the roots
struct VxWork {
    int nblocks;
    VxHeader* header;
    unsigned long long *keys_in, *keys;
    int *idx_in, *idx, *parent, *counts;
    size_t total;
};
static VxWork vx_work(int64_t N, void* ws) {
    Carver c(ws);
    VxWork w;
    w.nblocks = (int)((N + kVxScanBlock - 1) / kVxScanBlock);
    w.header = c.ptr<VxHeader>(sizeof(VxHeader));
    w.keys_in = c.ptr<unsigned long long>((size_t)N * sizeof(uint64_t));
    w.keys = c.ptr<unsigned long long>((size_t)N * sizeof(uint64_t));
    w.idx_in = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.idx = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.parent = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.counts = c.ptr<int>((size_t)w.nblocks * sizeof(int32_t));
    w.total = c.total();
    return w;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_label_voxels_work_bytes(int64_t N, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_label_voxels_work_bytes: null output");
    int rc = vx_check_n("avl_label_voxels_work_bytes", N);
    if (rc != AVL_OK) return rc;
    *bytes = vx_work(N, nullptr).total;
    return AVL_OK;
}

int avl_label_voxels(const int32_t* d_grid_pos, const uint8_t* d_mask, int64_t N, int connectivity, int32_t* d_labels, int32_t* d_n, void* ws,
                     size_t ws_bytes, void* stream) {
    int rc = vx_check_n("avl_label_voxels", N);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "avl_label_voxels: connectivity %d (6, 18 or 26)", connectivity);
    AVL_REQUIRE(d_grid_pos, "avl_label_voxels: null d_grid_pos");
    AVL_REQUIRE(d_mask, "avl_label_voxels: null d_mask");
    AVL_REQUIRE(d_labels, "avl_label_voxels: null d_labels");
    AVL_REQUIRE(d_n, "avl_label_voxels: null d_n");
    const VxWork w = vx_work(N, ws);
    AVL_REQUIRE(ws && ws_bytes >= w.total, "avl_label_voxels: workspace (ws) of %zu bytes, need %zu", ws_bytes, w.total);
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(d_n, 0, sizeof(int32_t), st));
    if (N == 0) return AVL_OK;
    keep_mempool_once();
    AVL_HIP_CHECK(hipMemsetAsync(d_labels, 0, (size_t)N * sizeof(int32_t), st));
    hipLaunchKernelGGL(vx_header_init_kernel, dim3(1), dim3(64), 0, st, w.header);
    hipLaunchKernelGGL(vx_box_kernel, dim3(std::min(stride_blocks(N), 512u)), dim3(256), 0, st, d_grid_pos, d_mask, N, w.header);
    VxHeader h;
    AVL_HIP_CHECK(hipMemcpyAsync(&h, w.header, sizeof(h), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    const int64_t M = h.count;
    if (M == 0) return AVL_OK;
    AVL_REQUIRE(M > 0 && M <= N, "avl_label_voxels: %lld masked voxels among %lld", (long long)M, (long long)N);
    const int64_t sx = (int64_t)h.mx[0] - h.mn[0] + 1, sy = (int64_t)h.mx[1] - h.mn[1] + 1, sz = (int64_t)h.mx[2] - h.mn[2] + 1;
    AVL_REQUIRE(sx >= 1 && sy >= 1 && sz >= 1 && sx <= kVxMaxSide && sy <= kVxMaxSide && sz <= kVxMaxSide,
                "avl_label_voxels: the masked voxels' bounding box is %lld x %lld x %lld cells (at most %d a side)", (long long)sx, (long long)sy,
                (long long)sz, kVxMaxSide);
    const int ny = (int)sy, nz = (int)sz;
    const unsigned long long cells = (unsigned long long)sx * (unsigned long long)sy * (unsigned long long)sz;       // at most 2^60
    int bits = 1;
    while (bits < 60 && (1ull << bits) < cells) ++bits;
    const dim3 scan_n((unsigned)w.nblocks), scan_t(kVxScanThreads);
    hipLaunchKernelGGL((count_flagged_kernel<kVxScanThreads, kVxScanPer, VxMasked>), scan_n, scan_t, 0, st, N, VxMasked{d_mask}, w.counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)w.counts, (int64_t)w.nblocks, w.counts,
                       (int*)nullptr, OpSum{}, 0);
    hipLaunchKernelGGL(vx_compact_kernel, scan_n, scan_t, 0, st, d_grid_pos, d_mask, N, (const int*)w.counts, h.mn[0], h.mn[1], h.mn[2], ny, nz, M,
                       w.keys_in, w.idx_in, w.parent);
    AVL_HIP_CHECK(hipGetLastError());
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    AVL_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, w.keys_in, w.keys, w.idx_in, w.idx, (size_t)M, 0, bits, st));
    AVL_HIP_CHECK(hipMallocAsync(&tmp, tmp_bytes ? tmp_bytes : 16, st));
    const hipError_t e = rocprim::radix_sort_pairs(tmp, tmp_bytes, w.keys_in, w.keys, w.idx_in, w.idx, (size_t)M, 0, bits, st);
    (void)hipFreeAsync(tmp, st);
    AVL_HIP_CHECK(e);
    const unsigned sb = stride_blocks(M);
    const int mblocks = (int)((M + kVxScanBlock - 1) / kVxScanBlock);
    int* rank_label = w.idx_in;
    const int axes = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
    hipLaunchKernelGGL(vx_merge_kernel, dim3(sb), dim3(256), 0, st, (const unsigned long long*)w.keys, (int)M, ny, nz, axes, w.parent);
    const dim3 scan_m((unsigned)mblocks);
    const UfIsRoot roots{w.parent};
    hipLaunchKernelGGL((uf_flatten_kernel<256>), dim3(sb), dim3(256), 0, st, w.parent, M);
    hipLaunchKernelGGL((count_flagged_kernel<kVxScanThreads, kVxScanPer, UfIsRoot>), scan_m, scan_t, 0, st, M, roots, w.counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)w.counts, (int64_t)mblocks, w.counts,
                       (int*)d_n, OpSum{}, 0);
    hipLaunchKernelGGL((number_flagged_kernel<kVxScanThreads, kVxScanPer, UfIsRoot>), scan_m, scan_t, 0, st, M, roots, (const int*)w.counts, rank_label);
    hipLaunchKernelGGL(vx_scatter_labels_kernel, dim3(sb), dim3(256), 0, st, (const int*)w.parent, (const int*)rank_label, (const int*)w.idx, (int)M, N,
                       (int*)d_labels);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_voxel_instance_table(const int32_t* d_grid_pos, const int32_t* d_labels, const float* d_scores, int64_t N, int32_t n, int64_t* d_table,
                             float* d_best_score, void* stream) {
    int rc = vx_check_n("avl_voxel_instance_table", N);
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
