// The scene inventory for gfx950: the objects of ALL classes of a sparse voxel list in one labelling, the score of every voxel's own
// class, and the score rows pooled per object in a pinned order.
//
// Upstream has no counterpart.  Its nearest lines stop at ONE category's mask: avlmaps/map/map.py:146-151 and
// avlmaps/map/vlmap_3d.py:75-100.  avl_instances.hip labels one mask; listing a scene with it takes one call, one sort and one
// read-back per category.  The table of the objects is avl_instances.hip's avl_voxel_instance_table, called with these labels.
//
// Labelling by class.  What is pinned: a voxel with a negative class takes part in nothing; two others are adjacent when their
// cells are adjacent as in avl_instances.hip (connectivity 6 / 18 / 26) AND their classes are equal; voxels of one cell with the
// same class belong together, with different classes they do not; objects are numbered 1 .. n in lexicographic order of
// (first cell (row, col, height), class).  That is scipy.ndimage.label run once per class on the class's dense array, all
// components then sorted by (first cell, class).  Every output is an integer minimum or count.
// The labeller is avl_voxel_label.h's under its class policy (VlClasses): the pipeline and the workspace are described there.
//
// Pooled rows.  sums[k - 1] = the sum of the rows whose label is k, in float64, in ONE order of additions (the header states it):
// members in ascending row index, chunks of kPoolChunk consecutive members summed sequentially from 0.0, the partials summed
// sequentially from 0.0.
//   keys     label (0 when outside 1 .. n) and row index of every row
//   sort     the stable radix sort by label over ceil(log2(n + 1)) bits: the members of an object in ascending row index
//   segments first[k] = the first sorted position with a key >= k (one binary search per object), k = 1 .. n + 1; the chunks of an
//            object counted from its members, scanned (avl_scan.h)
//   chunks   ONE WAVE per chunk, lanes = columns, C in sixty-fours: a member row is one contiguous read of 4 C bytes; the row
//            indices of 64 members are read at once and handed round the wave.  A lane adds its column's values one after the
//            other: no shuffle, no atomic, nothing whose order could vary
//   objects  ONE WAVE per object adds its partials in chunk order
#include <algorithm>
#include <climits>

#include "avl_common.h"
#include "avl_scan.h"
#include "avl_sort.h"
#include "avl_voxel_label.h"

namespace avl {

constexpr int kPoolChunk = 256;                 // members per partial sum (ops.POOL_CHUNK)
constexpr int kPoolWaves = 4;                   // chunks (or objects) per workgroup of the pooling kernels
constexpr int kPoolAhead = 8;                   // member rows a lane has in flight before it adds them, in member order

// ---------------------------------------------------------------------------------------------------------------- the column pick
__global__ __launch_bounds__(256) void ob_pick_columns_kernel(const float* __restrict__ rows, int64_t N, int C, int64_t ld,
                                                              const int32_t* __restrict__ cols, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = cols[i];
        out[i] = c >= 0 && c < C ? rows[i * ld + c] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the pooled rows
__global__ __launch_bounds__(256) void pool_keys_kernel(const int32_t* __restrict__ labels, int64_t N, int n, uint32_t* __restrict__ keys,
                                                        int* __restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int lab = labels[i];
        keys[i] = lab >= 1 && lab <= n ? (uint32_t)lab : 0u;
        idx[i] = (int)i;
    }
}

// first[k] = the first sorted position whose key is >= k + 1, k = 0 .. n: object k + 1's members are [first[k], first[k + 1]).
// chunks[k] = its number of chunks for k < n, 0 for k = n (the scan then leaves the total there)
__global__ __launch_bounds__(256) void pool_segments_kernel(const uint32_t* __restrict__ keys, int64_t N, int n, int* __restrict__ first,
                                                            int* __restrict__ chunks) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n) return;
    const uint32_t want[2] = {(uint32_t)k + 1u, (uint32_t)k + 2u};
    int at[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        int64_t lo = 0, hi = N;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < want[e]) lo = mid + 1;
            else hi = mid;
        }
        at[e] = (int)lo;
    }
    first[k] = at[0];
    chunks[k] = k < n ? (at[1] - at[0] + kPoolChunk - 1) / kPoolChunk : 0;
}

// One wave per chunk q < chunk_at[n].  Its object k is the one with chunk_at[k] <= q < chunk_at[k + 1] (objects without a member
// have an empty range and are passed over).  partial (chunks, C)
__global__ __launch_bounds__(kPoolWaves* kWave) void pool_chunks_kernel(const float* __restrict__ rows, int64_t N, int C, int64_t ld,
                                                                        const int* __restrict__ idx, const int* __restrict__ first,
                                                                        const int* __restrict__ chunk_at, int n, double* __restrict__ partial) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t q = (int64_t)blockIdx.x * kPoolWaves + threadIdx.x / kWave;
    if (q >= chunk_at[n]) return;
    int lo = 0, hi = n;                                               // the first k in [0, n] with chunk_at[k] > q, less one
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (chunk_at[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    const int k = lo - 1;
    const int64_t beg = (int64_t)first[k] + (q - chunk_at[k]) * kPoolChunk;
    const int len = (int)min((int64_t)kPoolChunk, (int64_t)first[k + 1] - beg);
    for (int c0 = 0; c0 < C; c0 += kWave) {
        const int c = c0 + lane;
        const bool on = c < C;
        double acc = 0.0;
        for (int j0 = 0; j0 < len; j0 += kWave) {
            int mine = j0 + lane < len ? idx[beg + j0 + lane] : 0;
            if (mine < 0 || mine >= N) mine = 0;                      // a foreign workspace: no read out of bounds
            const int cnt = min(kWave, len - j0);
            for (int j = 0; j < cnt; j += kPoolAhead) {               // kPoolAhead loads in flight, then their additions in member order
                float v[kPoolAhead];
#pragma unroll
                for (int u = 0; u < kPoolAhead; ++u) {
                    const int64_t i = __shfl(mine, min(j + u, cnt - 1), kWave);
                    v[u] = on ? rows[i * ld + c] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < kPoolAhead; ++u)
                    if (j + u < cnt) acc += (double)v[u];
            }
        }
        if (on) partial[q * C + c] = acc;
    }
}

// one wave per object: its partials in chunk order
__global__ __launch_bounds__(kPoolWaves* kWave) void pool_objects_kernel(const double* __restrict__ partial, const int* __restrict__ chunk_at, int n,
                                                                         int C, double* __restrict__ sums) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t k = (int64_t)blockIdx.x * kPoolWaves + threadIdx.x / kWave;
    if (k >= n) return;
    const int64_t p0 = chunk_at[k], p1 = chunk_at[k + 1];
    for (int c = lane; c < C; c += kWave) {
        double acc = 0.0;
        for (int64_t p = p0; p < p1; ++p) acc += partial[p * C + c];
        sums[k * C + c] = acc;
    }
}

// workspace of avl_pool_rows: labels as keys, sorted | row indices, sorted | first member and first chunk of every object and one
// past the last | a float64 row per chunk.  An object of m members has ceil(m / 256) <= m / 256 + 1 chunks: at most N / 256 + n in all
struct PoolWork {
    int64_t max_chunks;
    uint32_t *keys_in, *keys;
    int *idx_in, *idx, *first, *chunk_at;
    double* partial;
    size_t total;
};
static PoolWork pool_work(int64_t N, int C, int64_t n, void* ws) {
    Carver c(ws);
    PoolWork w;
    w.max_chunks = N / kPoolChunk + n;
    w.keys_in = c.ptr<uint32_t>((size_t)N * sizeof(uint32_t));
    w.keys = c.ptr<uint32_t>((size_t)N * sizeof(uint32_t));
    w.idx_in = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.idx = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.first = c.ptr<int>((size_t)(n + 1) * sizeof(int32_t));
    w.chunk_at = c.ptr<int>((size_t)(n + 1) * sizeof(int32_t));
    w.partial = c.ptr<double>((size_t)w.max_chunks * (size_t)C * sizeof(double));
    w.total = c.total();
    return w;
}

static int pool_check(const char* what, int64_t N, int C, int64_t n) {
    int rc = vl_check_n(what, N);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n >= 0 && n < INT_MAX, "%s: n = %lld objects (0 .. %d)", what, (long long)n, INT_MAX - 1);
    AVL_REQUIRE(C >= 1, "%s: C = %d columns (at least 1)", what, C);
    AVL_REQUIRE(N / kPoolChunk + n <= INT_MAX, "%s: N = %lld rows and n = %lld objects make more than %d chunks", what, (long long)N, (long long)n,
                INT_MAX);
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_label_classes_work_bytes(int64_t N, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_label_classes_work_bytes: null output");
    int rc = vl_check_n("avl_label_classes_work_bytes", N);
    if (rc != AVL_OK) return rc;
    *bytes = vl_work(N, nullptr).total;
    return AVL_OK;
}

int avl_label_classes(const int32_t* d_grid_pos, const int32_t* d_classes, int64_t N, int connectivity, int32_t* d_labels, int32_t* d_n,
                      void* ws, size_t ws_bytes, void* stream) {
    int rc = vl_check_n("avl_label_classes", N);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "avl_label_classes: connectivity %d (6, 18 or 26)", connectivity);
    AVL_REQUIRE(d_grid_pos, "avl_label_classes: null d_grid_pos");
    AVL_REQUIRE(d_classes, "avl_label_classes: null d_classes");
    AVL_REQUIRE(d_labels, "avl_label_classes: null d_labels");
    AVL_REQUIRE(d_n, "avl_label_classes: null d_n");
    return label_sparse_voxels("avl_label_classes", "participating", VlClasses{d_classes}, d_grid_pos, N, connectivity, d_labels, d_n, ws, ws_bytes, stream);
}

int avl_pick_columns(const float* d_rows, int64_t N, int C, int64_t ld, const int32_t* d_cols, float* d_out, void* stream) {
    int rc = vl_check_n("avl_pick_columns", N);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(C >= 1, "avl_pick_columns: C = %d columns (at least 1)", C);
    AVL_REQUIRE(ld >= C, "avl_pick_columns: ld = %lld elements for C = %d columns", (long long)ld, C);
    if (N == 0) return AVL_OK;
    AVL_REQUIRE(d_rows, "avl_pick_columns: null d_rows");
    AVL_REQUIRE(d_cols, "avl_pick_columns: null d_cols");
    AVL_REQUIRE(d_out, "avl_pick_columns: null d_out");
    hipLaunchKernelGGL(ob_pick_columns_kernel, dim3(stride_blocks(N)), dim3(256), 0, as_stream(stream), d_rows, N, C, ld, d_cols, d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_pool_rows_work_bytes(int64_t N, int C, int32_t n, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_pool_rows_work_bytes: null output");
    int rc = pool_check("avl_pool_rows_work_bytes", N, C, n);
    if (rc != AVL_OK) return rc;
    *bytes = pool_work(N, C, n, nullptr).total;
    return AVL_OK;
}

int avl_pool_rows(const float* d_rows, int64_t N, int C, int64_t ld, const int32_t* d_labels, int32_t n, double* d_sums, void* ws,
                  size_t ws_bytes, void* stream) {
    int rc = pool_check("avl_pool_rows", N, C, n);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(ld >= C, "avl_pool_rows: ld = %lld elements for C = %d columns", (long long)ld, C);
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_sums, "avl_pool_rows: null d_sums");
    AVL_REQUIRE(N == 0 || d_rows, "avl_pool_rows: null d_rows");
    AVL_REQUIRE(N == 0 || d_labels, "avl_pool_rows: null d_labels");
    const PoolWork w = pool_work(N, C, n, ws);
    AVL_REQUIRE(ws && ws_bytes >= w.total, "avl_pool_rows: workspace (ws) of %zu bytes, need %zu", ws_bytes, w.total);
    hipStream_t st = as_stream(stream);
    if (N == 0) {
        AVL_HIP_CHECK(hipMemsetAsync(d_sums, 0, (size_t)n * (size_t)C * sizeof(double), st));
        return AVL_OK;
    }
    keep_mempool_once();
    hipLaunchKernelGGL(pool_keys_kernel, dim3(stride_blocks(N)), dim3(256), 0, st, d_labels, N, (int)n, w.keys_in, w.idx_in);
    AVL_HIP_CHECK(hipGetLastError());
    rc = sort_pairs_pooled("avl_pool_rows", w.keys_in, w.keys, w.idx_in, w.idx, N, bits_for((unsigned long long)n + 1ull, 32), st);
    if (rc != AVL_OK) return rc;
    const int64_t entries = (int64_t)n + 1;
    hipLaunchKernelGGL(pool_segments_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, (const uint32_t*)w.keys, N, (int)n, w.first,
                       w.chunk_at);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)w.chunk_at, entries, w.chunk_at,
                       (int*)nullptr, OpSum{}, 0);
    hipLaunchKernelGGL(pool_chunks_kernel, dim3((unsigned)((w.max_chunks + kPoolWaves - 1) / kPoolWaves)), dim3(kPoolWaves * kWave), 0, st, d_rows, N, C,
                       ld, (const int*)w.idx, (const int*)w.first, (const int*)w.chunk_at, (int)n, w.partial);
    hipLaunchKernelGGL(pool_objects_kernel, dim3((unsigned)(((int64_t)n + kPoolWaves - 1) / kPoolWaves)), dim3(kPoolWaves * kWave), 0, st,
                       (const double*)w.partial, (const int*)w.chunk_at, (int)n, C, d_sums);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
