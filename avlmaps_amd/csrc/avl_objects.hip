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
// The work is done on the participating voxels in (cell, class, voxel index) order, on their ranks t = 0 .. M - 1:
//   box      bounding box, number M and the smallest and largest class of the participating voxels (one pass, read back: the
//            sorts need M, the key the box).  A side beyond 2^20 cells is refused here: the cell key has at most 60 bits
//   compact  the participating voxels in index order (avl_scan.h): voxel index and class - smallest class
//   sort 1   only with more than one class: rocPRIM's stable radix sort by class, over the bits of largest - smallest class
//   key      key = ((row - rmin) * ny + (col - cmin)) * nz + (height - hmin) as uint64 of every voxel of that order
//   sort 2   the stable radix sort by key.  Stable twice: ranks are in (cell, class, voxel index) order, so the smallest rank of
//            an object lies in its first cell and, among the objects that begin in one cell, ranks order them by class
//   merge    union-find on one int32 parent per rank (avl_unionfind.h).  A cell may hold a RUN of several ranks (in a built map
//            it holds one).  A voxel walks the run of its own cell backwards: an earlier rank of its class is united with it and
//            does the rest.  Otherwise it walks the run of the cell below it and of the cells of the four preceding columns
//            (ONE binary search per column among the ranks before it) and unites with the first rank of its class in each cell
//   flatten, number, scatter   as in avl_instances.hip: roots are first ranks, counted per 1024, scanned, numbered in rank order
// The workspace is 28 bytes per voxel whatever the box and the class ids: the class keys of sort 1 lie where sort 2 puts its sorted
// keys, the classes in rank order where its unsorted keys were, the labels of the roots where the unused index array was.
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

#include <rocprim/device/device_radix_sort.hpp>

#include "avl_common.h"
#include "avl_scan.h"
#include "avl_unionfind.h"

namespace avl {

constexpr int kObMaxSide = 1 << 20;
constexpr int64_t kObMaxVoxels = ((int64_t)1 << 31) - 1;
constexpr int kObScanThreads = 256;
constexpr int kObScanPer = 4;
constexpr int kObScanBlock = kObScanThreads * kObScanPer;
constexpr int kPoolChunk = 256;                 // members per partial sum (ops.POOL_CHUNK)
constexpr int kPoolWaves = 4;                   // chunks (or objects) per workgroup of the pooling kernels
constexpr int kPoolAhead = 8;                   // member rows a lane has in flight before it adds them, in member order

struct ObHeader {
    int mn[3], mx[3];
    int count;                                  // participating voxels
    int cls_min, cls_max;                       // their smallest and largest class
    int pad;
};

// the participating voxels, for avl_scan.h's counting kernel and the compaction
struct ObTakesPart {
    const int32_t* classes;
    __device__ __forceinline__ bool operator()(int64_t i) const { return classes[i] >= 0; }
};

__global__ void ob_header_init_kernel(ObHeader* __restrict__ h) {
    if (threadIdx.x < 3) {
        h->mn[threadIdx.x] = INT_MAX;
        h->mx[threadIdx.x] = INT_MIN;
    }
    if (threadIdx.x == 3) {
        h->count = h->pad = 0;
        h->cls_min = INT_MAX;
        h->cls_max = INT_MIN;
    }
}

// rows of red: minima of row, col, height, class | maxima of the same four | count
__global__ __launch_bounds__(256) void ob_box_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ classes, int64_t N,
                                                     ObHeader* __restrict__ h) {
    __shared__ int red[9][4];
    int mn[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX}, mx[4] = {INT_MIN, INT_MIN, INT_MIN, INT_MIN}, cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int cls = classes[i];
        if (cls < 0) continue;
        ++cnt;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int v = c < 3 ? pos[i * 3 + c] : cls;
            mn[c] = min(mn[c], v);
            mx[c] = max(mx[c], v);
        }
    }
    const int w = threadIdx.x / kWave;
    const bool first = (threadIdx.x & (kWave - 1)) == 0;
    cnt = wave_sum(cnt);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        mn[c] = wave_min(mn[c]);
        mx[c] = wave_max(mx[c]);
        if (first) {
            red[c][w] = mn[c];
            red[4 + c][w] = mx[c];
        }
    }
    if (first) red[8][w] = cnt;
    __syncthreads();
    if (threadIdx.x < 9) {
        const int c = threadIdx.x;
        int v = red[c][0];
        for (int k = 1; k < 4; ++k) v = c < 4 ? min(v, red[c][k]) : (c < 8 ? max(v, red[c][k]) : v + red[c][k]);
        if (c == 8) {
            if (v) atomicAdd(&h->count, v);
        } else if (red[8][0] + red[8][1] + red[8][2] + red[8][3]) {         // a workgroup without a participating voxel offers nothing
            if (c < 3) atomicMin(&h->mn[c], v);
            else if (c == 3) atomicMin(&h->cls_min, v);
            else if (c < 7) atomicMax(&h->mx[c - 4], v);
            else atomicMax(&h->cls_max, v);
        }
    }
}

// the participating voxels in index order: voxel index and, for sort 1, class - cls_min (cls_key = nullptr with one class).  M is
// the count of the box pass: nothing is written at or past it, whatever the classes hold by now
__global__ __launch_bounds__(kObScanThreads) void ob_compact_kernel(const int32_t* __restrict__ classes, int64_t N, const int* __restrict__ offsets,
                                                                    int cls_min, int64_t M, int* __restrict__ idx, uint32_t* __restrict__ cls_key) {
    __shared__ int s_w[kObScanThreads / kWave];
    const int64_t base = offsets[blockIdx.x];
    int64_t i0;
    int before, total;
    const int f = block_flags<kObScanThreads, kObScanPer>(N, ObTakesPart{classes}, s_w, &i0, &before, &total);
    int64_t t = base + before;
#pragma unroll
    for (int k = 0; k < kObScanPer; ++k) {
        if (!(f >> k & 1) || t >= M) continue;
        const int64_t i = i0 + k;
        idx[t] = (int)i;
        if (cls_key) cls_key[t] = (uint32_t)classes[i] - (uint32_t)cls_min;
        ++t;
    }
}

// the cell key of every voxel of idx (M entries, each in [0, N): ob_compact_kernel wrote them, a sort only moved them)
__global__ __launch_bounds__(256) void ob_keys_kernel(const int32_t* __restrict__ pos, const int* __restrict__ idx, int64_t M, int64_t N, int ox,
                                                      int oy, int oz, int ny, int nz, unsigned long long* __restrict__ keys) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < M; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx[t];
        if (i < 0 || i >= N) {                                        // a foreign workspace: no read out of bounds
            keys[t] = 0;
            continue;
        }
        const unsigned long long x = (unsigned)(pos[i * 3] - ox), y = (unsigned)(pos[i * 3 + 1] - oy), z = (unsigned)(pos[i * 3 + 2] - oz);
        keys[t] = (x * (unsigned long long)ny + y) * (unsigned long long)nz + z;
    }
}

// the class of every rank, and the rank as its own parent
__global__ __launch_bounds__(256) void ob_rank_class_kernel(const int32_t* __restrict__ classes, const int* __restrict__ idx, int64_t M, int64_t N,
                                                            int* __restrict__ cls, int* __restrict__ parent) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < M; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx[t];
        cls[t] = i >= 0 && i < N ? classes[i] : -1;
        parent[t] = (int)t;
    }
}

// the first rank in [0, hi) whose key is >= k
__device__ __forceinline__ int ob_lower_bound(const unsigned long long* __restrict__ keys, int hi, unsigned long long k) {
    int lo = 0;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// axes: 1, 2 or 3 = the number of axes on which adjacent cells may differ
__global__ __launch_bounds__(256) void ob_merge_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ cls, int64_t M, int ny,
                                                       int nz, int axes, int* __restrict__ parent) {
    for (int64_t t64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t64 < M; t64 += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)t64;
        if (t == 0) continue;
        const unsigned long long key = keys[t];
        const int c = cls[t];
        int r = t;                                                    // becomes the first rank of the cell's run
        bool found = false;
        while (r > 0 && keys[r - 1] == key) {
            --r;
            if (!found && cls[r] == c) {                              // an earlier voxel of the cell and the class: it does the rest
                uf_unite(parent, t, r);
                found = true;
            }
        }
        if (found) continue;
        const int z = (int)(key % (unsigned long long)nz);
        const unsigned long long col = key / (unsigned long long)nz;
        const int y = (int)(col % (unsigned long long)ny), x = (int)(col / (unsigned long long)ny);
        if (z > 0) {                                                  // the run of the cell below ends just before this cell's
            for (int s = r - 1; s >= 0 && keys[s] == key - 1; --s)
                if (cls[s] == c) {
                    uf_unite(parent, t, s);
                    break;
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dx = k < 3 ? -1 : 0, dy = k < 3 ? k - 1 : -1;   // (-1, -1) (-1, 0) (-1, +1) (0, -1)
            const int dz = min(axes - (dy != 0) - (dx != 0), 1);      // the height may differ by dz (0 or 1); < 0: no such neighbour
            const int a = x + dx, b = y + dy;
            if (dz < 0 || a < 0 || b < 0 || b >= ny) continue;
            const unsigned long long base = ((unsigned long long)a * (unsigned long long)ny + (unsigned long long)b) * (unsigned long long)nz;
            const unsigned long long lo = base + (unsigned long long)max(z - dz, 0), hi = base + (unsigned long long)min(z + dz, nz - 1);
            unsigned long long done = ~0ull;                          // no key: a key has at most 60 bits
            for (int s = ob_lower_bound(keys, r, lo); s < r; ++s) {
                const unsigned long long ks = keys[s];
                if (ks > hi) break;
                if (ks != done && cls[s] == c) {                      // the first voxel of the class in each neighbouring cell
                    uf_unite(parent, t, s);
                    done = ks;
                }
            }
        }
    }
}

// idx[t] < N by construction; the comparison only keeps a foreign workspace from writing out of bounds
__global__ __launch_bounds__(256) void ob_scatter_labels_kernel(const int* __restrict__ parent, const int* __restrict__ rank_label,
                                                                const int* __restrict__ idx, int64_t M, int64_t N, int* __restrict__ labels) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < M; t += (int64_t)gridDim.x * blockDim.x) {
        const int p = parent[t], i = idx[t];
        if (p >= 0 && p < M && i >= 0 && i < N) labels[i] = rank_label[p];
    }
}

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

static int ob_check_n(const char* what, int64_t N) {
    AVL_REQUIRE(N >= 0 && N <= kObMaxVoxels, "%s: N = %lld voxels (0 .. %lld)", what, (long long)N, (long long)kObMaxVoxels);
    return AVL_OK;
}

// workspace of avl_label_classes: header | cell keys, sorted cell keys | two index arrays | parents | one count per scan block.
// The class keys of sort 1 and their sorted copy are the two halves of the sorted cell keys' piece (sort 2 writes it later); after
// sort 2 the unsorted cell keys' piece takes the classes in rank order and the index array it did not write the labels of the roots
struct ObWork {
    int nblocks;
    ObHeader* header;
    unsigned long long *keys_in, *keys;
    int *idx_a, *idx_b, *parent, *counts;
    size_t total;
};
static ObWork ob_work(int64_t N, void* ws) {
    Carver c(ws);
    ObWork w;
    w.nblocks = (int)((N + kObScanBlock - 1) / kObScanBlock);
    w.header = c.ptr<ObHeader>(sizeof(ObHeader));
    w.keys_in = c.ptr<unsigned long long>((size_t)N * sizeof(uint64_t));
    w.keys = c.ptr<unsigned long long>((size_t)N * sizeof(uint64_t));
    w.idx_a = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.idx_b = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.parent = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.counts = c.ptr<int>((size_t)w.nblocks * sizeof(int32_t));
    w.total = c.total();
    return w;
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
    int rc = ob_check_n(what, N);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n >= 0 && n < INT_MAX, "%s: n = %lld objects (0 .. %d)", what, (long long)n, INT_MAX - 1);
    AVL_REQUIRE(C >= 1, "%s: C = %d columns (at least 1)", what, C);
    AVL_REQUIRE(N / kPoolChunk + n <= INT_MAX, "%s: N = %lld rows and n = %lld objects make more than %d chunks", what, (long long)N, (long long)n,
                INT_MAX);
    return AVL_OK;
}

// rocPRIM's stable radix sort of M pairs over the low `bits` bits of the keys, its temporary storage from the stream's pool
template <typename Key>
static int ob_sort_pairs(const char* what, Key* keys_in, Key* keys_out, int* vals_in, int* vals_out, int64_t M, int bits, hipStream_t st) {
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)M, 0, bits, st);
    if (e == hipSuccess) e = hipMallocAsync(&tmp, tmp_bytes ? tmp_bytes : 16, st);
    if (e == hipSuccess) {
        e = rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)M, 0, bits, st);
        (void)hipFreeAsync(tmp, st);
    }
    if (e != hipSuccess) {
        set_error("%s: the radix sort failed: %s", what, hipGetErrorString(e));
        return AVL_ERR_HIP;
    }
    return AVL_OK;
}

// the number of low bits that hold every value of 0 .. count - 1, at least 1
static int ob_bits_for(unsigned long long count, int most) {
    int bits = 1;
    while (bits < most && (1ull << bits) < count) ++bits;
    return bits;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_label_classes_work_bytes(int64_t N, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_label_classes_work_bytes: null output");
    int rc = ob_check_n("avl_label_classes_work_bytes", N);
    if (rc != AVL_OK) return rc;
    *bytes = ob_work(N, nullptr).total;
    return AVL_OK;
}

int avl_label_classes(const int32_t* d_grid_pos, const int32_t* d_classes, int64_t N, int connectivity, int32_t* d_labels, int32_t* d_n,
                      void* ws, size_t ws_bytes, void* stream) {
    int rc = ob_check_n("avl_label_classes", N);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "avl_label_classes: connectivity %d (6, 18 or 26)", connectivity);
    AVL_REQUIRE(d_grid_pos, "avl_label_classes: null d_grid_pos");
    AVL_REQUIRE(d_classes, "avl_label_classes: null d_classes");
    AVL_REQUIRE(d_labels, "avl_label_classes: null d_labels");
    AVL_REQUIRE(d_n, "avl_label_classes: null d_n");
    const ObWork w = ob_work(N, ws);
    AVL_REQUIRE(ws && ws_bytes >= w.total, "avl_label_classes: workspace (ws) of %zu bytes, need %zu", ws_bytes, w.total);
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(d_n, 0, sizeof(int32_t), st));
    if (N == 0) return AVL_OK;
    keep_mempool_once();
    AVL_HIP_CHECK(hipMemsetAsync(d_labels, 0, (size_t)N * sizeof(int32_t), st));
    hipLaunchKernelGGL(ob_header_init_kernel, dim3(1), dim3(64), 0, st, w.header);
    hipLaunchKernelGGL(ob_box_kernel, dim3(std::min(stride_blocks(N), 512u)), dim3(256), 0, st, d_grid_pos, d_classes, N, w.header);
    ObHeader h;
    AVL_HIP_CHECK(hipMemcpyAsync(&h, w.header, sizeof(h), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    const int64_t M = h.count;
    if (M == 0) return AVL_OK;
    AVL_REQUIRE(M > 0 && M <= N, "avl_label_classes: %lld participating voxels among %lld", (long long)M, (long long)N);
    AVL_REQUIRE(h.cls_min >= 0 && h.cls_min <= h.cls_max, "avl_label_classes: classes %d .. %d of the participating voxels", h.cls_min, h.cls_max);
    const int64_t sx = (int64_t)h.mx[0] - h.mn[0] + 1, sy = (int64_t)h.mx[1] - h.mn[1] + 1, sz = (int64_t)h.mx[2] - h.mn[2] + 1;
    AVL_REQUIRE(sx >= 1 && sy >= 1 && sz >= 1 && sx <= kObMaxSide && sy <= kObMaxSide && sz <= kObMaxSide,
                "avl_label_classes: the participating voxels' bounding box is %lld x %lld x %lld cells (at most %d a side)", (long long)sx,
                (long long)sy, (long long)sz, kObMaxSide);
    const int ny = (int)sy, nz = (int)sz;
    const int key_bits = ob_bits_for((unsigned long long)sx * (unsigned long long)sy * (unsigned long long)sz, 60);
    const bool many = h.cls_max > h.cls_min;
    const unsigned sb = stride_blocks(M);
    const dim3 scan_n((unsigned)w.nblocks), scan_t(kObScanThreads);
    const ObTakesPart part{d_classes};
    // sort 2 reads idx_b and writes idx_a; sort 1, when there is one, reads idx_a and writes idx_b
    uint32_t* cls_key = reinterpret_cast<uint32_t*>(w.keys);
    hipLaunchKernelGGL((count_flagged_kernel<kObScanThreads, kObScanPer, ObTakesPart>), scan_n, scan_t, 0, st, N, part, w.counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)w.counts, (int64_t)w.nblocks, w.counts,
                       (int*)nullptr, OpSum{}, 0);
    hipLaunchKernelGGL(ob_compact_kernel, scan_n, scan_t, 0, st, d_classes, N, (const int*)w.counts, h.cls_min, M, many ? w.idx_a : w.idx_b,
                       many ? cls_key : (uint32_t*)nullptr);
    AVL_HIP_CHECK(hipGetLastError());
    if (many) {
        const int cls_bits = ob_bits_for((unsigned long long)((int64_t)h.cls_max - h.cls_min) + 1ull, 32);
        rc = ob_sort_pairs("avl_label_classes", cls_key, cls_key + M, w.idx_a, w.idx_b, M, cls_bits, st);
        if (rc != AVL_OK) return rc;
    }
    hipLaunchKernelGGL(ob_keys_kernel, dim3(sb), dim3(256), 0, st, d_grid_pos, (const int*)w.idx_b, M, N, h.mn[0], h.mn[1], h.mn[2], ny, nz, w.keys_in);
    AVL_HIP_CHECK(hipGetLastError());
    rc = ob_sort_pairs("avl_label_classes", w.keys_in, w.keys, w.idx_b, w.idx_a, M, key_bits, st);
    if (rc != AVL_OK) return rc;
    int* cls = reinterpret_cast<int*>(w.keys_in);
    int* rank_label = w.idx_b;
    const int mblocks = (int)((M + kObScanBlock - 1) / kObScanBlock);
    const int axes = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
    hipLaunchKernelGGL(ob_rank_class_kernel, dim3(sb), dim3(256), 0, st, d_classes, (const int*)w.idx_a, M, N, cls, w.parent);
    hipLaunchKernelGGL(ob_merge_kernel, dim3(sb), dim3(256), 0, st, (const unsigned long long*)w.keys, (const int*)cls, M, ny, nz, axes, w.parent);
    const dim3 scan_m((unsigned)mblocks);
    const UfIsRoot roots{w.parent};
    hipLaunchKernelGGL((uf_flatten_kernel<256>), dim3(sb), dim3(256), 0, st, w.parent, M);
    hipLaunchKernelGGL((count_flagged_kernel<kObScanThreads, kObScanPer, UfIsRoot>), scan_m, scan_t, 0, st, M, roots, w.counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)w.counts, (int64_t)mblocks, w.counts,
                       (int*)d_n, OpSum{}, 0);
    hipLaunchKernelGGL((number_flagged_kernel<kObScanThreads, kObScanPer, UfIsRoot>), scan_m, scan_t, 0, st, M, roots, (const int*)w.counts, rank_label);
    hipLaunchKernelGGL(ob_scatter_labels_kernel, dim3(sb), dim3(256), 0, st, (const int*)w.parent, (const int*)rank_label, (const int*)w.idx_a, M, N,
                       (int*)d_labels);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_pick_columns(const float* d_rows, int64_t N, int C, int64_t ld, const int32_t* d_cols, float* d_out, void* stream) {
    int rc = ob_check_n("avl_pick_columns", N);
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
    rc = ob_sort_pairs("avl_pool_rows", w.keys_in, w.keys, w.idx_in, w.idx, N, ob_bits_for((unsigned long long)n + 1ull, 32), st);
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
