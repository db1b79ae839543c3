// The connected-component labeller of a SPARSE voxel list, shared by avl_label_voxels (avl_instances.hip: one mask) and
// avl_label_classes (avl_objects.hip: all classes at once).  Labelling a mask is labelling one class: avl_label_voxels(pos, mask)
// gives the bytes of avl_label_classes(pos, mask ? c : -1) for any constant c >= 0 (tests/test_objects_gpu.py).
// A participation policy (VlMask, VlClasses below) says which voxels take part and with which class.  Templates and static
// helpers: each source that launches a kernel instantiates it for itself, as with avl_scan.h.
//
// The work is done on the M participating voxels in (cell, class, voxel index) order, on their ranks t = 0 .. M - 1:
//   box      bounding box and number M of the participating voxels, VlClasses: also their smallest and largest class (one pass,
//            read back: the sorts need M, the key the box).  A side beyond 2^20 cells is refused here: three sides of 20 bits make
//            a key of at most 60 bits
//   compact  the participating voxels in index order (avl_scan.h: count_flagged_kernel per 1024 voxels, scan_counts_kernel, then
//            one write).  VlMask writes key, voxel index and the rank's own parent in this pass; VlClasses writes the voxel index
//            and, with more than one class, class - smallest class
//   sort 1   VlClasses with more than one class only: rocPRIM's stable radix sort by class, over the bits of largest - smallest class
//   key      key = ((row - rmin) * ny + (col - cmin)) * nz + (height - hmin) as uint64.  VlClasses computes it in a pass of its own,
//            for every voxel of sort 1's order
//   sort 2   the stable radix sort by key, value = the voxel index.  Equal cells keep their order, so ranks are in (cell, class,
//            voxel index) order: the smallest rank of an object lies in its first cell and is its smallest voxel index there, and
//            among the objects that begin in one cell ranks order them by class
//   class    VlClasses only: the class of every rank, and the rank as its own parent
//   merge    union-find on one int32 parent per rank (uf_unite; avl_unionfind.h states the invariant, an element being a rank).
//            A voxel looks at the 13 cells that precede it in raster order.  A cell may hold a RUN of several ranks (in a built
//            map it holds one).  An earlier rank of the voxel's own cell and class is united with it and does the rest.  Otherwise
//            it unites with the first rank of its class in the cell below it, whose run ends just before its own cell's, and in
//            the three cells of each of the four preceding columns (row - 1, col - 1 .. col + 1) and (row, col - 1): these are
//            consecutive ranks, found by ONE binary search per column among the ranks before its cell.  VlMask: every rank of a
//            cell is of the voxel's class, so the own cell and the cell below are the previous rank and no run is walked
//   flatten  parent = root (uf_flatten_kernel)
//   number   the roots counted per 1024 ranks, scanned, every root receives 1 + the number of roots before it (count_flagged_kernel,
//            scan_counts_kernel, number_flagged_kernel).  Roots are smallest ranks: numbering them in rank order is the
//            lexicographic order of (first cell (row, col, height), class)
//   scatter  labels[voxel of rank t] = label of t's root; the other voxels keep the 0 of the memset
// The workspace is 28 bytes per voxel of the list whatever the box and the class ids (no grid over the box is kept, not even one
// of bits); vl_work states how the pieces are reused.
#pragma once
#include <algorithm>
#include <climits>

#include "avl_common.h"
#include "avl_scan.h"
#include "avl_sort.h"
#include "avl_unionfind.h"

namespace avl {

constexpr int kVlMaxSide = 1 << 20;
constexpr int64_t kVlMaxVoxels = ((int64_t)1 << 31) - 1;
constexpr int kVlScanThreads = 256;
constexpr int kVlScanPer = 4;
constexpr int kVlScanBlock = kVlScanThreads * kVlScanPer;

struct VlHeader {
    int mn[3], mx[3];
    int count;                                  // participating voxels
    int cls_min, cls_max;                       // their smallest and largest class (VlMask never reads them)
    int pad;
};

// The policies: cls(i) = the class of voxel i, negative when it takes part in nothing; as a predicate (avl_scan.h's counting
// kernel, the compaction) "voxel i takes part".  VlMask: the voxels whose mask byte is set, all of class 0, which is known at
// compile time: no class array, no class sort, and the voxels of a cell all belong together.  VlClasses: the voxels whose class
// is >= 0; two of them belong together only when their classes are equal
struct VlMask {
    static constexpr bool kClasses = false;
    const uint8_t* mask;
    __device__ __forceinline__ int cls(int64_t i) const { return mask[i] ? 0 : -1; }
    __device__ __forceinline__ bool operator()(int64_t i) const { return mask[i] != 0; }
};
struct VlClasses {
    static constexpr bool kClasses = true;
    const int32_t* classes;
    __device__ __forceinline__ int cls(int64_t i) const { return classes[i]; }
    __device__ __forceinline__ bool operator()(int64_t i) const { return classes[i] >= 0; }
};

// the box of the participating voxels as the cell key sees it
struct VlGrid {
    int ox, oy, oz, ny, nz;
    __device__ __forceinline__ unsigned long long key(const int32_t* __restrict__ pos, int64_t i) const {
        const unsigned long long x = (unsigned)(pos[i * 3] - ox), y = (unsigned)(pos[i * 3 + 1] - oy), z = (unsigned)(pos[i * 3 + 2] - oz);
        return (x * (unsigned long long)ny + y) * (unsigned long long)nz + z;
    }
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void vl_header_init_kernel(VlHeader* __restrict__ h) {
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

// rows of red: minima of row, col, height (and class) | maxima of the same | count
template <typename P>
__global__ __launch_bounds__(256) void vl_box_kernel(const int32_t* __restrict__ pos, P part, int64_t N, VlHeader* __restrict__ h) {
    constexpr int D = P::kClasses ? 4 : 3;
    __shared__ int red[2 * D + 1][4];
    int mn[D], mx[D], cnt = 0;
#pragma unroll
    for (int c = 0; c < D; ++c) mn[c] = INT_MAX, mx[c] = INT_MIN;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int cls = part.cls(i);
        if (cls < 0) continue;
        ++cnt;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int v = c < 3 ? pos[i * 3 + c] : cls;
            mn[c] = min(mn[c], v);
            mx[c] = max(mx[c], v);
        }
    }
    const int w = threadIdx.x / kWave;
    const bool first = (threadIdx.x & (kWave - 1)) == 0;
    cnt = wave_sum(cnt);
#pragma unroll
    for (int c = 0; c < D; ++c) {
        mn[c] = wave_min(mn[c]);
        mx[c] = wave_max(mx[c]);
        if (first) {
            red[c][w] = mn[c];
            red[D + c][w] = mx[c];
        }
    }
    if (first) red[2 * D][w] = cnt;
    __syncthreads();
    if (threadIdx.x < 2 * D + 1) {
        const int c = threadIdx.x;
        int v = red[c][0];
        for (int k = 1; k < 4; ++k) v = c < D ? min(v, red[c][k]) : (c < 2 * D ? max(v, red[c][k]) : v + red[c][k]);
        if (c == 2 * D) {
            if (v) atomicAdd(&h->count, v);
        } else if (red[2 * D][0] + red[2 * D][1] + red[2 * D][2] + red[2 * D][3]) {     // a workgroup without a participating voxel offers nothing
            if (c < 3) atomicMin(&h->mn[c], v);
            else if (c < D) atomicMin(&h->cls_min, v);
            else if (c < D + 3) atomicMax(&h->mx[c - D], v);
            else atomicMax(&h->cls_max, v);
        }
    }
}

// The participating voxels in index order.  VlMask: key, voxel index and the rank's own parent.  VlClasses: voxel index and, for
// sort 1, class - cls_min (cls_key = nullptr with one class).  M is the count of the box pass: nothing is written at or past it,
// whatever the mask or the classes hold by now
template <typename P>
__global__ __launch_bounds__(kVlScanThreads) void vl_compact_kernel(const int32_t* __restrict__ pos, P part, int64_t N, const int* __restrict__ offsets,
                                                                    VlGrid g, int cls_min, int64_t M, unsigned long long* __restrict__ keys,
                                                                    int* __restrict__ idx, int* __restrict__ parent, uint32_t* __restrict__ cls_key) {
    __shared__ int s_w[kVlScanThreads / kWave];
    const int64_t base = offsets[blockIdx.x];
    int64_t i0;
    int before, total;
    const int f = block_flags<kVlScanThreads, kVlScanPer>(N, part, s_w, &i0, &before, &total);
    int64_t t = base + before;
#pragma unroll
    for (int k = 0; k < kVlScanPer; ++k) {
        if (!(f >> k & 1) || t >= M) continue;
        const int64_t i = i0 + k;
        idx[t] = (int)i;
        if constexpr (P::kClasses) {
            if (cls_key) cls_key[t] = (uint32_t)part.cls(i) - (uint32_t)cls_min;
        } else {
            keys[t] = g.key(pos, i);
            parent[t] = (int)t;
        }
        ++t;
    }
}

// VlClasses: the cell key of every voxel of idx (M entries, each in [0, N): vl_compact_kernel wrote them, a sort only moved them)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void vl_keys_kernel(const int32_t* __restrict__ pos, const int* __restrict__ idx, int64_t M, int64_t N, VlGrid g,
                                                          unsigned long long* __restrict__ keys) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < M; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx[t];
        keys[t] = i >= 0 && i < N ? g.key(pos, i) : 0;                // a foreign workspace: no read out of bounds
    }
}

// VlClasses: the class of every rank, and the rank as its own parent
template <int THREADS>
__global__ __launch_bounds__(THREADS) void vl_rank_class_kernel(VlClasses part, const int* __restrict__ idx, int64_t M, int64_t N,
                                                                int* __restrict__ cls, int* __restrict__ parent) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < M; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx[t];
        cls[t] = i >= 0 && i < N ? part.cls(i) : -1;
        parent[t] = (int)t;
    }
}

// the first rank in [0, hi) whose key is >= k
__device__ __forceinline__ int vl_lower_bound(const unsigned long long* __restrict__ keys, int hi, unsigned long long k) {
    int lo = 0;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// axes: 1, 2 or 3 = the number of axes on which adjacent cells may differ.  cls: the class of every rank (VlMask: not read)
template <typename P>
__global__ __launch_bounds__(256) void vl_merge_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ cls, int64_t M, int ny,
                                                       int nz, int axes, int* __restrict__ parent) {
    for (int64_t t64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t64 < M; t64 += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)t64;
        if (t == 0) continue;
        const unsigned long long key = keys[t];
        int c = 0, r = t;                                             // r becomes the first rank of the cell's run
        const auto same = [&](int s) {                                // rank s is of t's class
            if constexpr (P::kClasses) return cls[s] == c;
            else return true;
        };
        const unsigned long long prev = keys[t - 1];                  // VlMask reads nothing else of its own cell and the cell below
        bool found = false;                                           // an earlier voxel of the cell and the class: it does the rest
        if constexpr (P::kClasses) {
            c = cls[t];
            while (r > 0 && keys[r - 1] == key) {
                --r;
                if (!found && same(r)) {
                    uf_unite(parent, t, r);
                    found = true;
                }
            }
        } else if (prev == key) {                                     // every voxel of the cell is of the class: the previous rank
            uf_unite(parent, t, t - 1);
            found = true;
        }
        if (found) continue;
        const int z = (int)(key % (unsigned long long)nz);
        const unsigned long long col = key / (unsigned long long)nz;
        const int y = (int)(col % (unsigned long long)ny), x = (int)(col / (unsigned long long)ny);
        if constexpr (P::kClasses) {                                  // the run of the cell below ends just before this cell's
            for (int s = r - 1; z > 0 && s >= 0 && keys[s] == key - 1; --s)
                if (same(s)) {
                    uf_unite(parent, t, s);
                    break;
                }
        } else if (z > 0 && prev == key - 1) {
            uf_unite(parent, t, t - 1);
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
            for (int s = vl_lower_bound(keys, r, lo); s < r; ++s) {
                const unsigned long long ks = keys[s];
                if (ks > hi) break;
                if (ks != done && same(s)) {                          // the first voxel of the class in each neighbouring cell
                    uf_unite(parent, t, s);
                    done = ks;
                }
            }
        }
    }
}

// idx[t] < N by construction (vl_compact_kernel wrote it); the comparison only keeps a foreign workspace from writing out of bounds
template <int THREADS>
__global__ __launch_bounds__(THREADS) void vl_scatter_labels_kernel(const int* __restrict__ parent, const int* __restrict__ rank_label,
                                                                    const int* __restrict__ idx, int64_t M, int64_t N, int* __restrict__ labels) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < M; t += (int64_t)gridDim.x * blockDim.x) {
        const int p = parent[t], i = idx[t];
        if (p >= 0 && p < M && i >= 0 && i < N) labels[i] = rank_label[p];
    }
}

static int vl_check_n(const char* who, int64_t N) {
    AVL_REQUIRE(N >= 0 && N <= kVlMaxVoxels, "%s: N = %lld voxels (0 .. %lld)", who, (long long)N, (long long)kVlMaxVoxels);
    return AVL_OK;
}

// The workspace: header | cell keys, sorted cell keys | voxel indices, the same sorted by cell | parents | one count per scan
// block.  Pieces that are dead take what comes later:
//   the class keys of sort 1 and their sorted copy are the two halves of the sorted cell keys' piece (sort 2 writes it later),
//   and sort 1 moves the indices from the sorted piece to the unsorted one, where sort 2 reads them;
//   after sort 2 the unsorted cell keys' piece takes the classes in rank order,
//   and the unsorted indices' piece the labels of the roots
struct VlWork {
    int nblocks;
    VlHeader* header;
    unsigned long long *keys_in, *keys;
    int *idx_in, *idx, *parent, *counts;
    size_t total;
};
static VlWork vl_work(int64_t N, void* ws) {
    Carver c(ws);
    VlWork w;
    w.nblocks = (int)((N + kVlScanBlock - 1) / kVlScanBlock);
    w.header = c.ptr<VlHeader>(sizeof(VlHeader));
    w.keys_in = c.ptr<unsigned long long>((size_t)N * sizeof(uint64_t));
    w.keys = c.ptr<unsigned long long>((size_t)N * sizeof(uint64_t));
    w.idx_in = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.idx = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.parent = c.ptr<int>((size_t)N * sizeof(int32_t));
    w.counts = c.ptr<int>((size_t)w.nblocks * sizeof(int32_t));
    w.total = c.total();
    return w;
}

// The host sequence of both entry points, after their own argument checks.  who = the entry point, noun = what it calls the
// voxels that take part ("masked", "participating"): both only word the messages
template <typename P>
static int label_sparse_voxels(const char* who, const char* noun, P part, const int32_t* d_grid_pos, int64_t N, int connectivity, int32_t* d_labels,
                               int32_t* d_n, void* ws, size_t ws_bytes, void* stream) {
    const VlWork w = vl_work(N, ws);
    AVL_REQUIRE(ws && ws_bytes >= w.total, "%s: workspace (ws) of %zu bytes, need %zu", who, ws_bytes, w.total);
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(d_n, 0, sizeof(int32_t), st));
    if (N == 0) return AVL_OK;
    keep_mempool_once();
    AVL_HIP_CHECK(hipMemsetAsync(d_labels, 0, (size_t)N * sizeof(int32_t), st));
    hipLaunchKernelGGL((vl_header_init_kernel<64>), dim3(1), dim3(64), 0, st, w.header);
    hipLaunchKernelGGL((vl_box_kernel<P>), dim3(std::min(stride_blocks(N), 512u)), dim3(256), 0, st, d_grid_pos, part, N, w.header);
    VlHeader h;
    AVL_HIP_CHECK(hipMemcpyAsync(&h, w.header, sizeof(h), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    const int64_t M = h.count;
    if (M == 0) return AVL_OK;
    AVL_REQUIRE(M > 0 && M <= N, "%s: %lld %s voxels among %lld", who, (long long)M, noun, (long long)N);
    if constexpr (P::kClasses)
        AVL_REQUIRE(h.cls_min >= 0 && h.cls_min <= h.cls_max, "%s: classes %d .. %d of the %s voxels", who, h.cls_min, h.cls_max, noun);
    const int64_t sx = (int64_t)h.mx[0] - h.mn[0] + 1, sy = (int64_t)h.mx[1] - h.mn[1] + 1, sz = (int64_t)h.mx[2] - h.mn[2] + 1;
    AVL_REQUIRE(sx >= 1 && sy >= 1 && sz >= 1 && sx <= kVlMaxSide && sy <= kVlMaxSide && sz <= kVlMaxSide,
                "%s: the %s voxels' bounding box is %lld x %lld x %lld cells (at most %d a side)", who, noun, (long long)sx, (long long)sy,
                (long long)sz, kVlMaxSide);
    const VlGrid g{h.mn[0], h.mn[1], h.mn[2], (int)sy, (int)sz};
    const int key_bits = bits_for((unsigned long long)sx * (unsigned long long)sy * (unsigned long long)sz, 60);      // at most 2^60 cells
    const bool many = P::kClasses && h.cls_max > h.cls_min;
    const unsigned sb = stride_blocks(M);
    const dim3 scan_n((unsigned)w.nblocks), scan_t(kVlScanThreads);
    uint32_t* cls_key = reinterpret_cast<uint32_t*>(w.keys);
    hipLaunchKernelGGL((count_flagged_kernel<kVlScanThreads, kVlScanPer, P>), scan_n, scan_t, 0, st, N, part, w.counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)w.counts, (int64_t)w.nblocks, w.counts,
                       (int*)nullptr, OpSum{}, 0);
    // sort 2 reads idx_in and writes idx; sort 1, when there is one, reads idx and writes idx_in
    hipLaunchKernelGGL((vl_compact_kernel<P>), scan_n, scan_t, 0, st, d_grid_pos, part, N, (const int*)w.counts, g, h.cls_min, M, w.keys_in,
                       many ? w.idx : w.idx_in, w.parent, many ? cls_key : (uint32_t*)nullptr);
    AVL_HIP_CHECK(hipGetLastError());
    int rc;
    if constexpr (P::kClasses) {
        if (many) {
            rc = sort_pairs_pooled(who, cls_key, cls_key + M, w.idx, w.idx_in, M, bits_for((unsigned long long)((int64_t)h.cls_max - h.cls_min) + 1ull, 32), st);
            if (rc != AVL_OK) return rc;
        }
        hipLaunchKernelGGL((vl_keys_kernel<256>), dim3(sb), dim3(256), 0, st, d_grid_pos, (const int*)w.idx_in, M, N, g, w.keys_in);
        AVL_HIP_CHECK(hipGetLastError());
    }
    rc = sort_pairs_pooled(who, w.keys_in, w.keys, w.idx_in, w.idx, M, key_bits, st);
    if (rc != AVL_OK) return rc;
    int* cls = reinterpret_cast<int*>(w.keys_in);
    int* rank_label = w.idx_in;
    const int mblocks = (int)((M + kVlScanBlock - 1) / kVlScanBlock);
    const int axes = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
    if constexpr (P::kClasses) hipLaunchKernelGGL((vl_rank_class_kernel<256>), dim3(sb), dim3(256), 0, st, part, (const int*)w.idx, M, N, cls, w.parent);
    hipLaunchKernelGGL((vl_merge_kernel<P>), dim3(sb), dim3(256), 0, st, (const unsigned long long*)w.keys, (const int*)cls, M, g.ny, g.nz, axes, w.parent);
    const dim3 scan_m((unsigned)mblocks);
    const UfIsRoot roots{w.parent};
    hipLaunchKernelGGL((uf_flatten_kernel<256>), dim3(sb), dim3(256), 0, st, w.parent, M);
    hipLaunchKernelGGL((count_flagged_kernel<kVlScanThreads, kVlScanPer, UfIsRoot>), scan_m, scan_t, 0, st, M, roots, w.counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)w.counts, (int64_t)mblocks, w.counts,
                       (int*)d_n, OpSum{}, 0);
    hipLaunchKernelGGL((number_flagged_kernel<kVlScanThreads, kVlScanPer, UfIsRoot>), scan_m, scan_t, 0, st, M, roots, (const int*)w.counts, rank_label);
    hipLaunchKernelGGL((vl_scatter_labels_kernel<256>), dim3(sb), dim3(256), 0, st, (const int*)w.parent, (const int*)rank_label, (const int*)w.idx, M, N,
                       (int*)d_labels);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // namespace avl
