// Object islands of a 2-D mask for gfx950: 8-connected labelling, the island table, the outer contours, and the nearest pair of two
// contours.
//
// Replaces (upstream reference, path:line):
//   avlmaps/utils/navigation_utils.py:10-36   get_segment_islands_pos   cv2.findContours(RETR_EXTERNAL) + the extents of every contour.
//                                             Without OpenCV this project labels with scipy.ndimage.label and traces each island on
//                                             the host (utils/navigation_utils._trace_boundary); both steps run here instead.
//   avlmaps/map/map.py:351-364                find_middle_bewteen_contours   the |A| x |B| float64 distance matrix and its argmin
//
// What is pinned.  Labels, count and table are unique by definition: background 0, islands numbered 1..n in raster order of their
// first pixel, which is scipy.ndimage.label(mask, np.ones((3, 3))).  A contour is DEFINED by _trace_boundary (Moore tracing from the
// first pixel, neighbour order W NW N NE E SE S SW, the scan restarting at (d + 5) % 8, stop at the first return to the start) and
// is reproduced step for step; it is not cv2's corner-compressed polyline.  The nearest pair is the first minimum of the integer
// squared distances in row-major (i, j) order, which is np.argmin of the float64 norms: distinct integers below 2^52 have distinct
// square roots.
//
// Labelling.  Union-find on one int32 parent per pixel (avl_unionfind.h states the invariant; an element is a pixel's linear index):
//   init     a wave owns 64 columns of one row; a pixel starts at the first pixel of its horizontal run inside that segment (one
//            ballot), so a row run is at most one link deep per segment before any merge
//   merge    a pixel unites with the row above (N, else NW and NE; a pixel whose W and NW are set leaves N to its W neighbour) and, on
//            the first lane, with the segment to its left (uf_unite).  When the launch ends every island is one tree whose root is
//            its first pixel
//   flatten  parent = root (uf_flatten_kernel): one pass, however long a serpentine made a chain
//   number   avl_scan.h: the roots are counted per 1024 pixels (count_flagged_kernel), the counts scanned by one workgroup
//            (scan_counts_kernel), and every root receives 1 + the number of roots before it (number_flagged_kernel); the other
//            pixels copy their root's label
// Every result is a minimum, a maximum or a sum of integers: the bytes do not depend on the order in which the atomics land.
//
// Table.  Row k - 1 of label k: area, rmin, rmax, cmin, cmax, first_row, first_col, contour length (written by the count pass of the
// tracer).  Only the first pixel of a horizontal run inside a 64-column segment issues atomics, for the whole run.
//
// Tracing.  One thread per island; the eight neighbour labels of a step are loaded together, so a step is one memory round trip.
// The time is set by the longest contour.  Pass one counts, pass two writes (row, col) pairs at caller-given offsets and never past
// the counted length.
#include <algorithm>
#include <climits>

#include "avl_common.h"
#include "avl_scan.h"
#include "avl_unionfind.h"

namespace avl {

constexpr int kIslMaxSide = 16384;
constexpr int64_t kIslMaxCells = (int64_t)1 << 28;
constexpr int kIslSeg = 64;                     // columns per wave
constexpr int kIslWaves = 4;                    // rows per workgroup of the segment kernels
constexpr int kIslScanThreads = 256;
constexpr int kIslScanPer = 4;                  // pixels per thread of the counting kernels
constexpr int kIslScanBlock = kIslScanThreads * kIslScanPer;
constexpr int kIslTableCols = 8;
constexpr int kNpThreads = 256;
constexpr int kNpTile = 1024;                   // points of B staged in LDS at a time
constexpr int kNpMaxBlocks = 8192;              // workgroups of the pair kernel: beyond that a workgroup takes several tiles of B
constexpr int64_t kNpMaxPoints = (int64_t)1 << 24;

// the first set pixel of lane's run within the wave's ballot m (lane's own bit is set)
__device__ __forceinline__ int isl_run_start(unsigned long long m, int lane) {
    const unsigned long long zeros_below = ~m & ((1ull << lane) - 1ull);
    return zeros_below ? 64 - __clzll((long long)zeros_below) : 0;
}

__global__ __launch_bounds__(kIslSeg* kIslWaves) void isl_init_kernel(const uint8_t* __restrict__ img, int64_t ld, int H, int W,
                                                                      int* __restrict__ parent) {
    const int lane = threadIdx.x & (kIslSeg - 1);
    const int r = blockIdx.y * kIslWaves + threadIdx.x / kIslSeg, c = blockIdx.x * kIslSeg + lane;
    const bool in = r < H && c < W;
    const bool fg = in && img[(int64_t)r * ld + c] != 0;
    const unsigned long long m = __ballot(fg);
    if (!in) return;
    parent[r * W + c] = fg ? r * W + c - lane + isl_run_start(m, lane) : -1;
}

__global__ __launch_bounds__(kIslSeg* kIslWaves) void isl_merge_kernel(const uint8_t* __restrict__ img, int64_t ld, int H, int W,
                                                                       int* __restrict__ parent) {
    const int lane = threadIdx.x & (kIslSeg - 1);
    const int r = blockIdx.y * kIslWaves + threadIdx.x / kIslSeg, c = blockIdx.x * kIslSeg + lane;
    if (r >= H || c >= W) return;
    const uint8_t* row = img + (int64_t)r * ld;
    if (row[c] == 0) return;
    const int i = r * W + c;
    const bool w = c > 0 && row[c - 1] != 0;
    if (lane == 0 && w) uf_unite(parent, i, i - 1);
    if (r == 0) return;
    const uint8_t* up = row - ld;
    const bool n = up[c] != 0, nw = c > 0 && up[c - 1] != 0, ne = c + 1 < W && up[c + 1] != 0;
    if (n) {
        if (!(w && nw)) uf_unite(parent, i, i - W);          // w && nw: the W neighbour joins the same two runs
    } else {
        if (nw) uf_unite(parent, i, i - W - 1);
        if (ne) uf_unite(parent, i, i - W + 1);
    }
}

// every pixel that is not a root: background 0, else its root's label (the roots were numbered by the launch before)
__global__ __launch_bounds__(256) void isl_relabel_kernel(const int* __restrict__ parent, int64_t cells, int* labels) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = parent[i];
        if (p != (int)i) labels[i] = p < 0 ? 0 : labels[p];
    }
}

__global__ __launch_bounds__(256) void isl_table_init_kernel(int* __restrict__ table, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int* t = table + (int64_t)k * kIslTableCols;
    t[0] = 0;
    t[1] = INT_MAX;
    t[2] = -1;
    t[3] = INT_MAX;
    t[4] = -1;
    t[5] = INT_MAX;                                           // the first pixel's linear index until isl_table_finish_kernel
    t[6] = 0;
    t[7] = 0;
}

__device__ __forceinline__ void isl_min(int* p, int v) {
    if (v < uf_load(p)) atomicMin(p, v);
}
__device__ __forceinline__ void isl_max(int* p, int v) {
    if (v > uf_load(p)) atomicMax(p, v);
}

__global__ __launch_bounds__(kIslSeg* kIslWaves) void isl_table_fill_kernel(const int* __restrict__ labels, int H, int W, int n,
                                                                            int* __restrict__ table) {
    const int lane = threadIdx.x & (kIslSeg - 1);
    const int r = blockIdx.y * kIslWaves + threadIdx.x / kIslSeg, c = blockIdx.x * kIslSeg + lane;
    const int lab = r < H && c < W ? labels[r * W + c] : 0;
    const bool fg = lab > 0 && lab <= n;
    const unsigned long long m = __ballot(fg);
    if (!fg || (lane > 0 && (m >> (lane - 1) & 1ull))) return;         // only the first pixel of a run goes on
    const unsigned long long above = ~m >> lane;                        // bit 0 is this pixel: clear
    const int len = above ? __ffsll((long long)above) - 1 : kIslSeg - lane;
    int* t = table + (int64_t)(lab - 1) * kIslTableCols;
    atomicAdd(t + 0, len);
    isl_min(t + 1, r);
    isl_max(t + 2, r);
    isl_min(t + 3, c);
    isl_max(t + 4, c + len - 1);
    isl_min(t + 5, r * W + c);
}

__global__ __launch_bounds__(256) void isl_table_finish_kernel(int* __restrict__ table, int n, int W) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int* t = table + (int64_t)k * kIslTableCols;
    const int first = t[5];
    t[5] = first / W;
    t[6] = first % W;
}

// Moore tracing of island k + 1 from its first pixel, utils/navigation_utils._trace_boundary step for step.  Neighbour d of
// (r, c) is (r + dr[d], c + dc[d]) with d = 0..7 = W NW N NE E SE S SW; dr + 1 and dc + 1 are packed two bits per direction.
constexpr unsigned kIslDr = 1u | 0u << 2 | 0u << 4 | 0u << 6 | 1u << 8 | 2u << 10 | 2u << 12 | 2u << 14;
constexpr unsigned kIslDc = 0u | 0u << 2 | 1u << 4 | 2u << 6 | 2u << 8 | 2u << 10 | 1u << 12 | 0u << 14;

template <bool WRITE>
__global__ __launch_bounds__(64) void isl_trace_kernel(const int* __restrict__ labels, int H, int W, int n, int* __restrict__ table,
                                                       const int64_t* __restrict__ offsets, int* __restrict__ points, int64_t n_points) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int* t = table + (int64_t)k * kIslTableCols;
    const int lab = k + 1, sr = t[5], sc = t[6];
    if (sr < 0 || sr >= H || sc < 0 || sc >= W) return;                // not a table of this image
    const int64_t len = WRITE ? t[7] : 0, base = WRITE ? offsets[k] : 0;
    if (WRITE && (len < 1 || base < 0 || base + len > n_points)) return;
    int64_t cnt = 0;
    if (WRITE) {
        points[2 * base] = sr;
        points[2 * base + 1] = sc;
    }
    ++cnt;
    if (t[0] != 1) {
        const int64_t cap = 4 * (int64_t)H * W + 8;
        int r = sr, c = sc, back = 0;
        for (int64_t it = 0; it < cap; ++it) {
            unsigned hit = 0;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int rr = r + (int)(kIslDr >> (2 * d) & 3u) - 1, cc = c + (int)(kIslDc >> (2 * d) & 3u) - 1;
                const bool in = rr >= 0 && rr < H && cc >= 0 && cc < W;
                const int v = in ? labels[rr * W + cc] : 0;
                hit |= (unsigned)(v == lab) << d;
            }
            if (!hit) break;
            const unsigned rot = (hit >> back | hit << (8 - back)) & 0xFFu;     // bit j = direction (back + j) % 8
            const int d = (back + __ffs((int)rot) - 1) & 7;
            r += (int)(kIslDr >> (2 * d) & 3u) - 1;
            c += (int)(kIslDc >> (2 * d) & 3u) - 1;
            back = (d + 5) & 7;
            if (r == sr && c == sc) break;
            if (WRITE && cnt < len) {
                points[2 * (base + cnt)] = r;
                points[2 * (base + cnt) + 1] = c;
            }
            ++cnt;
        }
    }
    if (!WRITE) t[7] = (int)cnt;
}

// ------------------------------------------------------------------------------------------------ nearest pair of two point lists
struct NpBest {
    long long d2;
    int i, j;
};

__device__ __forceinline__ bool np_less(const NpBest& x, const NpBest& y) {
    return x.d2 != y.d2 ? x.d2 < y.d2 : (x.i != y.i ? x.i < y.i : x.j < y.j);
}

// lexicographic minimum over the workgroup, valid on thread 0
__device__ __forceinline__ NpBest np_block_min(NpBest v, NpBest* s_red) {
    for (int off = 32; off > 0; off >>= 1) {
        NpBest o;
        o.d2 = __shfl_xor(v.d2, off, kWave);
        o.i = __shfl_xor(v.i, off, kWave);
        o.j = __shfl_xor(v.j, off, kWave);
        if (np_less(o, v)) v = o;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < (int)blockDim.x / kWave; ++k)
            if (np_less(s_red[k], v)) v = s_red[k];
    return v;
}

// workgroup (x, y): 256 points of A against the tiles y, y + gridDim.y, ... of B; its best (d2, i, j) to partial[y * gridDim.x + x]
__global__ __launch_bounds__(kNpThreads) void np_partial_kernel(const int2* __restrict__ a, int na, const int2* __restrict__ b, int nb,
                                                                long long* __restrict__ partial) {
    __shared__ int2 s_b[kNpTile];
    __shared__ NpBest s_red[kNpThreads / kWave];
    const int i = blockIdx.x * kNpThreads + threadIdx.x;
    const bool active = i < na;
    const int2 pa = active ? a[i] : make_int2(0, 0);
    NpBest best = {LLONG_MAX, INT_MAX, INT_MAX};
    for (int j0 = blockIdx.y * kNpTile; j0 < nb; j0 += gridDim.y * kNpTile) {
        const int cnt = min(kNpTile, nb - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += kNpThreads) s_b[t] = b[j0 + t];
        __syncthreads();
        if (active) {
            for (int t = 0; t < cnt; ++t) {
                const long long dx = pa.x - s_b[t].x, dy = pa.y - s_b[t].y;
                const long long d2 = dx * dx + dy * dy;
                if (d2 < best.d2) {                           // j ascends: the first minimum of this row stays
                    best.d2 = d2;
                    best.i = i;
                    best.j = j0 + t;
                }
            }
        }
    }
    best = np_block_min(best, s_red);
    if (threadIdx.x == 0) {
        long long* p = partial + 3 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
        p[0] = best.d2;
        p[1] = best.i;
        p[2] = best.j;
    }
}

__global__ __launch_bounds__(kNpThreads) void np_final_kernel(const long long* __restrict__ partial, int count, long long* __restrict__ out) {
    __shared__ NpBest s_red[kNpThreads / kWave];
    NpBest best = {LLONG_MAX, INT_MAX, INT_MAX};
    for (int k = threadIdx.x; k < count; k += kNpThreads) {
        const NpBest v = {partial[3 * (int64_t)k], (int)partial[3 * (int64_t)k + 1], (int)partial[3 * (int64_t)k + 2]};
        if (np_less(v, best)) best = v;
    }
    best = np_block_min(best, s_red);
    if (threadIdx.x == 0) {
        out[0] = best.i;
        out[1] = best.j;
        out[2] = best.d2;
    }
}

static int isl_check_shape(const char* what, int H, int W) {
    AVL_REQUIRE(H > 0 && W > 0 && H <= kIslMaxSide && W <= kIslMaxSide && (int64_t)H * W <= kIslMaxCells,
                "%s: bad shape %d x %d (sides 1 .. %d, at most %lld cells)", what, H, W, kIslMaxSide, (long long)kIslMaxCells);
    return AVL_OK;
}

// workspace of avl_label_islands: the union-find parents, then one root count per scan block
struct IslWork { int nblocks, *parent, *counts; size_t total; };
static IslWork isl_work(int H, int W, void* ws) {
    const int64_t cells = (int64_t)H * W;
    Carver c(ws);
    IslWork w;
    w.nblocks = (int)((cells + kIslScanBlock - 1) / kIslScanBlock);
    w.parent = c.ptr<int>((size_t)cells * sizeof(int32_t));
    w.counts = c.ptr<int>((size_t)w.nblocks * sizeof(int32_t));
    w.total = c.total();
    return w;
}

static dim3 isl_seg_grid(int H, int W) { return dim3((unsigned)((W + kIslSeg - 1) / kIslSeg), (unsigned)((H + kIslWaves - 1) / kIslWaves)); }

static void np_grid(int64_t na, int64_t nb, unsigned* gx, unsigned* gy) {
    *gx = (unsigned)((na + kNpThreads - 1) / kNpThreads);
    *gy = (unsigned)std::min<int64_t>((nb + kNpTile - 1) / kNpTile, std::max<int64_t>(1, kNpMaxBlocks / *gx));
}

static int np_check(const char* what, int64_t na, int64_t nb) {
    AVL_REQUIRE(na >= 1 && nb >= 1 && na <= kNpMaxPoints && nb <= kNpMaxPoints, "%s: %lld and %lld points (1 .. %lld each)", what, (long long)na,
                (long long)nb, (long long)kNpMaxPoints);
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_label_islands_work_bytes(int H, int W, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_label_islands_work_bytes: null output");
    int rc = isl_check_shape("avl_label_islands_work_bytes", H, W);
    if (rc != AVL_OK) return rc;
    *bytes = isl_work(H, W, nullptr).total;
    return AVL_OK;
}

int avl_label_islands(const uint8_t* d_mask_u8, int64_t ld, int H, int W, int32_t* d_labels, int32_t* d_n, void* ws, size_t ws_bytes,
                      void* stream) {
    int rc = isl_check_shape("avl_label_islands", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_mask_u8 && d_labels && d_n, "avl_label_islands: null mask, label or count pointer");
    AVL_REQUIRE(ld >= W, "avl_label_islands: rows of %lld cells cannot hold %d columns", (long long)ld, W);
    const auto [nblocks, parent, counts, need] = isl_work(H, W, ws);
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_label_islands: workspace of %zu bytes, need %zu", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const int64_t cells = (int64_t)H * W;
    const dim3 seg = isl_seg_grid(H, W), segb(kIslSeg * kIslWaves);
    const unsigned sb = stride_blocks(cells);
    const dim3 scan_n((unsigned)nblocks), scan_t(kIslScanThreads);
    const UfIsRoot roots{parent};
    hipLaunchKernelGGL(isl_init_kernel, seg, segb, 0, st, d_mask_u8, ld, H, W, parent);
    hipLaunchKernelGGL(isl_merge_kernel, seg, segb, 0, st, d_mask_u8, ld, H, W, parent);
    hipLaunchKernelGGL((uf_flatten_kernel<256>), dim3(sb), dim3(256), 0, st, parent, cells);
    hipLaunchKernelGGL((count_flagged_kernel<kIslScanThreads, kIslScanPer, UfIsRoot>), scan_n, scan_t, 0, st, cells, roots, counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)counts, (int64_t)nblocks, counts,
                       (int*)d_n, OpSum{}, 0);
    hipLaunchKernelGGL((number_flagged_kernel<kIslScanThreads, kIslScanPer, UfIsRoot>), scan_n, scan_t, 0, st, cells, roots, (const int*)counts,
                       (int*)d_labels);
    hipLaunchKernelGGL(isl_relabel_kernel, dim3(sb), dim3(256), 0, st, (const int*)parent, cells, (int*)d_labels);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_island_table(const int32_t* d_labels, int H, int W, int32_t n, int32_t* d_table, void* stream) {
    int rc = isl_check_shape("avl_island_table", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n >= 0 && (int64_t)n <= (int64_t)((H + 1) / 2) * ((W + 1) / 2), "avl_island_table: %d islands cannot lie in a %d x %d image", n, H, W);
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_labels && d_table, "avl_island_table: null label or table pointer");
    hipStream_t st = as_stream(stream);
    const dim3 rows((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(isl_table_init_kernel, rows, dim3(256), 0, st, (int*)d_table, n);
    hipLaunchKernelGGL(isl_table_fill_kernel, isl_seg_grid(H, W), dim3(kIslSeg * kIslWaves), 0, st, (const int*)d_labels, H, W, n, (int*)d_table);
    hipLaunchKernelGGL(isl_table_finish_kernel, rows, dim3(256), 0, st, (int*)d_table, n, W);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_trace_islands(const int32_t* d_labels, int H, int W, int32_t n, int32_t* d_table, const int64_t* d_offsets, int32_t* d_points,
                      int64_t n_points, void* stream) {
    int rc = isl_check_shape("avl_trace_islands", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(n >= 0 && (int64_t)n <= (int64_t)((H + 1) / 2) * ((W + 1) / 2), "avl_trace_islands: %d islands cannot lie in a %d x %d image", n, H, W);
    AVL_REQUIRE((d_points == nullptr) == (d_offsets == nullptr), "avl_trace_islands: the write pass needs both d_offsets and d_points");
    AVL_REQUIRE(!d_points || n_points >= n, "avl_trace_islands: room for %lld points, %d islands", (long long)n_points, n);
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_labels && d_table, "avl_trace_islands: null label or table pointer");
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)((n + 63) / 64));
    if (d_points)
        hipLaunchKernelGGL(isl_trace_kernel<true>, grid, dim3(64), 0, st, (const int*)d_labels, H, W, n, (int*)d_table, d_offsets, (int*)d_points,
                           n_points);
    else
        hipLaunchKernelGGL(isl_trace_kernel<false>, grid, dim3(64), 0, st, (const int*)d_labels, H, W, n, (int*)d_table, (const int64_t*)nullptr,
                           (int*)nullptr, (int64_t)0);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_nearest_pair_work_bytes(int64_t na, int64_t nb, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_nearest_pair_work_bytes: null output");
    int rc = np_check("avl_nearest_pair_work_bytes", na, nb);
    if (rc != AVL_OK) return rc;
    unsigned gx, gy;
    np_grid(na, nb, &gx, &gy);
    *bytes = align256((size_t)gx * gy * 3 * sizeof(int64_t));
    return AVL_OK;
}

int avl_nearest_pair_i32(const int32_t* d_a, int64_t na, const int32_t* d_b, int64_t nb, int64_t* d_out3, void* ws, size_t ws_bytes,
                         void* stream) {
    size_t need = 0;
    int rc = np_check("avl_nearest_pair_i32", na, nb);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_a && d_b && d_out3, "avl_nearest_pair_i32: null point list or output pointer");
    rc = avl_nearest_pair_work_bytes(na, nb, &need);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_nearest_pair_i32: workspace of %zu bytes, need %zu", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    unsigned gx, gy;
    np_grid(na, nb, &gx, &gy);
    hipLaunchKernelGGL(np_partial_kernel, dim3(gx, gy), dim3(kNpThreads), 0, st, (const int2*)d_a, (int)na, (const int2*)d_b, (int)nb,
                       (long long*)ws);
    hipLaunchKernelGGL(np_final_kernel, dim3(1), dim3(kNpThreads), 0, st, (const long long*)ws, (int)(gx * gy), (long long*)d_out3);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
