// 2-D viewsheds on the explored map for gfx950: how many unknown cells become visible from a candidate cell within sensor range
// (the information gain of frontier exploration, per 45-degree sector), and which cells a set of eyes sees.
//
// Upstream has no counterpart: its generate_mask (utils/mapping_utils.py:403-454) is the unused seed of the explored map and
// predicts nothing.  Everything below is this project's own definition, written out in DESIGN.md 4.28; every output is an integer
// count or a 0/1 byte, so a scalar restatement (tests/_viewshed_ref.py) is compared with np.array_equal.
//
// CELLS of an (H, W) image.  OPAQUE: free == 0.  UNKNOWN: free != 0 and explored == 0 (an obstacle cell is known, as in
// avl_frontier_mask).  BLOCKING: opaque; with opaque_unknown also unknown.
//
// THE SIGHT LINE from eye e to target t is the walk of avl_sight.hip without the height axis: d = |t - e| per axis, s the signs,
// n = max(d_r, d_c); cells k = 0 .. n; between two cells each axis x with error e_x (starting at 2 d_x - n) does
// `if e_x > 0: x += s_x, e_x -= 2 n`, then `e_x += 2 d_x`, rows before columns.  The walk is NOT symmetric and always runs from the
// eye to the target.  Every axis only moves towards t and the walk ends on t: it never leaves the box between its ends.
//
// t is VISIBLE from e when both lie inside the image, t != e, dr^2 + dc^2 <= R^2 (equality counts) and no cell 1 <= k < n is
// blocking.  The eye's own cell never blocks, the target cell is never tested (the face of a wall is seen), and an eye may stand
// on any cell.
//
// OCTANT of an offset (dr, dc) != 0, sector k = [k * 45, (k + 1) * 45) degrees of atan2(dr, dc), in integers: if dc > 0 and
// dr >= 0 the sector is 0 when dr < dc, else 1; otherwise replace (dr, dc) by (-dc, dr), add 2 and repeat.
//
// gain[e, k] = the visible unknown targets of eye e in sector k, a row of -1 for an eye outside the image.  seen = 1 on every cell
// visible from at least one eye and on the eyes' own cells.
//
// Launch shape: a block of 256 threads owns an eye.  Every walk stays inside the eye's window of at most (2R + 1)^2 <= 255^2
// cells, clipped to the image, so the block first stages that window in LDS as two bit planes of 8 words per row (8160 bytes each
// at R = 127): `blocking`, and `target` = the cells the eye has to walk to (in range, not the eye; for the gain also unknown).  A
// wave stages 64 consecutive cells of a row with one byte load per lane and mask and one ballot per plane.  The target plane is
// then compacted, 256 words at a time (a popcount per thread and one workgroup scan), into an LDS list of packed window cells, and
// whenever the list holds more than kViewFlush entries -- and at the end -- the threads take its entries in turn and walk them: a
// cell that is no target costs its bit in a popcount and nothing else, and an unknown cell here and there no longer leaves 63 lanes
// of a wave idle.  The walk probes the LDS plane only and ends at the first blocker.  The gain is kept per thread in two 64-bit
// registers of four 16-bit counters (a thread walks fewer than 300 cells, a wave fewer than 2^16), summed over the wave, added to eight LDS counters
// by one lane per wave, and stored once per eye and sector: integer sums, independent of the order and of the launch geometry.
// The seen kernel stores a 1 byte per visible cell; racing stores carry the same value.
//
// AVL_VIEWSHED_GLOBAL_PROBE (tools/probe_viewshed.py's A/B through tools/build_variant.py, never in the shipped library): the walk
// reads free / explored from global memory instead of the LDS plane.  Staging, compaction and counting are unchanged.
#include <algorithm>
#include <climits>

#include "avl_wave.h"

namespace avl {

constexpr int kViewThreads = 256;
constexpr int kViewWaves = kViewThreads / kWave;
constexpr int kViewMaxRadius = 127;
constexpr int kViewMaxSide = 16384;                             // EXPLORE_MAX_SIDE
constexpr int kViewRows = 2 * kViewMaxRadius + 1;               // window rows and columns: 255
constexpr int kViewRowWords = 8;                                // 256 bits per row: a window cell is bit (row << 8) + col
constexpr int kViewPlaneWords = kViewRows * kViewRowWords;
constexpr int kViewChunk = kViewThreads * 32;                   // the most targets one compaction step adds
constexpr int kViewFlush = 4096;                                // walk the list once it holds more than this
constexpr int kViewList = kViewFlush + kViewChunk;              // uint16 entries: 24 KB

struct ViewParams {
    const uint8_t* free_u8;
    const uint8_t* explored;
    int H, W, R, opaque_unknown;
};

// the sector of (dr, dc) != (0, 0); at most three quarter turns
__device__ __forceinline__ int view_octant(int dr, int dc) {
    int k = 0;
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        if (!(dc > 0 && dr >= 0)) {
            const int t = dr;
            dr = -dc;
            dc = t;
            k += 2;
        }
    }
    return k + (dr < dc ? 0 : 1);
}

struct ViewWindow {
    int r0, c0, rows, cols;         // the window's first cell in the image and its size
    int er, ec;                     // the eye in window coordinates
};

// Is the window cell with bit index `lin` blocking?
__device__ __forceinline__ bool view_blocking(const ViewParams& p, const ViewWindow& w, const uint32_t* __restrict__ s_block, int lin) {
#ifdef AVL_VIEWSHED_GLOBAL_PROBE
    const size_t i = (size_t)(w.r0 + (lin >> 8)) * p.W + (w.c0 + (lin & 255));
    const bool is_free = p.free_u8[i] != 0;
    return !is_free || (p.opaque_unknown && p.explored[i] == 0);
#else
    return s_block[lin >> 5] >> (lin & 31) & 1u;
#endif
}

// no blocker strictly between the eye and the window cell (tr, tc)
__device__ __forceinline__ bool view_walk(const ViewParams& p, const ViewWindow& w, const uint32_t* __restrict__ s_block, int tr, int tc) {
    const int dr = abs(tr - w.er), dc = abs(tc - w.ec);
    const int n = max(dr, dc);
    const int sr = tr > w.er ? 256 : -256, sc = tc > w.ec ? 1 : -1;
    int er = 2 * dr - n, ec = 2 * dc - n;
    int lin = (w.er << 8) + w.ec;
    for (int k = 1; k < n; ++k) {
        if (er > 0) {
            lin += sr;
            er -= 2 * n;
        }
        er += 2 * dr;
        if (ec > 0) {
            lin += sc;
            ec -= 2 * n;
        }
        ec += 2 * dc;
        if (view_blocking(p, w, s_block, lin)) return false;
    }
    return true;
}

// kSeen = false: out = gain (E, 8) int32.  kSeen = true: out = seen (H, W) uint8.
template <bool kSeen>
__device__ __forceinline__ void viewshed_block(const ViewParams& p, const int32_t* __restrict__ eyes, void* __restrict__ out) {
    __shared__ uint32_t s_block[kViewPlaneWords];
    __shared__ uint32_t s_target[kViewPlaneWords];
    __shared__ uint16_t s_list[kViewList];
    __shared__ int s_scan[kViewWaves];
    __shared__ unsigned s_gain[8];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t e = blockIdx.x;
    const int eye_r = eyes[2 * e], eye_c = eyes[2 * e + 1];
    int32_t* gain = kSeen ? nullptr : (int32_t*)out + 8 * e;
    uint8_t* seen = kSeen ? (uint8_t*)out : nullptr;
    if (eye_r < 0 || eye_r >= p.H || eye_c < 0 || eye_c >= p.W) {          // block-uniform
        if (!kSeen && tid < 8) gain[tid] = -1;
        return;
    }
    ViewWindow w;
    w.r0 = max(eye_r - p.R, 0);
    w.c0 = max(eye_c - p.R, 0);
    w.rows = min(eye_r + p.R, p.H - 1) - w.r0 + 1;
    w.cols = min(eye_c + p.R, p.W - 1) - w.c0 + 1;
    w.er = eye_r - w.r0;
    w.ec = eye_c - w.c0;
    if (tid < 8) s_gain[tid] = 0;
    if (kSeen && tid == 0) seen[(size_t)eye_r * p.W + eye_c] = 1;

    // stage: item = (row, 64-column segment); all four segments of a row are written, the ones past the window as zeros
    const int R2 = p.R * p.R;
    for (int item = wave; item < w.rows * 4; item += kViewWaves) {
        const int row = item >> 2, col = (item & 3) * kWave + lane;
        bool blocking = false, target = false;
        if (col < w.cols) {
            const size_t i = (size_t)(w.r0 + row) * p.W + (w.c0 + col);
            const bool is_free = p.free_u8[i] != 0, unknown = is_free && p.explored[i] == 0;
            blocking = !is_free || (p.opaque_unknown && unknown);
            const int dr = row - w.er, dc = col - w.ec;
            target = (kSeen || unknown) && dr * dr + dc * dc <= R2 && (dr | dc) != 0;
        }
        const unsigned long long b = __ballot(blocking), t = __ballot(target);
        if (lane < 2) {
            const int word = row * kViewRowWords + (item & 3) * 2 + lane;
            s_block[word] = (uint32_t)(b >> (32 * lane));
            s_target[word] = (uint32_t)(t >> (32 * lane));
        }
    }
    __syncthreads();

    unsigned long long acc_lo = 0, acc_hi = 0;          // sectors 0 .. 3 and 4 .. 7, 16 bits each
    const int words = w.rows * kViewRowWords;
    int fill = 0;                                       // block-uniform
    for (int base = 0; base < words; base += kViewThreads) {
        const int word = base + tid;
        uint32_t bits = word < words ? s_target[word] : 0u;
        int total;
        int at = fill + block_excl_scan<kViewWaves>((int)__popc(bits), OpSum{}, 0, s_scan, &total);
        while (bits) {
            const int b = __ffs(bits) - 1;
            bits &= bits - 1;
            s_list[at++] = (uint16_t)((word >> 3 << 8) | ((word & 7) << 5) | b);
        }
        fill += total;
        __syncthreads();                                // the list is written, s_scan is read
        if (fill <= kViewFlush && base + kViewThreads < words) continue;
        for (int i = tid; i < fill; i += kViewThreads) {
            const int cell = s_list[i], tr = cell >> 8, tc = cell & 255;
            if (!view_walk(p, w, s_block, tr, tc)) continue;
            if (kSeen) {
                seen[(size_t)(w.r0 + tr) * p.W + (w.c0 + tc)] = 1;
            } else {
                const int k = view_octant(tr - w.er, tc - w.ec);
                const unsigned long long one = 1ull << (16 * (k & 3));
                acc_lo += k < 4 ? one : 0ull;
                acc_hi += k < 4 ? 0ull : one;
            }
        }
        fill = 0;
        __syncthreads();                                // the list is read
    }
    if (kSeen) return;
    // a thread walked fewer than 2^16 / 64 cells (255^2 / 256 and at most one more per flush), so a wave's sums fit their 16 bits
    acc_lo = wave_sum(acc_lo);
    acc_hi = wave_sum(acc_hi);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            atomicAdd(&s_gain[k], (unsigned)(acc_lo >> (16 * k)) & 0xFFFFu);
            atomicAdd(&s_gain[4 + k], (unsigned)(acc_hi >> (16 * k)) & 0xFFFFu);
        }
    }
    __syncthreads();
    if (tid < 8) gain[tid] = (int32_t)s_gain[tid];
}

__global__ __launch_bounds__(kViewThreads) void viewshed_gain_kernel(ViewParams p, const int32_t* __restrict__ eyes, int32_t* __restrict__ gain) {
    viewshed_block<false>(p, eyes, gain);
}

__global__ __launch_bounds__(kViewThreads) void viewshed_seen_kernel(ViewParams p, const int32_t* __restrict__ eyes, uint8_t* __restrict__ seen) {
    viewshed_block<true>(p, eyes, seen);
}

static int view_params(const char* who, const uint8_t* d_free_u8, const uint8_t* d_explored_u8, int H, int W, int64_t n_eyes, int radius,
                       int opaque_unknown, ViewParams* p) {
    AVL_REQUIRE(H >= 1 && W >= 1 && H <= kViewMaxSide && W <= kViewMaxSide, "%s: bad shape %d x %d (sides 1 .. %d)", who, H, W, kViewMaxSide);
    AVL_REQUIRE(radius >= 1 && radius <= kViewMaxRadius, "%s: radius %d (1 .. %d cells)", who, radius, kViewMaxRadius);
    AVL_REQUIRE(n_eyes >= 0 && n_eyes <= INT_MAX, "%s: %lld eyes (0 .. 2^31 - 1)", who, (long long)n_eyes);
    *p = ViewParams{d_free_u8, d_explored_u8, H, W, radius, opaque_unknown != 0};
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_viewshed_gain(const uint8_t* d_free_u8, const uint8_t* d_explored_u8, int H, int W, const int32_t* d_eyes, int64_t E, int radius,
                      int opaque_unknown, int32_t* d_gain, void* stream) {
    ViewParams p{};
    const int rc = view_params("avl_viewshed_gain", d_free_u8, d_explored_u8, H, W, E, radius, opaque_unknown, &p);
    if (rc != AVL_OK) return rc;
    if (E == 0) return AVL_OK;
    AVL_REQUIRE(d_free_u8 && d_explored_u8 && d_eyes && d_gain, "avl_viewshed_gain: null pointer");
    hipLaunchKernelGGL(viewshed_gain_kernel, dim3((unsigned)E), dim3(kViewThreads), 0, as_stream(stream), p, d_eyes, d_gain);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_viewshed_seen(const uint8_t* d_free_u8, const uint8_t* d_explored_u8, int H, int W, const int32_t* d_eyes, int64_t M, int radius,
                      int opaque_unknown, int accumulate, uint8_t* d_seen, void* stream) {
    ViewParams p{};
    const int rc = view_params("avl_viewshed_seen", d_free_u8, d_explored_u8, H, W, M, radius, opaque_unknown, &p);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_seen && (M == 0 || (d_free_u8 && d_explored_u8 && d_eyes)), "avl_viewshed_seen: null pointer");
    if (!accumulate) AVL_HIP_CHECK(hipMemsetAsync(d_seen, 0, (size_t)H * W, as_stream(stream)));
    if (M == 0) return AVL_OK;
    hipLaunchKernelGGL(viewshed_seen_kernel, dim3((unsigned)M), dim3(kViewThreads), 0, as_stream(stream), p, d_eyes, d_seen);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
