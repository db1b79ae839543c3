// Cell-to-cell line of sight through a voxel map for gfx950: is target cell t visible from eye cell e, and from which of E
// candidate cells can how many of T target voxels be seen.  The audit (avl_audit.hip) walks the rays of depth frames through the
// cell index; this walks the same integer line between two arbitrary cells of the map, so that a planner can ask where a camera
// has to stand to see an object -- which the 2-D obstacle map cannot say (under the table, behind a half-height partition).
//
// Upstream has no counterpart.  Everything below is this project's own definition, written out in DESIGN.md 4.22; every output is
// an integer count, minimum or index, so a scalar restatement (tests/_sight_ref.py) is compared with np.array_equal.
//
// CELLS.  (row, col, h) int32 on the gs x gs x vh grid of a cell index (avl_cellindex.h).  A cell is OCCUPIED when the index has an
// owner row for it; of several rows in one cell the largest owns it (the index's rule).
//
// THE SIGHT LINE from eye cell e to target cell t is the walk of avl_audit.hip step 12 with a = e, b = t: d = |t - e| per axis,
// s the signs, n = max(d); cells k = 0 .. n; between two cells every axis x with error e_x (starting at 2 d_x - n) does
// `if e_x > 0: x += s_x, e_x -= 2 n`, then `e_x += 2 d_x`.  The walk is NOT symmetric: (0,0,0) -> (2,1,0) passes (1,0,0), the
// reverse passes (1,1,0).  The direction is always eye -> target.  Every axis only moves towards t and the walk ends on t, so with
// both ends inside the grid it never leaves the box between them.
//
// BLOCKERS.  Cell k is a blocker when 1 <= k < n - end_margin, it is occupied, and `transparent` (an optional per-voxel uint8
// array) is absent or 0 at its owner row.  The eye's own cell never blocks, the target cell is never tested, end_margin >= 0; with
// n <= end_margin + 1 (n == 0 among them) nothing is tested.
//
// A pair is VISIBLE when it has no blocker, INVALID when either end is outside [0, gs)^2 x [0, vh), and IN RANGE when
// dr^2 + dc^2 + dh^2 <= max_range2 in int64 (max_range2 < 0: unlimited; equality counts).
//
// Launch shape.  los_pairs_kernel: a thread owns a pair.  los_count_kernel: a wave owns an eye and its lanes run over the targets;
// the four waves of a block share tiles of kSightTile target cells staged in LDS (12 bytes each; lane j reads dwords 3 j .. 3 j + 2,
// a stride coprime with the banks).  A lane tests validity and range first -- an out-of-range pair costs one compare -- then walks
// with an early exit at the first blocker.  A probe is one bit test on the index's bitmap (3.75 MB at gs = 1000, vh = 30); prefix,
// perm and transparent are read only on a set bit, and without `transparent` a set bit decides at once.  Targets come in
// increasing order, 64 at a time: the count is the popcount of the wave's ballot and `first` the lowest set bit of its first
// non-empty ballot.  No atomics, one store per eye and output: the result does not depend on the launch geometry.
#include <algorithm>
#include <climits>

#include "avl_cellindex.h"
#include "avl_wave.h"

namespace avl {

constexpr int kSightThreads = 256;
constexpr int kSightWaves = kSightThreads / kWave;      // eyes per block
constexpr int kSightTile = 1024;                        // target cells per LDS tile: 12 KB
constexpr int kSightMaxTargets = 65536;
constexpr int kLosVisible = -1, kLosInvalid = -2;

struct SightParams {
    int gs, vh, end_margin;
    const uint32_t* bits;
    const int32_t* prefix;
    const int32_t* perm;
    const uint8_t* transparent;
};

__device__ __forceinline__ bool los_inside(const SightParams& p, int r, int c, int h) {
    return r >= 0 && r < p.gs && c >= 0 && c < p.gs && h >= 0 && h < p.vh;
}

// The first blocker of the sight line (r, c, h) -> (tr, tc, th), both inside the grid: its voxel row, kLosVisible when there is none.
// kRow = false (the count only asks whether): any value >= 0 stands for a blocker, and perm is not read without `transparent`.
template <bool kRow>
__device__ __forceinline__ int los_walk(const SightParams& p, int r, int c, int h, int tr, int tc, int th) {
    const int dr = abs(tr - r), dc = abs(tc - c), dh = abs(th - h);
    const int n = max(dr, max(dc, dh));
    const int stop = n - p.end_margin;                  // cells 1 <= k < stop are tested (n <= 16383, end_margin >= 0: no overflow)
    const int plane = p.gs * p.vh;                      // the steps of the linear cell (gs * gs * vh < 2^31)
    const int sr = tr > r ? plane : -plane, sc = tc > c ? p.vh : -p.vh, sh = th > h ? 1 : -1;
    int er = 2 * dr - n, ec = 2 * dc - n, eh = 2 * dh - n;
    int lin = (r * p.gs + c) * p.vh + h;
    for (int k = 1; k < stop; ++k) {
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
        if (eh > 0) {
            lin += sh;
            eh -= 2 * n;
        }
        eh += 2 * dh;
        if (!(p.bits[lin >> 5] >> (lin & 31) & 1u)) continue;
        if (!kRow && !p.transparent) return 0;
        const int i = ci_probe(p.bits, p.prefix, p.perm, lin);
        if (!p.transparent || p.transparent[i] == 0) return i;
    }
    return kLosVisible;
}

__global__ __launch_bounds__(256) void los_pairs_kernel(SightParams p, const int32_t* __restrict__ eyes, const int32_t* __restrict__ targets, int64_t M,
                                                        int32_t* __restrict__ blocker) {
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
        const int r = eyes[3 * m], c = eyes[3 * m + 1], h = eyes[3 * m + 2];
        const int tr = targets[3 * m], tc = targets[3 * m + 1], th = targets[3 * m + 2];
        blocker[m] = los_inside(p, r, c, h) && los_inside(p, tr, tc, th) ? los_walk<true>(p, r, c, h, tr, tc, th) : kLosInvalid;
    }
}

__global__ __launch_bounds__(kSightThreads) void los_count_kernel(SightParams p, const int32_t* __restrict__ eyes, int64_t E,
                                                                 const int32_t* __restrict__ targets, int T, int64_t max_range2,
                                                                 unsigned* __restrict__ visible, int32_t* __restrict__ first) {
    __shared__ int32_t s_t[kSightTile * 3];
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t e = (int64_t)blockIdx.x * kSightWaves + threadIdx.x / kWave;
    int r = 0, c = 0, h = 0;
    if (e < E) {
        r = eyes[3 * e];
        c = eyes[3 * e + 1];
        h = eyes[3 * e + 2];
    }
    const bool eye_ok = e < E && los_inside(p, r, c, h);        // wave-uniform; a wave without an eye still stages and syncs
    unsigned count = 0;
    int lowest = -1;
    for (int t0 = 0; t0 < T; t0 += kSightTile) {
        const int nt = min(kSightTile, T - t0);
        if (t0) __syncthreads();                                // the readers of the tile before this one are done
        for (int i = threadIdx.x; i < 3 * nt; i += kSightThreads) s_t[i] = targets[(int64_t)3 * t0 + i];
        __syncthreads();
        if (!eye_ok) continue;
        for (int base = 0; base < nt; base += kWave) {
            const int j = base + lane;
            bool sees = false;
            if (j < nt) {
                const int tr = s_t[3 * j], tc = s_t[3 * j + 1], th = s_t[3 * j + 2];
                if (los_inside(p, tr, tc, th)) {
                    const int64_t qr = tr - r, qc = tc - c, qh = th - h;
                    if (max_range2 < 0 || qr * qr + qc * qc + qh * qh <= max_range2) sees = los_walk<false>(p, r, c, h, tr, tc, th) < 0;
                }
            }
            const unsigned long long saw = __ballot(sees);
            count += (unsigned)__popcll(saw);
            if (lowest < 0 && saw) lowest = t0 + base + __ffsll(saw) - 1;
        }
    }
    if (e < E && lane == 0) {
        visible[e] = count;
        if (first) first[e] = lowest;
    }
}

static int sight_params(const char* who, const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const uint8_t* d_transparent,
                        int end_margin, SightParams* p) {
    const int rc = ci_check_grid(who, N, gs, vh);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(end_margin >= 0, "%s: end_margin %d < 0", who, end_margin);
    AVL_REQUIRE(d_index, "%s: null index", who);
    const CellIndexView v = ci_layout(const_cast<void*>(d_index), N, gs, vh);
    AVL_REQUIRE(index_bytes >= v.total, "%s: the index buffer has %zu bytes, needs %zu", who, index_bytes, v.total);
    *p = SightParams{gs, vh, end_margin, v.bits, v.prefix, v.perm, d_transparent};
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_los_pairs(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const int32_t* d_eyes, const int32_t* d_targets, int64_t M,
                  const uint8_t* d_transparent, int end_margin, int32_t* d_blocker, void* stream) {
    SightParams p{};
    const int rc = sight_params("avl_los_pairs", d_index, index_bytes, N, gs, vh, d_transparent, end_margin, &p);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(M >= 0 && M < INT_MAX, "avl_los_pairs: %lld pairs (0 .. 2^31 - 2)", (long long)M);
    if (M == 0) return AVL_OK;
    AVL_REQUIRE(d_eyes && d_targets && d_blocker, "avl_los_pairs: null pointer");
    hipLaunchKernelGGL(los_pairs_kernel, dim3(stride_blocks(M)), dim3(256), 0, as_stream(stream), p, d_eyes, d_targets, M, d_blocker);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_los_count(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const int32_t* d_eyes, int64_t E, const int32_t* d_targets,
                  int64_t T, const uint8_t* d_transparent, int end_margin, int64_t max_range2, uint32_t* d_visible, int32_t* d_first,
                  void* stream) {
    SightParams p{};
    const int rc = sight_params("avl_los_count", d_index, index_bytes, N, gs, vh, d_transparent, end_margin, &p);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(E >= 0 && E <= INT_MAX, "avl_los_count: %lld eyes (0 .. 2^31 - 1)", (long long)E);
    AVL_REQUIRE(T >= 0 && T <= kSightMaxTargets, "avl_los_count: %lld targets (0 .. %d)", (long long)T, kSightMaxTargets);
    if (E == 0) return AVL_OK;
    AVL_REQUIRE(d_eyes && d_visible && (d_targets || T == 0), "avl_los_count: null pointer");
    const unsigned blocks = (unsigned)((E + kSightWaves - 1) / kSightWaves);
    hipLaunchKernelGGL(los_count_kernel, dim3(blocks), dim3(kSightThreads), 0, as_stream(stream), p, d_eyes, E, d_targets, (int)T, max_range2,
                       (unsigned*)d_visible, d_first);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
