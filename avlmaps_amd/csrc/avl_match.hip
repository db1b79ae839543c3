// Registration of depth frames to a voxel map for gfx950: correlative scan matching (Olson, "Real-time correlative scan matching",
// ICRA 2009) in the map's own cells.  The hit points of F depth frames are rasterised into (row, col, h) cells exactly as the
// builder rasterises them, once per angle of a table of planar rotations, and every rotated copy is slid over the map's occupancy
// bits: score = the number of points that land on an occupied cell, for every angle and every shift of a (2R + 1)^2 window.  An
// exhaustive search: no initial guess to fall out of, no local minimum, and nothing but integers after the cell.
//
// Upstream has no counterpart: avlmaps/map/vlmap_builder.py takes its poses.txt on trust, and nothing in the tree relates a second
// recording to an existing map.  Everything below is this project's own definition, written out in DESIGN.md 4.23; every output is
// an integer count or the winner of an integer order, so a restatement (tests/_match_ref.py) is compared with np.array_equal.
//
// THE DEFINITION.  Inputs: the cell index of the map (avl_cellindex.h; only its bits are read), F depth frames with their
// calibration and camera -> map transforms T (the priors) as avl_audit_rays takes them, a table of K angles as float64 (cos, sin),
// a radius R in cells (S = 2R + 1), an inclusive height band [h_lo, h_hi] in cells, stride, min_depth, max_depth, and a mode:
// joint (one volume, V = 1, all frames' points together) or per frame (V = F).
//    1  points: the lattice pixels of avl_sightray.h steps 1 - 2 (ray_pixel); kept when min_depth < p.z < max_depth (the builder's
//       and the vote's rule: HIT points only, no far rays); P = bp_transform(T, p); dropped unless P.x, P.y and P.z are finite
//    2  height: h = py_int(P.z / cs) (base_pos2grid_id_3d's, truncating); dropped unless h_lo <= h <= h_hi.  valid[v] counts the
//       points of volume v that reach this line; it does not depend on the angle
//    3  rotation by angle k = (c, s) about the pivot (px, py), float64, unfused, in this order:
//         dx = P.x - px, dy = P.y - py;  qx = px + (c * dx - s * dy),  qy = py + (s * dx + c * dy),  qz = P.z
//       and when c == 1 && s == 0 the point is P itself, not the expression: the zero angle gives the builder's cells exactly.
//       The pivot of a frame's points is the frame's own origin (T[0, 3], T[1, 3]) per frame, the caller's one pivot in joint mode
//    4  cell: row = ray_cell_rc(qx), col = ray_cell_rc(qy).  NOT clipped to the grid: a point at row -3 can be shifted in.  Dropped
//       only when no shift can bring it in: row or col outside [-R, gs - 1 + R]
//    5  score[v, k, di + R, dj + R], di, dj in [-R, R], uint32 = the number of points of (v, k) whose cell (row + di, col + dj, h)
//       lies inside the grid and has its bit set in the index.  A point counts once per point: two points of one cell count twice
//    6  the winner of volume v, best[v] = (k, di, dj, score) int32: the larger score; then the smaller di^2 + dj^2; then the smaller
//       |k - k0| (k0: the caller's prior index); then the smaller k, then di, then dj.  A volume without a valid point has all
//       scores 0 and so yields (k0, 0, 0, 0)
// The host turns a winner into a correction of the prior: C = Trans(-di * cs, -dj * cs, 0) Trans(pivot) Rz(c_k, s_k) Trans(-pivot),
// corrected T = C @ T (row = gs / 2 - int(x / cs): one row up is cs down in x).  The translation is accurate to one cell.
//
// THE KERNELS.
//   match_raster_kernel     the sight-ray front end's launch shape (avl_sightray.h): a thread owns a lattice pixel, lanes run along
//       an image row, blockIdx.y is the frame's slot, the pose and the angles are wave-uniform kernel arguments (up to kRayFrames
//       frames and kMatchAngles angles per launch).  It loops over the launch's angles and appends the surviving cells, packed as
//       the linear cell of the grid grown by R on every side, ((row + R) * (gs + 2R) + col + R) * vh + h, to the list of (v, k)
//       in the workspace.  Two passes round one reservation: pass 1 notes under which angles a point is kept (a bit each) and
//       counts every wave's points per angle in LDS, one integer atomic per BLOCK and angle then reserves the block's slots (a
//       joint volume has only K counters for all its frames: one atomic per wave made them the kernel's time), pass 2 computes
//       the cells again and writes them, the lanes' ranks coming from the ballot.  The order of a list is not defined and nothing
//       depends on it.  valid is counted by ballot, one atomic per wave
//   match_correlate_kernel  the hot path.  A block owns one (v, k), a tile of shifts and a range of the list.  Lanes run along dj
//       (wd = the power of two >= S, at most 64, lanes; 64 / wd rows of di share a wave): h is the fastest dimension of the linear
//       cell, so 64 neighbouring dj touch about 2 * vh consecutive index words.  The list is staged through LDS in chunks of 256
//       decoded points and read back as broadcasts; each lane keeps kMatchDi counters, its shifts' scores, in registers.
//       Probes are not branched round: a shift outside the grid reads a zero word of the workspace, so the 16 loads of four
//       points are in flight together (with a branch per probe every load was waited for on its own: 72 -> 26 ms for 32 joint
//       frames at R = 20).  A block whose range is the whole list stores its counters plainly; when the list is split over
//       several blocks (few (v, k) and many points: the joint mode) they add with integer atomics into scores zeroed by the
//       entry point.  Integer sums: the result does not depend on the split or on scheduling.  The split is the caller's
//       (`split` blocks per list at most) or, with split = 0, what brings the launch to kMatchWantBlocks blocks
//   match_finish_kernel     a block per volume folds score and tie rule into one 64-bit key per (k, di, dj) and takes the maximum:
//       score (31 bits: a volume has fewer than 2^31 points) | 16383 - (di^2 + dj^2) | 1023 - rank(k) | 255 - (di + R) | dj <= 0,
//       rank(k) = the place of k in the order (|k - k0|, k), below 1024; given di^2 + dj^2 and di, dj is one of two values
// Nothing is allocated: the lists live in the caller's workspace (avl_match_ws_bytes), 4 bytes per lattice pixel, frame and angle.
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_cellindex.h"
#include "avl_sightray.h"
#include "avl_wave.h"

namespace avl {

constexpr int kMatchThreads = 256;              // the correlate kernel's block
constexpr int kMatchRasterThreads = 1024;       // the rasterise kernel's: 16 waves share one atomic per angle
constexpr int kMatchMaxAngles = 1024;           // K
constexpr int kMatchMaxRadius = 64;             // R: di + R fits 8 bits, di^2 + dj^2 fits 14
constexpr int kMatchAngles = 64;                // angles per rasterise launch: 1 KB of kernel arguments
constexpr int kMatchDi = 4;                     // counters per lane of the correlate kernel
constexpr int kMatchChunk = 256;                // points staged through LDS at a time
constexpr int kMatchFinishThreads = 1024;
constexpr int kMatchWantBlocks = 8192;          // split = 0: the correlate kernel splits the lists until the launch has this many blocks, four
                                                // rounds of the 8 that fit each of an MI355X's 256 CUs, so that a last, partly filled round
                                                // costs a quarter at most.  A constant, not the device's CU count: which path a call takes
                                                // depends on its arguments alone
constexpr int kMatchMaxSplit = 65536;           // the largest split a caller may ask for
constexpr int kMatchOut = 1 << 20;              // a shift no cell survives: row + kMatchOut >= gs for every row >= -R

struct MatchAngleBatch {
    double cs[kMatchAngles][2];
};

struct MatchParams {
    RayParams ray;
    double px, py;                              // the joint pivot
    long long cap;                              // entries of one (v, k) list
    int vh, R, K, h_lo, h_hi, joint;
    const uint32_t* bits;
    const uint32_t* zero;                       // one word of 0: what a shift outside the grid reads
    uint32_t* counts;                           // (V * K) list lengths
    uint32_t* lists;                            // (V * K, cap) packed cells
};

struct MatchView {
    uint32_t* zero;
    uint32_t* counts;
    uint32_t* lists;
    long long cap, V;
    size_t total;
};

// the ONE layout of the workspace (the size query passes a null base)
static MatchView match_layout(void* base, int F, int rays, int K, int joint) {
    MatchView v{};
    v.V = joint ? 1 : F;
    v.cap = (long long)(joint ? F : 1) * rays;
    Carver c(base ? align256_ptr(base) : nullptr);
    v.zero = c.ptr<uint32_t>(4);
    v.counts = c.ptr<uint32_t>((size_t)std::max<long long>(v.V * K, 1) * 4);
    v.lists = c.ptr<uint32_t>((size_t)std::max<long long>(v.V * K * v.cap, 1) * 4);
    v.total = c.total() + 256;                  // the slack of a base that is not 256-aligned
    return v;
}

// (3 - 4) the cell of map point (gx, gy) = pivot + (dx, dy) under angle (c, s); false when no shift of [-R, R] brings it into the grid
__device__ __forceinline__ bool match_cell(const MatchParams& p, double c, double s, double gx, double gy, double dx, double dy, double px, double py,
                                           int& row, int& col) {
    double qx = gx, qy = gy;
    if (!(c == 1.0 && s == 0.0)) {
        qx = px + (c * dx - s * dy);
        qy = py + (s * dx + c * dy);
    }
    row = ray_cell_rc(p.ray, qx);
    col = ray_cell_rc(p.ray, qy);
    const int R = p.R, gs = p.ray.gs;
    return row >= -R && row <= gs - 1 + R && col >= -R && col <= gs - 1 + R;
}

__global__ __launch_bounds__(kMatchRasterThreads) void match_raster_kernel(MatchParams p, RayBatch batch, MatchAngleBatch ang, int f0, int k_first, int nk,
                                                                          const void* __restrict__ depth, uint32_t* __restrict__ valid) {
    __shared__ uint32_t s_wave[kMatchRasterThreads / kWave][kMatchAngles];      // a wave's points of an angle, then its first slot in the list
    const RayFrame& fr = batch.f[blockIdx.y];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int ray = blockIdx.x * kMatchRasterThreads + threadIdx.x;
    const long long v = p.joint ? 0 : f0 + (int)blockIdx.y;
    const double px = p.joint ? p.px : fr.t[3], py = p.joint ? p.py : fr.t[7];
    bool ok = ray < p.ray.nv * p.ray.nu;                                        // (every thread stays to the end: ballots and barriers see them all)
    double gx = 0.0, gy = 0.0;
    int h = 0;
    if (ok) {
        size_t pix;
        double p0, p1, p2, gz;
        ray_pixel(p.ray, depth, ray, blockIdx.y, pix, p0, p1, p2);              // (1)
        ok = p2 > p.ray.min_depth && p2 < p.ray.max_depth;
        if (ok) {
            bp_transform(fr.t, p0, p1, p2, gx, gy, gz);
            ok = isfinite(gx) && isfinite(gy) && isfinite(gz);
            h = py_int(gz / p.ray.cs);                                          // (2)
            ok = ok && h >= p.h_lo && h <= p.h_hi;
        }
    }
    const unsigned long long alive = __ballot(ok);
    if (k_first == 0 && lane == 0 && alive) atomicAdd(valid + v, (unsigned)__popcll(alive));
    const double dx = gx - px, dy = gy - py;
    // pass 1: under which of the launch's angles the point is kept (one bit each), and how many points every wave keeps
    unsigned long long mine = 0;
    for (int k = 0; k < nk; ++k) {
        int row, col;
        const bool keep = ok && match_cell(p, ang.cs[k][0], ang.cs[k][1], gx, gy, dx, dy, px, py, row, col);
        mine |= (unsigned long long)keep << k;
        const unsigned long long kept = __ballot(keep);
        if (lane == 0) s_wave[wave][k] = (unsigned)__popcll(kept);
    }
    __syncthreads();
    // one atomic per block and angle reserves the block's slots in the list of (v, k); the waves take theirs in wave order
    if ((int)threadIdx.x < nk) {
        const int k = threadIdx.x;
        unsigned total = 0;
        for (int w = 0; w < kMatchRasterThreads / kWave; ++w) total += s_wave[w][k];
        unsigned at = total ? atomicAdd(p.counts + v * p.K + k_first + k, total) : 0u;
        for (int w = 0; w < kMatchRasterThreads / kWave; ++w) {
            const unsigned n = s_wave[w][k];
            s_wave[w][k] = at;
            at += n;
        }
    }
    __syncthreads();
    // pass 2: the cells again (the same operations give the same cells), each written to its slot
    const int R = p.R, E = p.ray.gs + 2 * R;
    for (int k = 0; k < nk; ++k) {
        const bool keep = mine >> k & 1ull;
        const unsigned long long kept = __ballot(keep);
        if (!keep) continue;
        int row, col;
        match_cell(p, ang.cs[k][0], ang.cs[k][1], gx, gy, dx, dy, px, py, row, col);
        const long long vk = v * p.K + k_first + k;
        const long long at = (long long)s_wave[wave][k] + __popcll(kept & ((1ull << lane) - 1ull));
        if (at < p.cap)                                                         // (a list takes one entry per pixel and frame: always true)
            p.lists[vk * p.cap + at] = ((uint32_t)(row + R) * (uint32_t)E + (uint32_t)(col + R)) * (uint32_t)p.vh + (uint32_t)h;
    }
}

__global__ __launch_bounds__(kMatchThreads) void match_correlate_kernel(MatchParams p, int lwd, int di_tiles, int dj_tiles, int nsplit, long long per_split,
                                                                       uint32_t* __restrict__ scores) {
    __shared__ int4 pts[kMatchChunk];
    const int R = p.R, S = 2 * R + 1, gs = p.ray.gs, vh = p.vh, E = gs + 2 * R;
    const int tiles = di_tiles * dj_tiles;
    const long long inner = (long long)tiles * nsplit;
    const long long vk = blockIdx.x / inner;
    const int rest = (int)(blockIdx.x % inner), tile = rest % tiles, split = rest / tiles;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int wd = 1 << lwd, rpw = kWave >> lwd;                                // lanes along dj, rows of di per wave
    const int b = (tile % dj_tiles) * wd + (lane & (wd - 1));                   // dj + R
    const int a0 = (tile / dj_tiles) * (kMatchThreads / kWave * kMatchDi * rpw) + wave * kMatchDi * rpw + (lane >> lwd);        // di + R of counter 0
    const int dj = b < S ? b - R : kMatchOut;
    int di[kMatchDi];
    unsigned cnt[kMatchDi];
#pragma unroll
    for (int d = 0; d < kMatchDi; ++d) {
        di[d] = a0 + d * rpw < S ? a0 + d * rpw - R : kMatchOut;
        cnt[d] = 0;
    }
    const long long n = p.counts[vk] < p.cap ? p.counts[vk] : p.cap;
    const long long lo = (long long)split * per_split, hi = lo + per_split < n ? lo + per_split : n;
    if (nsplit > 1 && lo >= hi) return;                                         // (block-uniform; a lone block still writes its zeros)
    const uint32_t* list = p.lists + vk * p.cap;
    const int plane = gs * vh;                                                  // < 2^31 / gs
    for (long long c0 = lo; c0 < hi; c0 += kMatchChunk) {
        __syncthreads();                                                        // the chunk before this one has been read
        if (c0 + threadIdx.x < hi) {
            const uint32_t w = list[c0 + threadIdx.x], t = w / (uint32_t)vh;
            pts[threadIdx.x] = make_int4((int)(t / (uint32_t)E) - R, (int)(t % (uint32_t)E) - R, (int)(w % (uint32_t)vh), 0);
        }
        __syncthreads();
        const int m = hi - c0 < kMatchChunk ? (int)(hi - c0) : kMatchChunk;
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const int4 pt = pts[j];                                             // (one address for the wave: a broadcast)
            // No branch round a probe: a shift that leaves the grid reads the workspace's zero word instead of a word of the index
            // (the address is selected, not the load), so the loads of an unrolled step are all in flight before the first is
            // waited for.  Unsigned arithmetic: a shift marked kMatchOut may wrap, and is never used as an address
            const uint32_t col = (uint32_t)(pt.y + dj), at = col * (uint32_t)vh + (uint32_t)pt.z;
            const bool col_in = col < (uint32_t)gs;
#pragma unroll
            for (int d = 0; d < kMatchDi; ++d) {
                const uint32_t row = (uint32_t)(pt.x + di[d]), lin = row * (uint32_t)plane + at;         // inside the grid: < 2^31
                const uint32_t* word = col_in && row < (uint32_t)gs ? p.bits + (lin >> 5) : p.zero;
                cnt[d] += *word >> (lin & 31u) & 1u;
            }
        }
    }
    if (b >= S) return;
#pragma unroll
    for (int d = 0; d < kMatchDi; ++d) {
        const int a = a0 + d * rpw;
        if (a >= S) continue;
        uint32_t* out = scores + ((size_t)vk * S + a) * S + b;
        if (nsplit == 1) *out = cnt[d];
        else if (cnt[d]) atomicAdd(out, cnt[d]);
    }
}

__global__ __launch_bounds__(kMatchFinishThreads) void match_finish_kernel(const uint32_t* __restrict__ scores, int K, int R, int k0, int32_t* __restrict__ best) {
    __shared__ unsigned long long s_key[kMatchFinishThreads / kWave];
    __shared__ int s_at[kMatchFinishThreads / kWave];
    const int S = 2 * R + 1, SS = S * S, n = K * SS;                            // V * K * S^2 < 2^31
    const uint32_t* sc = scores + (size_t)blockIdx.x * n;
    const int m = min(k0, K - 1 - k0);                                          // angles on both sides of k0
    unsigned long long key = 0;                                                 // (below every real key: 16383 - d2 > 0)
    int at = 0;
    for (long long j = threadIdx.x; j < n; j += kMatchFinishThreads) {         // (n may be 2^31 - 1: the step is taken in 64 bits)
        const int i = (int)j, k = i / SS, r = i - k * SS, a = r / S, b = r - a * S, di = a - R, dj = b - R;
        const int d = abs(k - k0), rank = d <= m ? (d == 0 ? 0 : 2 * d - (k < k0 ? 1 : 0)) : m + d;          // < K <= 1024
        const unsigned long long x = (unsigned long long)sc[i] << 33 | (unsigned long long)(16383 - (di * di + dj * dj)) << 19 |
                                     (unsigned long long)(1023 - rank) << 9 | (unsigned long long)(255 - a) << 1 | (dj <= 0 ? 1ull : 0ull);
        if (x > key) {
            key = x;
            at = i;
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {                             // (keys of different (k, di, dj) differ: no ties)
        const unsigned long long ok = __shfl_xor(key, off, kWave);
        const int oa = __shfl_xor(at, off, kWave);
        if (ok > key) {
            key = ok;
            at = oa;
        }
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_key[threadIdx.x / kWave] = key;
        s_at[threadIdx.x / kWave] = at;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kMatchFinishThreads / kWave; ++w)
            if (s_key[w] > key) {
                key = s_key[w];
                at = s_at[w];
            }
        const int k = at / SS, r = at - k * SS, a = r / S;
        best[4 * blockIdx.x + 0] = k;
        best[4 * blockIdx.x + 1] = a - R;
        best[4 * blockIdx.x + 2] = r - a * S - R;
        best[4 * blockIdx.x + 3] = (int32_t)sc[at];
    }
}

// the limits the size query and the entry point share; *rays = the lattice pixels of one frame
static int match_check_batch(const char* who, int F, int H, int W, int stride, int K, int R, int joint, int* rays) {
    AVL_REQUIRE(F >= 0 && H > 0 && W > 0 && (int64_t)H * W < INT_MAX, "%s: bad batch of %d frames of %d x %d", who, F, H, W);
    AVL_REQUIRE(stride >= 1, "%s: stride %d < 1", who, stride);
    AVL_REQUIRE(K >= 1 && K <= kMatchMaxAngles, "%s: %d angles (1 .. %d)", who, K, kMatchMaxAngles);
    AVL_REQUIRE(R >= 0 && R <= kMatchMaxRadius, "%s: radius %d (0 .. %d cells)", who, R, kMatchMaxRadius);
    const int off = stride / 2;
    const int64_t nv = off < H ? (H - off + stride - 1) / stride : 0, nu = off < W ? (W - off + stride - 1) / stride : 0;
    AVL_REQUIRE((joint ? (int64_t)F : 1) * nv * nu < INT_MAX, "%s: %d frames of %lld pixels in one volume (fewer than 2^31 - 1 points)", who, F,
                (long long)(nv * nu));
    const int64_t V = joint ? 1 : F, S = 2 * R + 1;
    AVL_REQUIRE(V * K * S * S <= INT_MAX, "%s: %lld volumes x %d angles x %lld^2 shifts (fewer than 2^31 scores)", who, (long long)V, K, (long long)S);
    *rays = (int)(nv * nu);
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_match_ws_bytes(int F, int H, int W, int stride, int K, int R, int joint, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_match_ws_bytes: null output");
    int rays;
    const int rc = match_check_batch("avl_match_ws_bytes", F, H, W, stride, K, R, joint, &rays);
    if (rc != AVL_OK) return rc;
    *bytes = match_layout(nullptr, F, rays, K, joint).total;
    return AVL_OK;
}

int avl_match_frames(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const void* d_depth, int depth_is_u16, double depth_div,
                     int F, int H, int W, const double* h_calib_inv, const double* h_transforms, double cs, int stride, double min_depth,
                     double max_depth, const double* h_angles, int K, int R, int h_lo, int h_hi, int joint, double pivot_x, double pivot_y, int k0,
                     int split, uint32_t* d_scores, int32_t* d_best, uint32_t* d_valid, void* d_ws, size_t ws_bytes, void* stream) {
    int rc = ci_check_grid("avl_match_frames", N, gs, vh);
    if (rc != AVL_OK) return rc;
    MatchParams p{};
    rc = ray_params("avl_match_frames", depth_is_u16, depth_div, F, H, W, h_calib_inv, gs, 0, cs, stride, nullptr, min_depth, max_depth, &p.ray);
    if (rc != AVL_OK) return rc;
    int rays;
    if ((rc = match_check_batch("avl_match_frames", F, H, W, stride, K, R, joint, &rays)) != AVL_OK) return rc;
    const int64_t V = joint ? 1 : F, S = 2 * R + 1, E = (int64_t)gs + 2 * R;
    AVL_REQUIRE(h_lo >= 0 && h_lo <= h_hi && h_hi < vh, "avl_match_frames: height band [%d, %d] (0 <= h_lo <= h_hi < %d cells)", h_lo, h_hi, vh);
    AVL_REQUIRE(E * E * vh <= (int64_t)UINT_MAX, "avl_match_frames: grid %d + 2 * %d cells a side x %d: a packed cell needs (gs + 2R)^2 * vh < 2^32", gs,
                R, vh);
    AVL_REQUIRE(k0 >= 0 && k0 < K, "avl_match_frames: prior angle index %d (0 .. %d)", k0, K - 1);
    AVL_REQUIRE(split >= 0 && split <= kMatchMaxSplit, "avl_match_frames: split %d (0 = chosen here, or 1 .. %d blocks per list)", split, kMatchMaxSplit);
    AVL_REQUIRE(!joint || (std::isfinite(pivot_x) && std::isfinite(pivot_y)), "avl_match_frames: the pivot (%g, %g) is not finite", pivot_x, pivot_y);
    if (F == 0) return AVL_OK;
    AVL_REQUIRE(d_index && d_depth && h_calib_inv && h_transforms && h_angles && d_scores && d_best && d_valid && d_ws, "avl_match_frames: null pointer");
    for (int k = 0; k < K; ++k)
        AVL_REQUIRE(std::isfinite(h_angles[2 * k]) && std::isfinite(h_angles[2 * k + 1]), "avl_match_frames: angle %d (%g, %g) is not finite", k,
                    h_angles[2 * k], h_angles[2 * k + 1]);
    for (int f = 0; f < F && !joint; ++f)
        AVL_REQUIRE(std::isfinite(h_transforms[(size_t)f * 16 + 3]) && std::isfinite(h_transforms[(size_t)f * 16 + 7]),
                    "avl_match_frames: the pivot of frame %d, its origin (%g, %g), is not finite", f, h_transforms[(size_t)f * 16 + 3],
                    h_transforms[(size_t)f * 16 + 7]);
    const CellIndexView index = ci_layout(const_cast<void*>(d_index), N, gs, vh);
    AVL_REQUIRE(index_bytes >= index.total, "avl_match_frames: the index buffer has %zu bytes, needs %zu", index_bytes, index.total);
    const MatchView ws = match_layout(d_ws, F, rays, K, joint);
    AVL_REQUIRE(ws_bytes >= ws.total, "avl_match_frames: the workspace has %zu bytes, needs %zu", ws_bytes, ws.total);

    p.px = joint ? pivot_x : 0.0;
    p.py = joint ? pivot_y : 0.0;
    p.cap = ws.cap;
    p.vh = vh;
    p.R = R;
    p.K = K;
    p.h_lo = h_lo;
    p.h_hi = h_hi;
    p.joint = joint ? 1 : 0;
    p.bits = index.bits;
    p.zero = ws.zero;
    p.counts = ws.counts;
    p.lists = ws.lists;
    // the correlate kernel's shape: wd lanes along dj, 64 / wd rows of di per wave, kMatchDi counters per lane
    int lwd = 0;
    while ((1 << lwd) < S && lwd < 6) ++lwd;
    const int wd = 1 << lwd, rows = kMatchThreads / kWave * kMatchDi * (kWave / wd);
    const int dj_tiles = (int)((S + wd - 1) / wd), di_tiles = (int)((S + rows - 1) / rows);
    // the split of a list over blocks: the caller's, or as many blocks as bring the launch to kMatchWantBlocks; a block takes whole
    // chunks, so a list of at most one chunk is never split.  (Sized from the list's capacity, every lattice pixel: its length is
    // known on the device only.  Blocks past the list's end return at once)
    const int64_t shift_blocks = V * K * di_tiles * dj_tiles, chunks = (ws.cap + kMatchChunk - 1) / kMatchChunk;
    const int64_t asked = split ? split : (kMatchWantBlocks + shift_blocks - 1) / shift_blocks;
    int64_t nsplit = 1, per_split = std::max<int64_t>(ws.cap, 1);
    if (asked > 1 && chunks > 1) {
        nsplit = std::min<int64_t>(asked, chunks);
        per_split = ((ws.cap + nsplit - 1) / nsplit + kMatchChunk - 1) / kMatchChunk * kMatchChunk;
        nsplit = (ws.cap + per_split - 1) / per_split;
    }
    AVL_REQUIRE(shift_blocks * nsplit <= INT_MAX, "avl_match_frames: %lld blocks (fewer than 2^31: ask for a smaller split)", (long long)(shift_blocks * nsplit));

    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(ws.zero, 0, 4, st));
    AVL_HIP_CHECK(hipMemsetAsync(ws.counts, 0, (size_t)(V * K) * 4, st));
    AVL_HIP_CHECK(hipMemsetAsync(d_valid, 0, (size_t)V * 4, st));
    if (nsplit > 1) AVL_HIP_CHECK(hipMemsetAsync(d_scores, 0, (size_t)(V * K * S * S) * 4, st));
    if (rays) {
        const unsigned blocks = (unsigned)((rays + kMatchRasterThreads - 1) / kMatchRasterThreads);
        const size_t frame_bytes = (size_t)H * W * (depth_is_u16 ? sizeof(uint16_t) : sizeof(float));
        ray_launches(F, h_transforms, nullptr, [&](const RayBatch& b, int n, int f0) {
            for (int k_first = 0; k_first < K; k_first += kMatchAngles) {
                const int nk = std::min(kMatchAngles, K - k_first);
                MatchAngleBatch ang{};
                for (int k = 0; k < nk; ++k) ang.cs[k][0] = h_angles[2 * (k_first + k)], ang.cs[k][1] = h_angles[2 * (k_first + k) + 1];
                hipLaunchKernelGGL(match_raster_kernel, dim3(blocks, (unsigned)n), dim3(kMatchRasterThreads), 0, st, p, b, ang, f0, k_first, nk,
                                   (const void*)((const char*)d_depth + (size_t)f0 * frame_bytes), d_valid);
            }
        });
    }
    hipLaunchKernelGGL(match_correlate_kernel, dim3((unsigned)(shift_blocks * nsplit)), dim3(kMatchThreads), 0, st, p, lwd, di_tiles, dj_tiles, (int)nsplit,
                       (long long)per_split, d_scores);
    hipLaunchKernelGGL(match_finish_kernel, dim3((unsigned)V), dim3(kMatchFinishThreads), 0, st, (const uint32_t*)d_scores, K, R, k0, d_best);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
