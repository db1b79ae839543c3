// Visibility-graph navigation on the 2-D obstacle map for gfx950: path vertices, the all-pairs visibility bitset, the visibility
// of the start and goal points, and a float64 single-source shortest path over the graph.
//
// Replaces, in the upstream reference:
//   * avlmaps/navigator/navigator.py:7-65           Navigator.build_visgraph / plan_to
//   * avlmaps/utils/navigation_utils.py:77-197      build_visgraph_with_obs_map (cv2 contours -> pyvisgraph polygons, the
//                                                   rotational sweep) and plan_to_pos_v2 (pyvisgraph's Dijkstra)
//
// Geometric model (DESIGN.md "Navigation").  Obstacle pixel (r, c) is the point (r, c).  The obstacle set O is the union of
//   * bonds: the closed segment between every two 8-adjacent obstacle pixels, and
//   * fills: the convex hull of the obstacle corners of every 2 x 2 window of pixel centres (a dual-grid CELL) holding 3 or 4.
// Inside one closed cell, O is a function of the cell's 4 corners only (16 configurations).  A segment s is blocked iff
//   (a) it meets the open interior of a fill (a triangle or the unit square), or of the union of two fills that share an edge,
//   (b) it crosses a bond transversally at a point that is interior to both, or
//   (c) a run of obstacle pixels strictly inside s, consecutive ones bonded along s, has obstacle 8-neighbours strictly on both
//       sides of s (the segment passes from one side of a wall to the other through pixel centres).
// Touching, grazing corners, running along boundaries and passing wall tips are visible.
//
// The walk.  A segment is traversed in a reflected frame in which both coordinates are non-decreasing: the dual-grid cells it
// passes through, the grid lines it crosses between lattice points, and the lattice points on it, merged in order by comparing
// cross-multiplied crossing parameters (Amanatides-Woo without divisions).  In a cell the chord between two events is tested
// against the cell's configuration: a line function of the chord is linear, so "the open chord enters the triangle" is "one of
// its ends lies strictly beyond the hypotenuse", and "it crosses the diagonal bond" is "its ends lie strictly on both sides".
// Vertex-vertex segments run in int64 (exact); query segments run the same code in float64 with the same expression order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "avl_common.h"
#include "avl_scan.h"

namespace avl {

constexpr int64_t kNavMaxVertices = 65536;      // 65 536^2 bits = 512 MiB of bitset
constexpr int kNavMaxSide = 32768;
constexpr int kNavScanThreads = 256;             // vertex compaction: one block scans kNavScanThreads * kNavScanRounds pixels
constexpr int kNavScanRounds = 4;
constexpr int kNavRoundBatch = 8;                // shortest-path rounds launched between two convergence checks

// pix word of the padded (H + 2) x (W + 2) grid, pixel (r, c) at ((r + 1) * (W + 2) + c + 1), r in [-1, H], c in [-1, W]:
//   bit 8 = obstacle, bits 0..7 = obstacle 8-neighbours in the order E, NE, N, NW, W, SW, S, SE (45 degree steps).
// One word describes a whole dual-grid cell: corners (r, c) = bit 8, (r, c + 1) = E, (r + 1, c) = S, (r + 1, c + 1) = SE.
constexpr uint32_t kObs = 0x100;
__device__ __forceinline__ int nb_dr(int k) { return (int)((0xA901u >> (2 * k)) & 3u) - 1; }   // {0, -1, -1, -1, 0, 1, 1, 1}
__device__ __forceinline__ int nb_dc(int k) { return (int)((0x901Au >> (2 * k)) & 3u) - 1; }   // {1, 1, 0, -1, -1, -1, 0, 1}

struct NavGrid {
    const uint16_t* pix;
    int H, W;
};

__device__ __forceinline__ uint32_t pix_at(const NavGrid& g, long long r, long long c) {
    if (r < -1 || r > g.H || c < -1 || c > g.W) return 0u;
    return g.pix[(size_t)(r + 1) * (size_t)(g.W + 2) + (size_t)(c + 1)];
}

// an obstacle pixel whose obstacle 8-neighbours (at least one) lie within 135 degrees: 4 cyclically consecutive free directions
__device__ __forceinline__ bool is_vertex(uint32_t p) {
    if (!(p & kObs) || !(p & 0xFFu)) return false;
    const uint32_t f = (~p) & 0xFFu;
    const uint32_t ff = f | (f << 8);
    return ((ff & (ff >> 1) & (ff >> 2) & (ff >> 3)) & 0xFFu) != 0u;
}

template <typename T> __device__ __forceinline__ long long tfloor(T x);
template <> __device__ __forceinline__ long long tfloor<long long>(long long x) { return x; }
template <> __device__ __forceinline__ long long tfloor<double>(double x) { return (long long)floor(x); }

// rule (c) at an obstacle pixel inside the segment: bit 0 = an obstacle neighbour strictly on one side, bit 1 = on the other
template <typename T>
__device__ __forceinline__ uint32_t attach_sides(uint32_t p, T dr, T dc) {
    uint32_t sides = 0;
    for (int k = 0; k < 8; ++k) {
        const T cr = dr * (T)nb_dc(k) - dc * (T)nb_dr(k);
        const uint32_t s = (cr > (T)0 ? 1u : 0u) | (cr < (T)0 ? 2u : 0u);
        sides |= ((p >> k) & 1u) ? s : 0u;
    }
    return sides;
}

// rules (a) and (b) inside local cell (i, j) for the chord between the parameters n0 / d0 and n1 / d1 (d > 0); the local point at
// parameter t is (xa + t dx, ya + t dy)
template <typename T>
__device__ __forceinline__ bool cell_blocks(const NavGrid& g, int sr, int sc, long long i, long long j, T xa, T ya, T dx, T dy,
                                            T n0, T d0, T n1, T d1) {
    const long long R = sr > 0 ? i : -i - 1, C = sc > 0 ? j : -j - 1;
    const uint32_t p = pix_at(g, R, C);
    const uint32_t a = ((p >> 8) & 1u) | ((p & 1u) << 1) | (((p >> 6) & 1u) << 2) | (((p >> 7) & 1u) << 3);   // bit 2 * er + ec
    const uint32_t flip = (sr < 0 ? 2u : 0u) | (sc < 0 ? 1u : 0u);
    uint32_t m = 0;                                                                                           // bit 2 * e + f, local
    for (uint32_t b = 0; b < 4; ++b) m |= ((a >> (b ^ flip)) & 1u) << b;
    const int cnt = __popc(m);
    if (cnt == 4) return true;
    const T u0 = xa - (T)i, v0 = ya - (T)j;                   // local offsets of the segment origin in the cell
    if (cnt == 3) {
        const int miss = __ffs(~m & 0xFu) - 1;
        const int e = miss >> 1, f = miss & 1;
        const int su = 1 - 2 * e, sv = 1 - 2 * f;             // h = su (u - e) + sv (v - f): 0 at the free corner, 1 on the hypotenuse
        const T coef = (T)su * dx + (T)sv * dy;
        const T rhs = (T)(1 + su * e + sv * f) - (T)su * u0 - (T)sv * v0;
        return n0 * coef > d0 * rhs || n1 * coef > d1 * rhs;
    }
    if (cnt == 2 && (m == 0x9u || m == 0x6u)) {
        T s0, s1;
        if (m == 0x9u) {                                      // corners (0,0)-(1,1): u - v
            const T k = dx - dy, c0 = u0 - v0;
            s0 = n0 * k + d0 * c0;
            s1 = n1 * k + d1 * c0;
        } else {                                              // corners (0,1)-(1,0): u + v - 1
            const T k = dx + dy, c0 = u0 + v0 - (T)1;
            s0 = n0 * k + d0 * c0;
            s1 = n1 * k + d1 * c0;
        }
        return (s0 > (T)0 && s1 < (T)0) || (s0 < (T)0 && s1 > (T)0);
    }
    return false;
}

// Is the segment A -> Z visible?  Every loop is bounded by H + W + 8 steps.  (Per-lane state is kept in integers and the loops
// have one exit: every live per-lane bool would otherwise hold a 64-bit exec mask in SGPRs, and the walk would spill them.)
template <typename T>
__device__ bool nav_visible(const NavGrid& g, T ar, T ac, T zr, T zc) {
    const int sr = zr >= ar ? 1 : -1, sc = zc >= ac ? 1 : -1;
    const T xa = sr > 0 ? ar : -ar, xz = sr > 0 ? zr : -zr;
    const T ya = sc > 0 ? ac : -ac, yz = sc > 0 ? zc : -zc;
    const T dx = xz - xa, dy = yz - ya;
    const T dr = zr - ar, dc = zc - ac;                         // actual direction: the side of a neighbour is sign(d x offset)
    if (dx == (T)0 && dy == (T)0) return true;
    long long i = tfloor(xa), j = tfloor(ya);
    const int lattice = ((T)i == xa ? 1 : 0) | ((T)j == ya ? 2 : 0);
    const int guard = g.H + g.W + 8;
    // run state: bits 0-1 = sides seen on the current run of obstacle pixels, bit 2 = the last lattice point was an obstacle
    uint32_t run = (lattice == 3 && (pix_at(g, sr * i, sc * j) & kObs)) ? 4u : 0u;
    int blocked = 0, done = 0;

    if ((dx == (T)0 && (lattice & 1)) || (dy == (T)0 && (lattice & 2))) {
        // the segment lies on a grid line: edge pieces (rule (a) across the line) and lattice points (rule (c)), unit steps
        const int along_y = (dx == (T)0 && (lattice & 1)) ? 1 : 0;
        const long long fixed = along_y ? i : j;
        const T e = along_y ? yz : xz;
        const long long ax = along_y ? 0 : 1, ay = along_y ? 1 : 0;     // unit step along the line, local
        const long long ox = along_y ? 1 : 0, oy = along_y ? 0 : 1;     // unit step across it
        long long x = along_y ? fixed : i, y = along_y ? j : fixed;
        for (int it = 0; it < guard; ++it) {
            const uint32_t p0 = pix_at(g, sr * x, sc * y), p1 = pix_at(g, sr * (x + ax), sc * (y + ay));
            const uint32_t lo = pix_at(g, sr * (x - ox), sc * (y - oy)) | pix_at(g, sr * (x - ox + ax), sc * (y - oy + ay));
            const uint32_t hi = pix_at(g, sr * (x + ox), sc * (y + oy)) | pix_at(g, sr * (x + ox + ax), sc * (y + oy + ay));
            blocked = (p0 & p1 & lo & hi & kObs) ? 1 : 0;              // a bond with fills on both sides: interior to O
            const long long k1 = (along_y ? y : x) + 1;
            const int interior = (T)k1 < e ? 1 : 0;                     // (k1 == e: the far endpoint)
            if (interior && (p1 & kObs)) {
                run = ((run & 4u) ? (run & 3u) : 0u) | attach_sides<T>(p1, dr, dc) | 4u;
                blocked |= (run & 3u) == 3u ? 1 : 0;
            } else {
                run = 0;
            }
            x += ax;
            y += ay;
            done = interior ? 0 : 1;
            if (blocked | done) break;
        }
        return done && !blocked;
    }

    long long px = i, py = j;
    T n0 = (T)0, d0 = (T)1;
    for (int it = 0; it < guard; ++it) {
        const int rv = (T)(i + 1) < xz ? 1 : 0, cv = (T)(j + 1) < yz ? 1 : 0;
        const T nr = (T)(i + 1) - xa, nc = (T)(j + 1) - ya;
        const T A = nr * dy, B = nc * dx;
        // 0 end, 1 row line, 2 column line, 3 lattice point
        const int ev = (rv && cv) ? (A < B ? 1 : (B < A ? 2 : 3)) : (rv ? 1 : (cv ? 2 : 0));
        const T n1 = ev == 0 ? (T)1 : (ev == 2 ? nc : nr), d1 = ev == 0 ? (T)1 : (ev == 2 ? dy : dx);
        blocked = cell_blocks<T>(g, sr, sc, i, j, xa, ya, dx, dy, n0, d0, n1, d1) ? 1 : 0;
        // the crossed edge: (i+1, j)-(i+1, j+1) for a row line, (i, j+1)-(i+1, j+1) for a column line
        const long long ex = ev == 2 ? i : i + 1, ey = ev == 1 ? j : j + 1;
        const uint32_t pe = pix_at(g, sr * ex, sc * ey), pf = pix_at(g, sr * (i + 1), sc * (j + 1));
        blocked |= ((ev == 1 || ev == 2) && (pe & pf & kObs)) ? 1 : 0;
        i += (ev & 1) ? 1 : 0;
        j += (ev & 2) ? 1 : 0;
        if (ev == 3 && (pf & kObs)) {
            const uint32_t cont = ((run & 4u) && i - px <= 1 && j - py <= 1) ? (run & 3u) : 0u;
            run = cont | attach_sides<T>(pf, dr, dc) | 4u;
            blocked |= (run & 3u) == 3u ? 1 : 0;
            px = i;
            py = j;
        } else {
            run = 0;
        }
        n0 = n1;
        d0 = d1;
        done = ev == 0 ? 1 : 0;
        if (blocked | done) break;
    }
    return done && !blocked;                                    // (a walk has at most H + W events: the guard never ends it)
}

// ----------------------------------------------------------------------------------------------- vertices
__global__ __launch_bounds__(256) void nav_pix_kernel(const uint8_t* __restrict__ obs, int H, int W, uint16_t* __restrict__ pix) {
    const int64_t n = (int64_t)(H + 2) * (W + 2);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(t / (W + 2)) - 1, c = (int)(t % (W + 2)) - 1;
        uint32_t p = 0;
        if (r >= 0 && r < H && c >= 0 && c < W && obs[(size_t)r * W + c] == 0) p |= kObs;
        for (int k = 0; k < 8; ++k) {
            const int rr = r + nb_dr(k), cc = c + nb_dc(k);
            if (rr >= 0 && rr < H && cc >= 0 && cc < W && obs[(size_t)rr * W + cc] == 0) p |= 1u << k;
        }
        pix[t] = (uint16_t)p;
    }
}

// pass 1: vertices per block of kNavScanThreads * kNavScanRounds raster-consecutive pixels
__global__ __launch_bounds__(kNavScanThreads) void nav_vertex_count_kernel(const uint16_t* __restrict__ pix, int H, int W,
                                                                           int32_t* __restrict__ counts) {
    __shared__ int s_w[kNavScanThreads / kWave];
    const int64_t n = (int64_t)H * W;
    const int64_t base = (int64_t)blockIdx.x * kNavScanThreads * kNavScanRounds;
    int cnt = 0;
    for (int k = 0; k < kNavScanRounds; ++k) {
        const int64_t t = base + (int64_t)k * kNavScanThreads + threadIdx.x;
        bool v = false;
        if (t < n) v = is_vertex(pix[(size_t)(t / W + 1) * (W + 2) + (size_t)(t % W + 1)]);
        cnt += __popcll(__ballot(v));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kNavScanThreads / kWave; ++w) s += s_w[w];
        counts[blockIdx.x] = s;
    }
}

// pass 2 is avl_scan.h's scan_counts_kernel: the block counts become exclusive offsets in place, the total goes to counts[nb]
// pass 3: write the vertices in raster order (ballot prefix inside a round, wave totals through LDS, the block's scanned offset)
__global__ __launch_bounds__(kNavScanThreads) void nav_vertex_write_kernel(const uint16_t* __restrict__ pix, int H, int W,
                                                                           const int32_t* __restrict__ offsets, int64_t V,
                                                                           int32_t* __restrict__ verts) {
    __shared__ int s_w[kNavScanThreads / kWave];
    const int64_t n = (int64_t)H * W;
    const int64_t base = (int64_t)blockIdx.x * kNavScanThreads * kNavScanRounds;
    int64_t run = offsets[blockIdx.x];
    for (int k = 0; k < kNavScanRounds; ++k) {
        const int64_t t = base + (int64_t)k * kNavScanThreads + threadIdx.x;
        bool v = false;
        if (t < n) v = is_vertex(pix[(size_t)(t / W + 1) * (W + 2) + (size_t)(t % W + 1)]);
        int total;
        const int64_t idx = run + block_compact_rank<kNavScanThreads / kWave>(v, s_w, &total);
        if (v && idx < V) {
            verts[2 * idx] = (int32_t)(t / W);
            verts[2 * idx + 1] = (int32_t)(t % W);
        }
        run += total;
        __syncthreads();                                        // s_w is rewritten by the next round
    }
}

// span of every vertex: its obstacle neighbours occupy the directions e1 .. e2 (counter-clockwise, at most 135 degrees);
// vspan[v] = e1 | e2 << 4
__global__ __launch_bounds__(256) void nav_span_kernel(NavGrid g, const int32_t* __restrict__ verts, int64_t V,
                                                      uint8_t* __restrict__ vspan) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t m = pix_at(g, verts[2 * v], verts[2 * v + 1]) & 0xFFu;
        const uint32_t mm = m | (m << 8) | (m << 16);
        uint32_t e1 = 0, e2 = 0;
        for (uint32_t k = 0; k < 8; ++k) {
            if (!((m >> k) & 1u)) continue;
            if (!((mm >> (k + 4)) & 0xFu)) e1 = k;                  // the 4 directions before k are free
            if (!((mm >> (k + 9)) & 0xFu)) e2 = k;                  // the 4 directions after k are free
        }
        vspan[v] = (uint8_t)(e1 | (e2 << 4));
    }
}

// Walls along the edges: for every vertex v and direction k with an obstacle neighbour, walk the run v, v + s, v + 2s, ... of
// obstacle pixels (s = the unit step of k) and record in vrun[8 v + k] the first step p at which the obstacle neighbours of
// run[0 .. p], off the line of k, have appeared on both sides of it (INT32_MAX: never on the run).  An edge leaving v along k for
// m >= p steps runs along a wall whose two sides it would join (see scan_node).
__global__ __launch_bounds__(256) void nav_run_kernel(NavGrid g, const int32_t* __restrict__ verts, int64_t V,
                                                     int32_t* __restrict__ vrun) {
    const int64_t n = V * 8;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = t >> 3;
        const int k = (int)(t & 7);
        const long long r0 = verts[2 * v], c0 = verts[2 * v + 1];
        const int sr = nb_dr(k), sc = nb_dc(k);
        int32_t first = INT32_MAX;
        if ((pix_at(g, r0, c0) >> k) & 1u) {
            uint32_t sides = 0;
            const int guard = g.H + g.W + 2;
            for (int p = 0; p < guard; ++p) {
                const uint32_t q = pix_at(g, r0 + (long long)p * sr, c0 + (long long)p * sc);
                if (!(q & kObs)) break;
                sides |= attach_sides<int>(q, sr, sc);
                if (sides == 3u) {
                    first = p;
                    break;
                }
            }
        }
        vrun[t] = first;
    }
}

// the neighbour index k of a unit step (sr, sc), -1 for (0, 0)
__device__ __forceinline__ int step_dir(int sr, int sc) {
    const int idx = (sr + 1) * 3 + (sc + 1);                            // NW N NE / W . E / SW S SE
    const int k = (int)((0x7650F4123ull >> (4 * idx)) & 0xFull);
    return k == 15 ? -1 : k;
}

// ----------------------------------------------------------------------------------------------- visibility
// One workgroup per 64 x 64 tile (row block p, column word q >= p) of the upper triangle; each of its 4 waves takes 16 rows a and
// evaluates the 64 pairs (a, 64 q + lane) with b > a, one lane each, and the ballot is bitset word (a, q).  The 64 targets of a
// wave are raster-consecutive vertices, so their segments from a have similar lengths and directions.
__global__ __launch_bounds__(256) void nav_visibility_kernel(NavGrid g, const int32_t* __restrict__ verts, int64_t V, int64_t W64,
                                                            unsigned long long* __restrict__ bits) {
    const int64_t p = blockIdx.y, q = blockIdx.x;
    if (q < p) return;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const int64_t b = q * 64 + lane;
    long long br = 0, bc = 0;
    if (b < V) {
        br = verts[2 * b];
        bc = verts[2 * b + 1];
    }
    for (int k = 0; k < 16; ++k) {
        const int64_t a = p * 64 + w * 16 + k;
        bool vis = false;
        // (the wave-uniform source goes through a lane shuffle so that the walk keeps it in VGPRs: in SGPRs it spills)
        const int ar = a < V ? __shfl(verts[2 * a], lane, kWave) : 0, ac = a < V ? __shfl(verts[2 * a + 1], lane, kWave) : 0;
        if (a < V && b < V && b > a) vis = nav_visible<long long>(g, ar, ac, br, bc);
        const unsigned long long word = __ballot(vis);
        if (lane == 0) bits[(size_t)a * W64 + q] = word;
    }
}

// lower triangle: word (64 q + k, p) = the transpose of the 64 x 64 bit block (rows 64 p .., word q); on the diagonal the
// transposed bits are merged with the row's own upper bits.  One wave per block, 64 ballots.
__global__ __launch_bounds__(64) void nav_mirror_kernel(int64_t W64, unsigned long long* __restrict__ bits) {
    const int64_t p = blockIdx.y, q = blockIdx.x;
    if (q < p) return;
    const int lane = threadIdx.x;
    const unsigned long long u = bits[(size_t)(p * 64 + lane) * W64 + q];
    unsigned long long out = 0;
    for (int k = 0; k < 64; ++k) {
        const unsigned long long t = __ballot((u >> k) & 1ull);
        if (lane == k) out = t;
    }
    if (q == p) out |= u;
    bits[(size_t)(q * 64 + lane) * W64 + p] = out;
}

// ----------------------------------------------------------------------------------------------- queries
// word w of query row k: vertices 64 w .. 64 w + 63 visible from query point k (walked from the query point to the vertex).
// Thread V of row 0 walks from the start to the goal into *sg.
__global__ __launch_bounds__(256) void nav_query_kernel(NavGrid g, const int32_t* __restrict__ verts, int64_t V, int64_t W64,
                                                       double q0r, double q0c, double q1r, double q1c,
                                                       unsigned long long* __restrict__ qbits, int32_t* __restrict__ sg) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int k = (int)blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1);
    const double qr = __shfl(k == 0 ? q0r : q1r, lane, kWave), qc = __shfl(k == 0 ? q0c : q1c, lane, kWave);   // VGPRs (see above)
    bool vis = false;
    if (t < V) vis = nav_visible<double>(g, qr, qc, (double)verts[2 * t], (double)verts[2 * t + 1]);
    else if (t == V && k == 0) sg[0] = nav_visible<double>(g, qr, qc, q1r, q1c) ? 1 : 0;
    const unsigned long long word = __ballot(vis);
    if (lane == 0 && t / 64 < W64) qbits[(size_t)k * W64 + t / 64] = word;
}

// ----------------------------------------------------------------------------------------------- shortest path
// nodes 0 .. V-1 = vertices, V = start (the source), V + 1 = goal
struct NavNodes {
    const int32_t* verts;
    int64_t V, W64;
    const unsigned long long* bits;   // V x W64 (rows padded to 64)
    const unsigned long long* qbits;  // 2 x W64: row 0 = visible from the start, row 1 = from the goal
    const int32_t* sg;                // start-goal visible
    const uint8_t* vspan;             // per vertex: the span of its obstacle neighbours (nav_span_kernel)
    const int32_t* vrun;              // per vertex and direction: the wall-crossing step of its run (nav_run_kernel)
    double sr, sc, gr, gc;
};

// Is the direction (dr, dc) leaving a vertex strictly inside the angular span of its obstacle neighbours?  A path that bends
// at a vertex enters and leaves it outside that span (the tangent condition); an edge inside it would let a path pass from one
// side of a thin wall to the other through the vertex.  Such edges are visible but not used by the shortest path.
__device__ __forceinline__ bool in_span(uint32_t span, double dr, double dc) {
    const int e1 = span & 7, e2 = (span >> 4) & 7;
    const double ar = nb_dr(e1), ac = nb_dc(e1), br = nb_dr(e2), bc = nb_dc(e2);
    return ar * dc - ac * dr > 0.0 && dr * bc - dc * br > 0.0;
}

// Does the edge leaving vertex v by (dr, dc) run along a wall that has obstacle neighbours on both sides of it within the edge?
// A path that bends at v stays on the side away from v's neighbours (the tangent condition); along such a wall it would come out
// on the other side.  Only edges along one of the 8 unit steps can run along a wall.
__device__ __forceinline__ bool along_wall(const NavNodes& G, int64_t v, double dr, double dc) {
    const double ar = fabs(dr), ac = fabs(dc);
    if (!(dr == 0.0 || dc == 0.0 || ar == ac)) return false;
    const int k = step_dir(dr > 0.0 ? 1 : (dr < 0.0 ? -1 : 0), dc > 0.0 ? 1 : (dc < 0.0 ? -1 : 0));
    if (k < 0) return false;
    const double m = floor(fmax(ar, ac));                               // the unit steps of the edge
    return (double)G.vrun[8 * v + k] <= m;
}

// an edge is used by the shortest path only where it leaves each vertex end tangentially and not along a wall it would cross
__device__ __forceinline__ bool usable_end(const NavNodes& G, int64_t v, uint32_t span, double dr, double dc) {
    return !in_span(span, dr, dc) && !along_wall(G, v, dr, dc);
}

__device__ __forceinline__ double edge_len(double ar, double ac, double br, double bc) {
    const double dr = br - ar, dc = bc - ac;
    return sqrt(dr * dr + dc * dc);
}

__device__ __forceinline__ void node_pos(const NavNodes& G, int64_t v, double& r, double& c) {
    if (v < G.V) {
        r = (double)G.verts[2 * v];
        c = (double)G.verts[2 * v + 1];
    } else if (v == G.V) {
        r = G.sr;
        c = G.sc;
    } else {
        r = G.gr;
        c = G.gc;
    }
}

// Walk the in-neighbours of v in increasing id order: fn(u, word_bit_set) over vertex words, then start, then goal.
// MODE 0: the minimum of dist[u] + |uv|; MODE 1: the smallest u that attains dist[v].
template <int MODE>
__device__ __forceinline__ int64_t scan_node(const NavNodes& G, const double* __restrict__ dist, int64_t v, double target, double& best) {
    const int lane = threadIdx.x & (kWave - 1);
    double vr, vc;
    node_pos(G, v, vr, vc);
    best = INFINITY;
    const unsigned long long* row = nullptr;
    if (v < G.V) row = G.bits + (size_t)v * G.W64;
    else if (v == G.V + 1) row = G.qbits + G.W64;
    const uint32_t vspan = v < G.V ? G.vspan[v] : 0u;       // (e1 == e2 == 0 for the start and the goal: no span)
    if (row) {
        for (int64_t w = 0; w < G.W64; ++w) {
            const unsigned long long word = row[w];
            if (word == 0ull) continue;
            const int64_t u = w * 64 + lane;
            double cand = INFINITY;
            if ((word >> lane) & 1ull) {
                const double du = dist[u];
                const double ur = (double)G.verts[2 * u], uc = (double)G.verts[2 * u + 1];
                const bool tangent = usable_end(G, u, G.vspan[u], vr - ur, vc - uc) && (v >= G.V || usable_end(G, v, vspan, ur - vr, uc - vc));
                if (du < INFINITY && tangent) cand = du + edge_len(ur, uc, vr, vc);
            }
            if (MODE == 0) {
                best = fmin(best, cand);
            } else {
                const unsigned long long hit = __ballot(cand == target);
                if (hit) return w * 64 + (__ffsll((long long)hit) - 1);
            }
        }
    }
    // the start (id V) and the goal (id V + 1) as neighbours of v
    if (v != G.V) {
        const bool s_vis = v < G.V ? ((G.qbits[v / 64] >> (v % 64)) & 1ull) : (G.sg[0] != 0);
        if (s_vis && (v >= G.V || usable_end(G, v, vspan, G.sr - vr, G.sc - vc))) {
            const double cand = dist[G.V] + edge_len(G.sr, G.sc, vr, vc);
            if (MODE == 0) best = fmin(best, cand);
            else if (cand == target) return G.V;
        }
    }
    if (v < G.V && ((G.qbits[G.W64 + v / 64] >> (v % 64)) & 1ull) && usable_end(G, v, vspan, G.gr - vr, G.gc - vc)) {
        const double dg = dist[G.V + 1];
        if (dg < INFINITY) {
            const double cand = dg + edge_len(G.gr, G.gc, vr, vc);
            if (MODE == 0) best = fmin(best, cand);
            else if (cand == target) return G.V + 1;
        }
    }
    return -1;
}

__global__ __launch_bounds__(256) void nav_init_kernel(int64_t N, int64_t src, double* __restrict__ d0, double* __restrict__ d1) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < N; t += (int64_t)gridDim.x * blockDim.x) {
        d0[t] = t == src ? 0.0 : INFINITY;
        d1[t] = t == src ? 0.0 : INFINITY;
    }
}

// one synchronous round: dist_out[v] = min over in-neighbours u of dist_in[u] + |uv| (the start stays 0); one wave per node.
// flags[k] = 1 when some node changed.  A round whose predecessor changed nothing returns at once: both buffers are then equal.
__global__ __launch_bounds__(256) void nav_round_kernel(NavNodes G, const double* __restrict__ din, double* __restrict__ dout,
                                                       int32_t* __restrict__ flags, int64_t k) {
    if (k > 0 && flags[k - 1] == 0) return;
    const int64_t v = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int64_t N = G.V + 2;
    if (v >= N) return;
    double best = 0.0;
    if (v != G.V) {
        scan_node<0>(G, din, v, 0.0, best);
        best = wave_min(best);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        dout[v] = best;
        if (best != din[v]) flags[k] = 1;
    }
}

// predecessor of every reached node: the smallest id u with dist[u] + |uv| == dist[v]; -1 for the start and unreached nodes
__global__ __launch_bounds__(256) void nav_pred_kernel(NavNodes G, const double* __restrict__ dist, int32_t* __restrict__ pred) {
    const int64_t v = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int64_t N = G.V + 2;
    if (v >= N) return;
    int64_t u = -1;
    const double dv = dist[v];
    if (v != G.V && dv < INFINITY) {
        double dummy;
        u = scan_node<1>(G, dist, v, dv, dummy);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) pred[v] = (int32_t)u;
}

// ----------------------------------------------------------------------------------------------- many goals
// One wave per goal against the finished shortest-path tree `dist` of the start (the goal node took no part in it):
//   out_dist[k] = min(fl(dist[u] + |u g_k|) over vertices u that see g_k, dist[u] finite, usable_end at u; |s g_k| if the start sees it)
//   out_via[k]  = the node nav_pred_kernel would pick for the goal: the smallest vertex id attaining the minimum, else V (the
//                 start); -1 with +inf when nothing reaches the goal.
// The lanes hold 64 raster-consecutive vertices and the words are visited in ascending id order.  A lane walks to the goal only
// when its candidate can still win: strictly below the best so far, or equal to it while the best is the start's (a vertex beats
// the start on a tie; an equal vertex with a larger id never wins).  The walk runs from the goal to the vertex in float64, as
// nav_query_kernel's; the start-goal walk runs from the start.  walks[0] / walks[1] count the lanes that walked / had a finite
// candidate (integer atomics, for the probe only; null = not counted).
__global__ __launch_bounds__(256) void nav_goals_kernel(NavGrid g, NavNodes G, const double* __restrict__ dist,
                                                       const double* __restrict__ goals, int64_t M, double* __restrict__ out_dist,
                                                       int32_t* __restrict__ out_via, unsigned long long* __restrict__ walks) {
    const int64_t k = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (k >= M) return;
    const int lane = threadIdx.x & (kWave - 1);
    // (wave-uniform points go through a lane shuffle so that the walk keeps them in VGPRs, see nav_visibility_kernel)
    const double gr = __shfl(goals[2 * k], lane, kWave), gc = __shfl(goals[2 * k + 1], lane, kWave);
    const double sr = __shfl(G.sr, lane, kWave), sc = __shfl(G.sc, lane, kWave);
    // the start's candidate is kept apart from the vertices': a vertex needs best <= the start's (it wins that tie), and a strictly
    // smaller value than every vertex before it
    const int s_vis = nav_visible<double>(g, sr, sc, gr, gc) ? 1 : 0;
    const double s_best = s_vis ? dist[G.V] + edge_len(sr, sc, gr, gc) : INFINITY;
    double best = INFINITY;
    int via = -1;
    unsigned long long n_walk = 0, n_cand = 0;
    for (int64_t w = 0; w < G.W64; ++w) {
        const int64_t u = w * 64 + lane;
        double cand = INFINITY;
        double ur = 0.0, uc = 0.0;
        if (u < G.V) {
            const double du = dist[u];
            ur = (double)G.verts[2 * u];
            uc = (double)G.verts[2 * u + 1];
            if (du < INFINITY && usable_end(G, u, G.vspan[u], gr - ur, gc - uc)) cand = du + edge_len(ur, uc, gr, gc);
        }
        const int need = (cand < best && cand <= s_best) ? 1 : 0;
        if (walks) {
            n_cand += (unsigned long long)__popcll(__ballot(cand < INFINITY));
            n_walk += (unsigned long long)__popcll(__ballot(need));
        }
        if (!__ballot(need)) continue;
        int vis = 0;
        if (need) vis = nav_visible<double>(g, gr, gc, ur, uc) ? 1 : 0;
        const double m = wave_min(vis ? cand : INFINITY);
        if (m < best) {
            const unsigned long long hit = __ballot(vis && cand == m);
            best = m;
            via = (int)(w * 64) + (__ffsll((long long)hit) - 1);
        }
    }
    if (lane == 0) {
        const int by_vertex = via >= 0 ? 1 : 0;
        out_dist[k] = by_vertex ? best : s_best;
        out_via[k] = by_vertex ? via : (s_vis ? (int)G.V : -1);
        if (walks) {
            atomicAdd(&walks[0], n_walk);
            atomicAdd(&walks[1], n_cand);
        }
    }
}

// Is any cell of the map free?  (snapping needs one; asked once per graph)
__global__ __launch_bounds__(256) void nav_any_free_kernel(const uint16_t* __restrict__ pix, int H, int W, int32_t* __restrict__ flag) {
    const int64_t n = (int64_t)H * W;
    int any = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        any |= (pix[(size_t)(t / W + 1) * (W + 2) + (size_t)(t % W + 1)] & kObs) ? 0 : 1;
    if (__ballot(any) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(flag, 1);
}

// navigation_utils._in_obstacle + _nearest_free, one thread per point.  A point is inside the obstacle set when its int() cell is an
// obstacle, or when it lies strictly beyond the hypotenuse of the triangle fill whose free corner is that cell.  Such a point moves
// to the free cell with the smallest fl(fl(a * a) + fl(b * b)), a = fl(r - pr), b = fl(c - pc) (NumPy's float64 expression), the
// first in raster order on ties.  The search goes outward over the square rings round the int() cell (fr, fc): a cell of ring d has
// |r - pr| >= d - 1 or |c - pc| >= d - 1, d - 1 and its square are exact in float64 and rounding is monotone, so its value is at
// least (d - 1)^2; the search stops at the first ring whose bound exceeds the best value found (a cell further out neither beats
// nor ties it).  The map holds a free cell (checked by the host), so the search ends.
__global__ __launch_bounds__(256) void nav_snap_kernel(NavGrid g, const double* __restrict__ pts, int64_t M, double* __restrict__ out,
                                                      uint8_t* __restrict__ moved) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    const double pr = pts[2 * t], pc = pts[2 * t + 1];
    const int fr = (int)pr, fc = (int)pc;                               // points lie in [0, H - 1] x [0, W - 1]: int() = floor
    const uint32_t p = pix_at(g, fr, fc);
    int inside = (p & kObs) ? 1 : 0;
    if (!inside && pr != (double)fr && pc != (double)fc && fr + 1 < g.H && fc + 1 < g.W && (p & 1u) && (p & 0x40u) && (p & 0x80u))
        inside = (pr - (double)fr) + (pc - (double)fc) > 1.0 ? 1 : 0;   // E, S and SE are obstacles: the hypotenuse is u + v = 1
    double orr = pr, occ = pc;
    if (inside) {
        double best = INFINITY;
        int br = 0, bc = 0;
        const int dmax = max(max(fr, g.H - 1 - fr), max(fc, g.W - 1 - fc));
        if (!(p & kObs)) {                                              // ring 0, inside a fill: the free corner (fr, fc) itself
            const double a = (double)fr - pr, b = (double)fc - pc;
            best = a * a + b * b;
            br = fr;
            bc = fc;
        }
        for (int d = 1; d <= dmax; ++d) {
            const double lo = (double)(d - 1) * (double)(d - 1);
            if (lo > best) break;
            const int r0 = fr - d, r1 = fr + d, c0 = fc - d, c1 = fc + d;
            for (int r = max(r0, 0); r <= min(r1, g.H - 1); ++r) {
                const int full = (r == r0 || r == r1) ? 1 : 0;          // the ring's top and bottom rows; else its two side cells
                const int ca = full ? max(c0, 0) : c0, cb = full ? min(c1, g.W - 1) : c1, step = full ? 1 : c1 - c0;
                for (int c = ca; c <= cb; c += step) {
                    if (c < 0 || c >= g.W || (pix_at(g, r, c) & kObs)) continue;
                    const double a = (double)r - pr, b = (double)c - pc;
                    const double d2 = a * a + b * b;
                    if (d2 < best || (d2 == best && (r < br || (r == br && c < bc)))) {
                        best = d2;
                        br = r;
                        bc = c;
                    }
                }
            }
        }
        orr = (double)br;
        occ = (double)bc;
    }
    out[2 * t] = orr;
    out[2 * t + 1] = occ;
    moved[t] = (uint8_t)inside;
}

static unsigned nav_blocks(int64_t n, int threads) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + threads - 1) / threads, (int64_t)num_cus() * 16));
}

}  // namespace avl

using namespace avl;

struct AvlNavGraph {
    int H = 0, W = 0;
    int64_t V = 0, W64 = 0;
    uint16_t* pix = nullptr;
    int32_t* verts = nullptr;
    unsigned long long* bits = nullptr;
    unsigned long long* qbits = nullptr;
    int32_t* sg = nullptr;
    double* dist = nullptr;            // 2 x (V + 2)
    int32_t* flags = nullptr;          // V + 4
    int32_t* pred = nullptr;           // V + 2
    uint8_t* vspan = nullptr;          // V
    int32_t* vrun = nullptr;           // 8 V
    int planned = 0;
    double q[4] = {0, 0, 0, 0};
    int last_buf = 0;
    // many goals (avl_navmany_*): buffers of their own, so that avl_nav_last_plan keeps describing the last single plan
    unsigned long long* m_qbits = nullptr;   // 2 x W64: row 0 = visible from the start, row 1 = all zero (no goal node)
    int32_t* m_sg = nullptr;                 // 0: the goal node is not connected
    double* m_dist = nullptr;                // 2 x (V + 2): the tree of the last batch's start
    int32_t* m_flags = nullptr;              // V + 4
    int32_t* m_pred = nullptr;               // V + 2
    unsigned long long* m_walks = nullptr;   // 2 counters of the last batch: walks started, finite candidates
    double* m_goals = nullptr;               // 2 x m_cap points (goals of a batch, or the points of a snap)
    double* m_out = nullptr;                 // 2 x m_cap: per-goal distances (first m_cap), or the snapped points
    int32_t* m_via = nullptr;                // m_cap
    uint8_t* m_moved = nullptr;              // m_cap
    int32_t* m_free = nullptr;               // 1: the map has a free cell
    int64_t m_cap = 0;
    int free_known = 0, has_free = 0;
    int many_planned = 0;
    int64_t many_M = 0;
    int32_t* h_many_pred = nullptr;          // host copies for avl_navmany_path: the tree's predecessors and via[] of the last batch
    int32_t* h_many_via = nullptr;
    int64_t h_many_via_cap = 0;
    unsigned long long many_walks[2] = {0, 0};
    int count_walks = 0;                     // avl_navmany_count_walks: batches count their walks (off: the kernel gets no counters)
    int many_counted = 0;                    // the last batch counted
};

static void nav_free(AvlNavGraph* g) {
    if (!g) return;
    void* ptrs[] = {g->pix,     g->verts,  g->bits,   g->qbits,   g->sg,      g->dist,  g->flags, g->pred,  g->vspan,   g->vrun,
                    g->m_qbits, g->m_sg,   g->m_dist, g->m_flags, g->m_pred,  g->m_walks, g->m_goals, g->m_out, g->m_via, g->m_moved,
                    g->m_free};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete[] g->h_many_pred;
    delete[] g->h_many_via;
    delete g;
}

#define NAV_TRY(expr)                  \
    do {                               \
        const int _rc = (expr);        \
        if (_rc != AVL_OK) {           \
            nav_free(g);               \
            return _rc;                \
        }                              \
    } while (0)

static int nav_alloc(void** p, size_t bytes) {
    AVL_HIP_CHECK(hipMalloc(p, std::max<size_t>(bytes, 8)));
    return AVL_OK;
}

static int nav_build(AvlNavGraph* g, const uint8_t* h_obs, hipStream_t st) {
    const int H = g->H, W = g->W;
    const int64_t n = (int64_t)H * W;
    uint8_t* d_obs = nullptr;
    int32_t* d_counts = nullptr;
    const int64_t per_block = (int64_t)kNavScanThreads * kNavScanRounds;
    const int nb = (int)((n + per_block - 1) / per_block);
    int rc = AVL_OK;
    int32_t total = 0;
    do {
        if ((rc = nav_alloc((void**)&d_obs, (size_t)n)) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&d_counts, sizeof(int32_t) * (size_t)(nb + 1))) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&g->pix, sizeof(uint16_t) * (size_t)(H + 2) * (size_t)(W + 2))) != AVL_OK) break;
        hipError_t e = hipMemcpyAsync(d_obs, h_obs, (size_t)n, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) {
            set_error("avl_nav_create: upload failed: %s", hipGetErrorString(e));
            rc = AVL_ERR_HIP;
            break;
        }
        hipLaunchKernelGGL(nav_pix_kernel, dim3(nav_blocks((int64_t)(H + 2) * (W + 2), 256)), dim3(256), 0, st, d_obs, H, W, g->pix);
        hipLaunchKernelGGL(nav_vertex_count_kernel, dim3(nb), dim3(kNavScanThreads), 0, st, g->pix, H, W, d_counts);
        hipLaunchKernelGGL((scan_counts_kernel<256, int32_t, int32_t, OpSum>), dim3(1), dim3(256), 0, st, (const int32_t*)d_counts, (int64_t)nb,
                           d_counts, d_counts + nb, OpSum{}, 0);
        e = hipMemcpyAsync(&total, d_counts + nb, sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            set_error("avl_nav_create: vertex pass failed: %s", hipGetErrorString(e));
            rc = AVL_ERR_HIP;
            break;
        }
        if (total > kNavMaxVertices) {
            set_error("avl_nav_create: the map has %d path vertices, above the cap of %lld (a %lld-bit visibility bitset)", (int)total,
                      (long long)kNavMaxVertices, (long long)(kNavMaxVertices * kNavMaxVertices));
            rc = AVL_ERR_CAPACITY;
            break;
        }
        g->V = total;
        g->W64 = (total + 63) / 64;
        const int64_t Vpad = g->W64 * 64, N = g->V + 2;
        if ((rc = nav_alloc((void**)&g->verts, sizeof(int32_t) * 2 * (size_t)std::max<int64_t>(g->V, 1))) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&g->bits, sizeof(unsigned long long) * (size_t)std::max<int64_t>(Vpad * g->W64, 1))) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&g->qbits, sizeof(unsigned long long) * 2 * (size_t)std::max<int64_t>(g->W64, 1))) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&g->sg, sizeof(int32_t))) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&g->dist, sizeof(double) * 2 * (size_t)N)) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&g->flags, sizeof(int32_t) * (size_t)(N + 2))) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&g->pred, sizeof(int32_t) * (size_t)N)) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&g->vspan, (size_t)g->V)) != AVL_OK) break;
        if ((rc = nav_alloc((void**)&g->vrun, sizeof(int32_t) * 8 * (size_t)g->V)) != AVL_OK) break;
        hipLaunchKernelGGL(nav_vertex_write_kernel, dim3(nb), dim3(kNavScanThreads), 0, st, g->pix, H, W, d_counts, g->V, g->verts);
        if (g->V > 0) {
            hipLaunchKernelGGL(nav_span_kernel, dim3(nav_blocks(g->V, 256)), dim3(256), 0, st, NavGrid{g->pix, H, W}, g->verts, g->V, g->vspan);
            hipLaunchKernelGGL(nav_run_kernel, dim3(nav_blocks(8 * g->V, 256)), dim3(256), 0, st, NavGrid{g->pix, H, W}, g->verts, g->V, g->vrun);
        }
        if (g->V > 0) {
            e = hipMemsetAsync(g->bits, 0, sizeof(unsigned long long) * (size_t)(Vpad * g->W64), st);
            if (e != hipSuccess) {
                set_error("avl_nav_create: memset failed: %s", hipGetErrorString(e));
                rc = AVL_ERR_HIP;
                break;
            }
            const NavGrid grid{g->pix, H, W};
            const dim3 tiles((unsigned)g->W64, (unsigned)g->W64);
            hipLaunchKernelGGL(nav_visibility_kernel, tiles, dim3(256), 0, st, grid, g->verts, g->V, g->W64, g->bits);
            hipLaunchKernelGGL(nav_mirror_kernel, tiles, dim3(64), 0, st, g->W64, g->bits);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);     // the temporaries die here
        if (e != hipSuccess) {
            set_error("avl_nav_create: graph kernels failed: %s", hipGetErrorString(e));
            rc = AVL_ERR_HIP;
            break;
        }
    } while (0);
    if (rc != AVL_OK) (void)hipStreamSynchronize(st);
    if (d_obs) (void)hipFree(d_obs);
    if (d_counts) (void)hipFree(d_counts);
    return rc;
}

extern "C" int avl_nav_create(const uint8_t* h_obs, int H, int W, void* stream, void** h_graph) {
    AVL_REQUIRE(h_graph, "avl_nav_create: null handle pointer");
    *h_graph = nullptr;
    AVL_REQUIRE(h_obs, "avl_nav_create: null obstacle map");
    AVL_REQUIRE(H > 0 && W > 0 && H <= kNavMaxSide && W <= kNavMaxSide, "avl_nav_create: bad map size %d x %d (1 .. %d per side)", H,
                W, kNavMaxSide);
    AvlNavGraph* g = new (std::nothrow) AvlNavGraph();
    AVL_REQUIRE(g, "avl_nav_create: out of host memory");
    g->H = H;
    g->W = W;
    NAV_TRY(nav_build(g, h_obs, as_stream(stream)));
    *h_graph = g;
    return AVL_OK;
}

extern "C" int avl_nav_destroy(void* graph) {
    nav_free(static_cast<AvlNavGraph*>(graph));
    return AVL_OK;
}

extern "C" int avl_nav_num_vertices(void* graph, int64_t* h_V) {
    AVL_REQUIRE(graph && h_V, "avl_nav_num_vertices: null pointer");
    *h_V = static_cast<AvlNavGraph*>(graph)->V;
    return AVL_OK;
}

extern "C" int avl_nav_vertices(void* graph, int32_t* h_verts, void* stream) {
    AVL_REQUIRE(graph, "avl_nav_vertices: null handle");
    AvlNavGraph* g = static_cast<AvlNavGraph*>(graph);
    if (g->V == 0) return AVL_OK;
    AVL_REQUIRE(h_verts, "avl_nav_vertices: null output");
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemcpyAsync(h_verts, g->verts, sizeof(int32_t) * 2 * (size_t)g->V, hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    return AVL_OK;
}

extern "C" int avl_nav_export_visibility(void* graph, uint64_t* h_bits, void* stream) {
    AVL_REQUIRE(graph, "avl_nav_export_visibility: null handle");
    AvlNavGraph* g = static_cast<AvlNavGraph*>(graph);
    if (g->V == 0) return AVL_OK;
    AVL_REQUIRE(h_bits, "avl_nav_export_visibility: null output");
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemcpyAsync(h_bits, g->bits, sizeof(uint64_t) * (size_t)(g->V * g->W64), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    return AVL_OK;
}

// The rounds of the shortest path from node V over `nodes` (d0, d1: the two initialised distance buffers, flags: zeroed), then the
// predecessors.  After it both buffers hold the distances.
static int nav_relax(const NavNodes& nodes, double* d0, double* d1, int32_t* flags, int32_t* pred, const char* who, hipStream_t st) {
    const int64_t N = nodes.V + 2;
    const unsigned nblk = (unsigned)((N + 3) / 4);
    // a shortest path has at most N - 1 edges, so round N - 1 changes nothing: at most N + 1 rounds
    int64_t k = 0;
    bool converged = false;
    while (k <= N && !converged) {
        const int64_t k1 = std::min<int64_t>(k + kNavRoundBatch, N + 1);
        for (; k < k1; ++k) {
            const double* din = (k & 1) ? d1 : d0;
            double* dout = (k & 1) ? d0 : d1;
            hipLaunchKernelGGL(nav_round_kernel, dim3(nblk), dim3(256), 0, st, nodes, din, dout, flags, k);
        }
        AVL_HIP_CHECK(hipGetLastError());
        int32_t last = 1;
        AVL_HIP_CHECK(hipMemcpyAsync(&last, flags + (k - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
        AVL_HIP_CHECK(hipStreamSynchronize(st));
        converged = last == 0;
    }
    if (!converged) {
        set_error("%s: the relaxation did not converge in %lld rounds", who, (long long)(N + 1));
        return AVL_ERR_STATE;
    }
    // after a round that changed nothing both buffers hold the same distances
    hipLaunchKernelGGL(nav_pred_kernel, dim3(nblk), dim3(256), 0, st, nodes, d0, pred);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

extern "C" int avl_nav_plan(void* graph, double sr, double sc, double gr, double gc, double* h_dist, int32_t* h_path, int* h_len,
                            int cap, void* stream) {
    AVL_REQUIRE(graph && h_dist && h_len, "avl_nav_plan: null pointer");
    AvlNavGraph* g = static_cast<AvlNavGraph*>(graph);
    *h_len = 0;
    *h_dist = INFINITY;
    const double q[4] = {sr, sc, gr, gc};
    for (int k = 0; k < 4; ++k) AVL_REQUIRE(std::isfinite(q[k]), "avl_nav_plan: start and goal must be finite");
    AVL_REQUIRE(sr >= 0.0 && sr <= g->H - 1 && gr >= 0.0 && gr <= g->H - 1 && sc >= 0.0 && sc <= g->W - 1 && gc >= 0.0 && gc <= g->W - 1,
                "avl_nav_plan: start (%g, %g) or goal (%g, %g) outside the %d x %d map", sr, sc, gr, gc, g->H, g->W);
    AVL_REQUIRE(cap >= 0 && (cap == 0 || h_path), "avl_nav_plan: bad path buffer");
    hipStream_t st = as_stream(stream);
    const NavGrid grid{g->pix, g->H, g->W};
    const int64_t V = g->V, N = V + 2;
    hipLaunchKernelGGL(nav_query_kernel, dim3((unsigned)(V / 256 + 1), 2), dim3(256), 0, st, grid, g->verts, V, g->W64, sr, sc, gr, gc,
                       g->qbits, g->sg);
    double* d0 = g->dist;
    double* d1 = g->dist + N;
    hipLaunchKernelGGL(nav_init_kernel, dim3(nav_blocks(N, 256)), dim3(256), 0, st, N, V, d0, d1);
    AVL_HIP_CHECK(hipMemsetAsync(g->flags, 0, sizeof(int32_t) * (size_t)(N + 2), st));
    AVL_HIP_CHECK(hipGetLastError());
    const NavNodes nodes{g->verts, V, g->W64, g->bits, g->qbits, g->sg, g->vspan, g->vrun, sr, sc, gr, gc};
    const int rrc = nav_relax(nodes, d0, d1, g->flags, g->pred, "avl_nav_plan", st);
    if (rrc != AVL_OK) return rrc;
    int32_t* pred = new (std::nothrow) int32_t[(size_t)N];
    AVL_REQUIRE(pred, "avl_nav_plan: out of host memory");
    double dgoal = INFINITY;
    hipError_t e = hipMemcpyAsync(pred, g->pred, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&dgoal, d0 + V + 1, sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        delete[] pred;
        set_error("avl_nav_plan: readback failed: %s", hipGetErrorString(e));
        return AVL_ERR_HIP;
    }
    g->planned = 1;
    for (int i = 0; i < 4; ++i) g->q[i] = q[i];
    int rc = AVL_OK;
    *h_dist = dgoal;
    if (dgoal < INFINITY) {
        // goal -> start along the predecessors (distances strictly decrease: at most N nodes), then reversed
        int64_t len = 0, v = V + 1;
        for (; v >= 0 && len <= N; v = pred[v]) {
            if (len < cap) h_path[len] = (int32_t)v;
            ++len;
            if (v == V) break;
        }
        if (v != V) {
            set_error("avl_nav_plan: the predecessor chain of the goal does not reach the start");
            rc = AVL_ERR_STATE;
        } else if (len > cap) {
            set_error("avl_nav_plan: the path has %lld nodes, the buffer %d", (long long)len, cap);
            rc = AVL_ERR_INVALID;
        } else {
            std::reverse(h_path, h_path + len);
            *h_len = (int)len;
        }
    }
    delete[] pred;
    return rc;
}

extern "C" int avl_nav_last_plan(void* graph, double* h_dist, int32_t* h_pred, uint64_t* h_qbits, int32_t* h_sg, void* stream) {
    AVL_REQUIRE(graph, "avl_nav_last_plan: null handle");
    AvlNavGraph* g = static_cast<AvlNavGraph*>(graph);
    if (!g->planned) {
        set_error("avl_nav_last_plan: no plan has run on this graph");
        return AVL_ERR_STATE;
    }
    hipStream_t st = as_stream(stream);
    const int64_t N = g->V + 2;
    if (h_dist) AVL_HIP_CHECK(hipMemcpyAsync(h_dist, g->dist, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, st));
    if (h_pred) AVL_HIP_CHECK(hipMemcpyAsync(h_pred, g->pred, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost, st));
    if (h_qbits && g->W64)
        AVL_HIP_CHECK(hipMemcpyAsync(h_qbits, g->qbits, sizeof(uint64_t) * 2 * (size_t)g->W64, hipMemcpyDeviceToHost, st));
    if (h_sg) AVL_HIP_CHECK(hipMemcpyAsync(h_sg, g->sg, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    return AVL_OK;
}

// ----------------------------------------------------------------------------------------------- many goals: entry points
constexpr int64_t kNavManyMax = (int64_t)1 << 20;

// the per-point buffers of a batch or a snap, grown to M points (never shrunk)
static int navmany_reserve(AvlNavGraph* g, int64_t M) {
    if (M <= g->m_cap) return AVL_OK;
    int64_t cap = std::max<int64_t>(g->m_cap * 2, 1024);
    while (cap < M) cap *= 2;
    cap = std::min<int64_t>(cap, kNavManyMax);
    void** bufs[] = {(void**)&g->m_goals, (void**)&g->m_out, (void**)&g->m_via, (void**)&g->m_moved};
    for (void** b : bufs) {
        if (*b) (void)hipFree(*b);
        *b = nullptr;
    }
    g->m_cap = 0;
    int rc;
    if ((rc = nav_alloc((void**)&g->m_goals, sizeof(double) * 2 * (size_t)cap)) != AVL_OK) return rc;
    if ((rc = nav_alloc((void**)&g->m_out, sizeof(double) * 2 * (size_t)cap)) != AVL_OK) return rc;
    if ((rc = nav_alloc((void**)&g->m_via, sizeof(int32_t) * (size_t)cap)) != AVL_OK) return rc;
    if ((rc = nav_alloc((void**)&g->m_moved, (size_t)cap)) != AVL_OK) return rc;
    g->m_cap = cap;
    return AVL_OK;
}

static int navmany_check_points(const AvlNavGraph* g, const double* pts, int64_t M, const char* who) {
    for (int64_t k = 0; k < M; ++k) {
        const double r = pts[2 * k], c = pts[2 * k + 1];
        AVL_REQUIRE(std::isfinite(r) && std::isfinite(c), "%s: point %lld is not finite", who, (long long)k);
        AVL_REQUIRE(r >= 0.0 && r <= g->H - 1 && c >= 0.0 && c <= g->W - 1, "%s: point %lld (%g, %g) outside the %d x %d map", who,
                    (long long)k, r, c, g->H, g->W);
    }
    return AVL_OK;
}

extern "C" int avl_navmany_snap(void* graph, const double* h_pts, int64_t M, double* h_out, uint8_t* h_moved, void* stream) {
    AVL_REQUIRE(graph, "avl_navmany_snap: null handle");
    AvlNavGraph* g = static_cast<AvlNavGraph*>(graph);
    AVL_REQUIRE(M >= 0 && M <= kNavManyMax, "avl_navmany_snap: %lld points (0 .. %lld)", (long long)M, (long long)kNavManyMax);
    if (M == 0) return AVL_OK;
    AVL_REQUIRE(h_pts && h_out && h_moved, "avl_navmany_snap: null pointer");
    int rc = navmany_check_points(g, h_pts, M, "avl_navmany_snap");
    if (rc != AVL_OK) return rc;
    hipStream_t st = as_stream(stream);
    if (!g->free_known) {
        if (!g->m_free && (rc = nav_alloc((void**)&g->m_free, sizeof(int32_t))) != AVL_OK) return rc;
        int32_t any = 0;
        AVL_HIP_CHECK(hipMemsetAsync(g->m_free, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL(nav_any_free_kernel, dim3(nav_blocks((int64_t)g->H * g->W, 256)), dim3(256), 0, st, g->pix, g->H, g->W, g->m_free);
        AVL_HIP_CHECK(hipGetLastError());
        AVL_HIP_CHECK(hipMemcpyAsync(&any, g->m_free, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        AVL_HIP_CHECK(hipStreamSynchronize(st));
        g->has_free = any != 0;
        g->free_known = 1;
    }
    if (!g->has_free) {                 // every point lies on an obstacle cell and has nowhere to go
        set_error("avl_navmany_snap: the obstacle map has no free cell");
        return AVL_ERR_STATE;
    }
    if ((rc = navmany_reserve(g, M)) != AVL_OK) return rc;
    AVL_HIP_CHECK(hipMemcpyAsync(g->m_goals, h_pts, sizeof(double) * 2 * (size_t)M, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(nav_snap_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, NavGrid{g->pix, g->H, g->W}, g->m_goals, M,
                       g->m_out, g->m_moved);
    AVL_HIP_CHECK(hipGetLastError());
    AVL_HIP_CHECK(hipMemcpyAsync(h_out, g->m_out, sizeof(double) * 2 * (size_t)M, hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipMemcpyAsync(h_moved, g->m_moved, (size_t)M, hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    return AVL_OK;
}

extern "C" int avl_navmany_plan(void* graph, double sr, double sc, const double* h_goals, int64_t M, double* h_dist, int32_t* h_via,
                                int64_t* h_best, void* stream) {
    AVL_REQUIRE(graph && h_best, "avl_navmany_plan: null pointer");
    AvlNavGraph* g = static_cast<AvlNavGraph*>(graph);
    *h_best = -1;
    AVL_REQUIRE(M >= 0 && M <= kNavManyMax, "avl_navmany_plan: %lld goals (0 .. %lld)", (long long)M, (long long)kNavManyMax);
    AVL_REQUIRE(M == 0 || (h_goals && h_dist && h_via), "avl_navmany_plan: null pointer");
    const double s[2] = {sr, sc};
    int rc = navmany_check_points(g, s, 1, "avl_navmany_plan (start)");
    if (rc == AVL_OK) rc = navmany_check_points(g, h_goals, M, "avl_navmany_plan");
    if (rc != AVL_OK) return rc;
    hipStream_t st = as_stream(stream);
    const NavGrid grid{g->pix, g->H, g->W};
    const int64_t V = g->V, N = V + 2, W64 = g->W64;
    // (each buffer under its own check: a call that failed half way leaves nothing to allocate twice)
    if (!g->m_qbits && (rc = nav_alloc((void**)&g->m_qbits, sizeof(unsigned long long) * 2 * (size_t)std::max<int64_t>(W64, 1))) != AVL_OK) return rc;
    if (!g->m_sg && (rc = nav_alloc((void**)&g->m_sg, sizeof(int32_t))) != AVL_OK) return rc;
    if (!g->m_flags && (rc = nav_alloc((void**)&g->m_flags, sizeof(int32_t) * (size_t)(N + 2))) != AVL_OK) return rc;
    if (!g->m_pred && (rc = nav_alloc((void**)&g->m_pred, sizeof(int32_t) * (size_t)N)) != AVL_OK) return rc;
    if (!g->m_walks && (rc = nav_alloc((void**)&g->m_walks, sizeof(unsigned long long) * 2)) != AVL_OK) return rc;
    if (!g->m_dist && (rc = nav_alloc((void**)&g->m_dist, sizeof(double) * 2 * (size_t)N)) != AVL_OK) return rc;
    if (!g->h_many_pred) {
        g->h_many_pred = new (std::nothrow) int32_t[(size_t)N];
        AVL_REQUIRE(g->h_many_pred, "avl_navmany_plan: out of host memory");
    }
    if (M > g->h_many_via_cap) {
        delete[] g->h_many_via;
        g->h_many_via_cap = 0;
        g->h_many_via = new (std::nothrow) int32_t[(size_t)M];
        AVL_REQUIRE(g->h_many_via, "avl_navmany_plan: out of host memory");
        g->h_many_via_cap = M;
    }
    if ((rc = navmany_reserve(g, M)) != AVL_OK) return rc;
    g->many_planned = 0;
    // the tree: the start's row, an all-zero goal row and sg = 0, so that the goal node neither pulls nor is pulled from
    AVL_HIP_CHECK(hipMemsetAsync(g->m_qbits, 0, sizeof(unsigned long long) * 2 * (size_t)std::max<int64_t>(W64, 1), st));
    hipLaunchKernelGGL(nav_query_kernel, dim3((unsigned)(V / 256 + 1), 1), dim3(256), 0, st, grid, g->verts, V, W64, sr, sc, sr, sc,
                       g->m_qbits, g->m_sg);
    AVL_HIP_CHECK(hipMemsetAsync(g->m_sg, 0, sizeof(int32_t), st));      // (the kernel's start-"goal" bit is not wanted)
    double* d0 = g->m_dist;
    double* d1 = g->m_dist + N;
    hipLaunchKernelGGL(nav_init_kernel, dim3(nav_blocks(N, 256)), dim3(256), 0, st, N, V, d0, d1);
    AVL_HIP_CHECK(hipMemsetAsync(g->m_flags, 0, sizeof(int32_t) * (size_t)(N + 2), st));
    AVL_HIP_CHECK(hipMemsetAsync(g->m_walks, 0, sizeof(unsigned long long) * 2, st));
    AVL_HIP_CHECK(hipGetLastError());
    const NavNodes nodes{g->verts, V, W64, g->bits, g->m_qbits, g->m_sg, g->vspan, g->vrun, sr, sc, sr, sc};
    if ((rc = nav_relax(nodes, d0, d1, g->m_flags, g->m_pred, "avl_navmany_plan", st)) != AVL_OK) return rc;
    if (M > 0) {
        AVL_HIP_CHECK(hipMemcpyAsync(g->m_goals, h_goals, sizeof(double) * 2 * (size_t)M, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(nav_goals_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, grid, nodes, d0, g->m_goals, M, g->m_out,
                           g->m_via, g->count_walks ? g->m_walks : nullptr);
        AVL_HIP_CHECK(hipGetLastError());
        AVL_HIP_CHECK(hipMemcpyAsync(h_dist, g->m_out, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, st));
        AVL_HIP_CHECK(hipMemcpyAsync(g->h_many_via, g->m_via, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, st));
    }
    AVL_HIP_CHECK(hipMemcpyAsync(g->h_many_pred, g->m_pred, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipMemcpyAsync(g->many_walks, g->m_walks, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    int64_t best = -1;
    for (int64_t k = 0; k < M; ++k) {                    // the smallest k with the smallest finite distance
        h_via[k] = g->h_many_via[k];
        if (h_dist[k] < INFINITY && (best < 0 || h_dist[k] < h_dist[best])) best = k;
    }
    *h_best = best;
    g->many_M = M;
    g->many_planned = 1;
    g->many_counted = g->count_walks;
    return AVL_OK;
}

extern "C" int avl_navmany_path(void* graph, int64_t k, int32_t* h_path, int* h_len, int cap, void* stream) {
    (void)stream;                                        // the tree and via[] of the last batch are kept on the host
    AVL_REQUIRE(graph && h_len, "avl_navmany_path: null pointer");
    AvlNavGraph* g = static_cast<AvlNavGraph*>(graph);
    *h_len = 0;
    if (!g->many_planned) {
        set_error("avl_navmany_path: no batch has been planned on this graph");
        return AVL_ERR_STATE;
    }
    AVL_REQUIRE(k >= 0 && k < g->many_M, "avl_navmany_path: goal %lld of %lld", (long long)k, (long long)g->many_M);
    AVL_REQUIRE(cap >= 0 && (cap == 0 || h_path), "avl_navmany_path: bad path buffer");
    const int64_t V = g->V, N = V + 2;
    int64_t v = g->h_many_via[k];
    if (v < 0) return AVL_OK;                            // unreachable: an empty path
    // goal -> via -> the tree's predecessors -> start (distances strictly decrease: at most N nodes), then reversed
    int64_t len = 0;
    if (cap > 0) h_path[0] = (int32_t)(V + 1);
    len = 1;
    for (; v >= 0 && v <= V && len <= N; v = g->h_many_pred[v]) {
        if (len < cap) h_path[len] = (int32_t)v;
        ++len;
        if (v == V) break;
    }
    if (v != V) {
        set_error("avl_navmany_path: the predecessor chain of goal %lld does not reach the start", (long long)k);
        return AVL_ERR_STATE;
    }
    if (len > cap) {
        set_error("avl_navmany_path: the path has %lld nodes, the buffer %d", (long long)len, cap);
        return AVL_ERR_INVALID;
    }
    std::reverse(h_path, h_path + len);
    *h_len = (int)len;
    return AVL_OK;
}

// counting is off by default: a batch then hands the kernel no counters and pays nothing for them
extern "C" int avl_navmany_count_walks(void* graph, int on) {
    AVL_REQUIRE(graph, "avl_navmany_count_walks: null handle");
    static_cast<AvlNavGraph*>(graph)->count_walks = on ? 1 : 0;
    return AVL_OK;
}

// the pruning of the last batch, for the probe: h_counts[0] = walks started, h_counts[1] = candidates with a finite distance
extern "C" int avl_navmany_stats(void* graph, uint64_t* h_counts) {
    AVL_REQUIRE(graph && h_counts, "avl_navmany_stats: null pointer");
    AvlNavGraph* g = static_cast<AvlNavGraph*>(graph);
    if (!g->many_planned) {
        set_error("avl_navmany_stats: no batch has been planned on this graph");
        return AVL_ERR_STATE;
    }
    if (!g->many_counted) {
        set_error("avl_navmany_stats: the last batch did not count its walks (avl_navmany_count_walks)");
        return AVL_ERR_STATE;
    }
    h_counts[0] = g->many_walks[0];
    h_counts[1] = g->many_walks[1];
    return AVL_OK;
}
