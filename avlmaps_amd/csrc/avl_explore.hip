// Observed free space of the 2-D map for gfx950: the first frame whose sight rays crossed every cell, and the frontier of the
// explored area.
//
// Replaces (upstream reference, path:line):
//   avlmaps/utils/mapping_utils.py:403-454    get_frustum_4pts, generate_mask   one cv2.line per depth column and frame into a
//                                             top-down mask.  Nothing upstream calls it.
// This is NOT a mirror of those lines, on purpose.  generate_mask lives in the old camera-frame grid convention (pos2grid_id), its
// (row, col) order disagrees with its own cv2.line call (which takes (x, y) = (col, row)), it draws one line per COLUMN from the
// column's largest depth regardless of height, and cv2.line's clipped 8-connected line is not specified anywhere but in OpenCV,
// which no box of this project has.  The carver follows the project's own conventions instead -- the base frame, the builder's
// frame_transforms, base_pos2grid_id_3d -- and is defined below to the bit, so that a scalar NumPy restatement can be (and is)
// compared with np.array_equal.
//
// One ray per lattice pixel (rows and columns stride / 2, stride / 2 + stride, ... of the depth image), every float64 operation
// in this order and unfused (the file is compiled with -ffp-contract=off; the only fma() are bp_backproject's and bp_transform's,
// avl_pinhole.h, K1's own code):
//    1  z = depth[v, u]  (float32 metres, or uint16 / depth_div)
//    2  p = (Kinv @ (u + 0.5, v + 0.5, 1)) * z                                 bp_backproject
//    3  skip unless p.z > min_depth                                            (drops NaN, 0 and negative depths)
//    4  p.z >= max_depth: a FAR ray, s = max_depth / p.z, p = (p.x * s, p.y * s, p.z * s); it has no surface at its end.
//       Otherwise a HIT ray: a surface sits in its end cell
//    5  O = T[:3, 3],  P = T @ (p, 1)                                          bp_transform
//    6  height slab: dz = P.z - O.z.  dz == 0: the ray is kept whole (t0 = 0, t1 = 1) iff h_min <= O.z <= h_max.  Else
//       ta = (h_min - O.z) / dz, tb = (h_max - O.z) / dz (one division per bound), t0 = max(0, min(ta, tb)),
//       t1 = min(1, max(ta, tb)); the ray is skipped unless t0 <= t1.  t1 < 1: the ray leaves the band before its end and the end
//       no longer counts as a hit
//    7  end points: X(t) = O + t * (P - O) per coordinate, i.e. d = P.x - O.x; x = O.x + t * d (two roundings); X(0) = O and
//       X(1) = P exactly, not through the expression.  a = cell(X(t0)), b = cell(X(t1)) with base_pos2grid_id_3d's
//       row = int(gs / 2 - int(x / cs)), col = int(gs / 2 - int(y / cs)), both truncating toward zero
//    8  skipped whole: O, P or an end point not finite; a outside [0, gs)^2; |b.row| or |b.col| above 2^29 (the walk's int32
//       error term would overflow; only a transform that is no rigid motion gets there)
//    9  the all-octant integer Bresenham from a to b
//           dr = |br - ar|, dc = |bc - ac|, err = dc - dr
//           e2 = 2 * err;  if e2 > -dr: err -= dr, c += sc;  if e2 < dc: err += dc, r += sr
//       marks every visited cell, stops at the first cell outside the grid, and does not mark b when the ray is a hit with t1 == 1
//   10  the cell of O is marked once per frame whenever it lies in the grid, whatever the frame's rays do
// "Mark" is first_seen[r, c] = min(first_seen[r, c], frame id) as UNSIGNED 32-bit integers: the host's -1 ("never") is the largest
// unsigned value, so the device map has the host's encoding and needs no conversion; frame ids are >= 0.  The fold is an integer
// minimum: the map does not depend on the order of rays, frames or launches, and a second call continues the first.
//
// Launch shape.  A thread owns a ray, lanes run along an image row (neighbouring rays cross mostly the same cells: little
// divergence, and the cells' lines are shared in L2), blockIdx.y is the frame, so the pose is wave-uniform and comes from the
// kernel arguments through scalar loads (up to kCarveFrames frames per launch; a longer batch takes several launches).  A cell is
// read first and the atomic is issued only when the stored id is larger: the (gs, gs) map is 4 MB at gs = 1000 and stays in L2,
// and after the first frames nearly every visit ends at the read.  A stale read can only be too large, which costs a redundant
// atomic, never a wrong minimum.
//
// The frontier (avl_frontier_mask): a cell that is explored and free with a 4-neighbour inside the image that is unknown, i.e.
// not explored and free.  A cell that holds an obstacle is known whether or not a ray crossed it.
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_pinhole.h"

namespace avl {

constexpr int kCarveThreads = 256;
constexpr int kCarveFrames = 16;                // frames per launch: 16 * 104 bytes of kernel arguments
constexpr int kCarveMaxSide = 16384;            // gs, and the sides of avl_frontier_mask's images
constexpr int kCarveMaxCell = 1 << 29;          // |b.row|, |b.col|: 2 * err stays inside int32

struct CarveFrame {
    double t[12];                               // the first three rows of the frame's camera -> map transform
    int32_t id, pad;
};
struct CarveBatch {
    CarveFrame f[kCarveFrames];
};
struct CarveParams {
    double kinv[9];
    double cs, half_gs, h_min, h_max, min_depth, max_depth, depth_div;
    int H, W, gs, stride, nv, nu, depth_u16;
};

__device__ __forceinline__ void carve_mark(unsigned* __restrict__ first_seen, int gs, int r, int c, unsigned id) {
    unsigned* p = first_seen + (size_t)r * gs + c;
#ifdef AVL_CARVE_ALWAYS_ATOMIC
    atomicMin(p, id);       // the B side of tools/probe_explored.py's A/B (tools/build_variant.py), never in the shipped library
#else
    if (id < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, id);
#endif
}

__device__ __forceinline__ bool carve_in_grid(int r, int c, int gs) { return r >= 0 && r < gs && c >= 0 && c < gs; }

__global__ __launch_bounds__(kCarveThreads) void carve_kernel(CarveParams p, CarveBatch batch, const void* __restrict__ depth,
                                                             unsigned* __restrict__ first_seen) {
    const CarveFrame& fr = batch.f[blockIdx.y];
    const unsigned id = (unsigned)fr.id;
    const int ray = blockIdx.x * kCarveThreads + threadIdx.x;
    const double ox = fr.t[3], oy = fr.t[7], oz = fr.t[11];
    if (ray == 0) {                                                             // (10) the camera cell, once per frame
        const int r = py_int(p.half_gs - (double)py_int(ox / p.cs)), c = py_int(p.half_gs - (double)py_int(oy / p.cs));
        if (carve_in_grid(r, c, p.gs)) carve_mark(first_seen, p.gs, r, c, id);
    }
    if (ray >= p.nv * p.nu) return;
    const int v = p.stride / 2 + (ray / p.nu) * p.stride, u = p.stride / 2 + (ray % p.nu) * p.stride;
    const size_t pix = (size_t)blockIdx.y * p.H * p.W + (size_t)v * p.W + u;
    const double z = p.depth_u16 ? (double)reinterpret_cast<const uint16_t*>(depth)[pix] / p.depth_div
                                 : (double)reinterpret_cast<const float*>(depth)[pix];
    double p0, p1, p2;
    bp_backproject(p.kinv, (double)u + 0.5, (double)v + 0.5, z, p0, p1, p2);
    if (!(p2 > p.min_depth)) return;                                            // (3)
    const bool far = p2 >= p.max_depth;                                         // (4)
    if (far) {
        const double s = p.max_depth / p2;
        p0 = p0 * s;
        p1 = p1 * s;
        p2 = p2 * s;
    }
    double gx, gy, gz;
    bp_transform(fr.t, p0, p1, p2, gx, gy, gz);                                 // (5)
    if (!(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(gx) && isfinite(gy) && isfinite(gz))) return;
    double t0 = 0.0, t1 = 1.0;                                                  // (6)
    const double dz = gz - oz;
    if (dz == 0.0) {
        if (!(oz >= p.h_min && oz <= p.h_max)) return;
    } else {
        const double ta = (p.h_min - oz) / dz, tb = (p.h_max - oz) / dz;
        t0 = fmax(0.0, fmin(ta, tb));
        t1 = fmin(1.0, fmax(ta, tb));
        if (!(t0 <= t1)) return;
    }
    const double dx = gx - ox, dy = gy - oy;                                    // (7)
    const double ax = t0 == 0.0 ? ox : ox + t0 * dx, ay = t0 == 0.0 ? oy : oy + t0 * dy;
    const double bx = t1 == 1.0 ? gx : ox + t1 * dx, by = t1 == 1.0 ? gy : oy + t1 * dy;
    if (!(isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by))) return;
    int r = py_int(p.half_gs - (double)py_int(ax / p.cs)), c = py_int(p.half_gs - (double)py_int(ay / p.cs));
    const int br = py_int(p.half_gs - (double)py_int(bx / p.cs)), bc = py_int(p.half_gs - (double)py_int(by / p.cs));
    if (!carve_in_grid(r, c, p.gs)) return;                                     // (8)
    if (br > kCarveMaxCell || br < -kCarveMaxCell || bc > kCarveMaxCell || bc < -kCarveMaxCell) return;
    const bool skip_end = !far && t1 == 1.0;
    const int dr = abs(br - r), dc = abs(bc - c), sr = br > r ? 1 : -1, sc = bc > c ? 1 : -1;
    int err = dc - dr;
    for (int it = 0; it <= 2 * p.gs; ++it) {                                    // (9) (a walk inside the grid has at most 2 gs - 1 cells)
        if (!carve_in_grid(r, c, p.gs)) break;
        if (r == br && c == bc) {
            if (!skip_end) carve_mark(first_seen, p.gs, r, c, id);
            break;
        }
        carve_mark(first_seen, p.gs, r, c, id);
        const int e2 = 2 * err;
        if (e2 > -dr) {
            err -= dr;
            c += sc;
        }
        if (e2 < dc) {
            err += dc;
            r += sr;
        }
    }
}

__global__ __launch_bounds__(256) void frontier_kernel(const uint8_t* __restrict__ free_u8, const uint8_t* __restrict__ explored, int H,
                                                       int W, uint8_t* __restrict__ out) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= H || c >= W) return;
    const size_t i = (size_t)r * W + c;
    bool f = false;
    if (free_u8[i] != 0 && explored[i] != 0) {
        // unknown = not explored and free of obstacle voxels
        if (r > 0) f |= explored[i - W] == 0 && free_u8[i - W] != 0;
        if (r + 1 < H) f |= explored[i + W] == 0 && free_u8[i + W] != 0;
        if (c > 0) f |= explored[i - 1] == 0 && free_u8[i - 1] != 0;
        if (c + 1 < W) f |= explored[i + 1] == 0 && free_u8[i + 1] != 0;
    }
    out[i] = f ? 1 : 0;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_carve_free_space(const void* d_depth, int depth_is_u16, double depth_div, int F, int H, int W, const double* h_calib_inv,
                         const double* h_transforms, const int32_t* h_frame_ids, int gs, double cs, int stride, double h_min, double h_max,
                         double min_depth, double max_depth, int32_t* d_first_seen, void* stream) {
    AVL_REQUIRE(F >= 0 && H > 0 && W > 0 && (int64_t)H * W < INT_MAX, "avl_carve_free_space: bad batch of %d frames of %d x %d", F, H, W);
    AVL_REQUIRE(gs >= 1 && gs <= kCarveMaxSide, "avl_carve_free_space: grid size %d (1 .. %d)", gs, kCarveMaxSide);
    AVL_REQUIRE(std::isfinite(cs) && cs > 0, "avl_carve_free_space: cell size must be finite and positive");
    AVL_REQUIRE(stride >= 1, "avl_carve_free_space: stride %d < 1", stride);
    AVL_REQUIRE(std::isfinite(h_min) && std::isfinite(h_max) && h_min <= h_max, "avl_carve_free_space: height band [%g, %g]", h_min, h_max);
    AVL_REQUIRE(std::isfinite(min_depth) && std::isfinite(max_depth) && min_depth >= 0 && max_depth > min_depth,
                "avl_carve_free_space: depth range (%g, %g)", min_depth, max_depth);
    AVL_REQUIRE(!depth_is_u16 || (std::isfinite(depth_div) && depth_div > 0), "avl_carve_free_space: depth_div must be positive");
    if (F == 0) return AVL_OK;
    AVL_REQUIRE(d_depth && h_calib_inv && h_transforms && h_frame_ids && d_first_seen, "avl_carve_free_space: null pointer");
    for (int f = 0; f < F; ++f) AVL_REQUIRE(h_frame_ids[f] >= 0, "avl_carve_free_space: frame id %d is negative", h_frame_ids[f]);
    CarveParams p{};
    for (int i = 0; i < 9; ++i) p.kinv[i] = h_calib_inv[i];
    p.cs = cs;
    p.half_gs = (double)gs / 2.0;
    p.h_min = h_min;
    p.h_max = h_max;
    p.min_depth = min_depth;
    p.max_depth = max_depth;
    p.depth_div = depth_is_u16 ? depth_div : 1.0;
    p.H = H;
    p.W = W;
    p.gs = gs;
    p.stride = stride;
    const int off = stride / 2;
    p.nv = off < H ? (H - off + stride - 1) / stride : 0;
    p.nu = off < W ? (W - off + stride - 1) / stride : 0;
    p.depth_u16 = depth_is_u16 ? 1 : 0;
    const int rays = p.nv * p.nu;                                               // < H * W < 2^31
    const unsigned blocks = (unsigned)std::max(1, (rays + kCarveThreads - 1) / kCarveThreads);       // ray 0's thread marks the camera cell
    const size_t frame_bytes = (size_t)H * W * (depth_is_u16 ? sizeof(uint16_t) : sizeof(float));
    hipStream_t st = as_stream(stream);
    for (int f0 = 0; f0 < F; f0 += kCarveFrames) {
        const int n = std::min(kCarveFrames, F - f0);
        CarveBatch b{};
        for (int k = 0; k < n; ++k) {
            for (int i = 0; i < 12; ++i) b.f[k].t[i] = h_transforms[(size_t)(f0 + k) * 16 + i];
            b.f[k].id = h_frame_ids[f0 + k];
        }
        hipLaunchKernelGGL(carve_kernel, dim3(blocks, (unsigned)n), dim3(kCarveThreads), 0, st, p, b,
                           (const void*)((const char*)d_depth + (size_t)f0 * frame_bytes), (unsigned*)d_first_seen);
    }
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_frontier_mask(const uint8_t* d_free_u8, const uint8_t* d_explored_u8, int H, int W, uint8_t* d_out_u8, void* stream) {
    AVL_REQUIRE(H >= 1 && W >= 1 && H <= kCarveMaxSide && W <= kCarveMaxSide, "avl_frontier_mask: bad shape %d x %d (sides 1 .. %d)", H, W,
                kCarveMaxSide);
    AVL_REQUIRE(d_free_u8 && d_explored_u8 && d_out_u8, "avl_frontier_mask: null pointer");
    hipLaunchKernelGGL(frontier_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), dim3(256), 0, as_stream(stream), d_free_u8,
                       d_explored_u8, H, W, d_out_u8);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
