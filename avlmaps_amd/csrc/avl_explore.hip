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
// One ray per lattice pixel.  Steps 1 - 8 -- the pixel, its depth, the back-projection, the depth range, far and hit rays, the pose,
// the height slab with its t0 and t1, the end points A = X(t0) and B = X(t1) and the finiteness of their x and y -- are the sight
// ray of avl_sightray.h, defined there to the bit and shared with the visibility audit (avl_audit.hip).  The carver's own steps:
//    8' a = cell(A), b = cell(B) (row and col, ray_cell_rc); also skipped whole: a outside [0, gs)^2; |b.row| or |b.col| above 2^29
//       (the walk's int32 error term would overflow; only a transform that is no rigid motion gets there)
//    9  the all-octant integer Bresenham from a to b
//           dr = |br - ar|, dc = |bc - ac|, err = dc - dr
//           e2 = 2 * err;  if e2 > -dr: err -= dr, c += sc;  if e2 < dc: err += dc, r += sr
//       marks every visited cell, stops at the first cell outside the grid, and does not mark b when the ray is a hit with t1 == 1
//   10  the cell of O is marked once per frame whenever it lies in the grid, whatever the frame's rays do
// "Mark" is first_seen[r, c] = min(first_seen[r, c], frame id) as UNSIGNED 32-bit integers: the host's -1 ("never") is the largest
// unsigned value, so the device map has the host's encoding and needs no conversion; frame ids are >= 0.  The fold is an integer
// minimum: the map does not depend on the order of rays, frames or launches, and a second call continues the first.
//
// Launch shape: avl_sightray.h's (a thread owns a ray, blockIdx.y is the frame, the poses travel in the kernel arguments).
// Neighbouring rays cross mostly the same cells: little divergence, and the cells' lines are shared in L2.  A cell is
// read first and the atomic is issued only when the stored id is larger: the (gs, gs) map is 4 MB at gs = 1000 and stays in L2,
// and after the first frames nearly every visit ends at the read.  A stale read can only be too large, which costs a redundant
// atomic, never a wrong minimum.
//
// The frontier (avl_frontier_mask): a cell that is explored and free with a 4-neighbour inside the image that is unknown, i.e.
// not explored and free.  A cell that holds an obstacle is known whether or not a ray crossed it.
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_sightray.h"

namespace avl {

constexpr int kCarveThreads = 256;
constexpr int kCarveMaxSide = 16384;            // gs, and the sides of avl_frontier_mask's images
constexpr int kCarveMaxCell = 1 << 29;          // |b.row|, |b.col|: 2 * err stays inside int32

__device__ __forceinline__ void carve_mark(unsigned* __restrict__ first_seen, int gs, int r, int c, unsigned id) {
    unsigned* p = first_seen + (size_t)r * gs + c;
#ifdef AVL_CARVE_ALWAYS_ATOMIC
    atomicMin(p, id);       // the B side of tools/probe_explored.py's A/B (tools/build_variant.py), never in the shipped library
#else
    if (id < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, id);
#endif
}

__device__ __forceinline__ bool carve_in_grid(int r, int c, int gs) { return r >= 0 && r < gs && c >= 0 && c < gs; }

__global__ __launch_bounds__(kCarveThreads) void carve_kernel(RayParams p, RayBatch batch, const void* __restrict__ depth,
                                                             unsigned* __restrict__ first_seen) {
    const RayFrame& fr = batch.f[blockIdx.y];
    const unsigned id = (unsigned)fr.id;
    const int ray = blockIdx.x * kCarveThreads + threadIdx.x;
    SightRay s;
    ray_origin(fr, s);
    if (ray == 0) {                                                             // (10) the camera cell, once per frame
        const int r = ray_cell_rc(p, s.ox), c = ray_cell_rc(p, s.oy);
        if (carve_in_grid(r, c, p.gs)) carve_mark(first_seen, p.gs, r, c, id);
    }
    if (ray >= p.nv * p.nu) return;
    size_t pix;
    double p0, p1, p2;
    ray_pixel(p, depth, ray, blockIdx.y, pix, p0, p1, p2);                      // (1 - 2)
    if (!sight_ray(p, fr, p0, p1, p2, s)) return;                               // (3 - 8)
    int r = ray_cell_rc(p, s.ax), c = ray_cell_rc(p, s.ay);
    const int br = ray_cell_rc(p, s.bx), bc = ray_cell_rc(p, s.by);
    if (!carve_in_grid(r, c, p.gs)) return;                                     // (8')
    if (br > kCarveMaxCell || br < -kCarveMaxCell || bc > kCarveMaxCell || bc < -kCarveMaxCell) return;
    const bool skip_end = !s.far && s.ends;
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
    const double h_band[2] = {h_min, h_max};
    RayParams p;
    int rc = ray_params("avl_carve_free_space", depth_is_u16, depth_div, F, H, W, h_calib_inv, gs, kCarveMaxSide, cs, stride, h_band, min_depth,
                        max_depth, &p);
    if (rc != AVL_OK) return rc;
    if (F == 0) return AVL_OK;
    AVL_REQUIRE(d_depth && h_calib_inv && h_transforms && h_frame_ids && d_first_seen, "avl_carve_free_space: null pointer");
    if ((rc = ray_frame_ids("avl_carve_free_space", h_frame_ids, F)) != AVL_OK) return rc;
    const int rays = p.nv * p.nu;
    const unsigned blocks = (unsigned)std::max(1, (rays + kCarveThreads - 1) / kCarveThreads);       // ray 0's thread marks the camera cell
    const size_t frame_bytes = (size_t)H * W * (depth_is_u16 ? sizeof(uint16_t) : sizeof(float));
    hipStream_t st = as_stream(stream);
    ray_launches(F, h_transforms, h_frame_ids, [&](const RayBatch& b, int n, int f0) {
        hipLaunchKernelGGL(carve_kernel, dim3(blocks, (unsigned)n), dim3(kCarveThreads), 0, st, p, b,
                           (const void*)((const char*)d_depth + (size_t)f0 * frame_bytes), (unsigned*)d_first_seen);
    });
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
