// The sight ray of a depth pixel: the ONE front end of the kernels that walk or bin the rays of a depth frame -- the free-space
// carver (avl_explore.hip), the visibility audit (avl_audit.hip), the ground-truth vote (avl_gtmap.hip) and the pose search
// (avl_match.hip).  Like avl_pinhole.h,
// which it includes, it holds arithmetic that several files must round alike; the files that include it are
// compiled with -ffp-contract=off.
//
// One ray per lattice pixel (rows and columns stride / 2, stride / 2 + stride, ... of the depth image), every float64 operation
// in this order and unfused (the only fma() are bp_backproject's and bp_transform's, avl_pinhole.h, K1's own code):
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
//       X(1) = P exactly, not through the expression.  A = X(t0), B = X(t1) in all three coordinates.  A point's map cell is
//       base_pos2grid_id_3d's row = int(gs / 2 - int(x / cs)), col = int(gs / 2 - int(y / cs)), both truncating toward zero
//       (ray_cell_rc)
//    8  skipped whole: O or P not finite, or the x or y of an end point.  The z of A and B is the caller's to test if it reads it
//       (the audit does; the carver does not, and the compiler then drops that arithmetic from carve_kernel)
// ray_pixel is steps 1 - 2, sight_ray steps 3 - 8 (with ray_origin, the O of step 5, read ahead of them).  The carver and the audit take both and go on with their own cells, limits and
// walks.  The vote takes ray_pixel, its own range test (open at both ends, no far rays: the builder's rule), bp_transform and
// ray_cell_rc; the pose search takes the same four and rotates the point before its cell.
//
// Launch shape of all four (the pose search's rasterise kernel; its angles travel beside the poses).  A thread owns a ray, lanes run along an image row, blockIdx.y is the frame's slot in the launch, so
// the pose is wave-uniform and comes from the kernel arguments through scalar loads: up to kRayFrames frames per launch, a longer
// batch takes several launches (ray_launches).  Nothing is staged, nothing allocated.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_pinhole.h"

namespace avl {

constexpr int kRayFrames = 16;                  // frames per launch: 16 * 104 bytes of kernel arguments

struct RayFrame {
    double t[12];                               // the first three rows of the frame's camera -> map transform
    int32_t id, pad;                            // (the vote ignores the id)
};
struct RayBatch {
    RayFrame f[kRayFrames];
};
struct RayParams {
    double kinv[9];
    double cs, half_gs, h_min, h_max, min_depth, max_depth, depth_div;       // (the vote has no height band: h_min = h_max = 0, unread)
    int H, W, gs, stride, nv, nu, depth_u16;
};

// (1 - 2) the lattice pixel of ray `ray` in the frame of launch slot `slot`: its index in the launch's depth (and semantic)
// frames and its camera-frame point.  ray < p.nv * p.nu
__device__ __forceinline__ void ray_pixel(const RayParams& p, const void* __restrict__ depth, int ray, unsigned slot, size_t& pix,
                                          double& p0, double& p1, double& p2) {
    const int v = p.stride / 2 + (ray / p.nu) * p.stride, u = p.stride / 2 + (ray % p.nu) * p.stride;
    pix = (size_t)slot * p.H * p.W + (size_t)v * p.W + u;
    const double z = p.depth_u16 ? (double)reinterpret_cast<const uint16_t*>(depth)[pix] / p.depth_div
                                 : (double)reinterpret_cast<const float*>(depth)[pix];
    bp_backproject(p.kinv, (double)u + 0.5, (double)v + 0.5, z, p0, p1, p2);
}

// the row of a map point's x, the col of its y
__device__ __forceinline__ int ray_cell_rc(const RayParams& p, double x) { return py_int(p.half_gs - (double)py_int(x / p.cs)); }

struct SightRay {
    bool far, ends;                             // (4); ends: t1 == 1, the segment reaches P
    double ox, oy, oz, ax, ay, az, bx, by, bz;  // O, A = X(t0), B = X(t1)
};

// O of (5), for the caller to read at the top of its kernel: the three scalar loads go out there, ahead of the rows of T, and their
// values stay in registers (read after the carver's atomic of step 10 they are loaded a second time, with a wait of their own)
__device__ __forceinline__ void ray_origin(const RayFrame& fr, SightRay& r) { r.ox = fr.t[3], r.oy = fr.t[7], r.oz = fr.t[11]; }

// (3 - 8) from the camera-frame point of ray_pixel and the O of ray_origin; false for a ray that is skipped whole
__device__ __forceinline__ bool sight_ray(const RayParams& p, const RayFrame& fr, double p0, double p1, double p2, SightRay& r) {
    const double ox = r.ox, oy = r.oy, oz = r.oz;
    if (!(p2 > p.min_depth)) return false;                                      // (3)
    r.far = p2 >= p.max_depth;                                                  // (4)
    if (r.far) {
        const double s = p.max_depth / p2;
        p0 = p0 * s;
        p1 = p1 * s;
        p2 = p2 * s;
    }
    double gx, gy, gz;
    bp_transform(fr.t, p0, p1, p2, gx, gy, gz);                                 // (5)
    if (!(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(gx) && isfinite(gy) && isfinite(gz))) return false;
    double t0 = 0.0, t1 = 1.0;                                                  // (6)
    const double dz = gz - oz;
    if (dz == 0.0) {
        if (!(oz >= p.h_min && oz <= p.h_max)) return false;
    } else {
        const double ta = (p.h_min - oz) / dz, tb = (p.h_max - oz) / dz;
        t0 = fmax(0.0, fmin(ta, tb));
        t1 = fmin(1.0, fmax(ta, tb));
        if (!(t0 <= t1)) return false;
    }
    const double dx = gx - ox, dy = gy - oy;                                    // (7)
    r.ax = t0 == 0.0 ? ox : ox + t0 * dx, r.ay = t0 == 0.0 ? oy : oy + t0 * dy, r.az = t0 == 0.0 ? oz : oz + t0 * dz;
    r.bx = t1 == 1.0 ? gx : ox + t1 * dx, r.by = t1 == 1.0 ? gy : oy + t1 * dy, r.bz = t1 == 1.0 ? gz : oz + t1 * dz;
    r.ends = t1 == 1.0;
    return isfinite(r.ax) && isfinite(r.ay) && isfinite(r.bx) && isfinite(r.by);                                            // (8)
}

// ---------------------------------------------------------------------------------------------------------------- host
// The requirements that the four entry points share, with `who` in their messages, and the RayParams they allow.  h_band: {h_min,
// h_max}, or null for an entry point without a height band.  max_side: the largest gs, or 0 when the caller has checked its grid.
// kinv is copied when h_calib_inv is given: a missing one is refused by the entry point's own null-pointer check, which comes after
// its F == 0 return.
static int ray_params(const char* who, int depth_is_u16, double depth_div, int F, int H, int W, const double* h_calib_inv, int gs, int max_side,
                      double cs, int stride, const double* h_band, double min_depth, double max_depth, RayParams* out) {
    AVL_REQUIRE(F >= 0 && H > 0 && W > 0 && (int64_t)H * W < INT_MAX, "%s: bad batch of %d frames of %d x %d", who, F, H, W);
    AVL_REQUIRE(!max_side || (gs >= 1 && gs <= max_side), "%s: grid size %d (1 .. %d)", who, gs, max_side);
    AVL_REQUIRE(std::isfinite(cs) && cs > 0, "%s: cell size must be finite and positive", who);
    AVL_REQUIRE(stride >= 1, "%s: stride %d < 1", who, stride);
    AVL_REQUIRE(!h_band || (std::isfinite(h_band[0]) && std::isfinite(h_band[1]) && h_band[0] <= h_band[1]), "%s: height band [%g, %g]", who,
                h_band ? h_band[0] : 0.0, h_band ? h_band[1] : 0.0);
    AVL_REQUIRE(std::isfinite(min_depth) && std::isfinite(max_depth) && min_depth >= 0 && max_depth > min_depth, "%s: depth range (%g, %g)",
                who, min_depth, max_depth);
    AVL_REQUIRE(!depth_is_u16 || (std::isfinite(depth_div) && depth_div > 0), "%s: depth_div must be positive", who);
    RayParams p{};
    for (int i = 0; i < 9 && h_calib_inv; ++i) p.kinv[i] = h_calib_inv[i];
    p.cs = cs;
    p.half_gs = (double)gs / 2.0;
    p.h_min = h_band ? h_band[0] : 0.0;
    p.h_max = h_band ? h_band[1] : 0.0;
    p.min_depth = min_depth;
    p.max_depth = max_depth;
    p.depth_div = depth_is_u16 ? depth_div : 1.0;
    p.H = H;
    p.W = W;
    p.gs = gs;
    p.stride = stride;
    const int off = stride / 2;
    p.nv = off < H ? (H - off + stride - 1) / stride : 0;
    p.nu = off < W ? (W - off + stride - 1) / stride : 0;                       // nv * nu <= H * W < 2^31
    p.depth_u16 = depth_is_u16 ? 1 : 0;
    *out = p;
    return AVL_OK;
}

static int ray_frame_ids(const char* who, const int32_t* h_frame_ids, int F) {
    for (int f = 0; f < F; ++f) AVL_REQUIRE(h_frame_ids[f] >= 0, "%s: frame id %d is negative", who, h_frame_ids[f]);
    return AVL_OK;
}

// F frames in launches of kRayFrames: launch(batch, n, f0) starts frames f0 .. f0 + n - 1.  h_frame_ids may be null (ids of 0)
template <class Launch>
static void ray_launches(int F, const double* h_transforms, const int32_t* h_frame_ids, Launch launch) {
    for (int f0 = 0; f0 < F; f0 += kRayFrames) {
        const int n = std::min(kRayFrames, F - f0);
        RayBatch b{};
        for (int k = 0; k < n; ++k) {
            for (int i = 0; i < 12; ++i) b.f[k].t[i] = h_transforms[(size_t)(f0 + k) * 16 + i];
            b.f[k].id = h_frame_ids ? h_frame_ids[f0 + k] : 0;
        }
        launch(b, n, f0);
    }
}

}  // namespace avl
