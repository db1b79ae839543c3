// Exact 2-D Euclidean distance transform of an arbitrary mask for gfx950, and the decay maps built on it.
//
// Replaces (upstream reference, path:line):
//   avlmaps/robot/habitat_lang_robot.py:229-240  get_vl_distribution_map   distance_transform_edt(mask == 0), 1 - d * decay, negative
//                                                                          values to 0, min-max normalisation
//   avlmaps/robot/habitat_lang_robot.py:277-321  the gt / lseg / concept-fusion region maps: the same three steps on another mask
//   avlmaps/utils/visualize_utils.py:97-102      get_heatmap_from_mask_2d  the same with d / cell_size and without the normalisation
//
// Exactness.  scipy.ndimage.distance_transform_edt returns, per non-zero cell, the distance to the nearest zero cell.  The squared
// distance between integer cells is an exact integer, so the minimum is taken in integers and one correctly rounded fp64 sqrt gives
// SciPy's value; ties between equally near cells cannot matter because only the value is returned.  The decay and the normalisation
// are NumPy's float64 expressions, operation for operation (__ddiv_rn, and this file is compiled with -ffp-contract=off).
//
// Work.  Two launches, the classic separable form with a parallel second pass:
//   column pass  g[r][c] = the vertical distance from (r, c) to the nearest zero cell of column c, -1 when the column has none.  A
//                workgroup owns 64 columns; its 16 waves own 16 row segments of those columns.  Every wave finds the first and the
//                last zero row of its segment, the segments exchange them through LDS, and every wave then sweeps its segment down
//                and up once with the carries of the segments above and below: ~3 H / 16 dependent steps instead of 2 H.
//   row pass     a workgroup stages one row's g^2 in LDS together with the minimum of every 64-column tile.  A thread owns one cell
//                and searches outwards from its own column, left and right in turn, for min_j (g^2[j] + (c - j)^2); a direction
//                ends as soon as (c - j)^2 reaches the running minimum, and a whole tile is stepped over when its minimum plus the
//                squared distance to its nearest column cannot beat the running minimum.  A mask with one far feature -- empty
//                tiles everywhere -- therefore costs W / 64 steps per cell, not W.
// Sides are at most 16 384, so that g fits 16 bits in LDS, d^2 <= 2 * 16383^2, and the "none" sentinel plus any (c - j)^2 fit 32
// unsigned bits.
#include <algorithm>
#include <cmath>

#include "avl_common.h"
#include "avl_decay2d.h"
#include "avl_wave.h"

namespace avl {

constexpr int kEdtMaxSide = 16384;
constexpr int kEdtCols = 64;                    // columns per workgroup of the column pass (one wave wide)
constexpr int kEdtSegs = 16;                    // row segments = waves per workgroup of the column pass
constexpr int kEdtRowThreads = 256;
constexpr int kEdtTile = 64;                    // columns per tile of the row pass (one wave stages one tile)
constexpr unsigned kEdtNoneG = 46340;           // g of a column without a zero cell as LDS holds it (16 bits): its square is above
                                                // every real d^2 (<= 2 * 16383^2) and stays below 2^32 with 16383^2 added
constexpr int kEdtFar = 1 << 20;                // "no zero row on this side": farther than any row of the image

// zero cell = a cell the distance is measured TO.  invert = 0: SciPy's convention, the zero cells of the image; invert = 1: the
// non-zero cells (the distance to the nearest set cell of a mask: distance_transform_edt(mask == 0) without building mask == 0)
__device__ __forceinline__ bool edt_is_zero(const uint8_t* __restrict__ img, int64_t ld, int r, int c, int invert) {
    return (img[(int64_t)r * ld + c] != 0) == (invert != 0);
}

__global__ __launch_bounds__(kEdtCols* kEdtSegs) void edt_column_kernel(const uint8_t* __restrict__ img, int64_t ld, int H, int W, int invert,
                                                                        int32_t* __restrict__ g, int* __restrict__ found) {
    __shared__ int s_first[kEdtSegs][kEdtCols], s_last[kEdtSegs][kEdtCols];
    const int lane = threadIdx.x & (kEdtCols - 1), seg = threadIdx.x / kEdtCols;
    const int c = blockIdx.x * kEdtCols + lane;
    const int rows = (H + kEdtSegs - 1) / kEdtSegs;
    const int r0 = min(seg * rows, H), r1 = min(r0 + rows, H);
    const bool active = c < W;
    int first = kEdtFar, last = -kEdtFar;                               // first / last zero row of this segment of the column
    if (active) {
        for (int r = r0; r < r1; ++r) {
            if (edt_is_zero(img, ld, r, c, invert)) {
                if (first == kEdtFar) first = r;
                last = r;
            }
        }
    }
    s_first[seg][lane] = first;
    s_last[seg][lane] = last;
    __syncthreads();
    if (!active) return;
    int above = -kEdtFar, below = kEdtFar;                              // nearest zero row above / below the segment
    for (int s = 0; s < seg; ++s) above = max(above, s_last[s][lane]);
    for (int s = kEdtSegs - 1; s > seg; --s) below = min(below, s_first[s][lane]);
    if (seg == 0) {                                                     // one wave per workgroup reports whether a zero cell exists
        int any = below != kEdtFar || first != kEdtFar;
        if (__any(any) && lane == 0) atomicOr(found, 1);
    }
    int z = above;
    for (int r = r0; r < r1; ++r) {                                     // down: the distance to the nearest zero row at or above
        if (edt_is_zero(img, ld, r, c, invert)) z = r;
        g[(int64_t)r * W + c] = z == -kEdtFar ? -1 : r - z;
    }
    z = below;
    for (int r = r1 - 1; r >= r0; --r) {                                // up: the nearest zero row at or below, folded in
        const int up = g[(int64_t)r * W + c];
        if (up == 0) z = r;
        const int dn = z == kEdtFar ? -1 : z - r;
        g[(int64_t)r * W + c] = up < 0 ? dn : (dn < 0 ? up : min(up, dn));
    }
}

// One workgroup per row.  DECAY = false: out = sqrt(min d^2); true: out = decay_value(that) (avl_decay2d.h), and (minmax != nullptr)
// the minimum and maximum of the image by bit pattern (the values are >= +0: their IEEE patterns order like the values).
template <bool DECAY>
__global__ __launch_bounds__(kEdtRowThreads) void edt_row_kernel(const int32_t* __restrict__ g, int H, int W, double cell_size,
                                                                 double decay_rate, double* __restrict__ out,
                                                                 unsigned long long* __restrict__ minmax) {
    extern __shared__ unsigned s_dyn[];
    const int wpad = (W + kEdtTile - 1) / kEdtTile * kEdtTile;
    unsigned* s_tmin = s_dyn;                                           // [wpad / kEdtTile] tile minima of g^2
    unsigned short* s_g = reinterpret_cast<unsigned short*>(s_dyn + wpad / kEdtTile);   // [wpad] g, 16 bits: 32 KB at the largest side
    __shared__ double s_red[2 * kEdtRowThreads / kWave];
    const int r = blockIdx.x;
    const int32_t* row = g + (int64_t)r * W;
    for (int c = threadIdx.x; c < wpad; c += kEdtRowThreads) {          // a wave stages exactly one tile per step
        unsigned v = kEdtNoneG;
        if (c < W) {
            const int gv = row[c];
            if (gv >= 0) v = (unsigned)gv;
        }
        s_g[c] = (unsigned short)v;
        const unsigned m = wave_min(v);
        if ((threadIdx.x & (kWave - 1)) == 0) s_tmin[c / kEdtTile] = m * m;
    }
    __syncthreads();
    double mn = INFINITY, mx = -INFINITY;
    for (int c = threadIdx.x; c < W; c += kEdtRowThreads) {
        unsigned best = (unsigned)s_g[c] * (unsigned)s_g[c];
        int jl = c - 1, jr = c + 1;
        bool left = jl >= 0 && best != 0, right = jr < W && best != 0;
        while (left || right) {
            if (left) {
                const unsigned d = (unsigned)(c - jl), d2 = d * d;
                if (d2 >= best) {
                    left = false;
                } else if ((jl & (kEdtTile - 1)) == kEdtTile - 1 && s_tmin[jl / kEdtTile] + d2 >= best) {
                    jl -= kEdtTile;                                     // entered a tile at its nearest column: nothing in it is nearer
                } else {
                    const unsigned gv = s_g[jl];
                    best = min(best, gv * gv + d2);
                    --jl;
                }
                if (jl < 0) left = false;
            }
            if (right) {
                const unsigned d = (unsigned)(jr - c), d2 = d * d;
                if (d2 >= best) {
                    right = false;
                } else if ((jr & (kEdtTile - 1)) == 0 && s_tmin[jr / kEdtTile] + d2 >= best) {
                    jr += kEdtTile;
                } else {
                    const unsigned gv = s_g[jr];
                    best = min(best, gv * gv + d2);
                    ++jr;
                }
                if (jr >= W) right = false;
            }
        }
        double v = sqrt((double)best);
        if (DECAY) {
            v = decay_value(v, cell_size, decay_rate);
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        }
        out[(int64_t)r * W + c] = v;
    }
    if (DECAY && minmax) block_minmax_atomic<kEdtRowThreads>(mn, mx, minmax, s_red);
}

static int edt_check_shape(const char* what, int H, int W) {
    AVL_REQUIRE(H > 0 && W > 0 && H <= kEdtMaxSide && W <= kEdtMaxSide, "%s: bad shape %d x %d (sides 1 .. %d)", what, H, W, kEdtMaxSide);
    return AVL_OK;
}

// the two passes; decay = false gives the plain distance
static int edt_launch(const uint8_t* img, int64_t ld, int H, int W, int invert, bool decay, double cell_size, double decay_rate,
                      double* out, double* minmax, int32_t* found, void* ws, hipStream_t st) {
    int32_t* g = (int32_t*)ws;
    AVL_HIP_CHECK(hipMemsetAsync(found, 0, sizeof(int32_t), st));
    if (minmax) {
        const int rc = decay_minmax_reset(minmax, st);
        if (rc != AVL_OK) return rc;
    }
    hipLaunchKernelGGL(edt_column_kernel, dim3((unsigned)((W + kEdtCols - 1) / kEdtCols)), dim3(kEdtCols * kEdtSegs), 0, st, img, ld, H, W,
                       invert, g, (int*)found);
    const int wpad = (W + kEdtTile - 1) / kEdtTile * kEdtTile;
    const size_t lds = (size_t)(wpad / kEdtTile) * sizeof(unsigned) + (size_t)wpad * sizeof(unsigned short);
    if (decay)
        hipLaunchKernelGGL(edt_row_kernel<true>, dim3((unsigned)H), dim3(kEdtRowThreads), lds, st, (const int32_t*)g, H, W, cell_size,
                           decay_rate, out, reinterpret_cast<unsigned long long*>(minmax));
    else
        hipLaunchKernelGGL(edt_row_kernel<false>, dim3((unsigned)H), dim3(kEdtRowThreads), lds, st, (const int32_t*)g, H, W, 1.0, 0.0, out,
                           (unsigned long long*)nullptr);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_edt2d_work_bytes(int H, int W, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_edt2d_work_bytes: null output");
    int rc = edt_check_shape("avl_edt2d_work_bytes", H, W);
    if (rc != AVL_OK) return rc;
    *bytes = align256((size_t)H * W * sizeof(int32_t));
    return AVL_OK;
}

int avl_edt2d(const uint8_t* d_image_u8, int64_t ld, int H, int W, int invert, double* d_out_f64, int32_t* d_found, void* ws,
              size_t ws_bytes, void* stream) {
    size_t need = 0;
    int rc = edt_check_shape("avl_edt2d", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_image_u8 && d_out_f64 && d_found, "avl_edt2d: null image, output or flag pointer");
    AVL_REQUIRE(ld >= W, "avl_edt2d: rows of %lld cells cannot hold %d columns", (long long)ld, W);
    rc = avl_edt2d_work_bytes(H, W, &need);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_edt2d: workspace of %zu bytes, need %zu", ws_bytes, need);
    return edt_launch(d_image_u8, ld, H, W, invert, false, 1.0, 0.0, d_out_f64, nullptr, d_found, ws, as_stream(stream));
}

int avl_mask_decay_2d(const uint8_t* d_mask_u8, int64_t ld, int H, int W, double cell_size, double decay_rate, int normalize,
                      double* d_out_f64, double* d_minmax, int32_t* d_found, void* ws, size_t ws_bytes, void* stream) {
    size_t need = 0;
    int rc = edt_check_shape("avl_mask_decay_2d", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_mask_u8 && d_out_f64 && d_found, "avl_mask_decay_2d: null mask, output or flag pointer");
    AVL_REQUIRE(ld >= W, "avl_mask_decay_2d: rows of %lld cells cannot hold %d columns", (long long)ld, W);
    AVL_REQUIRE(std::isfinite(decay_rate) && decay_rate >= 0.0, "avl_mask_decay_2d: decay_rate must be finite and >= 0");
    AVL_REQUIRE(std::isfinite(cell_size) && cell_size > 0.0, "avl_mask_decay_2d: cell_size must be finite and > 0");
    AVL_REQUIRE(!normalize || d_minmax, "avl_mask_decay_2d: the normalisation needs d_minmax");
    rc = avl_edt2d_work_bytes(H, W, &need);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_mask_decay_2d: workspace of %zu bytes, need %zu", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    rc = edt_launch(d_mask_u8, ld, H, W, 1, true, cell_size, decay_rate, d_out_f64, d_minmax, d_found, ws, st);
    if (rc != AVL_OK || !normalize) return rc;
    return decay_normalize(d_out_f64, d_minmax, (int64_t)H * W, nullptr, st);
}

}  // extern "C"
