// 2-D image morphology for gfx950: the SciPy / OpenCV calls that smooth top-down masks upstream.
//
// Replaces (upstream reference, path:line):
//   avlmaps/map/map.py:169-181     Map._dilate_map   (cv2.resize x2 -> gaussian_filter -> > 0.5 -> binary_dilation(3 x 3) -> cv2.resize x1/2)
//   avlmaps/map/vlmap.py:166-171   VLMap.get_pos     (binary_closing(iterations=3) -> gaussian_filter(0.8) -> > 0.5 -> binary_dilation)
// Images are row-major uint8 (1 = true) or float64, at most 2 * gs per side: they live in L2 / Infinity Cache, so the number of
// launches and of dependent passes decides the time, not HBM.  This file is compiled with -ffp-contract=off: the gaussian adds
// and multiplies in SciPy's order (ni_filters.c NI_Correlate1D, symmetric branch) and must round like it.
//
// Binary morphology, k iterations of the 3 x 3 cross / box with border_value 0 = one pass with the L1 diamond / the Chebyshev
// square of radius k, cells outside the image counting as 0 for dilation AND erosion.
//   k <= kStencilMax   one launch: a (32 + 2k)^2 LDS tile, every output walks the footprint
//   larger k           two launches: (1) per cell the horizontal distance to the nearest TARGET cell of its row, capped at k + 1
//                      (target = a set cell for dilation, a clear cell or a column outside the image for erosion);
//                      (2) per cell: is there a row offset dr, |dr| <= k, with dist[r + dr][c] <= width(dr)?  width = k for the
//                      square, k - |dr| for the diamond; rows outside the image are all target for erosion.
#include <cmath>

#include "avl_common.h"

namespace avl {

constexpr int kStencilMax = 4;       // largest radius of the one-launch stencil
constexpr int kMorphMaxRadius = 127; // distances are bytes
constexpr int kGaussMaxRadius = 32;
constexpr int kTile = 32;

struct GaussW {
    double w[2 * kGaussMaxRadius + 1];
};

// scipy.ndimage mode 'reflect' (d c b a | a b c d | d c b a), any distance outside
__device__ __forceinline__ int reflect_index(int i, int n) {
    if (i >= 0 && i < n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// ---------------------------------------------------------------------------------------------- binary morphology
// in: (H, W) cells with row stride ld.  erode = 0: OR over the footprint, 1: AND (outside the image = 0 for both).
__global__ __launch_bounds__(256) void morph_stencil_kernel(const uint8_t* __restrict__ in, int64_t ld, int H, int W, int k, int box,
                                                            int erode, uint8_t* __restrict__ out) {
    __shared__ uint8_t tile[kTile + 2 * kStencilMax][kTile + 2 * kStencilMax + 4];
    const int r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
    const int side = kTile + 2 * k;
    for (int i = threadIdx.x; i < side * side; i += 256) {
        const int tr = i / side, tc = i - tr * side;
        const int r = r0 + tr - k, c = c0 + tc - k;
        tile[tr][tc] = (r >= 0 && r < H && c >= 0 && c < W) ? (in[(int64_t)r * ld + c] != 0) : 0;
    }
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = c0 + tx;
    for (int q = 0; q < 4; ++q) {
        const int lr = ty + 8 * q, r = r0 + lr;
        if (r >= H || c >= W) continue;
        int any = 0, all = 1;
        for (int dr = -k; dr <= k; ++dr) {
            const int w = box ? k : k - (dr < 0 ? -dr : dr);
            for (int dc = -w; dc <= w; ++dc) {
                const int v = tile[lr + k + dr][tx + k + dc];
                any |= v;
                all &= v;
            }
        }
        out[(int64_t)r * W + c] = (uint8_t)(erode ? all : any);
    }
}

__device__ __forceinline__ bool is_target(const uint8_t* __restrict__ in, int64_t ld, int W, int r, int c, int erode) {
    if (c < 0 || c >= W) return erode != 0;
    return (in[(int64_t)r * ld + c] != 0) != (erode != 0);
}

__global__ __launch_bounds__(256) void morph_rowdist_kernel(const uint8_t* __restrict__ in, int64_t ld, int H, int W, int k, int erode,
                                                            uint8_t* __restrict__ dist) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= H || c >= W) return;
    int d = 0;
    for (; d <= k; ++d)
        if (is_target(in, ld, W, r, c - d, erode) || is_target(in, ld, W, r, c + d, erode)) break;
    dist[(int64_t)r * W + c] = (uint8_t)d;      // k + 1 when no target lies within k
}

// found(r, c): a target within the footprint centred on (r, c), from the row distances
__device__ __forceinline__ bool footprint_hit(const uint8_t* __restrict__ dist, int H, int W, int r, int c, int k, int box, int erode) {
    for (int dr = -k; dr <= k; ++dr) {
        const int rr = r + dr;
        if (rr < 0 || rr >= H) {
            if (erode) return true;
            continue;
        }
        const int w = box ? k : k - (dr < 0 ? -dr : dr);
        if ((int)dist[(int64_t)rr * W + c] <= w) return true;
    }
    return false;
}

__global__ __launch_bounds__(256) void morph_coldist_kernel(const uint8_t* __restrict__ dist, int H, int W, int k, int box, int erode,
                                                            uint8_t* __restrict__ out) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= H || c >= W) return;
    const bool hit = footprint_hit(dist, H, W, r, c, k, box, erode);
    out[(int64_t)r * W + c] = (uint8_t)(erode ? !hit : hit);
}

// ---------------------------------------------------------------------------------------------- gaussian
struct SrcU8 {
    const uint8_t* p;
    int64_t ld;
    __device__ __forceinline__ double at(int r, int c) const { return p[(int64_t)r * ld + c] != 0 ? 1.0 : 0.0; }
};
struct SrcF64 {
    const double* p;
    int64_t ld;
    __device__ __forceinline__ double at(int r, int c) const { return p[(int64_t)r * ld + c]; }
};
struct SrcF32 {
    const float* p;
    int64_t ld;
    __device__ __forceinline__ double at(int r, int c) const { return (double)p[(int64_t)r * ld + c]; }
};
// the (2h, 2w) bilinear x2 up-sampling of an (h, w) 0/1 image, never stored (cv2.resize, INTER_LINEAR, half-pixel centres,
// replicated border): every value is a multiple of 1/16, exact in any evaluation order
struct SrcUp2 {
    const uint8_t* p;
    int h, w;
    __device__ __forceinline__ double at(int y, int x) const {
        // destination index i samples the source at (i + 0.5) / 2 - 0.5: floor = (i - 1) >> 1, fraction 0.75 (even i) / 0.25 (odd i)
        const int ys = (y - 1) >> 1, xs = (x - 1) >> 1;
        const double fy = (y & 1) ? 0.25 : 0.75, fx = (x & 1) ? 0.25 : 0.75;
        const int y0 = ys < 0 ? 0 : ys, y1 = ys + 1 > h - 1 ? h - 1 : ys + 1;
        const int x0 = xs < 0 ? 0 : xs, x1 = xs + 1 > w - 1 ? w - 1 : xs + 1;
        const double a = p[(int64_t)y0 * w + x0] != 0, b = p[(int64_t)y0 * w + x1] != 0;
        const double c = p[(int64_t)y1 * w + x0] != 0, d = p[(int64_t)y1 * w + x1] != 0;
        const double top = a * (1.0 - fx) + b * fx, bot = c * (1.0 - fx) + d * fx;
        return top * (1.0 - fy) + bot * fy;
    }
};

// axis 0 (down the columns): out[r, c] = sum_j w[j] src[reflect(r + j), c] in SciPy's symmetric order.  T = the array type SciPy
// filters in: double, or float for a float32 image -- SciPy then still accumulates every line in double and rounds what it stores
template <class Src, class T = double>
__global__ __launch_bounds__(256) void gauss_axis0_kernel(Src src, int H, int W, GaussW gw, int radius, T* __restrict__ out) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= H || c >= W) return;
    double tmp = src.at(r, c) * gw.w[radius];
    for (int j = -radius; j < 0; ++j) tmp += (src.at(reflect_index(r + j, H), c) + src.at(reflect_index(r - j, H), c)) * gw.w[j + radius];
    out[(int64_t)r * W + c] = (T)tmp;
}

// axis 1 (along the rows) of the intermediate (float64, or float32 rounded as SciPy stores it); optional value output, optional
// `> threshold` output of the stored value, and (any != nullptr) a flag that is set when one cell passes the threshold
template <class T = double>
__global__ __launch_bounds__(256) void gauss_axis1_kernel(const T* __restrict__ in, int H, int W, GaussW gw, int radius,
                                                          T* __restrict__ out, uint8_t* __restrict__ gt, double threshold,
                                                          int* __restrict__ any) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= H || c >= W) return;
    const T* row = in + (int64_t)r * W;
    double tmp = (double)row[c] * gw.w[radius];
    for (int j = -radius; j < 0; ++j)
        tmp += ((double)row[reflect_index(c + j, W)] + (double)row[reflect_index(c - j, W)]) * gw.w[j + radius];
    const T val = (T)tmp;
    if (out) out[(int64_t)r * W + c] = val;
    if (gt) {
        const bool on = (double)val > threshold;
        gt[(int64_t)r * W + c] = on;
        if (any && on) atomicOr(any, 1);
    }
}

// ---------------------------------------------------------------------------------------------- resizes
template <class Src>
__global__ __launch_bounds__(256) void resize_up_kernel(Src src, int h, int w, double* __restrict__ out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= 2 * h || x >= 2 * w) return;
    const int ys = (y - 1) >> 1, xs = (x - 1) >> 1;
    const double fy = (y & 1) ? 0.25 : 0.75, fx = (x & 1) ? 0.25 : 0.75;
    const int y0 = ys < 0 ? 0 : ys, y1 = ys + 1 > h - 1 ? h - 1 : ys + 1;
    const int x0 = xs < 0 ? 0 : xs, x1 = xs + 1 > w - 1 ? w - 1 : xs + 1;
    const double top = src.at(y0, x0) * (1.0 - fx) + src.at(y0, x1) * fx;
    const double bot = src.at(y1, x0) * (1.0 - fx) + src.at(y1, x1) * fx;
    out[(int64_t)y * (2 * w) + x] = top * (1.0 - fy) + bot * fy;
}

template <class Src>
__global__ __launch_bounds__(256) void resize_down_kernel(Src src, int h, int w, double* __restrict__ out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h || x >= w) return;
    const double s = (src.at(2 * y, 2 * x) + src.at(2 * y, 2 * x + 1)) + (src.at(2 * y + 1, 2 * x) + src.at(2 * y + 1, 2 * x + 1));
    out[(int64_t)y * w + x] = s * 0.25;
}

// ---------------------------------------------------------------------------------------------- tail of _dilate_map
// dist: row distances (radius k, dilation) of the (2h, 2w) thresholded image.  Per (h, w) cell the four box-dilated cells of its
// 2 x 2 block, their mean (the x1/2 resize) and `mean == 0`.
__global__ __launch_bounds__(256) void dilate_down_kernel(const uint8_t* __restrict__ dist, int h, int w, int k, double* __restrict__ out,
                                                          uint8_t* __restrict__ zero) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h || x >= w) return;
    const int H2 = 2 * h, W2 = 2 * w;
    int n = 0;
    for (int q = 0; q < 4; ++q) n += footprint_hit(dist, H2, W2, 2 * y + (q >> 1), 2 * x + (q & 1), k, 1, 0) ? 1 : 0;
    if (out) out[(int64_t)y * w + x] = (double)n * 0.25;
    if (zero) zero[(int64_t)y * w + x] = n == 0;
}

// dilate_iter = 0: SciPy iterates the 3 x 3 box until nothing changes -- one set cell fills the image
__global__ __launch_bounds__(256) void fill_from_flag_kernel(const int* __restrict__ any, int64_t cells, double* __restrict__ out,
                                                             uint8_t* __restrict__ zero) {
    const int on = *any != 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < cells; p += (int64_t)gridDim.x * blockDim.x) {
        if (out) out[p] = on ? 1.0 : 0.0;
        if (zero) zero[p] = !on;
    }
}

static dim3 grid2d(int H, int W) { return dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)); }

// one morphology op on an (H, W) image with row stride ld; d_tmp (H * W bytes) is used above the stencil radius only
static int launch_morph(const uint8_t* in, int64_t ld, int H, int W, int erode, int box, int k, uint8_t* out, uint8_t* tmp, hipStream_t st) {
    if (k <= kStencilMax) {
        hipLaunchKernelGGL(morph_stencil_kernel, dim3((W + kTile - 1) / kTile, (H + kTile - 1) / kTile), dim3(256), 0, st, in, ld, H, W, k, box,
                           erode, out);
    } else {
        hipLaunchKernelGGL(morph_rowdist_kernel, grid2d(H, W), dim3(256), 0, st, in, ld, H, W, k, erode, tmp);
        hipLaunchKernelGGL(morph_coldist_kernel, grid2d(H, W), dim3(256), 0, st, (const uint8_t*)tmp, H, W, k, box, erode, out);
    }
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

static int make_weights(const double* h_weights, int radius, GaussW* gw, const char* what) {
    AVL_REQUIRE(h_weights && radius >= 0 && radius <= kGaussMaxRadius, "%s: radius %d outside [0, %d] or null weights", what, radius,
                kGaussMaxRadius);
    for (int i = 0; i < 2 * radius + 1; ++i) gw->w[i] = h_weights[i];
    for (int i = 2 * radius + 1; i < 2 * kGaussMaxRadius + 1; ++i) gw->w[i] = 0.0;
    return AVL_OK;
}

// scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius) in float64, in its order of operations
static void gaussian_weights(double sigma, int radius, double* w) {
    const double s2 = sigma * sigma;
    double sum = 0.0;
    for (int i = 0; i < 2 * radius + 1; ++i) {
        const double x = (double)(i - radius);
        w[i] = exp(-0.5 / s2 * (x * x));
    }
    for (int i = 0; i < 2 * radius + 1; ++i) sum += w[i];
    for (int i = 0; i < 2 * radius + 1; ++i) w[i] /= sum;
}

constexpr int kMaxSide = 32768;

// workspace of avl_dilate_map for an (H, W) map: a flag word, then three images at twice the resolution
static bool dilate_shape_ok(int H, int W) { return H > 0 && W > 0 && H <= kMaxSide / 2 && W <= kMaxSide / 2; }
struct DilateWork { int* any; double* tmp; uint8_t *thr, *dist; size_t total; };
static DilateWork dilate_work(int H, int W, void* ws) {
    const size_t up = (size_t)4 * H * W;
    Carver c(ws);
    DilateWork w;
    w.any = c.ptr<int>(sizeof(int));
    w.tmp = c.ptr<double>(up * sizeof(double));
    w.thr = c.ptr<uint8_t>(up);
    w.dist = c.ptr<uint8_t>(up);
    w.total = c.total();
    return w;
}

// workspace of avl_mask_foreground for an (H, W) crop
static bool foreground_shape_ok(int H, int W) { return H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide; }
struct ForegroundWork { double* tmp; uint8_t *a, *b; size_t total; };
static ForegroundWork foreground_work(int H, int W, void* ws) {
    const size_t cells = (size_t)H * W;
    Carver c(ws);
    ForegroundWork w;
    w.tmp = c.ptr<double>(cells * sizeof(double));
    w.a = c.ptr<uint8_t>(cells);
    w.b = c.ptr<uint8_t>(cells);
    w.total = c.total();
    return w;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_morph_binary(const uint8_t* d_in, int H, int W, int op, int structure, int iterations, uint8_t* d_out, uint8_t* d_tmp,
                     void* stream) {
    AVL_REQUIRE(H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide && d_in && d_out, "avl_morph_binary: bad image arguments");
    AVL_REQUIRE(op == AVL_MORPH_DILATE || op == AVL_MORPH_ERODE, "avl_morph_binary: op %d is neither dilate nor erode", op);
    AVL_REQUIRE(structure == AVL_MORPH_CROSS || structure == AVL_MORPH_BOX, "avl_morph_binary: structure %d is neither cross nor box", structure);
    AVL_REQUIRE(iterations >= 1 && iterations <= kMorphMaxRadius, "avl_morph_binary: iterations %d outside [1, %d]", iterations, kMorphMaxRadius);
    AVL_REQUIRE(d_in != d_out, "avl_morph_binary: in-place call");
    AVL_REQUIRE(iterations <= kStencilMax || d_tmp, "avl_morph_binary: more than %d iterations need d_tmp (H * W bytes)", kStencilMax);
    return launch_morph(d_in, W, H, W, op == AVL_MORPH_ERODE, structure == AVL_MORPH_BOX, iterations, d_out, d_tmp, as_stream(stream));
}

int avl_gauss2d_f64(const void* d_in, int in_is_u8, int H, int W, const double* h_weights, int radius, double* d_out_f64,
                    uint8_t* d_out_gt_u8, double threshold, double* d_tmp, void* stream) {
    AVL_REQUIRE(H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide && d_in && d_tmp, "avl_gauss2d_f64: bad image arguments");
    AVL_REQUIRE(d_out_f64 || d_out_gt_u8, "avl_gauss2d_f64: no output requested");
    GaussW gw;
    int rc = make_weights(h_weights, radius, &gw, "avl_gauss2d_f64");
    if (rc != AVL_OK) return rc;
    hipStream_t st = as_stream(stream);
    if (in_is_u8)
        hipLaunchKernelGGL(gauss_axis0_kernel<SrcU8>, grid2d(H, W), dim3(256), 0, st, SrcU8{(const uint8_t*)d_in, W}, H, W, gw, radius, d_tmp);
    else
        hipLaunchKernelGGL(gauss_axis0_kernel<SrcF64>, grid2d(H, W), dim3(256), 0, st, SrcF64{(const double*)d_in, W}, H, W, gw, radius, d_tmp);
    hipLaunchKernelGGL(gauss_axis1_kernel<double>, grid2d(H, W), dim3(256), 0, st, (const double*)d_tmp, H, W, gw, radius, d_out_f64, d_out_gt_u8,
                       threshold, (int*)nullptr);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_gauss2d_f32(const void* d_in, int in_is_u8, int64_t ld, int H, int W, const double* h_weights, int radius, float* d_out_f32,
                    uint8_t* d_out_gt_u8, double threshold, float* d_tmp, void* stream) {
    AVL_REQUIRE(H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide && d_in && d_tmp && ld >= W, "avl_gauss2d_f32: bad image arguments");
    AVL_REQUIRE(d_out_f32 || d_out_gt_u8, "avl_gauss2d_f32: no output requested");
    GaussW gw;
    int rc = make_weights(h_weights, radius, &gw, "avl_gauss2d_f32");
    if (rc != AVL_OK) return rc;
    hipStream_t st = as_stream(stream);
    if (in_is_u8)
        hipLaunchKernelGGL((gauss_axis0_kernel<SrcU8, float>), grid2d(H, W), dim3(256), 0, st, SrcU8{(const uint8_t*)d_in, ld}, H, W, gw, radius,
                           d_tmp);
    else
        hipLaunchKernelGGL((gauss_axis0_kernel<SrcF32, float>), grid2d(H, W), dim3(256), 0, st, SrcF32{(const float*)d_in, ld}, H, W, gw, radius,
                           d_tmp);
    hipLaunchKernelGGL(gauss_axis1_kernel<float>, grid2d(H, W), dim3(256), 0, st, (const float*)d_tmp, H, W, gw, radius, d_out_f32, d_out_gt_u8,
                       threshold, (int*)nullptr);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_resize2x_up_f64(const void* d_in, int in_is_u8, int H, int W, double* d_out, void* stream) {
    AVL_REQUIRE(H > 0 && W > 0 && H <= kMaxSide / 2 && W <= kMaxSide / 2 && d_in && d_out, "avl_resize2x_up_f64: bad arguments");
    hipStream_t st = as_stream(stream);
    if (in_is_u8)
        hipLaunchKernelGGL(resize_up_kernel<SrcU8>, grid2d(2 * H, 2 * W), dim3(256), 0, st, SrcU8{(const uint8_t*)d_in, W}, H, W, d_out);
    else
        hipLaunchKernelGGL(resize_up_kernel<SrcF64>, grid2d(2 * H, 2 * W), dim3(256), 0, st, SrcF64{(const double*)d_in, W}, H, W, d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_resize2x_down_f64(const void* d_in, int in_is_u8, int H, int W, double* d_out, void* stream) {
    AVL_REQUIRE(H > 0 && W > 0 && H <= kMaxSide / 2 && W <= kMaxSide / 2 && d_in && d_out, "avl_resize2x_down_f64: bad arguments");
    hipStream_t st = as_stream(stream);
    if (in_is_u8)
        hipLaunchKernelGGL(resize_down_kernel<SrcU8>, grid2d(H, W), dim3(256), 0, st, SrcU8{(const uint8_t*)d_in, 2 * (int64_t)W}, H, W, d_out);
    else
        hipLaunchKernelGGL(resize_down_kernel<SrcF64>, grid2d(H, W), dim3(256), 0, st, SrcF64{(const double*)d_in, 2 * (int64_t)W}, H, W, d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_dilate_map_work_bytes(int H, int W, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_dilate_map_work_bytes: null output");
    AVL_REQUIRE(dilate_shape_ok(H, W), "avl_dilate_map_work_bytes: bad shape %d x %d", H, W);
    *bytes = dilate_work(H, W, nullptr).total;
    return AVL_OK;
}

int avl_dilate_map(const uint8_t* d_binary_u8, int H, int W, int dilate_iter, double sigma, double* d_out_f64, uint8_t* d_out_zero_u8,
                   void* ws, size_t ws_bytes, void* stream) {
    AVL_REQUIRE(dilate_shape_ok(H, W), "avl_dilate_map: bad shape %d x %d", H, W);
    const auto [any, tmp, thr, dist, need] = dilate_work(H, W, ws);
    AVL_REQUIRE(d_binary_u8 && (d_out_f64 || d_out_zero_u8), "avl_dilate_map: null input or no output requested");
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_dilate_map: workspace of %zu bytes, need %zu", ws_bytes, need);
    AVL_REQUIRE(dilate_iter >= 0 && 2 * dilate_iter <= kMorphMaxRadius, "avl_dilate_map: dilate_iter %d outside [0, %d]", dilate_iter,
                kMorphMaxRadius / 2);
    AVL_REQUIRE(sigma > 1e-15, "avl_dilate_map: sigma must be positive");     // (SciPy skips the filter below that)
    const int radius = (int)(3.0 * sigma + 0.5);
    AVL_REQUIRE(radius <= kGaussMaxRadius, "avl_dilate_map: sigma %g gives radius %d > %d", sigma, radius, kGaussMaxRadius);
    GaussW gw;
    for (int i = 0; i < 2 * kGaussMaxRadius + 1; ++i) gw.w[i] = 0.0;
    gaussian_weights(sigma, radius, gw.w);
    hipStream_t st = as_stream(stream);
    const int H2 = 2 * H, W2 = 2 * W;
    if (dilate_iter == 0) AVL_HIP_CHECK(hipMemsetAsync(any, 0, sizeof(int), st));
    hipLaunchKernelGGL(gauss_axis0_kernel<SrcUp2>, grid2d(H2, W2), dim3(256), 0, st, SrcUp2{d_binary_u8, H, W}, H2, W2, gw, radius, tmp);
    hipLaunchKernelGGL(gauss_axis1_kernel<double>, grid2d(H2, W2), dim3(256), 0, st, (const double*)tmp, H2, W2, gw, radius, (double*)nullptr, thr, 0.5,
                       dilate_iter == 0 ? any : (int*)nullptr);
    if (dilate_iter == 0) {
        const int64_t cells = (int64_t)H * W;
        int64_t b = (cells + 255) / 256;
        if (b > 4096) b = 4096;
        hipLaunchKernelGGL(fill_from_flag_kernel, dim3((unsigned)b), dim3(256), 0, st, (const int*)any, cells, d_out_f64, d_out_zero_u8);
    } else {
        const int k = 2 * dilate_iter;
        hipLaunchKernelGGL(morph_rowdist_kernel, grid2d(H2, W2), dim3(256), 0, st, (const uint8_t*)thr, (int64_t)W2, H2, W2, k, 0, dist);
        hipLaunchKernelGGL(dilate_down_kernel, grid2d(H, W), dim3(256), 0, st, (const uint8_t*)dist, H, W, k, d_out_f64, d_out_zero_u8);
    }
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_mask_foreground_work_bytes(int H, int W, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_mask_foreground_work_bytes: null output");
    AVL_REQUIRE(foreground_shape_ok(H, W), "avl_mask_foreground_work_bytes: bad shape %d x %d", H, W);
    *bytes = foreground_work(H, W, nullptr).total;
    return AVL_OK;
}

int avl_mask_foreground(const uint8_t* d_mask2d_u8, int64_t ld, int r0, int r1, int c0, int c1, uint8_t* d_out_u8, void* ws, size_t ws_bytes,
                        void* stream) {
    AVL_REQUIRE(d_mask2d_u8 && d_out_u8 && r0 >= 0 && c0 >= 0 && r1 > r0 && c1 > c0 && (int64_t)c1 <= ld,
                "avl_mask_foreground: bad crop [%d:%d, %d:%d] of rows of %lld cells", r0, r1, c0, c1, (long long)ld);
    const int H = r1 - r0, W = c1 - c0;
    AVL_REQUIRE(foreground_shape_ok(H, W), "avl_mask_foreground: bad shape %d x %d", H, W);
    const auto [tmp, a, b, need] = foreground_work(H, W, ws);
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_mask_foreground: workspace of %zu bytes, need %zu", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const int radius = 2;                       // int(3 * 0.8 + 0.5)
    GaussW gw;
    for (int i = 0; i < 2 * kGaussMaxRadius + 1; ++i) gw.w[i] = 0.0;
    gaussian_weights(0.8, radius, gw.w);
    // binary_closing(iterations=3): dilation, then erosion, both with the crop's own border
    int rc = launch_morph(d_mask2d_u8 + (int64_t)r0 * ld + c0, ld, H, W, 0, 0, 3, a, nullptr, st);
    if (rc != AVL_OK) return rc;
    rc = launch_morph(a, W, H, W, 1, 0, 3, b, nullptr, st);
    if (rc != AVL_OK) return rc;
    hipLaunchKernelGGL(gauss_axis0_kernel<SrcU8>, grid2d(H, W), dim3(256), 0, st, SrcU8{b, W}, H, W, gw, radius, tmp);
    hipLaunchKernelGGL(gauss_axis1_kernel<double>, grid2d(H, W), dim3(256), 0, st, (const double*)tmp, H, W, gw, radius, (double*)nullptr, a, 0.5,
                       (int*)nullptr);
    AVL_HIP_CHECK(hipGetLastError());
    return launch_morph(a, W, H, W, 0, 0, 1, d_out_u8, nullptr, st);
}

}  // extern "C"
