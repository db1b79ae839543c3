// Headless rendering of per-voxel heat for gfx950: colour blend, top-down overlay and a z-buffered camera splat.
//
// Replaces (upstream reference, path:line):
//   avlmaps/utils/visualize_utils.py:59-64    convert_heatmap_to_rgb     (NumPy + cv2.applyColorMap over all N voxels)
//   avlmaps/utils/visualize_utils.py:117-128  visualize_heatmap_2d       (the same blend on the top-down image)
//   avlmaps/utils/visualize_utils.py:10-26    visualize_rgb_map_3d       (an Open3D window upstream; here a pinhole splat)
// The colour table is DATA: 256 RGB triples in a 768-byte device buffer.  Nothing here knows what JET looks like.
//
// The blend is NumPy 2's arithmetic for `float32_array * python_float + uint8_array * python_float`:
//   float32(table[idx]) * float32(t)   is a float32 product (the Python float is a weak scalar next to a float32 array),
//   rgb * (1 - t)                      is a float64 product (an integer array next to a Python float gives the default float),
//   and their sum is float64.  The file is compiled with -ffp-contract=off: none of it may fuse.
// Every image is unique: the two scatters are integer atomicMax / atomicMin on keys that no two voxels share.
#include "avl_common.h"

namespace avl {

constexpr int kErrPos = 1;    // a voxel position outside the map
constexpr int kErrHeat = 2;   // a heat outside [0, 1] or NaN: (heat * 255).astype(uint8) is undefined there

static unsigned render_grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    const int64_t maxb = (int64_t)num_cus() * 16;
    if (b > maxb) b = maxb;
    return (unsigned)(b < 1 ? 1 : b);
}

// idx = (heat * 255).astype(np.uint8), the product in the heat's own dtype; false when the cast is undefined
__device__ __forceinline__ bool heat_index_f32(float h, int& idx) {
    if (!(h >= 0.0f && h <= 1.0f)) return false;
    idx = (int)(h * 255.0f);
    return true;
}
__device__ __forceinline__ bool heat_index_f64(double h, int& idx) {
    if (!(h >= 0.0 && h <= 1.0)) return false;
    idx = (int)(h * 255.0);
    return true;
}
__device__ __forceinline__ bool heat_index(const void* heat, int is_f64, int64_t i, int& idx) {
    return is_f64 ? heat_index_f64(((const double*)heat)[i], idx) : heat_index_f32(((const float*)heat)[i], idx);
}

__device__ __forceinline__ double blend(uint8_t tab, uint8_t rgb, float t32, double one_minus_t) {
    const float a = (float)tab * t32;                 // float32 product
    return (double)a + (double)rgb * one_minus_t;     // float64 product and sum
}

__global__ __launch_bounds__(256) void colorize_kernel(const void* __restrict__ heat, int is_f64, const uint8_t* __restrict__ rgb,
                                                       const uint8_t* __restrict__ table, int64_t N, float t32, double one_minus_t,
                                                       double* __restrict__ out_f64, uint8_t* __restrict__ out_u8, int* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        int idx = 0;
        if (!heat_index(heat, is_f64, i, idx)) { atomicOr(err, kErrHeat); continue; }
        for (int k = 0; k < 3; ++k) {
            const double v = blend(table[3 * idx + k], rgb[3 * i + k], t32, one_minus_t);
            if (out_f64) out_f64[3 * i + k] = v;
            if (out_u8) out_u8[3 * i + k] = (uint8_t)(int)v;      // .astype(np.uint8) of a value in [0, 256): truncation
        }
    }
}

// Top-down pass 1.  top[cell] = max over the column of ((h ^ sign) << 32) | (id + 1): the highest voxel, 0 = empty (id + 1 >= 1);
// hmax[cell] = max of the heat's bit pattern (non-negative floats order as unsigned integers; float32 bits are zero-extended).
__global__ __launch_bounds__(256) void topdown_scatter_kernel(const int32_t* __restrict__ pos, const void* __restrict__ heat, int is_f64,
                                                              int64_t N, int gs, int rmin, int rmax, int cmin, int cmax,
                                                              unsigned long long* __restrict__ top, unsigned long long* __restrict__ hmax,
                                                              int* __restrict__ err) {
    const int W = cmax - cmin + 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        int r = pos[3 * i], c = pos[3 * i + 1];
        const int h = pos[3 * i + 2];
        if (r < 0) r += gs;     // numpy index wrap
        if (c < 0) c += gs;
        if (r < 0 || r >= gs || c < 0 || c >= gs) { atomicOr(err, kErrPos); continue; }
        unsigned long long bits;
        if (is_f64) {
            const double v = ((const double*)heat)[i];
            if (!(v >= 0.0 && v <= 1.0)) { atomicOr(err, kErrHeat); continue; }
            bits = (unsigned long long)__double_as_longlong(v);
        } else {
            const float v = ((const float*)heat)[i];
            if (!(v >= 0.0f && v <= 1.0f)) { atomicOr(err, kErrHeat); continue; }
            bits = (unsigned long long)__float_as_uint(v);
        }
        if (r < rmin || r > rmax || c < cmin || c > cmax) continue;
        const int64_t cell = (int64_t)(r - rmin) * W + (c - cmin);
        const unsigned long long key = ((unsigned long long)((uint32_t)h ^ 0x80000000u) << 32) | (unsigned long long)((uint32_t)i + 1u);
        atomicMax(&top[cell], key);
        atomicMax(&hmax[cell], bits);
    }
}

__global__ __launch_bounds__(256) void topdown_paint_heat_kernel(const unsigned long long* __restrict__ top,
                                                                 const unsigned long long* __restrict__ hmax, int is_f64,
                                                                 const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ table,
                                                                 int64_t cells, float t32, double one_minus_t, uint8_t bg0, uint8_t bg1,
                                                                 uint8_t bg2, uint8_t* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < cells; p += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = top[p];
        if (key == 0ull) {
            out[3 * p + 0] = bg0;
            out[3 * p + 1] = bg1;
            out[3 * p + 2] = bg2;
            continue;
        }
        const int64_t id = (int64_t)(uint32_t)(key & 0xFFFFFFFFull) - 1;
        const unsigned long long bits = hmax[p];
        const int idx = is_f64 ? (int)(__longlong_as_double((long long)bits) * 255.0) : (int)(__uint_as_float((uint32_t)bits) * 255.0f);
        for (int k = 0; k < 3; ++k) out[3 * p + k] = (uint8_t)(int)blend(table[3 * idx + k], rgb[3 * id + k], t32, one_minus_t);
    }
}

struct Mat34 {
    double m[12];
};

// Camera pass 1, one voxel per thread, float64 in the documented operation order.  zbuf[pixel] = min of
// (bits(float32(z)) << 32) | id: z > znear >= 0, so the float32 bits order like the depth; the nearest voxel wins and an equal
// float32 depth goes to the smaller id.  ~0 = empty (no key reaches it: id < 2^31).
__global__ __launch_bounds__(256) void view_splat_kernel(const int32_t* __restrict__ pos, int64_t N, Mat34 T, double fx, double fy, double cx,
                                                         double cy, int W, int H, double znear, double smax,
                                                         unsigned long long* __restrict__ zbuf) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const double row = (double)pos[3 * i], col = (double)pos[3 * i + 1], hh = (double)pos[3 * i + 2];
        const double x = T.m[0] * row + T.m[1] * col + T.m[2] * hh + T.m[3] * 1.0;
        const double y = T.m[4] * row + T.m[5] * col + T.m[6] * hh + T.m[7] * 1.0;
        const double z = T.m[8] * row + T.m[9] * col + T.m[10] * hh + T.m[11] * 1.0;
        if (!(z > znear)) continue;
        const double u = fx * x / z + cx;
        const double v = fy * y / z + cy;
        const double half = fmin(0.5 * fx / z, 0.5 * smax);
        const double ulo = floor(u - half), uhi = floor(u + half), vlo = floor(v - half), vhi = floor(v + half);
        // compared as doubles before any conversion: a NaN or a huge coordinate never reaches an int
        if (!(uhi >= 0.0 && ulo <= (double)(W - 1) && vhi >= 0.0 && vlo <= (double)(H - 1))) continue;
        const int x0 = (int)fmax(ulo, 0.0), x1 = (int)fmin(uhi, (double)(W - 1));
        const int y0 = (int)fmax(vlo, 0.0), y1 = (int)fmin(vhi, (double)(H - 1));
        const unsigned long long key = ((unsigned long long)__float_as_uint((float)z) << 32) | (unsigned long long)(uint32_t)i;
        for (int py = y0; py <= y1; ++py)
            for (int px = x0; px <= x1; ++px) atomicMin(&zbuf[(int64_t)py * W + px], key);
    }
}

__global__ __launch_bounds__(256) void view_resolve_kernel(const unsigned long long* __restrict__ zbuf, const uint8_t* __restrict__ color,
                                                           int64_t pixels, uint8_t bg0, uint8_t bg1, uint8_t bg2,
                                                           uint8_t* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = zbuf[p];
        if (key == ~0ull) {
            out[3 * p + 0] = bg0;
            out[3 * p + 1] = bg1;
            out[3 * p + 2] = bg2;
        } else {
            const int64_t id = (int64_t)(key & 0xFFFFFFFFull);
            out[3 * p + 0] = color[3 * id + 0];
            out[3 * p + 1] = color[3 * id + 1];
            out[3 * p + 2] = color[3 * id + 2];
        }
    }
}

struct RenderErr {
    int* d = nullptr;
    hipStream_t st;
    int init(hipStream_t s) {
        st = s;
        AVL_HIP_CHECK(hipMallocAsync((void**)&d, sizeof(int), st));
        AVL_HIP_CHECK(hipMemsetAsync(d, 0, sizeof(int), st));
        return AVL_OK;
    }
    int finish(const char* what) {   // synchronises
        int h = 0;
        AVL_HIP_CHECK(hipMemcpyAsync(&h, d, sizeof(int), hipMemcpyDeviceToHost, st));
        AVL_HIP_CHECK(hipStreamSynchronize(st));
        (void)hipFreeAsync(d, st);
        if (h & kErrPos) {
            set_error("%s: a voxel position indexes outside the 2-D map (the reference raises IndexError here)", what);
            return AVL_ERR_INVALID;
        }
        if (h & kErrHeat) {
            set_error("%s: a heat value is NaN or outside [0, 1]: (heat * 255).astype(uint8) is undefined there", what);
            return AVL_ERR_INVALID;
        }
        return AVL_OK;
    }
};

static bool transparency_ok(double t) { return t >= 0.0 && t <= 1.0; }

constexpr int kViewMaxSide = 8192;

}  // namespace avl

using namespace avl;

extern "C" {

int avl_render_colorize(const void* d_heat, int heat_is_f64, const uint8_t* d_grid_rgb, const uint8_t* d_table, int64_t N,
                        double transparency, double* d_out_f64, uint8_t* d_out_u8, void* stream) {
    AVL_REQUIRE(N >= 0 && (heat_is_f64 == 0 || heat_is_f64 == 1), "avl_render_colorize: bad arguments");
    AVL_REQUIRE(transparency_ok(transparency), "avl_render_colorize: transparency %g is not in [0, 1]", transparency);
    AVL_REQUIRE(d_out_f64 || d_out_u8, "avl_render_colorize: null output (one of the two forms is required)");
    if (N == 0) return AVL_OK;
    AVL_REQUIRE(d_heat && d_grid_rgb && d_table, "avl_render_colorize: null input");
    hipStream_t st = as_stream(stream);
    RenderErr ef;
    int rc = ef.init(st);
    if (rc != AVL_OK) return rc;
    hipLaunchKernelGGL(colorize_kernel, dim3(render_grid_for(N)), dim3(256), 0, st, d_heat, heat_is_f64, d_grid_rgb, d_table, N,
                       (float)transparency, 1.0 - transparency, d_out_f64, d_out_u8, ef.d);
    AVL_HIP_CHECK(hipGetLastError());
    return ef.finish("avl_render_colorize");
}

int avl_render_topdown_work_bytes(int H, int W, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_render_topdown_work_bytes: null output");
    AVL_REQUIRE(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "avl_render_topdown_work_bytes: bad shape (%d, %d)", H, W);
    *bytes = (size_t)H * (size_t)W * 2 * sizeof(unsigned long long);
    return AVL_OK;
}

int avl_render_topdown(const int32_t* d_grid_pos, const void* d_heat, int heat_is_f64, const uint8_t* d_grid_rgb, const uint8_t* d_table,
                       int64_t N, int gs, int rmin, int rmax, int cmin, int cmax, double transparency, const uint8_t* h_background3,
                       uint8_t* d_out, void* ws, size_t ws_bytes, void* stream) {
    AVL_REQUIRE(N >= 0 && N < (1ll << 31) && gs > 0 && gs <= 16384 && (heat_is_f64 == 0 || heat_is_f64 == 1), "avl_render_topdown: bad arguments");
    AVL_REQUIRE(0 <= rmin && rmin <= rmax && rmax < gs && 0 <= cmin && cmin <= cmax && cmax < gs,
                "avl_render_topdown: window rows [%d, %d] columns [%d, %d] is not inside the (%d, %d) map", rmin, rmax, cmin, cmax, gs, gs);
    AVL_REQUIRE(transparency_ok(transparency), "avl_render_topdown: transparency %g is not in [0, 1]", transparency);
    AVL_REQUIRE(h_background3 && d_out, "avl_render_topdown: null background or output");
    const int H = rmax - rmin + 1, W = cmax - cmin + 1;
    size_t need = 0;
    int rc = avl_render_topdown_work_bytes(H, W, &need);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_render_topdown: workspace of %zu bytes, need %zu", ws_bytes, need);
    AVL_REQUIRE(N == 0 || (d_grid_pos && d_heat && d_grid_rgb && d_table), "avl_render_topdown: null input");
    hipStream_t st = as_stream(stream);
    const int64_t cells = (int64_t)H * W;
    unsigned long long* top = (unsigned long long*)ws;
    unsigned long long* hmax = top + cells;
    AVL_HIP_CHECK(hipMemsetAsync(ws, 0, need, st));
    RenderErr ef;
    rc = ef.init(st);
    if (rc != AVL_OK) return rc;
    if (N > 0)
        hipLaunchKernelGGL(topdown_scatter_kernel, dim3(render_grid_for(N)), dim3(256), 0, st, d_grid_pos, d_heat, heat_is_f64, N, gs, rmin,
                           rmax, cmin, cmax, top, hmax, ef.d);
    hipLaunchKernelGGL(topdown_paint_heat_kernel, dim3(render_grid_for(cells)), dim3(256), 0, st, top, hmax, heat_is_f64, d_grid_rgb, d_table,
                       cells, (float)transparency, 1.0 - transparency, h_background3[0], h_background3[1], h_background3[2], d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return ef.finish("avl_render_topdown");
}

int avl_render_view_work_bytes(int W, int H, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_render_view_work_bytes: null output");
    AVL_REQUIRE(H >= 1 && W >= 1 && H <= kViewMaxSide && W <= kViewMaxSide, "avl_render_view_work_bytes: bad image size %d x %d", W, H);
    *bytes = (size_t)H * (size_t)W * sizeof(unsigned long long);
    return AVL_OK;
}

int avl_render_view(const int32_t* d_grid_pos, const uint8_t* d_color_u8, int64_t N, const double* h_T34, double fx, double fy, double cx,
                    double cy, int W, int H, double znear, double smax, const uint8_t* h_background3, uint8_t* d_out, void* ws,
                    size_t ws_bytes, void* stream) {
    AVL_REQUIRE(N >= 0 && N < (1ll << 31), "avl_render_view: bad voxel count");
    size_t need = 0;
    int rc = avl_render_view_work_bytes(W, H, &need);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(h_T34 && h_background3 && d_out, "avl_render_view: null matrix, background or output");
    AVL_REQUIRE(znear >= 0.0 && znear < 1e300, "avl_render_view: znear %g must be finite and >= 0", znear);
    AVL_REQUIRE(smax >= 1.0 && smax <= (double)kViewMaxSide, "avl_render_view: footprint cap %g is not in [1, %d]", smax, kViewMaxSide);
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_render_view: workspace of %zu bytes, need %zu", ws_bytes, need);
    AVL_REQUIRE(N == 0 || (d_grid_pos && d_color_u8), "avl_render_view: null input");
    hipStream_t st = as_stream(stream);
    const int64_t pixels = (int64_t)H * W;
    unsigned long long* zbuf = (unsigned long long*)ws;
    AVL_HIP_CHECK(hipMemsetAsync(ws, 0xFF, need, st));
    if (N > 0) {
        Mat34 T;
        for (int k = 0; k < 12; ++k) T.m[k] = h_T34[k];
        hipLaunchKernelGGL(view_splat_kernel, dim3(render_grid_for(N)), dim3(256), 0, st, d_grid_pos, N, T, fx, fy, cx, cy, W, H, znear, smax, zbuf);
    }
    hipLaunchKernelGGL(view_resolve_kernel, dim3(render_grid_for(pixels)), dim3(256), 0, st, zbuf, d_color_u8, pixels, h_background3[0],
                       h_background3[1], h_background3[2], d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
