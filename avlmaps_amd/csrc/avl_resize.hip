// Resizing 8-bit images the way Pillow does, and CLIP's preprocess on top of it, for gfx950: a batch of frames goes from its uint8
// pixels to the (B, 3, n_px, n_px) tensor the image tower eats without a host pass over the pixels.
//
// Replaces (upstream reference, path:line):
//   avlmaps/utils/clip_utils.py:96-130   preprocess(Image.fromarray(img)) per image on a CPU core: CLIP's _transform(n_px), i.e.
//                                        Resize(n_px, BICUBIC), CenterCrop(n_px), ToTensor, Normalize
//   avlmaps/map/area_map.py:66-98        the same call per frame of the area map
//
// The resize is Pillow's ImagingResample for 8 bits per channel, which is integer arithmetic once its coefficient tables exist.
// The tables are data here (ops.resize_coeffs builds them on the host in float64): per output index xx of an axis a row of ksize
// int32 coefficients k[xx][0 .. ksize) scaled by 2^22 and a pair bounds[xx] = (xmin, count).  One pass along an axis is, per channel,
//     acc = 2^21 + sum over i < count of pixel[xmin + i] * k[xx][i]        (int32; the wrapper checks 255 * sum|k| + 2^21 < 2^31)
//     out = clamp(acc >> 22, 0, 255)                                        (arithmetic shift)
// The horizontal pass runs first and is rounded to uint8; the vertical pass reads those bytes.  A pass whose table is NULL leaves its
// axis as it is.  Only an output window (top, left, out_h, out_w) of the resized image is produced: the horizontal pass computes
// the window's columns of the input rows the vertical pass will read, and nothing else.
//
// Two kernels, no atomics, nothing waits on another workgroup:
//   rsz_rows_kernel   the horizontal pass (or, without a table, the crop).  A workgroup of 4 waves owns 64 output columns of 4
//                     rows: wave w its row, lane l its column, all C channels.  The bytes of the row that the 64 columns read are
//                     one span [xmin of the first column, xmin + count of the last): each wave copies its row's span into LDS,
//                     whole aligned dwords in the middle and single bytes at the two ragged ends (nothing outside the span is
//                     read), when it has at most kRszLdsSpan bytes; the tile's 64 * ksize coefficients go to LDS when they
//                     number at most kRszLdsCoefs.  Beyond either budget, or for a column whose taps leave the span (tables that
//                     are not monotone), the operand is read from global memory instead.  With a vertical pass to follow, the
//                     grid covers all H input rows and a workgroup whose rows the vertical table never reads returns at once (the
//                     range is bounds_v[top] .. bounds_v[top + out_h - 1], read on the device); the bytes go to the workspace,
//                     (B, H, pitch) with pitch = out_w * C rounded up to 4.  Without one they go to the output.
//   rsz_cols_kernel   the vertical pass.  It does not care where a pixel ends: a lane owns 4 consecutive bytes of a workspace row
//                     and reads one aligned dword per tap, a wave 256 contiguous bytes; the coefficients of an output row are the
//                     same for the whole wave and come through the scalar cache.
// Both end in rsz_emit: a uint8 of the (B, out_h, out_w, C) output, or, for avl_clip_preprocess, the 32- or 16-bit pattern that the
// caller's (256, C) table holds for (value, channel), stored channel-planar.  The file has no floating-point arithmetic: ToTensor
// and Normalize are that table, which the host computed.
// Every index taken from a table is clamped to the image before it is used, so a wrong table gives wrong pixels, not a fault.
#include <algorithm>

#include "avl_common.h"

namespace avl {

constexpr int kRszBits = 22;
constexpr int kRszMaxSide = 16384;
constexpr int kRszMaxBatch = 65535;                   // the batch is the grid's z
constexpr int kRszMaxChannels = 4;
constexpr int kRszMaxTaps = 4 * kRszMaxSide + 1;          // bicubic from 16 384 to 1: ceil(2 * 16 384) * 2 + 1
constexpr int kRszTileW = kWave;                      // output columns per workgroup of the horizontal pass, one per lane
constexpr int kRszTileR = 4;                          // rows per workgroup, one per wave
constexpr int kRszThreads = kRszTileW * kRszTileR;
constexpr int kRszLdsCoefs = 4096;                    // a tile's coefficients are staged in LDS up to this many (16 KiB: ksize <= 64)
constexpr int kRszLdsSpan = 4096;                     // a row's span is staged in LDS up to this many bytes (16 KiB for 4 rows)
constexpr int kRszSpanPitch = kRszLdsSpan + 8;        // room for the span's misalignment, a multiple of 4
enum { kOutU8 = 0, kOutF32 = 1, kOutF16 = 2 };

__device__ __forceinline__ int rsz_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int kOut>
__device__ __forceinline__ void rsz_emit(void* __restrict__ out, const void* __restrict__ table, int64_t b, int y, int x, int c, int C,
                                         int out_h, int out_w, int v) {
    if (kOut == kOutU8) {
        static_cast<uint8_t*>(out)[((b * out_h + y) * out_w + x) * C + c] = (uint8_t)v;
    } else {
        const int64_t at = ((b * C + c) * out_h + y) * out_w + x;
        if (kOut == kOutF32)
            static_cast<uint32_t*>(out)[at] = static_cast<const uint32_t*>(table)[v * C + c];
        else
            static_cast<uint16_t*>(out)[at] = static_cast<const uint16_t*>(table)[v * C + c];
    }
}

// acc[c] += sum over i < cnt of p[i * C + c] * k[i]
template <typename PX, typename KK>
__device__ __forceinline__ void rsz_taps(const PX* p, const KK* k, int cnt, int C, int* acc) {
    for (int i = 0; i < cnt; ++i, p += C) {
        const int kv = k[i];
#pragma unroll
        for (int c = 0; c < kRszMaxChannels; ++c)
            if (c < C) acc[c] += (int)p[c] * kv;
    }
}

template <bool kCoefLds, int kOut>
__global__ __launch_bounds__(kRszThreads) void rsz_rows_kernel(const uint8_t* __restrict__ in, int H, int W, int C,
                                                              const int32_t* __restrict__ kh, const int32_t* __restrict__ bh, int ksize,
                                                              const int32_t* __restrict__ bv, int top, int left, int out_h, int out_w,
                                                              uint8_t* __restrict__ tmp, int pitch, void* __restrict__ out,
                                                              const void* __restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rsz_lds[];      // [64 * ksize int32 if kCoefLds][4 rows of span]
    int32_t* s_k = reinterpret_cast<int32_t*>(rsz_lds);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned char* s_row = rsz_lds + (kCoefLds ? kRszTileW * ksize * 4 : 0) + wave * kRszSpanPitch;
    const int64_t b = blockIdx.z;
    const int x0 = blockIdx.x * kRszTileW;                                        // the tile's first column, relative to the window
    const int nx = min(kRszTileW, out_w - x0);

    // the rows this pass produces: the input rows the vertical pass reads, or the window's rows
    int row_lo = 0, row_hi = out_h;
    if (bv) {
        const int32_t* first = bv + 2 * (int64_t)top;
        const int32_t* last = bv + 2 * (int64_t)(top + out_h - 1);
        row_lo = rsz_clamp(first[0], 0, H);
        row_hi = min(rsz_clamp(last[0], row_lo, H) + rsz_clamp(last[1], 0, H), H);
    }
    const int rbase = blockIdx.y * kRszTileR;
    if (rbase >= row_hi || rbase + kRszTileR <= row_lo) return;                   // the whole workgroup, before any barrier
    const int r = rbase + wave;
    const bool row_on = r >= row_lo && r < row_hi;
    const int src_row = bv ? r : top + r;

    // the span of input columns the tile reads
    int s0 = left + x0, s1 = left + x0 + nx;
    if (kh) {
        const int32_t* first = bh + 2 * (int64_t)(left + x0);
        const int32_t* last = bh + 2 * (int64_t)(left + x0 + nx - 1);
        s0 = rsz_clamp(first[0], 0, W);
        s1 = min(rsz_clamp(last[0], s0, W) + rsz_clamp(last[1], 0, W), W);
    }
    const int nbytes = (s1 - s0) * C;
    const bool span_lds = nbytes <= kRszLdsSpan;

    if (kCoefLds) {
        const int32_t* g = kh + (int64_t)(left + x0) * ksize;
        for (int i = threadIdx.x; i < nx * ksize; i += kRszThreads) s_k[i] = g[i];
    }
    const uint8_t* g_row = in + (b * H + (row_on ? src_row : 0)) * ((int64_t)W * C);
    const uint8_t* src = g_row + (int64_t)s0 * C;
    const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);                  // s_row[mis + i] = src[i]: LDS and global dwords line up
    if (row_on && span_lds) {
        const int head = min((4 - mis) & 3, nbytes);
        if (lane < head) s_row[mis + lane] = src[lane];
        const int ndw = (nbytes - head) >> 2;
        const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src + head);
        uint32_t* dst4 = reinterpret_cast<uint32_t*>(s_row + mis + head);
        for (int i = lane; i < ndw; i += kWave) dst4[i] = src4[i];
        const int done = head + 4 * ndw;
        if (lane < nbytes - done) s_row[mis + done + lane] = src[done + lane];
    }
    __syncthreads();
    if (!row_on || lane >= nx) return;

    const int x = x0 + lane;
    int xmin = left + x, cnt = 1;
    if (kh) {
        const int32_t* bb = bh + 2 * (int64_t)(left + x);
        xmin = rsz_clamp(bb[0], 0, W - 1);
        cnt = rsz_clamp(bb[1], 0, min(ksize, W - xmin));
    }
    const bool from_lds = span_lds && xmin >= s0 && xmin + cnt <= s1;
    int v[kRszMaxChannels];
    if (kh) {
        int acc[kRszMaxChannels] = {1 << (kRszBits - 1), 1 << (kRszBits - 1), 1 << (kRszBits - 1), 1 << (kRszBits - 1)};
        const int32_t* kg = kh + (int64_t)(left + x) * ksize;
        if (from_lds) {
            const unsigned char* p = s_row + mis + (xmin - s0) * C;
            if (kCoefLds) rsz_taps(p, s_k + lane * ksize, cnt, C, acc);
            else rsz_taps(p, kg, cnt, C, acc);
        } else {
            const uint8_t* p = g_row + (int64_t)xmin * C;
            if (kCoefLds) rsz_taps(p, s_k + lane * ksize, cnt, C, acc);
            else rsz_taps(p, kg, cnt, C, acc);
        }
#pragma unroll
        for (int c = 0; c < kRszMaxChannels; ++c) v[c] = rsz_clamp(acc[c] >> kRszBits, 0, 255);
    } else {
#pragma unroll
        for (int c = 0; c < kRszMaxChannels; ++c)
            v[c] = c >= C ? 0 : from_lds ? s_row[mis + (xmin - s0) * C + c] : g_row[(int64_t)xmin * C + c];
    }
    if (bv) {
        uint8_t* d = tmp + (b * H + r) * pitch + x * C;
#pragma unroll
        for (int c = 0; c < kRszMaxChannels; ++c)
            if (c < C) d[c] = (uint8_t)v[c];
    } else {
#pragma unroll
        for (int c = 0; c < kRszMaxChannels; ++c)
            if (c < C) rsz_emit<kOut>(out, table, b, r, x, c, C, out_h, out_w, v[c]);
    }
}

template <int kOut>
__global__ __launch_bounds__(kRszThreads) void rsz_cols_kernel(const uint8_t* __restrict__ tmp, int H, int pitch, int C,
                                                              const int32_t* __restrict__ kv, const int32_t* __restrict__ bv, int ksize,
                                                              int top, int out_h, int out_w, void* __restrict__ out,
                                                              const void* __restrict__ table) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int y = blockIdx.y * kRszTileR + wave;
    const int f0 = (blockIdx.x * kWave + lane) * 4;                               // this lane's 4 bytes of the row of out_w * C
    const int row_bytes = out_w * C;
    if (y >= out_h || f0 >= row_bytes) return;
    const int64_t b = blockIdx.z;
    const int yy = __builtin_amdgcn_readfirstlane(top + y);                       // the same for the wave: scalar loads below
    const int ymin = rsz_clamp(bv[2 * (int64_t)yy], 0, H - 1);
    const int cnt = rsz_clamp(bv[2 * (int64_t)yy + 1], 0, min(ksize, H - ymin));
    const int32_t* kk = kv + (int64_t)yy * ksize;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(tmp + (b * H + ymin) * pitch + f0);
    const int step = pitch >> 2;
    int a0 = 1 << (kRszBits - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int i = 0; i < cnt; ++i, p += step) {
        const uint32_t w = *p;
        const int k = kk[i];
        a0 += (int)(w & 255u) * k;
        a1 += (int)((w >> 8) & 255u) * k;
        a2 += (int)((w >> 16) & 255u) * k;
        a3 += (int)(w >> 24) * k;
    }
    const int v[4] = {rsz_clamp(a0 >> kRszBits, 0, 255), rsz_clamp(a1 >> kRszBits, 0, 255), rsz_clamp(a2 >> kRszBits, 0, 255),
                      rsz_clamp(a3 >> kRszBits, 0, 255)};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int f = f0 + q;
        if (f < row_bytes) {
            const int x = f / C;
            rsz_emit<kOut>(out, table, b, y, x, f - x * C, C, out_h, out_w, v[q]);
        }
    }
}

struct RszArgs {
    const uint8_t* in;
    int B, H, W, C;
    const int32_t *kh, *bh;
    int ksize_h, ow;
    const int32_t *kv, *bv;
    int ksize_v, oh;
    int top, left, out_h, out_w;
};

static int rsz_pitch(int out_w, int C) { return (out_w * C + 3) & ~3; }

// the one layout of the workspace: the horizontal pass's bytes when a vertical pass follows, plus the slack of aligning the base here
static size_t rsz_layout(int B, int H, int C, int out_w, bool vertical, void* base, uint8_t** tmp) {
    Carver cv(align256_ptr(base));
    uint8_t* t = cv.ptr<uint8_t>(vertical ? (size_t)B * H * rsz_pitch(out_w, C) : 0);
    if (tmp) *tmp = t;
    return cv.total() + 256;
}

static int rsz_check_dims(const char* who, int B, int H, int W, int C) {
    AVL_REQUIRE(B >= 1 && B <= kRszMaxBatch, "%s: B=%d outside 1 .. %d", who, B, kRszMaxBatch);
    AVL_REQUIRE(H >= 1 && H <= kRszMaxSide && W >= 1 && W <= kRszMaxSide, "%s: image of %d x %d, sides outside 1 .. %d", who, H, W,
                kRszMaxSide);
    AVL_REQUIRE(C >= 1 && C <= kRszMaxChannels, "%s: C=%d outside 1 .. %d", who, C, kRszMaxChannels);
    return AVL_OK;
}

static int rsz_check(const char* who, const RszArgs& a, const void* d_out) {
    AVL_REQUIRE(a.in && d_out, "%s: null image or output pointer", who);
    int rc = rsz_check_dims(who, a.B, a.H, a.W, a.C);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(!a.kh == !a.bh && !a.kv == !a.bv, "%s: a pass needs both its coefficients and its bounds, or neither (null)", who);
    AVL_REQUIRE(a.oh >= 1 && a.oh <= kRszMaxSide && a.ow >= 1 && a.ow <= kRszMaxSide, "%s: resized to %d x %d, sides outside 1 .. %d", who,
                a.oh, a.ow, kRszMaxSide);
    AVL_REQUIRE(a.kh || a.ow == a.W, "%s: no horizontal pass, but the width changes from %d to %d", who, a.W, a.ow);
    AVL_REQUIRE(a.kv || a.oh == a.H, "%s: no vertical pass, but the height changes from %d to %d", who, a.H, a.oh);
    AVL_REQUIRE(!a.kh || (a.ksize_h >= 1 && a.ksize_h <= kRszMaxTaps), "%s: ksize_h=%d outside 1 .. %d", who, a.ksize_h,
                kRszMaxTaps);
    AVL_REQUIRE(!a.kv || (a.ksize_v >= 1 && a.ksize_v <= kRszMaxTaps), "%s: ksize_v=%d outside 1 .. %d", who, a.ksize_v,
                kRszMaxTaps);
    AVL_REQUIRE(a.top >= 0 && a.left >= 0 && a.out_h >= 1 && a.out_w >= 1 && a.out_h <= a.oh - a.top && a.out_w <= a.ow - a.left,
                "%s: the window (top %d, left %d, %d x %d) leaves the resized image of %d x %d", who, a.top, a.left, a.out_h, a.out_w, a.oh,
                a.ow);
    AVL_REQUIRE(((uintptr_t)a.kh & 3) == 0 && ((uintptr_t)a.bh & 3) == 0 && ((uintptr_t)a.kv & 3) == 0 && ((uintptr_t)a.bv & 3) == 0,
                "%s: a table is not aligned to 4 bytes", who);
    return AVL_OK;
}

template <int kOut>
static int rsz_run(const char* who, const RszArgs& a, void* d_out, const void* d_table, void* ws, size_t ws_bytes, hipStream_t st) {
    uint8_t* tmp = nullptr;
    const bool vertical = a.kv != nullptr;
    const size_t need = rsz_layout(a.B, a.H, a.C, a.out_w, vertical, ws, &tmp);
    AVL_REQUIRE(!vertical || (ws && ws_bytes >= need), "%s: workspace of %zu bytes, need %zu", who, ws_bytes, need);
    const int pitch = rsz_pitch(a.out_w, a.C);
    const bool coef_lds = a.kh && kRszTileW * (int64_t)a.ksize_h <= kRszLdsCoefs;
    const size_t lds = (coef_lds ? (size_t)kRszTileW * a.ksize_h * 4 : 0) + (size_t)kRszTileR * kRszSpanPitch;
    const int rows = vertical ? a.H : a.out_h;
    const dim3 grid_h((a.out_w + kRszTileW - 1) / kRszTileW, (rows + kRszTileR - 1) / kRszTileR, a.B), block(kRszThreads);
    // with a vertical pass to follow the horizontal one writes workspace bytes, whatever the output's type
    if (vertical) {
        auto kern = coef_lds ? rsz_rows_kernel<true, kOutU8> : rsz_rows_kernel<false, kOutU8>;
        hipLaunchKernelGGL(kern, grid_h, block, lds, st, a.in, a.H, a.W, a.C, a.kh, a.bh, a.ksize_h, a.bv, a.top, a.left, a.out_h, a.out_w,
                           tmp, pitch, (void*)nullptr, (const void*)nullptr);
        AVL_HIP_CHECK(hipGetLastError());
        const dim3 grid_v((pitch / 4 + kWave - 1) / kWave, (a.out_h + kRszTileR - 1) / kRszTileR, a.B);
        hipLaunchKernelGGL(rsz_cols_kernel<kOut>, grid_v, block, 0, st, (const uint8_t*)tmp, a.H, pitch, a.C, a.kv, a.bv, a.ksize_v, a.top,
                           a.out_h, a.out_w, d_out, d_table);
    } else {
        auto kern = coef_lds ? rsz_rows_kernel<true, kOut> : rsz_rows_kernel<false, kOut>;
        hipLaunchKernelGGL(kern, grid_h, block, lds, st, a.in, a.H, a.W, a.C, a.kh, a.bh, a.ksize_h, (const int32_t*)nullptr, a.top, a.left,
                           a.out_h, a.out_w, (uint8_t*)nullptr, pitch, d_out, d_table);
    }
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_resize_limits(int* h_tile_w, int* h_lds_coefs, int* h_lds_span) {
    AVL_REQUIRE(h_tile_w && h_lds_coefs && h_lds_span, "avl_resize_limits: null pointer");
    *h_tile_w = kRszTileW;
    *h_lds_coefs = kRszLdsCoefs;
    *h_lds_span = kRszLdsSpan;
    return AVL_OK;
}

int avl_resize_work_bytes(int B, int H, int C, int out_w, int vertical, size_t* h_bytes) {
    AVL_REQUIRE(h_bytes, "avl_resize_work_bytes: null output");
    int rc = rsz_check_dims("avl_resize_work_bytes", B, H, 1, C);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(out_w >= 1 && out_w <= kRszMaxSide, "avl_resize_work_bytes: out_w=%d outside 1 .. %d", out_w, kRszMaxSide);
    *h_bytes = rsz_layout(B, H, C, out_w, vertical != 0, nullptr, nullptr);
    return AVL_OK;
}

int avl_resize_u8(const uint8_t* d_in, int B, int H, int W, int C, const int32_t* d_kh, const int32_t* d_bh, int ksize_h, int ow,
                  const int32_t* d_kv, const int32_t* d_bv, int ksize_v, int oh, int top, int left, int out_h, int out_w, uint8_t* d_out,
                  void* d_ws, size_t ws_bytes, void* stream) {
    const RszArgs a{d_in, B, H, W, C, d_kh, d_bh, ksize_h, ow, d_kv, d_bv, ksize_v, oh, top, left, out_h, out_w};
    int rc = rsz_check("avl_resize_u8", a, d_out);
    if (rc != AVL_OK) return rc;
    return rsz_run<kOutU8>("avl_resize_u8", a, d_out, nullptr, d_ws, ws_bytes, as_stream(stream));
}

int avl_clip_preprocess(const uint8_t* d_in, int B, int H, int W, const int32_t* d_kh, const int32_t* d_bh, int ksize_h, int ow,
                        const int32_t* d_kv, const int32_t* d_bv, int ksize_v, int oh, int top, int left, int out_h, int out_w,
                        const void* d_table, int out_f16, void* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    const RszArgs a{d_in, B, H, W, 3, d_kh, d_bh, ksize_h, ow, d_kv, d_bv, ksize_v, oh, top, left, out_h, out_w};
    int rc = rsz_check("avl_clip_preprocess", a, d_out);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_table, "avl_clip_preprocess: null table");
    AVL_REQUIRE(out_f16 == 0 || out_f16 == 1, "avl_clip_preprocess: out_f16=%d, 0 (float32) or 1 (float16)", out_f16);
    const uintptr_t al = out_f16 ? 1 : 3;
    AVL_REQUIRE(((uintptr_t)d_table & al) == 0 && ((uintptr_t)d_out & al) == 0, "avl_clip_preprocess: the table or the output is not aligned to its element size");
    return out_f16 ? rsz_run<kOutF16>("avl_clip_preprocess", a, d_out, d_table, d_ws, ws_bytes, as_stream(stream))
                   : rsz_run<kOutF32>("avl_clip_preprocess", a, d_out, d_table, d_ws, ws_bytes, as_stream(stream));
}

}  // extern "C"
