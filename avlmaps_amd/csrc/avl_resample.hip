// Loading a recording at any sample rate and PCM width, for gfx950: a rational polyphase resampler and the decoding of 24- and
// 32-bit PCM.  With csrc/avl_audio.hip a recording goes from the bytes of its file to the encoder's batches without a host pass
// over its samples.
//
// Replaces (upstream reference, path:line):
//   avlmaps/utils/audio_mapping_utils.py:238   librosa.load(path, sr=sample_rate): decode any PCM width, resample to sample_rate
// The filter is scipy.signal.resample_poly's default (a Kaiser-windowed sinc, beta 5), NOT librosa's soxr_hq; neither librosa nor
// soxr was available to compare with.
//
// Resampling.  With up / down the reduced ratio, the taps h[0 .. n_taps) (n_taps odd, half = (n_taps - 1) / 2; the host designs
// them, they are data here) and n_out = ceil(n * up / down):
//   y[m] = float32( sum over k of h[m * down + half - k * up] * float64(x[k]) ),   0 <= k < n,  0 <= tap index < n_taps
// added in ASCENDING k, the product and the sum separate float64 operations (the file is built with -ffp-contract=off), one
// rounding to float32 at the end: upfirdn with zero padding at both ends, which is what resample_poly computes.  For output m, with
// a = m * down + half, q = a div up and p = a mod up, the terms are k = q - j with tap index p + j * up (the phase p of the
// polyphase filter), so k runs over [max(0, q - (n_taps - 1 - p) div up), min(q, n - 1)]: about 2 * half / up + 1 terms, 21 when
// upsampling, 20 * down / up when downsampling.  The lower bound equals ceil((m * down - half) / up): both bounds grow with m, so
// the inputs a tile of kResTile consecutive outputs needs are one window of at most ((kResTile - 1) * down + 2 * half) / up + 1
// samples.  All of m * down and k * up is int64 and is formed once per tile; an output's own arithmetic is relative to the
// tile's window, where it fits int32 (at most 1023 * down + 2 * half).
//
// One kernel, four variants by where the two operands are read from.  A workgroup of 256 threads owns tiles of 1024 consecutive
// outputs (lane l of round i computes output m0 + 256 i + l, so a wave stores 256 contiguous bytes and reads nearly contiguous
// inputs) and takes tile after tile in a grid-stride loop, so that the tap table is read into LDS once per workgroup and not once
// per tile:
//   taps     in LDS when n_taps <= kResLdsTaps (72 KiB of float64: every ratio with max(up, down) <= 460, 44 100 <-> 48 000 and
//            44 100 -> 16 000 among them); otherwise read from global memory, where a table of at most 640 KiB stays in L2
//   window   in LDS when it has at most kResLdsWindow floats (32 KiB: down / up up to about 7.8); otherwise read from global memory
// Dynamic LDS, so that a small ratio (2 / 1: 41 taps, 1 045 floats) keeps its occupancy.  No atomics, nothing waits on another
// workgroup.  About 22 terms per output at 12 bytes of LDS reads each; the terms of one output are one dependent chain of float64
// adds, which is what the definition asks for.
//
// PCM.  out[i] = float32( (sum over c of float64(s[i, c]) / 2^(8 width - 1)) / channels ): the scaled samples and their sum (at most
// 8 channels of at most 32 bits) are exact in float64, then one float64 division and one rounding to float32.  Width 3 reads packed
// little-endian 24-bit frames byte by byte (no alignment is assumed), width 4 reads int32, which is also how a 24-bit sample
// left-justified in 32 bits arrives: v * 2^8 / 2^31 == v / 2^23.
#include <algorithm>
#include <climits>

#include "avl_common.h"

namespace avl {

constexpr int kResThreads = 256;
constexpr int kResPer = 4;                            // outputs per thread and tile
constexpr int kResTile = kResThreads * kResPer;       // 1024 outputs per tile
constexpr int kResLdsTaps = 9216;                     // the tap table is staged in LDS up to this many float64 taps (72 KiB)
constexpr int kResLdsWindow = 8192;                   // a tile's input window is staged in LDS up to this many floats (32 KiB)
constexpr int kResMaxRatio = 4096;                    // 1 <= up, down <= 4096
constexpr int kResMaxTaps = 20 * kResMaxRatio + 1;
constexpr int kResMaxBlocks = 2048;                   // the grid; more tiles are taken in a grid-stride loop
constexpr int64_t kResMaxSamples = INT_MAX;
constexpr int kPcmMaxChannels = 8;

// first input sample with a tap for output m: max(0, ceil((m * down - half) / up))
__device__ __forceinline__ int64_t res_k_lo(int64_t m, int up, int down, int half) {
    const int64_t a = m * down - half;
    return a <= 0 ? 0 : (a + up - 1) / up;
}

// last one: min(n - 1, floor((m * down + half) / up))
__device__ __forceinline__ int64_t res_k_hi(int64_t m, int up, int down, int half, int64_t n) {
    return min((m * down + half) / up, n - 1);
}

template <bool kTapsLds, bool kWinLds>
__global__ __launch_bounds__(kResThreads) void aud_resample_kernel(const float* __restrict__ x, int64_t n, int up, int down,
                                                                  const double* __restrict__ taps, int n_taps, float* __restrict__ out,
                                                                  int64_t n_out, int64_t tiles, int win_cap) {
    extern __shared__ __attribute__((aligned(16))) double res_lds[];      // [n_taps float64 if kTapsLds][win_cap float32 if kWinLds]
    double* s_taps = res_lds;
    float* s_win = reinterpret_cast<float*>(res_lds + (kTapsLds ? n_taps : 0));
    const int half = (n_taps - 1) / 2;
    if (kTapsLds)
        for (int i = threadIdx.x; i < n_taps; i += kResThreads) s_taps[i] = taps[i];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {            // the same trips for every thread of a workgroup
        const int64_t m0 = tile * kResTile, m1 = min(m0 + kResTile, n_out) - 1;
        const int64_t ks = res_k_lo(m0, up, down, half);
        if (kWinLds) {
            __syncthreads();                                                      // the previous tile's window has been read
            const int w = (int)min(res_k_hi(m1, up, down, half, n) - ks + 1, (int64_t)win_cap);
            for (int i = threadIdx.x; i < w; i += kResThreads) s_win[i] = x[ks + i];
        }
        if (kTapsLds || kWinLds) __syncthreads();
        // relative to the window: a - ks * up = (m - m0) * down + base fits int32 (at most 1023 * down + 2 * half), so the
        // division that splits it into the offset of the last input and the phase is a 32-bit one
        const int base = (int)(m0 * down + half - ks * up);
        const int64_t last = n - 1 - ks;                                          // the recording's last sample, relative
#pragma unroll
        for (int r = 0; r < kResPer; ++r) {
            const int64_t m = m0 + r * kResThreads + threadIdx.x;
            if (m > m1) break;
            const int b = base + (r * kResThreads + (int)threadIdx.x) * down;     // < 0 (a table shorter than up only): no term either
            const unsigned q = (unsigned)max(b, 0) / (unsigned)up;                // the last input with a tap is ks + q
            const int p = max(b, 0) - (int)(q * (unsigned)up);                    // the phase
            const int room = n_taps - 1 - p;                                      // < 0: a table shorter than the phase, no term at all
            const int lo = room < 0 ? (int)q + 1 : (int)max((int64_t)q - room / up, -ks);
            const int hi = (int)min((int64_t)q, last);
            int t = b - lo * up;                                                  // <= p + (room div up) * up < n_taps where a term exists
            const int cnt = b < 0 ? 0 : hi - lo + 1;
            double acc = 0.0;
            if (kWinLds) {
                const float* w = s_win + lo;
#pragma unroll 4
                for (int i = 0; i < cnt; ++i, t -= up) acc = acc + (kTapsLds ? s_taps[t] : taps[t]) * (double)w[i];
            } else {
                const float* w = x + (ks + lo);
#pragma unroll 4
                for (int i = 0; i < cnt; ++i, t -= up) acc = acc + (kTapsLds ? s_taps[t] : taps[t]) * (double)w[i];
            }
            out[m] = (float)acc;
        }
    }
}

template <int kWidth>
__global__ __launch_bounds__(kResThreads) void aud_decode_pcm_kernel(const uint8_t* __restrict__ pcm, int64_t n, int channels,
                                                                    float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kResThreads + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    if (kWidth == 3) {
        const uint8_t* p = pcm + i * channels * 3;
        for (int c = 0; c < channels; ++c, p += 3) {
            const int32_t v = (int32_t)((uint32_t)p[0] << 8 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 24) >> 8;      // sign-extended
            s += (double)v / 8388608.0;
        }
    } else {
        const int32_t* p = reinterpret_cast<const int32_t*>(pcm) + i * channels;
        for (int c = 0; c < channels; ++c) s += (double)p[c] / 2147483648.0;
    }
    out[i] = (float)(s / (double)channels);
}

template <bool kTapsLds, bool kWinLds>
static int res_launch(const float* d_audio, int64_t n, int up, int down, const double* d_taps, int n_taps, float* d_out, int64_t n_out,
                      int64_t tiles, int win, hipStream_t st) {
    const size_t lds = (kTapsLds ? (size_t)n_taps * sizeof(double) : 0) + (kWinLds ? (size_t)win * sizeof(float) : 0);
    auto kern = aud_resample_kernel<kTapsLds, kWinLds>;
    if (lds > 64 * 1024)                              // above HIP's default limit for dynamic LDS; only the largest tables get here
        AVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(tiles, kResMaxBlocks)), dim3(kResThreads), lds, st, d_audio, n, up, down,
                       d_taps, n_taps, d_out, n_out, tiles, kWinLds ? win : 0);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_audio_resample_limits(int* h_tile, int* h_lds_taps, int* h_lds_window) {
    AVL_REQUIRE(h_tile && h_lds_taps && h_lds_window, "avl_audio_resample_limits: null pointer");
    *h_tile = kResTile;
    *h_lds_taps = kResLdsTaps;
    *h_lds_window = kResLdsWindow;
    return AVL_OK;
}

int avl_audio_resample(const float* d_audio, int64_t n, int up, int down, const double* d_taps, int64_t n_taps, float* d_out,
                       int64_t n_out, void* stream) {
    AVL_REQUIRE(d_audio && d_taps && d_out, "avl_audio_resample: null pointer");
    AVL_REQUIRE(n >= 1 && n <= kResMaxSamples, "avl_audio_resample: n=%lld outside 1 .. 2^31 - 1", (long long)n);
    AVL_REQUIRE(up >= 1 && up <= kResMaxRatio && down >= 1 && down <= kResMaxRatio, "avl_audio_resample: ratio %d / %d outside 1 .. %d",
                up, down, kResMaxRatio);
    AVL_REQUIRE(n_taps >= 1 && n_taps <= kResMaxTaps && (n_taps & 1) == 1, "avl_audio_resample: n_taps=%lld is not an odd count in 1 .. %d",
                (long long)n_taps, kResMaxTaps);
    AVL_REQUIRE(n_out >= 1 && n_out <= kResMaxSamples, "avl_audio_resample: n_out=%lld outside 1 .. 2^31 - 1", (long long)n_out);
    AVL_REQUIRE(n_out == (n * up + down - 1) / down, "avl_audio_resample: n_out=%lld is not ceil(%lld * %d / %d)", (long long)n_out,
                (long long)n, up, down);
    AVL_REQUIRE(((uintptr_t)d_audio & 3) == 0 && ((uintptr_t)d_out & 3) == 0 && ((uintptr_t)d_taps & 7) == 0,
                "avl_audio_resample: a buffer is not aligned to its element size");
    const int64_t tiles = (n_out + kResTile - 1) / kResTile;
    const int64_t win = ((int64_t)(kResTile - 1) * down + (n_taps - 1)) / up + 1;      // the most inputs a tile reads
    const bool taps_lds = n_taps <= kResLdsTaps, win_lds = win <= kResLdsWindow;
    hipStream_t st = as_stream(stream);
    if (taps_lds)
        return win_lds ? res_launch<true, true>(d_audio, n, up, down, d_taps, (int)n_taps, d_out, n_out, tiles, (int)win, st)
                       : res_launch<true, false>(d_audio, n, up, down, d_taps, (int)n_taps, d_out, n_out, tiles, 0, st);
    return win_lds ? res_launch<false, true>(d_audio, n, up, down, d_taps, (int)n_taps, d_out, n_out, tiles, (int)win, st)
                   : res_launch<false, false>(d_audio, n, up, down, d_taps, (int)n_taps, d_out, n_out, tiles, 0, st);
}

int avl_audio_decode_pcm(const void* d_pcm, int64_t n, int channels, int width, float* d_out, void* stream) {
    AVL_REQUIRE(d_pcm && d_out, "avl_audio_decode_pcm: null pointer");
    AVL_REQUIRE(n >= 1 && n <= kResMaxSamples, "avl_audio_decode_pcm: n=%lld outside 1 .. 2^31 - 1", (long long)n);
    AVL_REQUIRE(channels >= 1 && channels <= kPcmMaxChannels, "avl_audio_decode_pcm: channels=%d outside 1 .. %d", channels,
                kPcmMaxChannels);
    AVL_REQUIRE(width == 3 || width == 4, "avl_audio_decode_pcm: width=%d, 3 (packed 24-bit) or 4 (int32) bytes per sample are decoded", width);
    AVL_REQUIRE(width == 3 || ((uintptr_t)d_pcm & 3) == 0, "avl_audio_decode_pcm: int32 samples are not aligned to 4 bytes");
    AVL_REQUIRE(((uintptr_t)d_out & 3) == 0, "avl_audio_decode_pcm: d_out is not aligned to 4 bytes");
    const dim3 grid((unsigned)((n + kResThreads - 1) / kResThreads)), block(kResThreads);
    const uint8_t* p = static_cast<const uint8_t*>(d_pcm);
    if (width == 3)
        hipLaunchKernelGGL(aud_decode_pcm_kernel<3>, grid, block, 0, as_stream(stream), p, n, channels, d_out);
    else
        hipLaunchKernelGGL(aud_decode_pcm_kernel<4>, grid, block, 0, as_stream(stream), p, n, channels, d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
