// The audio side of the sound map for gfx950: PCM16 decoding, silence segmentation of a whole recording, and the zero-padded
// fixed-length batch the audio encoder reads.  The recording stays in HBM from the upload to the encoder's batch.
//
// Replaces (upstream reference, path:line):
//   avlmaps/utils/audio_utils.py:515-546   segment_audio_with_silence   a Python loop over every sample above the threshold
//   avlmaps/utils/audio_utils.py:569-583   get_five_second_contexts_audio   one zero-padded float64 host buffer per segment
//   avlmaps/utils/audio_mapping_utils.py:85   x.astype(np.float32) * 32768.0 per segment
//
// Segmentation.  A sample i is loud iff audio[i] > threshold (float32 compare, so NaN is never loud).  With prev(i) the last loud
// sample before i, a loud sample STARTS a segment iff it has no prev or i - prev(i) >= gap.  Segment k is (l_k, r_k): its start and
// the last loud sample before the next start (the last loud sample of all for the last segment).  That is upstream's loop in closed
// form: its `r` is always the previous loud sample when a new loud one is looked at.  prev is an exclusive running maximum of
// "index if loud else -1", a scan; the starts are then flagged independently and numbered by a second scan.  Reduce-then-scan, five
// launches, no workgroup waits on another and there are no atomics:
//   (a) tile_last   every tile of 256 threads x 16 samples: its last loud index or -1
//   (b) carry       one workgroup: exclusive running maximum of the tile summaries (scan_counts_kernel under OpMax from -1; a loop
//                   when there are more tiles than threads)
//   (c) count       every tile again with its carried value: the starts are flagged and counted
//   (d) offsets     one workgroup: exclusive sum of the counts, the total to d_count (scan_counts_kernel under OpSum, int64 out)
//   (e) write       every tile a third time: start k writes l_k and r_(k-1) = its prev; the last tile writes the last r from the
//                   final summary
// A thread keeps its 16 samples as a 16-bit loud mask (four 16-byte loads when the pointer allows), the scans inside a tile are wave
// shuffles over 64 lanes plus one LDS step over the four waves.  Indices fit int32: n <= 2^31 - 1.
//
// Pack.  out[k, j] = audio[start_k + j] * scale for j < min(stop_k - start_k, L), else +0.  Rows are independent: a workgroup owns
// a chunk of one row and stores 16 bytes per lane when L and the output pointer allow.  Ranges are clamped to [0, n] in the kernel, so
// whatever the device array holds nothing is read out of bounds.
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_common.h"
#include "avl_scan.h"

namespace avl {

constexpr int kAudThreads = 256;
constexpr int kAudPer = 16;                           // samples per thread
constexpr int kAudTile = kAudThreads * kAudPer;       // 4096 samples per workgroup
constexpr int kAudWaves = kAudThreads / kWave;
constexpr int kAudMaxChannels = 8;
constexpr int64_t kAudMaxSamples = INT_MAX;
constexpr int kPackPer = 16;                          // floats per thread of the pack kernel
constexpr int kPackChunk = kAudThreads * kPackPer;
constexpr int kPackMaxRowsY = 32768;

static inline int64_t aud_tiles(int64_t n) { return (n + kAudTile - 1) / kAudTile; }

// 16-bit mask of the loud samples among the 16 of this thread; base is the index of the first one
__device__ __forceinline__ unsigned aud_loud_mask(const float* __restrict__ audio, int64_t n, int64_t base, float threshold, bool vec) {
    unsigned m = 0;
    if (vec && base + kAudPer <= n) {
        const float4* p = reinterpret_cast<const float4*>(audio + base);
#pragma unroll
        for (int q = 0; q < kAudPer / 4; ++q) {
            const float4 v = p[q];
            m |= (unsigned)(v.x > threshold) << (4 * q) | (unsigned)(v.y > threshold) << (4 * q + 1) |
                 (unsigned)(v.z > threshold) << (4 * q + 2) | (unsigned)(v.w > threshold) << (4 * q + 3);
        }
    } else {
#pragma unroll
        for (int j = 0; j < kAudPer; ++j)
            if (base + j < n && audio[base + j] > threshold) m |= 1u << j;
    }
    return m;
}

__device__ __forceinline__ int aud_mask_last(unsigned m, int64_t base) { return m ? (int)base + 31 - __clz((int)m) : -1; }

// The scans below are block_excl_scan over the kAudWaves waves of a tile: the running maximum starts at -1 ("no loud sample yet"),
// the sums at 0.  A kernel that scans twice uses two LDS arrays.
// (a)
__global__ __launch_bounds__(kAudThreads) void aud_tile_last_kernel(const float* __restrict__ audio, int64_t n, float threshold, bool vec,
                                                                   int* __restrict__ tile_last) {
    __shared__ int lds[kAudWaves];
    const int64_t base = (int64_t)blockIdx.x * kAudTile + (int64_t)threadIdx.x * kAudPer;
    const unsigned m = aud_loud_mask(audio, n, base, threshold, vec);
    const int v = wave_max(aud_mask_last(m, base));
    if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        int r = lds[0];
#pragma unroll
        for (int w = 1; w < kAudWaves; ++w) r = max(r, lds[w]);
        tile_last[blockIdx.x] = r;
    }
}

// (b) and (d) are avl_scan.h's scan_counts_kernel: under the maximum from -1 over the tile summaries, under the sum over the counts
// the starts among this thread's samples, given prev = the last loud index before its first sample (or -1): a 16-bit mask.
// The writer repeats the walk, because it needs every start's own prev.
__device__ __forceinline__ unsigned aud_start_mask(unsigned m, int64_t base, int prev, int64_t gap) {
    unsigned s = 0;
    while (m) {
        const int j = __ffs((int)m) - 1;
        m &= m - 1;
        const int i = (int)base + j;
        if (prev < 0 || (int64_t)i - prev >= gap) s |= 1u << j;
        prev = i;
    }
    return s;
}

// (c)
__global__ __launch_bounds__(kAudThreads) void aud_count_kernel(const float* __restrict__ audio, int64_t n, float threshold, int64_t gap,
                                                               bool vec, const int* __restrict__ carry, int* __restrict__ tile_count) {
    __shared__ int lds[kAudWaves];
    __shared__ int lds2[kAudWaves];
    const int64_t base = (int64_t)blockIdx.x * kAudTile + (int64_t)threadIdx.x * kAudPer;
    const unsigned m = aud_loud_mask(audio, n, base, threshold, vec);
    int total;
    const int prev = max(carry[blockIdx.x], block_excl_scan<kAudWaves>(aud_mask_last(m, base), OpMax{}, -1, lds, &total));
    const int c = __popc(aud_start_mask(m, base, prev, gap));
    int sum;
    block_excl_scan<kAudWaves>(c, OpSum{}, 0, lds2, &sum);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = sum;
}

// (e)
__global__ __launch_bounds__(kAudThreads) void aud_write_kernel(const float* __restrict__ audio, int64_t n, float threshold, int64_t gap,
                                                               bool vec, const int* __restrict__ carry, const int* __restrict__ tile_last,
                                                               const int64_t* __restrict__ offsets, int64_t* __restrict__ segments,
                                                               int64_t cap) {
    __shared__ int lds[kAudWaves];
    __shared__ int lds2[kAudWaves];
    const int64_t base = (int64_t)blockIdx.x * kAudTile + (int64_t)threadIdx.x * kAudPer;
    unsigned m = aud_loud_mask(audio, n, base, threshold, vec);
    int total;
    int prev = max(carry[blockIdx.x], block_excl_scan<kAudWaves>(aud_mask_last(m, base), OpMax{}, -1, lds, &total));
    const unsigned s = aud_start_mask(m, base, prev, gap);
    int sum;
    int64_t k = offsets[blockIdx.x] + block_excl_scan<kAudWaves>((int)__popc(s), OpSum{}, 0, lds2, &sum);
    while (m) {
        const int j = __ffs((int)m) - 1;
        m &= m - 1;
        const int i = (int)base + j;
        if (s >> j & 1u) {
            if (k < cap) segments[2 * k] = i;
            if (k >= 1 && k - 1 < cap) segments[2 * (k - 1) + 1] = prev;      // k >= 1: a start with an earlier start has a prev
            ++k;
        }
        prev = i;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const int64_t count = offsets[blockIdx.x] + sum;
        if (count >= 1 && count - 1 < cap) segments[2 * (count - 1) + 1] = max(carry[blockIdx.x], tile_last[blockIdx.x]);
    }
}

__global__ __launch_bounds__(kAudThreads) void aud_decode_kernel(const int16_t* __restrict__ pcm, int64_t n, int channels,
                                                                float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kAudThreads + threadIdx.x;
    if (i >= n) return;
    const int16_t* p = pcm + i * channels;
    float s = (float)p[0] / 32768.0f;
    for (int c = 1; c < channels; ++c) s += (float)p[c] / 32768.0f;
    out[i] = s / (float)channels;
}

template <bool kVec>
__global__ __launch_bounds__(kAudThreads) void aud_pack_kernel(const float* __restrict__ audio, int64_t n, const int64_t* __restrict__ ranges,
                                                              int64_t S, int64_t L, float scale, float* __restrict__ out) {
    const int64_t j0 = (int64_t)blockIdx.x * kPackChunk;
    for (int64_t k = blockIdx.y; k < S; k += gridDim.y) {
        const int64_t start = min(max(ranges[2 * k], (int64_t)0), n);
        const int64_t stop = min(max(ranges[2 * k + 1], start), n);
        const int64_t len = min(stop - start, L);
        const float* src = audio + start;
        float* dst = out + k * L;
        if (kVec) {
#pragma unroll
            for (int q = 0; q < kPackPer / 4; ++q) {
                const int64_t j = j0 + ((int64_t)q * kAudThreads + threadIdx.x) * 4;
                if (j >= L) break;                    // L % 4 == 0: a group of four is inside the row or outside
                float4 v;
                v.x = j < len ? src[j] * scale : 0.0f;
                v.y = j + 1 < len ? src[j + 1] * scale : 0.0f;
                v.z = j + 2 < len ? src[j + 2] * scale : 0.0f;
                v.w = j + 3 < len ? src[j + 3] * scale : 0.0f;
                *reinterpret_cast<float4*>(dst + j) = v;
            }
        } else {
#pragma unroll
            for (int q = 0; q < kPackPer; ++q) {
                const int64_t j = j0 + (int64_t)q * kAudThreads + threadIdx.x;
                if (j >= L) break;
                dst[j] = j < len ? src[j] * scale : 0.0f;
            }
        }
    }
}

// workspace of avl_audio_segment: one value per tile in each piece
struct AudWork { int *tile_last, *carry, *tile_count; int64_t* offsets; size_t total; };
static AudWork aud_work(int64_t n, void* ws) {
    const size_t t = (size_t)aud_tiles(n);
    Carver c(ws);
    AudWork w;
    w.tile_last = c.ptr<int>(t * sizeof(int));
    w.carry = c.ptr<int>(t * sizeof(int));
    w.tile_count = c.ptr<int>(t * sizeof(int));
    w.offsets = c.ptr<int64_t>(t * sizeof(int64_t));
    w.total = c.total();
    return w;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_audio_decode_pcm16(const int16_t* d_pcm, int64_t n, int channels, float* d_audio_f32, void* stream) {
    AVL_REQUIRE(d_pcm && d_audio_f32, "avl_audio_decode_pcm16: null pointer");
    AVL_REQUIRE(n >= 1 && n <= kAudMaxSamples, "avl_audio_decode_pcm16: n=%lld outside 1 .. 2^31 - 1", (long long)n);
    AVL_REQUIRE(channels >= 1 && channels <= kAudMaxChannels, "avl_audio_decode_pcm16: channels=%d outside 1 .. %d", channels,
                kAudMaxChannels);
    const unsigned blocks = (unsigned)((n + kAudThreads - 1) / kAudThreads);
    hipLaunchKernelGGL(aud_decode_kernel, dim3(blocks), dim3(kAudThreads), 0, as_stream(stream), d_pcm, n, channels, d_audio_f32);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_audio_segment_work_bytes(int64_t n, size_t* h_bytes) {
    AVL_REQUIRE(h_bytes, "avl_audio_segment_work_bytes: null pointer");
    AVL_REQUIRE(n >= 1 && n <= kAudMaxSamples, "avl_audio_segment_work_bytes: n=%lld outside 1 .. 2^31 - 1", (long long)n);
    *h_bytes = aud_work(n, nullptr).total;
    return AVL_OK;
}

int avl_audio_segment(const float* d_audio, int64_t n, float threshold, int64_t gap, int64_t* d_segments, int64_t cap, int64_t* d_count,
                      void* d_ws, size_t ws_bytes, void* stream) {
    AVL_REQUIRE(d_audio && d_count && d_ws, "avl_audio_segment: null pointer");
    AVL_REQUIRE(n >= 1 && n <= kAudMaxSamples, "avl_audio_segment: n=%lld outside 1 .. 2^31 - 1", (long long)n);
    AVL_REQUIRE(gap >= 1, "avl_audio_segment: gap=%lld, at least one sample is required", (long long)gap);
    AVL_REQUIRE(!std::isnan(threshold), "avl_audio_segment: the threshold is NaN");
    AVL_REQUIRE(cap >= 0 && (cap == 0 || d_segments), "avl_audio_segment: cap=%lld without a segment buffer", (long long)cap);
    AVL_REQUIRE(((uintptr_t)d_audio & 3) == 0, "avl_audio_segment: d_audio is not aligned to 4 bytes");
    const AudWork w = aud_work(n, d_ws);
    AVL_REQUIRE(ws_bytes >= w.total, "avl_audio_segment: workspace of %zu bytes, %zu needed", ws_bytes, w.total);
    const int64_t tiles = aud_tiles(n);
    const bool vec = ((uintptr_t)d_audio & 15) == 0;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)tiles), block(kAudThreads);
    hipLaunchKernelGGL(aud_tile_last_kernel, grid, block, 0, st, d_audio, n, threshold, vec, w.tile_last);
    hipLaunchKernelGGL((scan_counts_kernel<kAudThreads, int, int, OpMax>), dim3(1), block, 0, st, (const int*)w.tile_last, tiles, w.carry,
                       (int*)nullptr, OpMax{}, -1);
    hipLaunchKernelGGL(aud_count_kernel, grid, block, 0, st, d_audio, n, threshold, gap, vec, w.carry, w.tile_count);
    hipLaunchKernelGGL((scan_counts_kernel<kAudThreads, int, int64_t, OpSum>), dim3(1), block, 0, st, (const int*)w.tile_count, tiles, w.offsets,
                       d_count, OpSum{}, (int64_t)0);
    hipLaunchKernelGGL(aud_write_kernel, grid, block, 0, st, d_audio, n, threshold, gap, vec, w.carry, w.tile_last, w.offsets, d_segments, cap);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_audio_pack(const float* d_audio, int64_t n, const int64_t* d_ranges, int64_t S, int64_t L, float scale, float* d_out,
                   void* stream) {
    AVL_REQUIRE(d_audio && d_out && (d_ranges || S == 0), "avl_audio_pack: null pointer");
    AVL_REQUIRE(n >= 1 && n <= kAudMaxSamples, "avl_audio_pack: n=%lld outside 1 .. 2^31 - 1", (long long)n);
    AVL_REQUIRE(L >= 1 && L <= kAudMaxSamples, "avl_audio_pack: L=%lld outside 1 .. 2^31 - 1", (long long)L);
    AVL_REQUIRE(S >= 0 && S <= ((int64_t)1 << 40) / L, "avl_audio_pack: S=%lld rows of %lld samples are out of range", (long long)S,
                (long long)L);
    AVL_REQUIRE(((uintptr_t)d_audio & 3) == 0 && ((uintptr_t)d_out & 3) == 0, "avl_audio_pack: a buffer is not aligned to 4 bytes");
    if (S == 0) return AVL_OK;
    const dim3 grid((unsigned)((L + kPackChunk - 1) / kPackChunk), (unsigned)std::min<int64_t>(S, kPackMaxRowsY));
    const bool vec = (L & 3) == 0 && ((uintptr_t)d_out & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(aud_pack_kernel<true>, grid, dim3(kAudThreads), 0, as_stream(stream), d_audio, n, d_ranges, S, L, scale, d_out);
    else
        hipLaunchKernelGGL(aud_pack_kernel<false>, grid, dim3(kAudThreads), 0, as_stream(stream), d_audio, n, d_ranges, S, L, scale, d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
