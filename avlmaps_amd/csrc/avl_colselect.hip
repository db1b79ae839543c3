// Open-set queries for gfx950: exact order statistics of the columns of the resident (N, Q) score matrix, and the per-category
// membership words, counts and voxel mask of "score above the column's own threshold".
//
// Stands in for (upstream reference, path:line):
//   avlmaps/map/clip_map.py:62-75   CLIPMap.load_categories: per category, the cells whose score lies above np.percentile(column, 95)
//                                   (the file cannot be imported upstream: its imports name a utils package that does not exist)
// Upstream partitions a host copy of every column.  Here the quantile's two order statistics come from a most-significant-digit
// radix select on the device and the interpolation between them is done by the caller in float64 (ops/select.py).
//
// Order (np.sort's): key(x) = the order-preserving map of the float32 bits to uint32 (negative: ~bits, else bits | 2^31) after
// -0 -> +0 and NaN -> 0xFFFFFFFF, so -inf < ... < -0 = +0 < ... < +inf < NaN, every NaN is the one largest value, and denormals are
// ordered by their bits (nothing is flushed: no float arithmetic touches a score).  A selected zero comes back as +0.
//
// avl_colselect_f32, per group of at most kSelectSlots slots (column, k), on one stream, a fixed sequence of launches:
//    init      prefix = 0, remaining k = k, global histogram = 0                                       (slots are kernel arguments)
//    4 x { histogram pass p; pick p }
//              pass p streams the matrix once and counts digit (key >> (24 - 8 p)) & 255 of every element whose key agrees with the
//              slot's prefix in the 8 p bits above it; pick p (one workgroup per slot) scans the 256 bins, fixes the digit of the
//              bin that holds the remaining k and takes the bins below it off k.  After pick 3 the prefix is key(v_k), k minus the
//              remaining k is count_lt, and that plus the last bin is count_le.
//    last pass the smallest key above key(v_k) and the number of NaNs
//    finish    v_k, v_next (= v_k when count_le > k + 1 or k = N - 1, else the smallest key above), the three counts
// Launch shape of a pass: thread t of a workgroup of 1024 owns slot t % n and row t / n of a block of 1024 / n rows, so a wave reads
// consecutive slots of a row (coalesced when the slots name consecutive columns, which is how column_quantiles orders them) and the
// slot's column and prefix stay in registers.  A workgroup walks chunks of kSelectUnroll such blocks in a grid-stride loop with all
// loads of a chunk issued before the first count.  Counters: uint32 in LDS (n x 256; bin b of slot s lies at s * 256 + (b + s) % 256
// so that the lanes of a wave, which hold different slots and on real scores the same digit, fall on different banks), flushed with
// one 64-bit atomic per non-empty bin and workgroup.  A workgroup takes fewer than 2^32 elements per slot (N < 2^31).  Every
// counter is an integer and every result a count, a minimum or a selected element: the bytes do not depend on scheduling.
//
// avl_cols_above_f32: a wave owns 64 rows x 64 columns: it reads a row at a time (256 contiguous bytes), ballots
// (double)score > threshold into the row's word, and lane i keeps row i's word, so the words (and the optional mask bytes) of 64 rows
// are stored together.  A lane counts its own column in a register; the four waves of a workgroup add up in LDS and the workgroup
// adds one 64-bit atomic per column with a non-zero count (one per WAVE is what made gt_vote slow).
#include <algorithm>
#include <climits>

#include "avl_wave.h"

namespace avl {

constexpr int kSelectSlots = 64;                // slots of one group: 64 x 256 x 4 B = 64 KiB of LDS counters
constexpr int kSelectThreads = 1024;             // of a pass: two such workgroups fill a CU's 32 waves beside their 2 x 64 KiB of counters
constexpr int kSelectBins = 256;                // 8-bit digits, four passes
constexpr int kSelectUnroll = 4;                // row blocks whose loads are in flight together
constexpr int kSelectBlocksPerCu = 2;
constexpr int kAboveThreads = 256;
constexpr int kAboveMaxColumns = 1 << 20;       // 16384 word groups: blockIdx.y

struct SelectSlots {
    long long k[kSelectSlots];
    int col[kSelectSlots];
    int n;
};

// the per-group state in the workspace; one layout function for the size query and the consumer
struct SelectWork {
    unsigned long long* hist;                   // n x 256, zero between passes (a pick zeroes what it has read)
    long long* k_rem;
    unsigned long long* eq;                     // elements whose key is the selected one (after pick 3)
    unsigned long long* nan;
    unsigned* prefix;
    unsigned* next_key;                         // smallest key above the selected one, UINT_MAX when there is none
    size_t total;
};

static SelectWork select_layout(void* base) {
    Carver c(base);
    SelectWork w{};
    w.hist = c.ptr<unsigned long long>(sizeof(unsigned long long) * kSelectSlots * kSelectBins);
    w.k_rem = c.ptr<long long>(sizeof(long long) * kSelectSlots);
    w.eq = c.ptr<unsigned long long>(sizeof(unsigned long long) * kSelectSlots);
    w.nan = c.ptr<unsigned long long>(sizeof(unsigned long long) * kSelectSlots);
    w.prefix = c.ptr<unsigned>(sizeof(unsigned) * kSelectSlots);
    w.next_key = c.ptr<unsigned>(sizeof(unsigned) * kSelectSlots);
    w.total = c.total() + 256;                  // the entry point aligns the caller's base itself
    return w;
}

constexpr unsigned kNanKey = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned select_key(float x) {
    unsigned b = __float_as_uint(x);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return kNanKey;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float select_value(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

__global__ __launch_bounds__(kSelectThreads) void select_init_kernel(SelectSlots slots, SelectWork w) {
    for (int i = threadIdx.x; i < slots.n * kSelectBins; i += kSelectThreads) w.hist[i] = 0ull;
    if ((int)threadIdx.x < slots.n) {
        w.k_rem[threadIdx.x] = slots.k[threadIdx.x];
        w.prefix[threadIdx.x] = 0u;
        w.eq[threadIdx.x] = 0ull;
        w.nan[threadIdx.x] = 0ull;
        w.next_key[threadIdx.x] = UINT_MAX;
    }
}

// this thread's slot and row of a block of rows; false for the threads past the last whole row of the block
__device__ __forceinline__ bool select_place(int n, int* slot, int* row, int* rows) {
    *rows = kSelectThreads / n;
    *row = threadIdx.x / n;
    *slot = threadIdx.x - *row * n;
    return *row < *rows;
}

// PASS 0 .. 3: the digit histogram; shift = 24 - 8 * PASS
template <int PASS>
__global__ __launch_bounds__(kSelectThreads) void select_hist_kernel(const float* __restrict__ scores, long long N, long long ld,
                                                                     SelectSlots slots, SelectWork w) {
    extern __shared__ unsigned s_hist[];
    const int n = slots.n;
    for (int i = threadIdx.x; i < n * kSelectBins; i += kSelectThreads) s_hist[i] = 0u;
    __syncthreads();
    int slot, row, rows;
    if (select_place(n, &slot, &row, &rows)) {
        constexpr int shift = 24 - 8 * PASS, above = PASS ? shift + 8 : 0;              // the bits above the digit: the prefix so far
        const float* column = scores + slots.col[slot];
        const unsigned prefix = PASS ? w.prefix[slot] >> above : 0u;
        unsigned* mine = s_hist + slot * kSelectBins;
        const long long chunk = (long long)rows * kSelectUnroll;
        for (long long r0 = (long long)blockIdx.x * chunk + row; r0 < N; r0 += (long long)gridDim.x * chunk) {
            float x[kSelectUnroll];
#pragma unroll
            for (int u = 0; u < kSelectUnroll; ++u) {
                const long long r = r0 + (long long)u * rows;
                x[u] = column[(size_t)(r < N ? r : r0) * (size_t)ld];      // (a row past the end reads row r0 again and is dropped)
            }
#pragma unroll
            for (int u = 0; u < kSelectUnroll; ++u) {
                const unsigned key = select_key(x[u]);
                const bool in = r0 + (long long)u * rows < N && (PASS == 0 || (key >> above) == prefix);
                if (in) atomicAdd(mine + (((key >> shift) + slot) & (kSelectBins - 1)), 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n * kSelectBins; i += kSelectThreads) {
        const unsigned c = s_hist[i];
        if (c) {
            const int s = i / kSelectBins, b = (i - s) & (kSelectBins - 1);                 // undo the bank rotation
            atomicAdd(w.hist + s * kSelectBins + b, (unsigned long long)c);
        }
    }
}

// one workgroup per slot, thread b owns bin b
template <int PASS>
__global__ __launch_bounds__(kSelectBins) void select_pick_kernel(SelectWork w) {
    __shared__ unsigned long long s_w[kSelectBins / kWave];
    const int slot = blockIdx.x;
    unsigned long long* bin = w.hist + slot * kSelectBins + threadIdx.x;
    const unsigned long long c = *bin, k = (unsigned long long)w.k_rem[slot];
    *bin = 0ull;
    unsigned long long total;
    const unsigned long long below = block_excl_scan<kSelectBins / kWave>(c, OpSum{}, 0ull, s_w, &total);
    if (below <= k && k < below + c) {                                                    // exactly one bin: the counts sum to more than k
        w.prefix[slot] |= threadIdx.x << (24 - 8 * PASS);
        w.k_rem[slot] = (long long)(k - below);
        if (PASS == 3) w.eq[slot] = c;
    }
}

__global__ __launch_bounds__(kSelectThreads) void select_last_kernel(const float* __restrict__ scores, long long N, long long ld,
                                                                     SelectSlots slots, SelectWork w) {
    __shared__ unsigned s_next[kSelectSlots];
    __shared__ unsigned s_nan[kSelectSlots];
    const int n = slots.n;
    if ((int)threadIdx.x < n) {
        s_next[threadIdx.x] = UINT_MAX;
        s_nan[threadIdx.x] = 0u;
    }
    __syncthreads();
    int slot, row, rows;
    if (select_place(n, &slot, &row, &rows)) {
        const float* column = scores + slots.col[slot];
        const unsigned chosen = w.prefix[slot];
        unsigned next = UINT_MAX, nans = 0u;
        const long long chunk = (long long)rows * kSelectUnroll;
        for (long long r0 = (long long)blockIdx.x * chunk + row; r0 < N; r0 += (long long)gridDim.x * chunk) {
            float x[kSelectUnroll];
#pragma unroll
            for (int u = 0; u < kSelectUnroll; ++u) {
                const long long r = r0 + (long long)u * rows;
                x[u] = column[(size_t)(r < N ? r : r0) * (size_t)ld];      // (row r0 again: a minimum and a guarded count do not mind)
            }
#pragma unroll
            for (int u = 0; u < kSelectUnroll; ++u) {
                const unsigned key = select_key(x[u]);
                if (key > chosen && key < next) next = key;
                nans += (r0 + (long long)u * rows < N && key == kNanKey) ? 1u : 0u;
            }
        }
        if (next != UINT_MAX) atomicMin(s_next + slot, next);
        if (nans) atomicAdd(s_nan + slot, nans);
    }
    __syncthreads();
    if ((int)threadIdx.x < n) {
        if (s_next[threadIdx.x] != UINT_MAX) atomicMin(w.next_key + threadIdx.x, s_next[threadIdx.x]);
        if (s_nan[threadIdx.x]) atomicAdd(w.nan + threadIdx.x, (unsigned long long)s_nan[threadIdx.x]);
    }
}

__global__ __launch_bounds__(kSelectSlots) void select_finish_kernel(long long N, SelectSlots slots, SelectWork w, float* __restrict__ v_k,
                                                                     float* __restrict__ v_next, long long* __restrict__ count_lt,
                                                                     long long* __restrict__ count_le, long long* __restrict__ nan_count) {
    const int s = threadIdx.x;
    if (s >= slots.n) return;
    const long long k = slots.k[s], lt = k - w.k_rem[s], le = lt + (long long)w.eq[s];
    const unsigned chosen = w.prefix[s];
    v_k[s] = select_value(chosen);
    v_next[s] = select_value((le > k + 1 || k == N - 1) ? chosen : w.next_key[s]);
    count_lt[s] = lt;
    count_le[s] = le;
    nan_count[s] = (long long)w.nan[s];
}

__global__ __launch_bounds__(kAboveThreads) void cols_above_kernel(const float* __restrict__ scores, long long N, int Q, long long ld,
                                                                   const double* __restrict__ thr, int mask_column,
                                                                   unsigned long long* __restrict__ bits, unsigned long long* __restrict__ counts,
                                                                   uint8_t* __restrict__ mask) {
    __shared__ unsigned s_count[kAboveThreads];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, group = blockIdx.y, groups = gridDim.y;
    const int col = group * kWave + lane;
    const bool has_col = col < Q;
    const double t = has_col ? thr[col] : 0.0;
    const float* column = scores + (has_col ? col : 0);
    const bool masks = mask && mask_column / kWave == group;
    const long long tiles = (N + kWave - 1) / kWave;
    unsigned mine = 0u;
    for (long long tile = (long long)blockIdx.x * (kAboveThreads / kWave) + wave; tile < tiles;
         tile += (long long)gridDim.x * (kAboveThreads / kWave)) {                         // (wave-uniform: the ballots see whole waves)
        const long long r0 = tile * kWave;
        const int here = (int)(N - r0 < kWave ? N - r0 : kWave);
        unsigned long long word = 0ull;
#pragma unroll 8
        for (int i = 0; i < kWave; ++i) {
            const bool live = has_col && i < here;
            const float x = column[(size_t)(live ? r0 + i : r0) * (size_t)ld];
            const bool above = live && (double)x > t;                                      // (NaN on either side: false)
            const unsigned long long b = __ballot(above);
            mine += above ? 1u : 0u;
            if (lane == i) word = b;
        }
        if (lane < here) {
            bits[(size_t)(r0 + lane) * groups + group] = word;
            if (masks) mask[r0 + lane] = (uint8_t)(word >> (mask_column & (kWave - 1)) & 1ull);
        }
    }
    s_count[threadIdx.x] = mine;
    __syncthreads();
    if (wave == 0 && has_col) {
        unsigned long long sum = 0ull;
#pragma unroll
        for (int v = 0; v < kAboveThreads / kWave; ++v) sum += s_count[v * kWave + lane];
        if (sum) atomicAdd(counts + col, sum);
    }
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_colselect_workspace_bytes(int n_slots, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_colselect_workspace_bytes: null pointer");
    AVL_REQUIRE(n_slots >= 0, "avl_colselect_workspace_bytes: %d slots", n_slots);
    *bytes = select_layout(nullptr).total;      // the groups of a call share one workspace: the size does not grow with the slots
    return AVL_OK;
}

int avl_colselect_f32(const float* d_scores, int64_t N, int Q, int64_t ld, const int32_t* h_columns, const int64_t* h_ks, int n_slots,
                      float* d_v_k, float* d_v_next, int64_t* d_count_lt, int64_t* d_count_le, int64_t* d_nan_count, void* ws,
                      size_t ws_bytes, void* stream) {
    AVL_REQUIRE(N >= 1 && N <= INT_MAX, "avl_colselect_f32: N = %lld rows (1 .. 2^31 - 1)", (long long)N);
    AVL_REQUIRE(Q >= 1, "avl_colselect_f32: Q = %d columns", Q);
    AVL_REQUIRE(ld >= Q, "avl_colselect_f32: row stride ld = %lld < Q = %d", (long long)ld, Q);
    AVL_REQUIRE(n_slots >= 0, "avl_colselect_f32: %d slots", n_slots);
    if (n_slots == 0) return AVL_OK;
    AVL_REQUIRE(h_columns && h_ks, "avl_colselect_f32: null pointer (slot tables)");
    for (int s = 0; s < n_slots; ++s) {
        AVL_REQUIRE(h_columns[s] >= 0 && h_columns[s] < Q, "avl_colselect_f32: slot %d names column %d of %d", s, h_columns[s], Q);
        AVL_REQUIRE(h_ks[s] >= 0 && h_ks[s] < N, "avl_colselect_f32: slot %d asks for k = %lld of N = %lld", s, (long long)h_ks[s],
                    (long long)N);
    }
    AVL_REQUIRE(d_scores && d_v_k && d_v_next && d_count_lt && d_count_le && d_nan_count, "avl_colselect_f32: null pointer");
    AVL_REQUIRE(ws, "avl_colselect_f32: null pointer (workspace ws)");
    void* base = align256_ptr(ws);
    const SelectWork w = select_layout(base);
    AVL_REQUIRE(ws_bytes >= w.total, "avl_colselect_f32: workspace (ws) of %zu bytes, %zu needed", ws_bytes, w.total);
    hipStream_t st = as_stream(stream);
    for (int s0 = 0; s0 < n_slots; s0 += kSelectSlots) {
        SelectSlots slots{};
        slots.n = std::min(kSelectSlots, n_slots - s0);
        for (int s = 0; s < slots.n; ++s) {
            slots.col[s] = h_columns[s0 + s];
            slots.k[s] = h_ks[s0 + s];
        }
        const size_t lds = (size_t)slots.n * kSelectBins * sizeof(unsigned);
        const int64_t chunk = (int64_t)(kSelectThreads / slots.n) * kSelectUnroll, chunks = (N + chunk - 1) / chunk;
        const unsigned blocks = (unsigned)std::min<int64_t>(chunks, (int64_t)num_cus() * kSelectBlocksPerCu);
        const dim3 grid(blocks), threads(kSelectThreads);
        hipLaunchKernelGGL(select_init_kernel, dim3(1), threads, 0, st, slots, w);
        hipLaunchKernelGGL(select_hist_kernel<0>, grid, threads, lds, st, d_scores, (long long)N, (long long)ld, slots, w);
        hipLaunchKernelGGL(select_pick_kernel<0>, dim3(slots.n), dim3(kSelectBins), 0, st, w);
        hipLaunchKernelGGL(select_hist_kernel<1>, grid, threads, lds, st, d_scores, (long long)N, (long long)ld, slots, w);
        hipLaunchKernelGGL(select_pick_kernel<1>, dim3(slots.n), dim3(kSelectBins), 0, st, w);
        hipLaunchKernelGGL(select_hist_kernel<2>, grid, threads, lds, st, d_scores, (long long)N, (long long)ld, slots, w);
        hipLaunchKernelGGL(select_pick_kernel<2>, dim3(slots.n), dim3(kSelectBins), 0, st, w);
        hipLaunchKernelGGL(select_hist_kernel<3>, grid, threads, lds, st, d_scores, (long long)N, (long long)ld, slots, w);
        hipLaunchKernelGGL(select_pick_kernel<3>, dim3(slots.n), dim3(kSelectBins), 0, st, w);
        hipLaunchKernelGGL(select_last_kernel, grid, threads, 0, st, d_scores, (long long)N, (long long)ld, slots, w);
        hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(kSelectSlots), 0, st, (long long)N, slots, w, d_v_k + s0, d_v_next + s0,
                           (long long*)d_count_lt + s0, (long long*)d_count_le + s0, (long long*)d_nan_count + s0);
        AVL_HIP_CHECK(hipGetLastError());
    }
    return AVL_OK;
}

int avl_cols_above_f32(const float* d_scores, int64_t N, int Q, int64_t ld, const double* d_thresholds, int mask_column, uint64_t* d_bits,
                       int64_t* d_counts, uint8_t* d_mask, void* stream) {
    AVL_REQUIRE(N >= 0 && N <= INT_MAX, "avl_cols_above_f32: N = %lld rows (0 .. 2^31 - 1)", (long long)N);
    AVL_REQUIRE(Q >= 1 && Q <= kAboveMaxColumns, "avl_cols_above_f32: Q = %d columns (1 .. %d)", Q, kAboveMaxColumns);
    AVL_REQUIRE(ld >= Q, "avl_cols_above_f32: row stride ld = %lld < Q = %d", (long long)ld, Q);
    AVL_REQUIRE(d_mask ? (mask_column >= 0 && mask_column < Q) : mask_column == -1,
                "avl_cols_above_f32: mask column %d of %d (a column with d_mask, -1 without)", mask_column, Q);
    AVL_REQUIRE(d_thresholds && d_counts && (N == 0 || (d_scores && d_bits)), "avl_cols_above_f32: null pointer");
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)Q, st));
    if (N == 0) return AVL_OK;
    const int groups = (Q + kWave - 1) / kWave, waves = kAboveThreads / kWave;
    const int64_t tiles = (N + kWave - 1) / kWave, want = (tiles + waves - 1) / waves;
    const unsigned blocks = (unsigned)std::min<int64_t>(want, std::max<int64_t>(1, (int64_t)num_cus() * 8 / groups));
    hipLaunchKernelGGL(cols_above_kernel, dim3(blocks, (unsigned)groups), dim3(kAboveThreads), 0, st, d_scores, (long long)N, Q, (long long)ld,
                       d_thresholds, mask_column, (unsigned long long*)d_bits, (unsigned long long*)d_counts, d_mask);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
