// K travel-distance fields on one free map in one batch for gfx950, the set-to-set arrivals read from their planes, and the sound
// field that decays around walls.  Upstream has no counterpart.
//
// Definition.  Field k is avl_travel.hip's field whose sources are the cells cells[offsets[k] .. offsets[k + 1]):
// the same legal-step rule, the same exact order of the pairs (travel_less), the same 64-bit state word.  A set may repeat a cell
// and its cells may lie on obstacles.
//
// Work.  One work item is a (field, tile) pair: a flat grid of K * tiles workgroups, workgroup k * tiles + t runs tile t of field k
// when mark [k * tiles + t] of the round is set and returns at once otherwise.  The tile's body is the shared one of
// avl_travel_tile.h, here travel_tile_relax<false, true>: unit steps, the source bit read off the state word.  Two mark buffers
// of K * tiles words, one `activated` counter per round for the whole batch, and the host loop travel_run_rounds with
// tiles := K * tiles: the batch has converged when a round wakes no pair, so it runs as many rounds as its slowest field and
// shares every launch and every synchronisation.
//
// What differs from the single field:
//   * The free bits are ONE plane of H * W bytes for all K fields (copied out of the caller's strided image once).
//   * A field's source bit is not stored.  A cell is a source of field k exactly when its state word is (0, 0): the initialisation
//     writes (0, 0) on the sources alone, every other stored word is "a stored neighbour + a legal step" and so has a + b >= 1, and
//     a source is never relaxed.  The LDS passability byte is therefore free | (state == 0) << 1 at load time and the legal-step
//     rule applies unchanged.  A (0, 0) word never changes, so a halo read that races with a neighbour's write-back sees the same bit.
//   * A mark made by field k stays inside field k: the neighbour tile (ur, uc) is bounds-checked against (th, tw) first and then
//     offset by k * tiles, so no index of field k can fall into the marks of field k - 1 or k + 1.
//
// Workspace.  256 + align256(256) + align256(8 K T) + align256(H W) + align256(8 K H W) bytes with T = ceil(H / 32) * ceil(W / 32):
// a header, two mark words per (field, tile) pair, the shared free plane, a state word per field and cell.  align256(K x) <= K *
// align256(x), so this is at most K * avl_travel2d_workspace_bytes(H, W), which is what the entry point asks for.
//
// The convergence argument is avl_travel.hip's per field: the fields share nothing that is written but the round's counter.
#include <algorithm>
#include <cmath>

#include "avl_common.h"
#include "avl_travel_tile.h"
#include "avl_wave.h"

namespace avl {

constexpr int kManyMaxFields = 1024;
constexpr int64_t kManyMaxPairs = 1ll << 28;     // K * tiles: the flat grid

// the shared free plane, every state word unreached, and zeros in the header, both mark buffers (`words` uint32 from hdr on) and the
// stats: one launch instead of a kernel and two memsets.  `span` = the largest of the four counts.
__global__ __launch_bounds__(256) void many_init_kernel(const uint8_t* __restrict__ free_u8, int64_t ld_free, int H, int W, int64_t total,
                                                        int64_t words, int n_stats, int64_t span, uint8_t* __restrict__ freep,
                                                        unsigned long long* __restrict__ state, unsigned* __restrict__ hdr,
                                                        unsigned long long* __restrict__ stats) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < total) state[i] = kTravelUnreached;
        if (i < n) {
            const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
            freep[i] = free_u8[(int64_t)r * ld_free + c] != 0 ? kTravelFree : (uint8_t)0;
        }
        if (i < words) hdr[i] = 0u;
        if (i < n_stats) stats[i] = 0ull;
    }
}

// (0, 0) on the cells of every set; the tile of every source and its eight neighbours start active in the set's own marks.  The field
// of cell i is the last k with offsets[k] <= i.  A cell outside the map, and one that no set covers, is passed over.
__global__ __launch_bounds__(256) void many_sources_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ cells, int K,
                                                           int64_t L, int H, int W, unsigned long long* __restrict__ state,
                                                           unsigned* __restrict__ flags, unsigned* __restrict__ hdr) {
    const int tw = travel_tiles(W), th = travel_tiles(H);
    const int64_t n = (int64_t)H * W, tiles = (int64_t)tw * th;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (int64_t)gridDim.x * blockDim.x) {
        int lo = 0, hi = K;                           // offsets[lo] <= i < offsets[hi] when the offsets are CSR offsets
        while (hi - lo > 1) {
            const int mid = (lo + hi) / 2;
            if (offsets[mid] <= i) lo = mid; else hi = mid;
        }
        if (i < offsets[lo] || i >= offsets[lo + 1]) continue;
        const int r = cells[2 * i], c = cells[2 * i + 1];
        if (r < 0 || r >= H || c < 0 || c >= W) continue;
        travel_store(&state[(int64_t)lo * n + (int64_t)r * W + c], 0ull);
        if (hdr[kTravelHdrAny] == 0u) atomicExch(&hdr[kTravelHdrAny], 1u);
        travel_mark_around<kTravelTile>(flags + (int64_t)lo * tiles, r, c, th, tw, &hdr[kTravelHdrInit]);
    }
}

// One round of every (field, tile) pair: see the head of the file.  cur / next: the active marks of this round and of the coming one.
__global__ __launch_bounds__(kTravelThreads) void many_round_kernel(const uint8_t* __restrict__ freep, unsigned long long* state_all, int H, int W,
                                                                    unsigned tiles, unsigned* __restrict__ cur, unsigned* __restrict__ next,
                                                                    unsigned* __restrict__ activated) {
    __shared__ TravelTileLds lds;
    if (!travel_take_mark(cur, &lds.active, &lds.dirty)) return;
    const unsigned field = blockIdx.x / tiles, tile = blockIdx.x - field * tiles;
    const int tile_r = (int)tile / travel_tiles(W), tile_c = (int)tile - tile_r * travel_tiles(W);
    // the field's own words and marks: K * tiles <= 2^28
    travel_tile_relax<false, true>(lds, freep, nullptr, 0, state_all + (int64_t)field * ((int64_t)H * W), H, W, tile_r, tile_c,
                                   (int)(field * tiles), next, activated);
}

// the two int32 planes of field blockIdx.y, its number of reached cells, and the host's counters into
// d_stats = [rounds, tile runs, reached_0 .. reached_{K - 1}]
__global__ __launch_bounds__(256) void many_unpack_kernel(const unsigned long long* __restrict__ state, int64_t n, int32_t* __restrict__ straight,
                                                          int32_t* __restrict__ diagonal, long long rounds, long long tile_runs,
                                                          unsigned long long* __restrict__ stats) {
    const int64_t at = (int64_t)blockIdx.y * n;
    unsigned long long reached = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long s = state[at + i];
        straight[at + i] = (int32_t)(unsigned)(s >> 32);
        diagonal[at + i] = (int32_t)(unsigned)s;
        reached += s != kTravelUnreached;
    }
    reached = wave_sum(reached);
    if ((threadIdx.x & (kWave - 1)) == 0 && reached) atomicAdd(&stats[2 + blockIdx.y], reached);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        stats[0] = (unsigned long long)rounds;
        stats[1] = (unsigned long long)tile_runs;
    }
}

// One wave per (field k, target set j): see avl_travel_arrive in the header.  A candidate is (word, cell index, direction); the
// smaller word wins, then the smaller cell index; inside a cell the first direction wins because only a smaller word replaces.
__global__ __launch_bounds__(256) void many_arrive_kernel(const uint8_t* __restrict__ free_u8, int64_t ld_free, int H, int W,
                                                          const int32_t* __restrict__ straight, const int32_t* __restrict__ diagonal, int K,
                                                          const int64_t* __restrict__ offsets, const int32_t* __restrict__ cells, int M, int64_t L,
                                                          int32_t* __restrict__ out_a, int32_t* __restrict__ out_b, int32_t* __restrict__ out_cell,
                                                          int32_t* __restrict__ out_from) {
    const int64_t pair = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
    if (pair >= (int64_t)K * M) return;               // whole waves leave: the shuffles below see all 64 lanes
    const int k = (int)(pair / M), j = (int)(pair - (int64_t)k * M);
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n = (int64_t)H * W;
    const int32_t* A = straight + (int64_t)k * n;
    const int32_t* B = diagonal + (int64_t)k * n;
    int64_t b = offsets[j], e = offsets[j + 1];       // (clamped to [0, L]: never read past the cells)
    b = b < 0 ? 0 : (b > L ? L : b);
    e = e < b ? b : (e > L ? L : e);
    unsigned long long best = kTravelUnreached;
    long long best_cell = -1;
    int best_from = -1;
    for (int64_t i = b + lane; i < e; i += kWave) {
        const int r = cells[2 * i], c = cells[2 * i + 1];
        if (r < 0 || r >= H || c < 0 || c >= W) continue;
        unsigned long long w = kTravelUnreached;
        int from = -1;
        if (A[(int64_t)r * W + c] == 0 && B[(int64_t)r * W + c] == 0) {
            w = 0ull;                                   // the target is a source of field k
        } else {
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int ur = r + travel_dr(d), uc = c + travel_dc(d);
                if (ur < 0 || ur >= H || uc < 0 || uc >= W) continue;
                const int32_t a = A[(int64_t)ur * W + uc];
                if (a < 0) continue;
                if ((d & 1) && !(free_u8[(int64_t)ur * ld_free + c] != 0 && free_u8[(int64_t)r * ld_free + uc] != 0)) continue;
                const unsigned long long cand =
                    ((unsigned long long)(unsigned)a << 32 | (unsigned)B[(int64_t)ur * W + uc]) + ((d & 1) ? kTravelDiagonal : kTravelStraight);
                if (w == kTravelUnreached || travel_less(cand, w)) {
                    w = cand;
                    from = d;
                }
            }
        }
        if (w != kTravelUnreached && (best == kTravelUnreached || travel_less(w, best))) {      // i grows: ties keep the earlier cell
            best = w;
            best_cell = i;
            best_from = from;
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned long long ow = __shfl_xor(best, off, kWave);
        const long long oc = __shfl_xor(best_cell, off, kWave);
        const int of = __shfl_xor(best_from, off, kWave);
        if (ow == kTravelUnreached) continue;
        if (best == kTravelUnreached || travel_less(ow, best) || (ow == best && oc < best_cell)) {
            best = ow;
            best_cell = oc;
            best_from = of;
        }
    }
    if (lane == 0) {
        const bool ok = best != kTravelUnreached;
        out_a[pair] = ok ? (int32_t)(unsigned)(best >> 32) : -1;
        out_b[pair] = ok ? (int32_t)(unsigned)best : -1;
        out_cell[pair] = ok ? (int32_t)best_cell : -1;
        out_from[pair] = ok ? best_from : -1;
    }
}

// field_sound_kernel with the travel distance: for every cell and for the segments s = 0 .. K - 1 in order
//   d = double(a) + double(b) * sqrt(2) (unfused);  t = p - (p * d) * decay in float64, < 0 -> 0, unreached -> 0;  acc = float(double(acc) + t)
// on zeros (first) or on what the field holds; [min, max] of the field by bit pattern
__global__ __launch_bounds__(256) void many_sound_kernel(const int32_t* __restrict__ straight, const int32_t* __restrict__ diagonal, int K,
                                                         int64_t n, const float* __restrict__ peaks, double decay, int first,
                                                         float* __restrict__ field, unsigned int* __restrict__ minmax) {
    __shared__ double s_red[2 * 256 / kWave];
    double mn = INFINITY, mx = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float acc = first ? 0.0f : field[i];
        for (int s = 0; s < K; ++s) {
            const float p = peaks[s];
            if (p == 0.0f) continue;                                       // adds exactly +0 everywhere
            const int32_t a = straight[(int64_t)s * n + i], b = diagonal[(int64_t)s * n + i];
            double t = 0.0;
            if (a >= 0 && b >= 0) {
                const double pd = (double)p;
                const double d = (double)a + (double)b * 1.4142135623730951;
                t = pd - (pd * d) * decay;
                if (t < 0.0) t = 0.0;
            }
            acc = (float)((double)acc + t);
        }
        field[i] = acc;
        mn = fmin(mn, (double)acc);
        mx = fmax(mx, (double)acc);
    }
    block_minmax_atomic<256>(mn, mx, minmax, s_red);
}

// field_normalize_kernel's float32 expression on an (H, W) field
__global__ __launch_bounds__(256) void many_sound_normalize_kernel(const float* __restrict__ field, const float* __restrict__ minmax, int64_t n,
                                                                   float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        out[i] = __fdiv_rn(field[i] - minmax[0], minmax[1] - minmax[0]);
    }
}

static int many_check_shape(const char* what, int H, int W, int K) {
    int rc = travel_check_shape(what, H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(K >= 1 && K <= kManyMaxFields, "%s: %d fields (1 .. %d)", what, K, kManyMaxFields);
    return AVL_OK;
}

struct ManyLayout {
    size_t hdr, flags, free, state, total;
};

static ManyLayout many_layout(int H, int W, int K) {
    const size_t tiles = (size_t)travel_tiles(H) * (size_t)travel_tiles(W);
    Carver c;
    ManyLayout l;
    l.hdr = c.take(kTravelHdrWords * sizeof(unsigned));
    l.flags = c.take(2 * (size_t)K * tiles * sizeof(unsigned));
    l.free = c.take((size_t)H * W);
    l.state = c.take((size_t)K * H * W * sizeof(unsigned long long));
    l.total = c.total() + 256;                        // the entry point aligns the base itself
    return l;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_travel2d_many(const uint8_t* d_free, int64_t ld_free, int H, int W, const int64_t* d_offsets, const int32_t* d_cells, int K, int64_t L,
                      int32_t* d_straight, int32_t* d_diagonal, int64_t* d_stats, void* ws, size_t ws_bytes, void* stream) {
    int rc = many_check_shape("avl_travel2d_many", H, W, K);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_free && d_offsets && d_cells, "avl_travel2d_many: null free image, offsets or cells");
    AVL_REQUIRE(d_straight && d_diagonal && d_stats, "avl_travel2d_many: null output plane or stats pointer");
    AVL_REQUIRE(ld_free >= W, "avl_travel2d_many: free rows of %lld cells cannot hold %d columns", (long long)ld_free, W);
    AVL_REQUIRE(L >= K && L <= (1ll << 40), "avl_travel2d_many: %lld cells for %d sets (every set holds one or more)", (long long)L, K);
    const int64_t tiles1 = (int64_t)travel_tiles(W) * travel_tiles(H);
    AVL_REQUIRE((int64_t)K * tiles1 <= kManyMaxPairs, "avl_travel2d_many: %d fields of %lld tiles exceed 2^28 (field, tile) pairs", K,
                (long long)tiles1);
    const size_t need = (size_t)K * travel_layout(H, W).total;
    const ManyLayout l = many_layout(H, W, K);
    AVL_REQUIRE(ws && ws_bytes >= need, "avl_travel2d_many: workspace of %zu bytes, need %zu (%d x avl_travel2d_workspace_bytes)", ws_bytes,
                need, K);
    AVL_REQUIRE(l.total <= need, "avl_travel2d_many: layout of %zu bytes above %zu", l.total, need);      // cannot happen: see the head of the file
    hipStream_t st = as_stream(stream);
    char* base = (char*)align256_ptr(ws);
    unsigned* hdr = (unsigned*)(base + l.hdr);
    unsigned* flags = (unsigned*)(base + l.flags);
    uint8_t* freep = (uint8_t*)(base + l.free);
    unsigned long long* state = (unsigned long long*)(base + l.state);
    const unsigned tiles = (unsigned)tiles1, pairs = (unsigned)(K * tiles1);
    const int64_t n = (int64_t)H * W, total = (int64_t)K * n;

    const int64_t words = (int64_t)((l.free - l.hdr) / sizeof(unsigned));   // the header and both mark buffers
    const int64_t span = std::max<int64_t>(std::max<int64_t>(total, words), 2 + K);
    hipLaunchKernelGGL(many_init_kernel, dim3(stride_blocks(span)), dim3(256), 0, st, d_free, ld_free, H, W, total, words, 2 + K, span, freep,
                       state, hdr, reinterpret_cast<unsigned long long*>(d_stats));
    hipLaunchKernelGGL(many_sources_kernel, dim3(stride_blocks(L)), dim3(256), 0, st, d_offsets, d_cells, K, L, H, W, state, flags, hdr);
    AVL_HIP_CHECK(hipGetLastError());

    // a shortest walk has fewer than H * W steps and every round moves every pending walk of every field on by a step or more
    const int64_t max_rounds = n + 1;
    int64_t rounds = 0, tile_runs = 0;
    unsigned host[kTravelHdrWords];
    rc = travel_run_rounds(
        "avl_travel2d_many", max_rounds, hdr, flags, pairs, st,
        [&](int64_t, unsigned* cur, unsigned* next, unsigned* activated) {
            hipLaunchKernelGGL(many_round_kernel, dim3(pairs), dim3(kTravelThreads), 0, st, (const uint8_t*)freep, state, H, W, tiles, cur, next,
                               activated);
        },
        &rounds, &tile_runs, host);
    if (rc != AVL_OK) return rc;
    const unsigned xb = std::max(1u, std::min(stride_blocks(n), (unsigned)((num_cus() * 16 + K - 1) / K)));
    hipLaunchKernelGGL(many_unpack_kernel, dim3(xb, (unsigned)K), dim3(256), 0, st, (const unsigned long long*)state, n, d_straight, d_diagonal,
                       (long long)rounds, (long long)tile_runs, reinterpret_cast<unsigned long long*>(d_stats));
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_travel_arrive(const uint8_t* d_free, int64_t ld_free, int H, int W, const int32_t* d_straight, const int32_t* d_diagonal, int K,
                      const int64_t* d_offsets, const int32_t* d_cells, int M, int64_t L, int32_t* d_a, int32_t* d_b, int32_t* d_cell,
                      int32_t* d_from, void* stream) {
    int rc = many_check_shape("avl_travel_arrive", H, W, K);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(M >= 1 && M <= kManyMaxFields, "avl_travel_arrive: %d target sets (1 .. %d)", M, kManyMaxFields);
    AVL_REQUIRE(L >= 0 && L < (1ll << 31), "avl_travel_arrive: %lld target cells (0 .. 2^31 - 1)", (long long)L);
    AVL_REQUIRE(d_free && d_straight && d_diagonal && d_offsets && (L == 0 || d_cells), "avl_travel_arrive: null input pointer");
    AVL_REQUIRE(d_a && d_b && d_cell && d_from, "avl_travel_arrive: null output pointer");
    AVL_REQUIRE(ld_free >= W, "avl_travel_arrive: free rows of %lld cells cannot hold %d columns", (long long)ld_free, W);
    const int64_t pairs = (int64_t)K * M;
    hipLaunchKernelGGL(many_arrive_kernel, dim3((unsigned)((pairs + 256 / kWave - 1) / (256 / kWave))), dim3(256), 0, as_stream(stream), d_free,
                       ld_free, H, W, d_straight, d_diagonal, K, d_offsets, d_cells, M, L, d_a, d_b, d_cell, d_from);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_travel_sound2d(const int32_t* d_straight, const int32_t* d_diagonal, int K, int H, int W, const float* d_peaks, double decay_rate,
                       int first, float* d_field, float* d_minmax, void* stream) {
    int rc = many_check_shape("avl_travel_sound2d", H, W, K);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_straight && d_diagonal && d_peaks && d_field && d_minmax, "avl_travel_sound2d: null pointer");
    AVL_REQUIRE(decay_rate >= 0.0 && std::isfinite(decay_rate), "avl_travel_sound2d: decay_rate must be finite and >= 0");
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(d_minmax, 0xFF, sizeof(float), st));       // min: all ones = above every non-negative value
    AVL_HIP_CHECK(hipMemsetAsync(d_minmax + 1, 0, sizeof(float), st));      // max: +0
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(many_sound_kernel, dim3(stride_blocks(n)), dim3(256), 0, st, d_straight, d_diagonal, K, n, d_peaks, decay_rate, first,
                       d_field, reinterpret_cast<unsigned int*>(d_minmax));
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_travel_sound_normalize(const float* d_field, const float* d_minmax, int H, int W, float* d_out, void* stream) {
    int rc = many_check_shape("avl_travel_sound_normalize", H, W, 1);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_field && d_minmax && d_out, "avl_travel_sound_normalize: null pointer");
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(many_sound_normalize_kernel, dim3(stride_blocks(n)), dim3(256), 0, as_stream(stream), d_field, d_minmax, n, d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
