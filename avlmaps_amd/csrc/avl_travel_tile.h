// The tile scheme of the travel-distance field (avl_travel.hip), the cost field (avl_costfield.hip), the batch of K fields
// (avl_travel_many.hip) and the label growth (avl_rooms.hip), one definition of each piece so that the kernel families cannot drift
// apart: the tile geometry, the packed state word and the exact order of two of them, the single-word loads and stores, the
// passability bits, the active marks, the legal-step rule, the relaxation of one tile (travel_tile_relax, which the three field
// families instantiate), its prologue and epilogue (travel_take_mark and travel_wake, which the label growth uses around a sweep of
// its own), the single field's workspace and the host loop that launches rounds in batches until one activates no tile.
#pragma once
#include <algorithm>

#include "avl_common.h"

namespace avl {

constexpr int kTravelMaxSide = 16384;            // avl_edt2d.hip's kEdtMaxSide: the decay maps of both families cover the same crops
constexpr int kTravelTile = 32;                  // cells per tile side
constexpr int kTravelThreads = 256;
constexpr int kTravelCells = kTravelTile * kTravelTile / kTravelThreads;   // cells per thread: 4, rows ty, ty + 8, ty + 16, ty + 24
constexpr int kTravelSweeps = 64;                // in-tile sweep cap: an open tile converges in ~33, a corridor maze continues next round
constexpr int kTravelHalo = kTravelTile + 2;
constexpr int kTravelRoundBatch = 8;             // rounds launched between two convergence checks
constexpr unsigned long long kTravelUnreached = ~0ull;
constexpr unsigned long long kTravelStraight = 1ull << 32, kTravelDiagonal = 1ull;
constexpr uint8_t kTravelFree = 1, kTravelSource = 2;

// header words of the workspace (uint32)
constexpr int kTravelHdrAny = 0;                 // a source exists
constexpr int kTravelHdrInit = 1;                // tiles the initialisation marked active
constexpr int kTravelHdrRound = 8;               // [kTravelRoundBatch] tiles marked active by each round of the current batch
constexpr int kTravelHdrWords = 64;

__device__ __forceinline__ unsigned long long travel_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void travel_store(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// tiles along a side of `cells` cells
__host__ __device__ __forceinline__ constexpr int travel_tiles(int cells) { return (cells + kTravelTile - 1) / kTravelTile; }

// a1 + b1 sqrt(2) < a2 + b2 sqrt(2) for two reached words, exactly and in integers: the sign cases of da against db, then da^2
// against 2 db^2 in int64.  No floating-point key is involved.  Bounds: a step field has a, b <= H * W <= 2^28, a cost field
// A, B < 2^30 (kCostMaxCells cells of price <= 255); either way da and db fit an int and da^2 < 2^60, 2 db^2 < 2^61 stay in int64.
__device__ __forceinline__ bool travel_less(unsigned long long p, unsigned long long q) {
    const int da = (int)(unsigned)(p >> 32) - (int)(unsigned)(q >> 32);
    const int db = (int)(unsigned)p - (int)(unsigned)q;
    if (da <= 0 && db <= 0) return (da | db) != 0;
    if (da >= 0 && db >= 0) return false;
    const long long a2 = (long long)da * da, b2 = 2ll * ((long long)db * db);
    return da < 0 ? a2 > b2 : a2 < b2;               // da < 0 < db: |da| > db sqrt(2);  db < 0 < da: da < |db| sqrt(2)
}

// marks tile t active for the coming round; *count counts the tiles that were not marked yet
__device__ __forceinline__ void travel_mark(unsigned* __restrict__ flags, int t, unsigned* __restrict__ count) {
    if (atomicExch(&flags[t], 1u) == 0u) atomicAdd(count, 1u);
}

// marks the tile of cell (r, c) and its eight neighbours (the cell may be their halo) active, counted in *count
template <int TILE>
__device__ __forceinline__ void travel_mark_around(unsigned* __restrict__ flags, int r, int c, int th, int tw, unsigned* __restrict__ count) {
    const int tr = r / TILE, tc = c / TILE;
#pragma unroll
    for (int dr = -1; dr <= 1; ++dr) {
#pragma unroll
        for (int dc = -1; dc <= 1; ++dc) {
            const int ur = tr + dr, uc = tc + dc;
            if (ur < 0 || ur >= th || uc < 0 || uc >= tw) continue;
            if (flags[ur * tw + uc] == 0u) travel_mark(flags, ur * tw + uc, count);
        }
    }
}

// the eight directions in 45 degree steps, E first (avl_nav.hip's order): odd = diagonal
__device__ __forceinline__ constexpr int travel_dr(int k) { return k == 0 || k == 4 ? 0 : (k < 4 ? -1 : 1); }
__device__ __forceinline__ constexpr int travel_dc(int k) { return k == 2 || k == 6 ? 0 : (k == 3 || k == 4 || k == 5 ? -1 : 1); }

// The legal-step rule on a tile's passability bytes in LDS (rows of HALO cells, `at` inside the tile).  Bit k: the step from the
// neighbour in direction k to this cell is legal.  A source keeps (0, 0) and a blocked cell is never entered: both get 0.
template <int HALO>
__device__ __forceinline__ unsigned travel_legal_in(const uint8_t* s_pass, int at) {
    unsigned m = 0;
    const uint8_t pv = s_pass[at];
    if ((pv & kTravelFree) && !(pv & kTravelSource)) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            bool ok = s_pass[at + travel_dr(k) * HALO + travel_dc(k)] != 0;      // u is free or a source
            if (k & 1) ok = ok && (s_pass[at + travel_dr(k) * HALO] & kTravelFree) && (s_pass[at + travel_dc(k)] & kTravelFree);
            m |= ok ? 1u << k : 0u;
        }
    }
    return m;
}

// bit k of the result: the neighbour tile in direction k reads the tile's cell (lr, lc) as halo
template <int TILE>
__device__ __forceinline__ unsigned travel_halo_readers(int lr, int lc) {
    const bool n = lr == 0, s = lr == TILE - 1, w = lc == 0, e = lc == TILE - 1;
    return (e ? 1u << 0 : 0u) | (n && e ? 1u << 1 : 0u) | (n ? 1u << 2 : 0u) | (n && w ? 1u << 3 : 0u) | (w ? 1u << 4 : 0u) |
           (s && w ? 1u << 5 : 0u) | (s ? 1u << 6 : 0u) | (s && e ? 1u << 7 : 0u);
}

// The initialisation of cell i = r * W + c: pass = passable | source << 1, state = (0, 0) on a source and unreached elsewhere; a
// source sets the header's "a source exists" and starts its tile and the eight around it (it may be their halo) active.
__device__ __forceinline__ void travel_init_cell(int64_t i, int r, int c, bool passable, bool source, int th, int tw, uint8_t* __restrict__ pass,
                                                 unsigned long long* __restrict__ state, unsigned* __restrict__ flags,
                                                 unsigned* __restrict__ hdr) {
    pass[i] = (uint8_t)((passable ? kTravelFree : 0) | (source ? kTravelSource : 0));
    state[i] = source ? 0ull : kTravelUnreached;
    if (source) {
        if (hdr[kTravelHdrAny] == 0u) atomicExch(&hdr[kTravelHdrAny], 1u);
        travel_mark_around<kTravelTile>(flags, r, c, th, tw, &hdr[kTravelHdrInit]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One round of one tile.
//
// Work.  The grid is cut into 32 x 32 tiles, one 256-thread workgroup each, four cells per thread.  A round is one plain launch
// over all work items (a tile, or a (field, tile) pair of the batch); workgroup blockIdx.x owns mark blockIdx.x and returns at once
// when it is not set (travel_take_mark).  An active tile loads its cells and a one-cell halo of state and passability into LDS,
// turns passability into one byte per cell of legal incoming directions (travel_legal_in, registers), and sweeps pull-relaxations
// over its cells: every thread reads the neighbours of its cells, a barrier, every thread writes what got smaller, a barrier that
// also ORs "something changed".  The sweeps end when one changes nothing or after kTravelSweeps of them.  The tile writes the cells
// that changed back, marks each of its eight neighbours active for the next round when a cell they see as halo changed, and marks
// itself when it ran into the sweep cap (travel_wake).  The host launches kTravelRoundBatch rounds, reads how many tiles each round
// activated, and stops when the last round of a batch activated none (travel_run_rounds).
//
// One state buffer, read and written in place with single aligned 64-bit accesses (relaxed atomics of device scope, so the
// compiler can neither split nor duplicate them).  Only the workgroup that owns a cell writes it.  A neighbour that reads the
// cell as halo in the same round sees the old or the new word, never a mixture; both are lengths of real walks.  If it saw the
// old one, the owner has marked it active for the next round, whose launch boundary makes the new word visible.
//
// No grid-wide barrier, no wait on another workgroup; every device loop has a compile-time bound.

// the LDS of travel_tile_relax; a kernel with a sweep of its own uses the two flags
struct TravelTileLds {
    unsigned long long state[kTravelHalo * kTravelHalo];
    uint8_t pass[kTravelHalo * kTravelHalo];
    unsigned active, dirty;
};

// Takes the workgroup's mark of this round, cur[blockIdx.x], and clears the dirty bits: false = the work item is not active and the
// workgroup returns.  Every thread calls it.
__device__ __forceinline__ bool travel_take_mark(unsigned* __restrict__ cur, unsigned* s_active, unsigned* s_dirty) {
    if (threadIdx.x == 0) {
        *s_active = cur[blockIdx.x];
        *s_dirty = 0u;
        if (*s_active) cur[blockIdx.x] = 0u;          // this buffer takes the marks of the round after the next
    }
    __syncthreads();
    return *s_active != 0u;
}

// After the write-back, every thread: dirty = the OR of travel_halo_readers over the thread's changed cells.  Wakes the neighbour
// tile in every direction whose bit some thread set, and the workgroup itself when `more` (the sweep cap: go on in the next round).
// base: the index of the marks of tile (0, 0), 0 but in the batch, where a field's marks are bounds-checked before they are offset.
__device__ __forceinline__ void travel_wake(unsigned dirty, bool more, unsigned* s_dirty, int tile_r, int tile_c, int th, int tw, int base,
                                            unsigned* __restrict__ next, unsigned* __restrict__ activated) {
    if (dirty) atomicOr(s_dirty, dirty);
    __syncthreads();
    if (threadIdx.x < 8) {
        const int k = threadIdx.x;
        const int ur = tile_r + travel_dr(k), uc = tile_c + travel_dc(k);
        if ((*s_dirty >> k & 1u) && ur >= 0 && ur < th && uc >= 0 && uc < tw) travel_mark(next, base + ur * tw + uc, activated);
    } else if (threadIdx.x == 8 && more) {
        travel_mark(next, (int)blockIdx.x, activated);
    }
}

// The halo load, the legal masks, the sweeps, the write-back and the wake-up of the active tile (tile_r, tile_c) of one H x W
// field, state word `state`; the workgroup has taken its mark.  PRICED: a step costs the price of the cell it enters, cost_u8 with
// rows of ld_cost cells, held in registers (candidate = neighbour + price * step); otherwise 1, and cost_u8 (nullptr) is not looked
// at.  SOURCE_IS_ZERO: `pass` holds the free bit only and a cell is a source exactly when its word is (0, 0) at load time; otherwise
// `pass` holds both bits.  base: travel_wake's.
template <bool PRICED, bool SOURCE_IS_ZERO>
__device__ __forceinline__ void travel_tile_relax(TravelTileLds& lds, const uint8_t* __restrict__ pass, const uint8_t* __restrict__ cost_u8,
                                                  int64_t ld_cost, unsigned long long* state, int H, int W, int tile_r, int tile_c, int base,
                                                  unsigned* __restrict__ next, unsigned* __restrict__ activated) {
    const int r0 = tile_r * kTravelTile - 1, c0 = tile_c * kTravelTile - 1;    // the halo's origin
#pragma unroll
    for (int k = 0; k < (kTravelHalo * kTravelHalo + kTravelThreads - 1) / kTravelThreads; ++k) {
        const int i = k * kTravelThreads + threadIdx.x;
        if (i < kTravelHalo * kTravelHalo) {
            const int r = r0 + i / kTravelHalo, c = c0 + i % kTravelHalo;
            const bool in = r >= 0 && r < H && c >= 0 && c < W;
            const unsigned long long s = in ? travel_load(&state[(int64_t)r * W + c]) : kTravelUnreached;
            lds.state[i] = s;
            if (SOURCE_IS_ZERO) lds.pass[i] = in ? (uint8_t)(pass[(int64_t)r * W + c] | (s == 0ull ? kTravelSource : 0)) : (uint8_t)0;
            else lds.pass[i] = in ? pass[(int64_t)r * W + c] : (uint8_t)0;
        }
    }
    __syncthreads();
    const int tx = threadIdx.x % kTravelTile, ty = threadIdx.x / kTravelTile;
    unsigned long long first[kTravelCells], mine[kTravelCells];
    unsigned long long price[kTravelCells];           // PRICED: the price of entering this cell
    unsigned legal[kTravelCells];                     // bit k: the step from the neighbour in direction k to this cell is legal
#pragma unroll
    for (int j = 0; j < kTravelCells; ++j) {
        const int at = (ty + 8 * j + 1) * kTravelHalo + tx + 1;
        first[j] = mine[j] = lds.state[at];
        legal[j] = travel_legal_in<kTravelHalo>(lds.pass, at);
        // a cell with a legal incoming step is passable, so it lies inside the map and its price is 1 .. 255
        if (PRICED) price[j] = legal[j] ? (unsigned long long)cost_u8[(int64_t)(r0 + 1 + ty + 8 * j) * ld_cost + (c0 + 1 + tx)] : 0ull;
    }
    bool more = true;
    for (int sweep = 0; sweep < kTravelSweeps && more; ++sweep) {
        unsigned long long best[kTravelCells];
#pragma unroll
        for (int j = 0; j < kTravelCells; ++j) {
            const int at = (ty + 8 * j + 1) * kTravelHalo + tx + 1;
            unsigned long long b = mine[j];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!(legal[j] >> k & 1u)) continue;
                const unsigned long long s = lds.state[at + travel_dr(k) * kTravelHalo + travel_dc(k)];
                if (s == kTravelUnreached) continue;
                const unsigned long long step = (k & 1) ? kTravelDiagonal : kTravelStraight;
                const unsigned long long cand = s + (PRICED ? price[j] * step : step);
                if (b == kTravelUnreached || travel_less(cand, b)) b = cand;      // the first smaller candidate wins
            }
            best[j] = b;
        }
        __syncthreads();                               // every read of this sweep is done
        int changed = 0;
#pragma unroll
        for (int j = 0; j < kTravelCells; ++j) {
            if (best[j] != mine[j]) {
                mine[j] = best[j];
                lds.state[(ty + 8 * j + 1) * kTravelHalo + tx + 1] = best[j];
                changed = 1;
            }
        }
        more = __syncthreads_or(changed) != 0;
    }
    // write back; bit k of dirty: the neighbour tile in direction k reads a changed cell as halo
    unsigned dirty = 0;
#pragma unroll
    for (int j = 0; j < kTravelCells; ++j) {
        if (mine[j] == first[j]) continue;
        const int lr = ty + 8 * j, lc = tx;
        travel_store(&state[(int64_t)(r0 + 1 + lr) * W + (c0 + 1 + lc)], mine[j]);     // changed cells lie inside the map
        dirty |= travel_halo_readers<kTravelTile>(lr, lc);
    }
    travel_wake(dirty, more, &lds.dirty, tile_r, tile_c, travel_tiles(H), travel_tiles(W), base, next, activated);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The single field's workspace and its last kernel, defined in avl_travel.hip; avl_costfield2d runs on the same.

int travel_check_shape(const char* what, int H, int W);      // "bad shape" unless 1 <= H, W <= kTravelMaxSide

struct TravelLayout {
    size_t hdr, flags, pass, state, total;
};
TravelLayout travel_layout(int H, int W);

// queues travel_unpack_kernel: the two int32 planes of n state words and d_stats = [rounds, tile runs, reached, any source]
int travel_unpack(const unsigned long long* state, int64_t n, int32_t* d_straight, int32_t* d_diagonal, int64_t rounds, int64_t tile_runs,
                  bool any_source, int64_t* d_stats, hipStream_t st);

// Launches rounds in batches of kTravelRoundBatch and reads the header after each batch: launch(k, cur, next, activated) queues
// round k.  flags: two mark buffers of `tiles` words, hdr: the header.  Stops when the last round of a batch activated no tile
// (rounds after an empty round find no active tile and return at once).  *rounds: the rounds that had an active tile, *tile_runs:
// the tiles that ran; host: kTravelHdrWords words, the header as last read.  AVL_ERR_STATE when max_rounds rounds did not converge.
template <typename Launch>
static int travel_run_rounds(const char* who, int64_t max_rounds, unsigned* hdr, unsigned* flags, unsigned tiles, hipStream_t st, Launch launch,
                             int64_t* rounds, int64_t* tile_runs, unsigned* host) {
    int64_t k = 0;
    unsigned carry = 0;                                 // tiles active in the first round of the batch
    bool first_batch = true, converged = false;
    *rounds = *tile_runs = 0;
    while (k < max_rounds && !converged) {
        const int64_t k0 = k, k1 = std::min<int64_t>(k + kTravelRoundBatch, max_rounds);
        if (!first_batch) AVL_HIP_CHECK(hipMemsetAsync(hdr + kTravelHdrRound, 0, kTravelRoundBatch * sizeof(unsigned), st));
        for (; k < k1; ++k) {
            unsigned* cur = flags + (size_t)(k & 1) * tiles;
            unsigned* next = flags + (size_t)((k + 1) & 1) * tiles;
            launch(k, cur, next, hdr + kTravelHdrRound + (int)(k - k0));
        }
        AVL_HIP_CHECK(hipGetLastError());
        AVL_HIP_CHECK(hipMemcpyAsync(host, hdr, kTravelHdrWords * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        AVL_HIP_CHECK(hipStreamSynchronize(st));
        if (first_batch) {
            carry = host[kTravelHdrInit];
            first_batch = false;
        }
        for (int64_t j = 0; j < k1 - k0; ++j) {
            *rounds += carry != 0;
            *tile_runs += carry;
            carry = host[kTravelHdrRound + j];
        }
        converged = carry == 0;
    }
    if (!converged) {
        set_error("%s: did not converge in %lld rounds", who, (long long)max_rounds);
        return AVL_ERR_STATE;
    }
    return AVL_OK;
}

}  // namespace avl
