// What the travel-distance field (avl_travel.hip), the label growth on it (avl_rooms.hip) and the batch of K fields
// (avl_travel_many.hip) share: the packed state word and the exact order of two of them, the single-word loads and stores, the
// passability bits, the active marks, the legal-step rule and the host loop that launches rounds in batches until one activates no
// tile.  One definition of each, so that the kernel families cannot drift apart.  The tile
// geometry (side, threads, sweep cap) belongs to each family's source; the helpers here take the side as a template argument.
#pragma once
#include <algorithm>

#include "avl_common.h"

namespace avl {

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

// a1 + b1 sqrt(2) < a2 + b2 sqrt(2) for two reached words, exactly
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
