// Rooms and doorways on the free space of a 2-D obstacle map for gfx950: label growth along the travel field (a geodesic Voronoi
// partition with exact ties), the seeds of the morphological room segmentation, the room and door tables and the lift of a label
// image onto voxels.  Upstream has no counterpart (Bormann et al., ICRA 2016 for the segmentation).
//
// Label growth, definition.  free (H, W) uint8, seeds (H, W) int32; a seed is > 0 and is a label, a seed may lie on an obstacle cell.
// (A, B) is the travel field of DESIGN.md 4.26 from the source set seeds > 0: the same legal-step rule and the same pairs
// (avl_travel_tile.h holds the one definition of the rule).  owner[c] = seeds[c] on a source, 0 where the field does not reach, and
// otherwise the smallest label of any source from which a legal walk of exactly the cell's pair ends on c.  Equivalently
//     owner[c] = min over the tight predecessors u of owner[u],
// where u is tight when the step u -> c is legal and (A, B)[u] + step == (A, B)[c].  sqrt(2) is irrational, so "same length" means
// "same pair": no floating point enters.
//
// Two phases, kept apart.  First the distance field runs to convergence through avl_travel2d, unchanged.  Then the label rounds run
// on the fixed field.  A label is NOT packed next to (a, b) and relaxed with it: a halo reader could then pair a new distance with
// an old label, a pair that belongs to no real walk, and monotone relaxation never repairs it (the distance is already final, so
// nothing wakes the cell again).  With the field fixed, the tight predecessors of a cell are a constant 8-bit mask.
//
// The fixed point is unique.  A tight step strictly increases the length a + b sqrt(2), so the tight predecessors form a DAG whose
// sources are the seeds.  In a topological order every owner is determined by owners that come earlier: the equation has exactly
// one solution, and by induction along that order it is the minimum label over all tight walks, that is, over all shortest walks.
// Every reached cell that is not a source has a tight predecessor (the field is the Bellman fixed point), so it gets a label.
//
// State.  One aligned 32-bit word per cell, "no label yet" = all ones, the largest unsigned value, so that a sweep is a plain
// unsigned minimum.  Only the workgroup that owns a cell writes it, with single relaxed stores of device scope, and the word only
// decreases.  A neighbour that reads the cell as halo in the same round sees the old or the new word; the old one is a larger label
// or none, both upper bounds of the true owner, and its reader has been marked active for the next round, whose launch boundary
// makes the new word visible.
//
// Work, on the tile scheme of avl_travel_tile.h with a sweep of its own between the shared prologue (travel_take_mark) and epilogue
// (travel_wake): 32 x 32 tiles, 256 threads, 4 cells per thread.  An active tile loads a one-cell
// halo of the converged 64-bit state, the pass byte and the owner word into LDS, computes ONCE per tile run the mask of tight legal
// predecessors of each of its cells (registers), and sweeps: a minimum over at most 8 LDS words, a barrier, the writes of what got
// smaller, a barrier that ORs "something changed".  It writes back only the cells that changed, wakes the neighbours that see a
// changed halo cell and wakes itself at the sweep cap.  Initially the tiles of the seeds and their 8 neighbours are active.
//
// Convergence.  Every stored word is a seed's label on a source, or a copy of a tight predecessor's stored word: the label of a
// source with a tight walk to the cell, never below the owner.  Words only decrease, and a changed word wakes every tile that can
// read it, so when no tile is active every cell equals the minimum over its tight predecessors: the unique fixed point above,
// whatever order the tiles ran in.  The owner of a cell whose tight walk has k steps is in place after at most k rounds; the host
// gives up after H * W + 1 rounds, which cannot happen unless the device misbehaves.
//
// No grid-wide barrier, no wait on another workgroup; every device loop has a compile-time bound or is a grid-stride loop.
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_common.h"
#include "avl_scan.h"
#include "avl_sort.h"
#include "avl_travel_tile.h"
#include "avl_wave.h"

namespace avl {

constexpr unsigned kGrowNone = ~0u;              // no label yet
constexpr int kGrowHdrNegative = 2;              // header word: a negative seed was seen

constexpr int kRoomSeg = 32;                     // consecutive cells of a row per thread in the table passes
constexpr int kRoomCols = 10;
constexpr int kRoomMaxRooms = 1 << 24;
constexpr int kDoorAcc = 7;                      // contacts, rmin, rmax, cmin, cmax, max E bits, min raster index
constexpr int kDoorProbes = 4096;                // probe cap of the pair table
constexpr unsigned long long kDoorEmpty = ~0ull;
constexpr int kSeedScanThreads = 256, kSeedScanPer = 4;

__device__ __forceinline__ unsigned grow_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void grow_store(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the travel sources of a seed image: mask = seed > 0; a negative seed is reported in the header
__global__ __launch_bounds__(256) void grow_mask_kernel(const int32_t* __restrict__ seeds, int64_t ld_seeds, int H, int W,
                                                        uint8_t* __restrict__ mask, unsigned* __restrict__ hdr) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
        const int32_t s = seeds[(int64_t)r * ld_seeds + c];
        mask[i] = s > 0;
        if (s < 0 && hdr[kGrowHdrNegative] == 0u) atomicExch(&hdr[kGrowHdrNegative], 1u);
    }
}

// pass, the packed converged state and the owner words; the tiles of the seeds and their eight neighbours start active
__global__ __launch_bounds__(256) void grow_init_kernel(const uint8_t* __restrict__ free_u8, int64_t ld_free, const int32_t* __restrict__ seeds,
                                                        int64_t ld_seeds, const int32_t* __restrict__ straight,
                                                        const int32_t* __restrict__ diagonal, int H, int W, uint8_t* __restrict__ pass,
                                                        unsigned long long* __restrict__ state, unsigned* __restrict__ owner,
                                                        unsigned* __restrict__ flags, unsigned* __restrict__ hdr) {
    const int tw = travel_tiles(W), th = travel_tiles(H);
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
        const int32_t s = seeds[(int64_t)r * ld_seeds + c];
        const bool fr = free_u8[(int64_t)r * ld_free + c] != 0, sr = s > 0;
        const int32_t a = straight[i], b = diagonal[i];
        pass[i] = (uint8_t)((fr ? kTravelFree : 0) | (sr ? kTravelSource : 0));
        state[i] = a < 0 ? kTravelUnreached : ((unsigned long long)(unsigned)a << 32 | (unsigned)b);
        owner[i] = sr ? (unsigned)s : kGrowNone;
        if (sr) travel_mark_around<kTravelTile>(flags, r, c, th, tw, &hdr[kTravelHdrInit]);
    }
}

// One label round: see the head of the file.  cur / next: the active marks of this round and of the coming one.
__global__ __launch_bounds__(kTravelThreads) void grow_round_kernel(const uint8_t* __restrict__ pass, const unsigned long long* __restrict__ state,
                                                                  unsigned* owner, int H, int W, unsigned* __restrict__ cur,
                                                                  unsigned* __restrict__ next, unsigned* __restrict__ activated) {
    __shared__ unsigned long long s_state[kTravelHalo * kTravelHalo];
    __shared__ unsigned s_owner[kTravelHalo * kTravelHalo];
    __shared__ uint8_t s_pass[kTravelHalo * kTravelHalo];
    __shared__ unsigned s_active, s_dirty;
    if (!travel_take_mark(cur, &s_active, &s_dirty)) return;
    const int tw = travel_tiles(W), th = travel_tiles(H);
    const int tile_r = blockIdx.x / tw, tile_c = blockIdx.x - tile_r * tw;
    const int r0 = tile_r * kTravelTile - 1, c0 = tile_c * kTravelTile - 1;    // the halo's origin
#pragma unroll
    for (int k = 0; k < (kTravelHalo * kTravelHalo + kTravelThreads - 1) / kTravelThreads; ++k) {
        const int i = k * kTravelThreads + threadIdx.x;
        if (i < kTravelHalo * kTravelHalo) {
            const int r = r0 + i / kTravelHalo, c = c0 + i % kTravelHalo;
            const bool in = r >= 0 && r < H && c >= 0 && c < W;
            s_state[i] = in ? state[(int64_t)r * W + c] : kTravelUnreached;
            s_owner[i] = in ? grow_load(&owner[(int64_t)r * W + c]) : kGrowNone;
            s_pass[i] = in ? pass[(int64_t)r * W + c] : (uint8_t)0;
        }
    }
    __syncthreads();
    const int tx = threadIdx.x % kTravelTile, ty = threadIdx.x / kTravelTile;
    unsigned first[kTravelCells], mine[kTravelCells];
    unsigned tight[kTravelCells];                     // bit k: the neighbour in direction k is a tight legal predecessor
#pragma unroll
    for (int j = 0; j < kTravelCells; ++j) {
        const int at = (ty + 8 * j + 1) * kTravelHalo + tx + 1;
        first[j] = mine[j] = s_owner[at];
        const unsigned legal = travel_legal_in<kTravelHalo>(s_pass, at);
        const unsigned long long here = s_state[at];
        unsigned m = 0;
        if (here != kTravelUnreached) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned long long s = s_state[at + travel_dr(k) * kTravelHalo + travel_dc(k)];
                const bool ok = (legal >> k & 1u) && s != kTravelUnreached && s + ((k & 1) ? kTravelDiagonal : kTravelStraight) == here;
                m |= ok ? 1u << k : 0u;
            }
        }
        tight[j] = m;
    }
    bool more = true;
    for (int sweep = 0; sweep < kTravelSweeps && more; ++sweep) {
        unsigned best[kTravelCells];
#pragma unroll
        for (int j = 0; j < kTravelCells; ++j) {
            const int at = (ty + 8 * j + 1) * kTravelHalo + tx + 1;
            unsigned b = mine[j];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (tight[j] >> k & 1u) b = min(b, s_owner[at + travel_dr(k) * kTravelHalo + travel_dc(k)]);
            best[j] = b;
        }
        __syncthreads();                               // every read of this sweep is done
        int changed = 0;
#pragma unroll
        for (int j = 0; j < kTravelCells; ++j) {
            if (best[j] != mine[j]) {
                mine[j] = best[j];
                s_owner[(ty + 8 * j + 1) * kTravelHalo + tx + 1] = best[j];
                changed = 1;
            }
        }
        more = __syncthreads_or(changed) != 0;
    }
    unsigned dirty = 0;
#pragma unroll
    for (int j = 0; j < kTravelCells; ++j) {
        if (mine[j] == first[j]) continue;
        const int lr = ty + 8 * j, lc = tx;
        grow_store(&owner[(int64_t)(r0 + 1 + lr) * W + (c0 + 1 + lc)], mine[j]);       // changed cells lie inside the map
        dirty |= travel_halo_readers<kTravelTile>(lr, lc);
    }
    travel_wake(dirty, more, &s_dirty, tile_r, tile_c, th, tw, 0, next, activated);
}

// the int32 owner plane (no label -> 0) and the label phase's counters into stats[4 .. 7]
__global__ __launch_bounds__(256) void grow_finish_kernel(const unsigned* __restrict__ owner, int64_t n, int32_t* __restrict__ out,
                                                          long long rounds, long long tile_runs, int negative, long long* __restrict__ stats) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned o = owner[i];
        out[i] = o == kGrowNone ? 0 : (int32_t)o;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[4] = rounds;
        stats[5] = tile_runs;
        stats[6] = negative;
        stats[7] = 0;
    }
}

struct GrowLayout {
    size_t hdr, flags, pass, state, owner, mask, travel, travel_bytes, total;
};

static GrowLayout grow_layout(int H, int W) {
    const size_t tiles = (size_t)travel_tiles(H) * (size_t)travel_tiles(W);
    Carver c;
    GrowLayout l;
    l.hdr = c.take(kTravelHdrWords * sizeof(unsigned));
    l.flags = c.take(2 * tiles * sizeof(unsigned));
    l.pass = c.take((size_t)H * W);
    l.state = c.take((size_t)H * W * sizeof(unsigned long long));
    l.owner = c.take((size_t)H * W * sizeof(unsigned));
    l.mask = c.take((size_t)H * W);
    l.travel_bytes = travel_layout(H, W).total;       // phase 1 runs avl_travel2d on a workspace of its own
    l.travel = c.take(l.travel_bytes);
    l.total = c.total() + 256;                        // the entry point aligns the base itself
    return l;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// seeds of the room segmentation: core = E > radius, its islands, the small ones dropped and the rest renumbered in their old order

__global__ __launch_bounds__(256) void seed_core_kernel(const double* __restrict__ E, int64_t n, double radius, uint8_t* __restrict__ core) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) core[i] = E[i] > radius;
}

// a thread owns kRoomSeg consecutive cells of one row and adds a run of equal labels with one atomic
__global__ __launch_bounds__(256) void seed_sizes_kernel(const int32_t* __restrict__ labels, int H, int W, int n, int* __restrict__ sizes) {
    const int spr = (W + kRoomSeg - 1) / kRoomSeg;
    const int64_t segs = (int64_t)H * spr;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < segs; s += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(s / spr), c0 = (int)(s - (int64_t)r * spr) * kRoomSeg;
        int cur = 0, run = 0;
#pragma unroll 4
        for (int k = 0; k < kRoomSeg; ++k) {
            const int c = c0 + k;
            const int lab = c < W ? labels[(int64_t)r * W + c] : 0;
            if (lab != cur) {
                if (cur > 0 && cur <= n) atomicAdd(&sizes[cur - 1], run);
                cur = lab;
                run = 0;
            }
            ++run;
        }
        if (cur > 0 && cur <= n) atomicAdd(&sizes[cur - 1], run);
    }
}

struct SeedKept {
    const int* sizes;
    long long least;
    __device__ __forceinline__ bool operator()(int64_t i) const { return (long long)sizes[i] >= least; }
};

__global__ __launch_bounds__(256) void seed_relabel_kernel(int32_t* __restrict__ labels, int64_t cells, int n, const int* __restrict__ renumber) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
        const int lab = labels[i];
        labels[i] = lab > 0 && lab <= n ? renumber[lab - 1] : 0;
    }
}

struct SeedWork {
    size_t isl_bytes, total;
    int max_n, nblocks;
    uint8_t* core;
    void* isl;
    int *sizes, *renumber, *counts, *n;
};

static int seed_work(int H, int W, void* ws, SeedWork* w) {
    int rc = avl_label_islands_work_bytes(H, W, &w->isl_bytes);
    if (rc != AVL_OK) return rc;
    w->max_n = ((H + 1) / 2) * ((W + 1) / 2);         // avl_label_islands' bound on the island count
    w->nblocks = (w->max_n + kSeedScanThreads * kSeedScanPer - 1) / (kSeedScanThreads * kSeedScanPer);
    Carver c(ws);
    w->core = c.ptr<uint8_t>((size_t)H * W);
    w->isl = c.ptr<void>(w->isl_bytes);
    w->sizes = c.ptr<int>((size_t)w->max_n * sizeof(int));
    w->renumber = c.ptr<int>((size_t)w->max_n * sizeof(int));
    w->counts = c.ptr<int>((size_t)w->nblocks * sizeof(int));
    w->n = c.ptr<int>(sizeof(int));
    w->total = c.total();
    return AVL_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// room table

__global__ __launch_bounds__(256) void room_table_init_kernel(long long* __restrict__ table, int K) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    long long* row = table + (int64_t)k * kRoomCols;
    row[0] = 0;
    row[1] = LLONG_MAX;
    row[2] = -1;
    row[3] = LLONG_MAX;
    row[4] = -1;
    row[5] = row[6] = row[7] = 0;
    row[8] = -1;                                      // the largest E of the room by bit pattern (E >= 0: the integer order is the float order)
    row[9] = LLONG_MAX;                               // the smallest raster index among the cells with that E
}

// counts, boxes, sums, seed cells and the largest E: a run of equal labels inside a thread's segment costs one set of atomics
__global__ __launch_bounds__(256) void room_table_fill_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ seeds,
                                                              const double* __restrict__ E, int H, int W, int K, long long* __restrict__ table) {
    const int spr = (W + kRoomSeg - 1) / kRoomSeg;
    const int64_t segs = (int64_t)H * spr;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < segs; s += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(s / spr), c0 = (int)(s - (int64_t)r * spr) * kRoomSeg;
        int cur = 0, cmin = 0, cmax = 0;
        long long cnt = 0, csum = 0, nseed = 0, emax = -1;
        for (int k = 0; k <= kRoomSeg; ++k) {
            const int c = c0 + k;
            const bool in = k < kRoomSeg && c < W;
            const int lab = in ? labels[(int64_t)r * W + c] : 0;
            if (lab != cur) {
                if (cur > 0 && cur <= K) {
                    long long* row = table + (int64_t)(cur - 1) * kRoomCols;
                    atomicAdd((unsigned long long*)&row[0], (unsigned long long)cnt);
                    atomicMin(&row[1], (long long)r);
                    atomicMax(&row[2], (long long)r);
                    atomicMin(&row[3], (long long)cmin);
                    atomicMax(&row[4], (long long)cmax);
                    atomicAdd((unsigned long long*)&row[5], (unsigned long long)(cnt * r));
                    atomicAdd((unsigned long long*)&row[6], (unsigned long long)csum);
                    if (nseed) atomicAdd((unsigned long long*)&row[7], (unsigned long long)nseed);
                    atomicMax(&row[8], emax);
                }
                cur = lab;
                cmin = c;
                cnt = csum = nseed = 0;
                emax = -1;
            }
            if (in && lab > 0) {
                ++cnt;
                csum += c;
                cmax = c;
                nseed += seeds[(int64_t)r * W + c] == lab;
                emax = max(emax, (long long)__double_as_longlong(E[(int64_t)r * W + c]));
            }
        }
    }
}

// the smallest raster index among a room's cells with the largest E
__global__ __launch_bounds__(256) void room_table_centre_kernel(const int32_t* __restrict__ labels, const double* __restrict__ E, int64_t cells, int K,
                                                                long long* __restrict__ table) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
        const int lab = labels[i];
        if (lab <= 0 || lab > K) continue;
        long long* row = table + (int64_t)(lab - 1) * kRoomCols;
        if ((long long)__double_as_longlong(E[i]) == row[8] && i < row[9]) atomicMin(&row[9], (long long)i);
    }
}

__global__ __launch_bounds__(256) void room_table_finish_kernel(long long* __restrict__ table, int K, int W) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    long long* row = table + (int64_t)k * kRoomCols;
    if (row[0] == 0) {                                // a label without a cell: an empty box and no centre
        row[1] = row[2] = row[3] = row[4] = row[8] = row[9] = -1;
        return;
    }
    const long long at = row[9];
    row[8] = at / W;
    row[9] = at % W;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// door table: an open-addressing table of the pairs (i < j) that touch, sorted by (i, j) afterwards, so the rows do not depend on
// the order in which the contacts arrived

struct DoorWork {
    int64_t cap;
    unsigned long long *keys, *keys_sorted;
    long long* acc;
    int *slots, *slots_sorted;
    long long* hdr;                                   // [0] pairs, [1] the table overflowed
    size_t total;
};

static DoorWork door_work(int K, void* ws) {
    const long long pairs = (long long)K * (K - 1) / 2;
    long long want = std::max<long long>(64, std::min<long long>(2 * pairs, 16ll * K));
    int64_t cap = 64;
    while (cap < want) cap <<= 1;
    Carver c(ws);
    DoorWork w;
    w.cap = cap;
    w.hdr = c.ptr<long long>(2 * sizeof(long long));
    w.keys = c.ptr<unsigned long long>((size_t)cap * sizeof(unsigned long long));
    w.keys_sorted = c.ptr<unsigned long long>((size_t)cap * sizeof(unsigned long long));
    w.acc = c.ptr<long long>((size_t)cap * kDoorAcc * sizeof(long long));
    w.slots = c.ptr<int>((size_t)cap * sizeof(int));
    w.slots_sorted = c.ptr<int>((size_t)cap * sizeof(int));
    w.total = c.total() + 256;
    return w;
}

__global__ __launch_bounds__(256) void door_init_kernel(unsigned long long* __restrict__ keys, long long* __restrict__ acc, int* __restrict__ slots,
                                                        int64_t cap) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = kDoorEmpty;
        slots[i] = (int)i;
        long long* a = acc + i * kDoorAcc;
        a[0] = 0;
        a[1] = LLONG_MAX;
        a[2] = -1;
        a[3] = LLONG_MAX;
        a[4] = -1;
        a[5] = -1;
        a[6] = LLONG_MAX;
    }
}

__device__ __forceinline__ int64_t door_hash(unsigned long long key, int64_t cap) {
    key ^= key >> 33;
    key *= 0xff51afd7ed558ccdull;
    key ^= key >> 33;
    return (int64_t)(key & (unsigned long long)(cap - 1));
}

// the slot of `key`, claimed when INSERT and not there yet; -1 after kDoorProbes probes without finding it
template <bool INSERT>
__device__ __forceinline__ int64_t door_slot(unsigned long long* keys, int64_t cap, unsigned long long key, long long* hdr) {
    int64_t h = door_hash(key, cap);
    for (int p = 0; p < kDoorProbes; ++p) {
        unsigned long long seen = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == key) return h;
        if (seen == kDoorEmpty) {
            if (!INSERT) return -1;
            seen = atomicCAS(&keys[h], kDoorEmpty, key);
            if (seen == kDoorEmpty) {
                atomicAdd((unsigned long long*)&hdr[0], 1ull);
                return h;
            }
            if (seen == key) return h;
        }
        h = (h + 1) & (cap - 1);
    }
    return -1;
}

// FIRST: contacts, the box and the largest E of every pair.  Second pass (!FIRST): the smallest raster index with that E.
template <bool FIRST>
__global__ __launch_bounds__(256) void door_contacts_kernel(const int32_t* __restrict__ labels, const double* __restrict__ E, int H, int W, int K,
                                                            unsigned long long* keys, long long* __restrict__ acc, int64_t cap,
                                                            long long* __restrict__ hdr) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int lu = labels[i];
        if (lu <= 0 || lu > K) continue;
        const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
#pragma unroll
        for (int d = 0; d < 2; ++d) {                  // v right of u, v below u
            const int vr = r + d, vc = c + 1 - d;
            if (vr >= H || vc >= W) continue;
            const int64_t iv = (int64_t)vr * W + vc;
            const int lv = labels[iv];
            if (lv <= 0 || lv > K || lv == lu) continue;
            const unsigned long long key = (unsigned long long)(unsigned)min(lu, lv) << 32 | (unsigned)max(lu, lv);
            const int64_t slot = door_slot<FIRST>(keys, cap, key, hdr);
            if (slot < 0) {
                if (FIRST) atomicExch((unsigned long long*)&hdr[1], 1ull);
                continue;
            }
            long long* a = acc + slot * kDoorAcc;
            const long long eu = __double_as_longlong(E[i]), ev = __double_as_longlong(E[iv]);
            if (FIRST) {
                atomicAdd((unsigned long long*)&a[0], 1ull);
                atomicMin(&a[1], (long long)r);
                atomicMax(&a[2], (long long)vr);
                atomicMin(&a[3], (long long)c);
                atomicMax(&a[4], (long long)vc);
                atomicMax(&a[5], max(eu, ev));
            } else {
                const long long top = a[5];
                if (eu == top) atomicMin(&a[6], (long long)i);
                else if (ev == top) atomicMin(&a[6], (long long)iv);      // i < iv: u wins a tie between the two
            }
        }
    }
}

__global__ __launch_bounds__(256) void door_rows_kernel(const unsigned long long* __restrict__ keys_sorted, const int* __restrict__ slots_sorted,
                                                        const long long* __restrict__ acc, int64_t D, int W, long long* __restrict__ table) {
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < D; d += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = keys_sorted[d];
        const long long* a = acc + (int64_t)slots_sorted[d] * kDoorAcc;
        long long* row = table + d * kRoomCols;
        row[0] = (long long)(key >> 32);
        row[1] = (long long)(key & 0xffffffffull);
        row[2] = a[0];
        row[3] = a[1];
        row[4] = a[2];
        row[5] = a[3];
        row[6] = a[4];
        row[7] = a[6] / W;
        row[8] = a[6] % W;
        row[9] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void lift_labels_kernel(const int32_t* __restrict__ labels, int H, int W, const int32_t* __restrict__ grid_pos,
                                                          int64_t N, int rmin, int cmin, int32_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const long long r = (long long)grid_pos[3 * i] - rmin, c = (long long)grid_pos[3 * i + 1] - cmin;
        out[i] = r >= 0 && r < H && c >= 0 && c < W ? labels[r * W + c] : 0;
    }
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_grow_labels_workspace_bytes(int H, int W, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_grow_labels_workspace_bytes: null output");
    int rc = travel_check_shape("avl_grow_labels_workspace_bytes", H, W);
    if (rc != AVL_OK) return rc;
    *bytes = grow_layout(H, W).total;
    return AVL_OK;
}

int avl_grow_labels(const uint8_t* d_free, int64_t ld_free, const int32_t* d_seeds, int64_t ld_seeds, int H, int W, int32_t* d_straight,
                    int32_t* d_diagonal, int32_t* d_owner, int64_t* d_stats, void* ws, size_t ws_bytes, void* stream) {
    int rc = travel_check_shape("avl_grow_labels", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_free && d_seeds, "avl_grow_labels: null free or seed image");
    AVL_REQUIRE(d_straight && d_diagonal && d_owner && d_stats, "avl_grow_labels: null output plane or stats pointer");
    AVL_REQUIRE(ld_free >= W, "avl_grow_labels: free rows of %lld cells cannot hold %d columns", (long long)ld_free, W);
    AVL_REQUIRE(ld_seeds >= W, "avl_grow_labels: seed rows of %lld cells cannot hold %d columns", (long long)ld_seeds, W);
    const GrowLayout l = grow_layout(H, W);
    AVL_REQUIRE(ws && ws_bytes >= l.total, "avl_grow_labels: workspace of %zu bytes, need %zu", ws_bytes, l.total);
    hipStream_t st = as_stream(stream);
    char* base = (char*)align256_ptr(ws);
    unsigned* hdr = (unsigned*)(base + l.hdr);
    unsigned* flags = (unsigned*)(base + l.flags);
    uint8_t* pass = (uint8_t*)(base + l.pass);
    unsigned long long* state = (unsigned long long*)(base + l.state);
    unsigned* owner = (unsigned*)(base + l.owner);
    uint8_t* mask = (uint8_t*)(base + l.mask);
    const unsigned tiles = (unsigned)(travel_tiles(W) * travel_tiles(H));
    const int64_t n = (int64_t)H * W;

    AVL_HIP_CHECK(hipMemsetAsync(hdr, 0, l.pass - l.hdr, st));              // the header and both mark buffers
    hipLaunchKernelGGL(grow_mask_kernel, dim3(stride_blocks(n)), dim3(256), 0, st, d_seeds, ld_seeds, H, W, mask, hdr);
    AVL_HIP_CHECK(hipGetLastError());
    // phase 1: the distance field, to convergence (stats[0 .. 3])
    rc = avl_travel2d(d_free, ld_free, mask, W, H, W, d_straight, d_diagonal, d_stats, base + l.travel, l.travel_bytes, stream);
    if (rc != AVL_OK) return rc;
    // phase 2: the labels on the fixed field
    hipLaunchKernelGGL(grow_init_kernel, dim3(stride_blocks(n)), dim3(256), 0, st, d_free, ld_free, d_seeds, ld_seeds, (const int32_t*)d_straight,
                       (const int32_t*)d_diagonal, H, W, pass, state, owner, flags, hdr);
    AVL_HIP_CHECK(hipGetLastError());
    int64_t rounds = 0, tile_runs = 0;
    unsigned host[kTravelHdrWords];
    rc = travel_run_rounds(
        "avl_grow_labels", n + 1, hdr, flags, tiles, st,
        [&](int64_t, unsigned* cur, unsigned* next, unsigned* activated) {
            hipLaunchKernelGGL(grow_round_kernel, dim3(tiles), dim3(kTravelThreads), 0, st, (const uint8_t*)pass, (const unsigned long long*)state, owner,
                               H, W, cur, next, activated);
        },
        &rounds, &tile_runs, host);
    if (rc != AVL_OK) return rc;
    hipLaunchKernelGGL(grow_finish_kernel, dim3(stride_blocks(n)), dim3(256), 0, st, (const unsigned*)owner, n, d_owner, (long long)rounds,
                       (long long)tile_runs, (int)(host[kGrowHdrNegative] != 0), reinterpret_cast<long long*>(d_stats));
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_room_seeds_workspace_bytes(int H, int W, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_room_seeds_workspace_bytes: null output");
    int rc = travel_check_shape("avl_room_seeds_workspace_bytes", H, W);
    if (rc != AVL_OK) return rc;
    SeedWork w;
    rc = seed_work(H, W, nullptr, &w);
    if (rc != AVL_OK) return rc;
    *bytes = w.total + 256;
    return AVL_OK;
}

int avl_room_seeds(const double* d_clearance, int H, int W, double radius, int64_t min_seed_cells, int32_t* d_seeds, int32_t* d_k, void* ws,
                   size_t ws_bytes, void* stream) {
    int rc = travel_check_shape("avl_room_seeds", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_clearance && d_seeds && d_k, "avl_room_seeds: null clearance, seed or count pointer");
    AVL_REQUIRE(std::isfinite(radius) && radius >= 0.0, "avl_room_seeds: radius must be finite and >= 0");
    AVL_REQUIRE(min_seed_cells >= 1, "avl_room_seeds: min_seed_cells must be >= 1, got %lld", (long long)min_seed_cells);
    SeedWork w;
    rc = seed_work(H, W, ws ? align256_ptr(ws) : nullptr, &w);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(ws && ws_bytes >= w.total + 256, "avl_room_seeds: workspace of %zu bytes, need %zu", ws_bytes, w.total + 256);
    hipStream_t st = as_stream(stream);
    const int64_t cells = (int64_t)H * W;
    const unsigned sb = stride_blocks(cells);
    hipLaunchKernelGGL(seed_core_kernel, dim3(sb), dim3(256), 0, st, d_clearance, cells, radius, w.core);
    AVL_HIP_CHECK(hipGetLastError());
    rc = avl_label_islands(w.core, W, H, W, d_seeds, w.n, w.isl, w.isl_bytes, stream);
    if (rc != AVL_OK) return rc;
    int n = 0;
    AVL_HIP_CHECK(hipMemcpyAsync(&n, w.n, sizeof(int), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    AVL_HIP_CHECK(hipMemsetAsync(d_k, 0, sizeof(int32_t), st));
    if (n <= 0) return AVL_OK;                         // no core: the label image is all zero already
    if (n > w.max_n) {
        set_error("avl_room_seeds: %d islands in a %d x %d image", n, H, W);
        return AVL_ERR_STATE;
    }
    AVL_HIP_CHECK(hipMemsetAsync(w.sizes, 0, (size_t)n * sizeof(int), st));
    AVL_HIP_CHECK(hipMemsetAsync(w.renumber, 0, (size_t)n * sizeof(int), st));
    const int64_t segs = (int64_t)H * ((W + kRoomSeg - 1) / kRoomSeg);
    hipLaunchKernelGGL(seed_sizes_kernel, dim3(stride_blocks(segs)), dim3(256), 0, st, (const int32_t*)d_seeds, H, W, n, w.sizes);
    const int nblocks = (n + kSeedScanThreads * kSeedScanPer - 1) / (kSeedScanThreads * kSeedScanPer);
    const dim3 scan_n((unsigned)nblocks), scan_t(kSeedScanThreads);
    const SeedKept kept{w.sizes, (long long)min_seed_cells};
    hipLaunchKernelGGL((count_flagged_kernel<kSeedScanThreads, kSeedScanPer, SeedKept>), scan_n, scan_t, 0, st, (int64_t)n, kept, w.counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)w.counts, (int64_t)nblocks, w.counts,
                       (int*)d_k, OpSum{}, 0);
    hipLaunchKernelGGL((number_flagged_kernel<kSeedScanThreads, kSeedScanPer, SeedKept>), scan_n, scan_t, 0, st, (int64_t)n, kept,
                       (const int*)w.counts, w.renumber);
    hipLaunchKernelGGL(seed_relabel_kernel, dim3(sb), dim3(256), 0, st, d_seeds, cells, n, (const int*)w.renumber);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_room_table(const int32_t* d_labels, const int32_t* d_seeds, const double* d_clearance, int H, int W, int32_t K, int64_t* d_table,
                   void* stream) {
    int rc = travel_check_shape("avl_room_table", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(K >= 0 && K <= kRoomMaxRooms, "avl_room_table: %d rooms (0 .. %d)", K, kRoomMaxRooms);
    if (K == 0) return AVL_OK;
    AVL_REQUIRE(d_labels && d_seeds && d_clearance && d_table, "avl_room_table: null label, seed, clearance or table pointer");
    hipStream_t st = as_stream(stream);
    const int64_t cells = (int64_t)H * W, segs = (int64_t)H * ((W + kRoomSeg - 1) / kRoomSeg);
    const dim3 rows((unsigned)((K + 255) / 256));
    long long* table = reinterpret_cast<long long*>(d_table);
    hipLaunchKernelGGL(room_table_init_kernel, rows, dim3(256), 0, st, table, K);
    hipLaunchKernelGGL(room_table_fill_kernel, dim3(stride_blocks(segs)), dim3(256), 0, st, d_labels, d_seeds, d_clearance, H, W, K, table);
    hipLaunchKernelGGL(room_table_centre_kernel, dim3(stride_blocks(cells)), dim3(256), 0, st, d_labels, d_clearance, cells, K, table);
    hipLaunchKernelGGL(room_table_finish_kernel, rows, dim3(256), 0, st, table, K, W);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_room_doors_workspace_bytes(int32_t K, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_room_doors_workspace_bytes: null output");
    AVL_REQUIRE(K >= 0 && K <= kRoomMaxRooms, "avl_room_doors_workspace_bytes: %d rooms (0 .. %d)", K, kRoomMaxRooms);
    *bytes = door_work(K, nullptr).total;
    return AVL_OK;
}

int avl_room_doors(const int32_t* d_labels, const double* d_clearance, int H, int W, int32_t K, int64_t* d_count, void* ws, size_t ws_bytes,
                   void* stream) {
    int rc = travel_check_shape("avl_room_doors", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(K >= 0 && K <= kRoomMaxRooms, "avl_room_doors: %d rooms (0 .. %d)", K, kRoomMaxRooms);
    AVL_REQUIRE(d_labels && d_clearance && d_count, "avl_room_doors: null label, clearance or count pointer");
    const DoorWork w = door_work(K, ws ? align256_ptr(ws) : nullptr);
    AVL_REQUIRE(ws && ws_bytes >= w.total, "avl_room_doors: workspace of %zu bytes, need %zu", ws_bytes, w.total);
    hipStream_t st = as_stream(stream);
    const int64_t cells = (int64_t)H * W;
    AVL_HIP_CHECK(hipMemsetAsync(w.hdr, 0, 2 * sizeof(long long), st));
    hipLaunchKernelGGL(door_init_kernel, dim3(stride_blocks(w.cap)), dim3(256), 0, st, w.keys, w.acc, w.slots, w.cap);
    hipLaunchKernelGGL(door_contacts_kernel<true>, dim3(stride_blocks(cells)), dim3(256), 0, st, d_labels, d_clearance, H, W, K, w.keys, w.acc, w.cap,
                       w.hdr);
    hipLaunchKernelGGL(door_contacts_kernel<false>, dim3(stride_blocks(cells)), dim3(256), 0, st, d_labels, d_clearance, H, W, K, w.keys, w.acc, w.cap,
                       w.hdr);
    AVL_HIP_CHECK(hipGetLastError());
    rc = sort_pairs_pooled("avl_room_doors", w.keys, w.keys_sorted, w.slots, w.slots_sorted, w.cap, 64, st);      // empty slots sort last
    if (rc != AVL_OK) return rc;
    AVL_HIP_CHECK(hipMemcpyAsync(d_count, w.hdr, 2 * sizeof(long long), hipMemcpyDeviceToDevice, st));
    return AVL_OK;
}

int avl_room_door_table(const void* ws, size_t ws_bytes, int32_t K, int W, int64_t D, int64_t* d_table, void* stream) {
    AVL_REQUIRE(K >= 0 && K <= kRoomMaxRooms, "avl_room_door_table: %d rooms (0 .. %d)", K, kRoomMaxRooms);
    AVL_REQUIRE(W > 0 && W <= kTravelMaxSide, "avl_room_door_table: bad width %d", W);
    const DoorWork w = door_work(K, ws ? align256_ptr(const_cast<void*>(ws)) : nullptr);
    AVL_REQUIRE(D >= 0 && D <= w.cap, "avl_room_door_table: %lld pairs, the table of %d rooms holds %lld", (long long)D, K, (long long)w.cap);
    if (D == 0) return AVL_OK;
    AVL_REQUIRE(ws && ws_bytes >= w.total, "avl_room_door_table: workspace of %zu bytes, need %zu", ws_bytes, w.total);
    AVL_REQUIRE(d_table, "avl_room_door_table: null table pointer");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(door_rows_kernel, dim3(stride_blocks(D)), dim3(256), 0, st, (const unsigned long long*)w.keys_sorted, (const int*)w.slots_sorted,
                       (const long long*)w.acc, D, W, reinterpret_cast<long long*>(d_table));
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_lift_labels_2d(const int32_t* d_labels, int H, int W, const int32_t* d_grid_pos, int64_t N, int rmin, int cmin, int32_t* d_out,
                       void* stream) {
    int rc = travel_check_shape("avl_lift_labels_2d", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(N >= 0, "avl_lift_labels_2d: negative voxel count %lld", (long long)N);
    if (N == 0) return AVL_OK;
    AVL_REQUIRE(d_labels && d_grid_pos && d_out, "avl_lift_labels_2d: null label, position or output pointer");
    hipLaunchKernelGGL(lift_labels_kernel, dim3(stride_blocks(N)), dim3(256), 0, as_stream(stream), d_labels, H, W, d_grid_pos, N, rmin, cmin, d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
