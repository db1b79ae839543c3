// The relations between the objects of a voxel map for gfx950: for every pair of objects that come within R cells of each other,
// how far apart they are, where the gap is, who rests on whom and how much they touch.  One neighbourhood pass over the voxel list,
// its per-voxel object labels (avl_objects.hip's avl_label_classes, or any labels 1 .. n) and the cell index of avl_cellindex.h.
//
// Upstream has no counterpart.  Its nearest lines are the 2-D island helpers of avlmaps/map/map.py:183-240 (get_nearest_pos and
// friends), which work on ONE category's pooled top-down mask and cannot tell a mug on the table from a mug under it.  Everything
// below is this project's own definition, written out in DESIGN.md 4.25; every output is an integer minimum or an integer count,
// so a brute-force restatement (tests/_scene_graph_ref.py) is compared with np.array_equal.
//
// THE SCAN.  Every voxel row i whose label a lies in 1 .. n and whose cell lies inside the grid scans every offset
// d = (dr, dc, dh) with dr^2 + dc^2 + dh^2 <= R^2, d = 0 included, 1 <= R <= 15.  An offset whose cell cell(i) + d lies outside
// the grid is skipped, per component (the linear cell of (r, c, vh) is the bottom of the NEXT column).  With j the owner of that
// cell in the index (the largest row of the cell; none: no event) and b = labels[j]: when b lies in 1 .. n and b != a, the
// unordered pair (min(a, b), max(a, b)) exists and the EVENT (i, d, j) belongs to it.  A pair collects
//   d2        the minimum of |d|^2 over its events
//   i, j      the witness of that minimum: among the events with |d|^2 = d2 the one with the smallest scanning row i, then the
//             smallest offset code ((dr + R)(2R + 1) + (dc + R))(2R + 1) + (dh + R)
//   lo_on_hi  the events with d = (0, 0, -1) whose scanning voxel has the LOWER label: a voxel of the lower-numbered object with
//             a cell of the higher-numbered one directly beneath it (larger h is up)
//   hi_on_lo  the same with the roles exchanged
//   contacts  the events with 0 < |d|^2 <= 3 (the 26-neighbourhood), from either side
// Several rows in one cell make the scan ASYMMETRIC: a row that does not own its cell scans but is never seen.  Two rows of
// different objects in one cell give d2 = 0 (the non-owner sees the owner at d = 0).
//
// THE PASS.  rel_scan_kernel: one lane per voxel, the voxels in the order of their cells (the index's ranks; the kernel says how the
// rows that own no cell come in), the offset loop with dh innermost.  The cells of a column are consecutive bits
// of the index's bitmap, so the <= 31 cells of an offset column are one or two word loads and a shift; prefix, perm and the label
// are read only for set bits.  Pairs live in an open-addressing table of H slots in the workspace, H the power of two
// >= 2 * max_pairs: 64-bit keys lo * (n + 1) + hi claimed with atomicCAS (linear probing); whoever claims an empty slot bumps the
// pair counter.  A lane keeps the slot of the last b it met -- the neighbours along a column are mostly one object -- together
// with that pair's minimum and its two counters in registers, and flushes them when b changes and at the end: the minimum
// d2 << 46 | i << 15 | code (8 + 31 + 15 bits: 225 < 2^8, i < 2^31, 31^3 < 2^15) with ONE 64-bit atomicMin, issued only when a
// plain load says it would lower the slot, the counters with integer atomicAdds when they are not zero.  Integer minima and sums:
// nothing depends on the order in which the atomics land.
// More pairs than max_pairs: the counter passes max_pairs, lanes that see that stop, and a lane that finds the table full gives
// up (then all H >= 2 * max_pairs slots are claimed and counted).  The count is the caller's signal; the table is unspecified.
//
// THE FINISH.  The claimed slots are compacted in slot order (avl_scan.h), sorted by key with rocPRIM's radix sort over
// max_pairs entries (the tail is padded with the all-ones key, larger than any pair's), and rel_rows_kernel unpacks
// [lo, hi, d2, i, j, lo_on_hi, hi_on_lo, contacts]; j is looked up again from i and the offset code.
#include <algorithm>
#include <climits>

#include "avl_cellindex.h"
#include "avl_scan.h"
#include "avl_sort.h"

namespace avl {

constexpr int kRelMaxRadius = 15;
constexpr int64_t kRelMaxPairs = (int64_t)1 << 28;
constexpr int kRelCols = 8;
constexpr int kRelScanThreads = 256;
constexpr int kRelScanPer = 4;
constexpr int kRelScanBlock = kRelScanThreads * kRelScanPer;
constexpr unsigned long long kRelEmpty = ~0ull;

struct RelHeader {
    unsigned int pairs;                                 // claimed slots
    unsigned int pad[63];
};

struct RelParams {
    int gs, vh, R, n;
    int64_t N, nwords, max_pairs;
    unsigned long long H;                               // slots, a power of two
    const uint32_t* bits;
    const int32_t* prefix;
    const int32_t* perm;
    const int32_t* pos;
    const int32_t* labels;
    unsigned long long* keys;
    unsigned long long* mins;
    unsigned long long* counters;                       // (H, 3): lo_on_hi, hi_on_lo, contacts
    RelHeader* header;
};

struct RelClaimed {
    const unsigned long long* keys;
    __device__ __forceinline__ bool operator()(int64_t s) const { return keys[s] != kRelEmpty; }
};

__device__ __forceinline__ unsigned long long rel_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the slot of `key`, claimed when it is new; -1 when every slot is taken by other keys
__device__ __forceinline__ long long rel_slot(const RelParams& p, unsigned long long key) {
    unsigned long long x = key * 0x9E3779B97F4A7C15ull;
    unsigned long long s = (x ^ (x >> 29)) & (p.H - 1);
    for (unsigned long long tries = 0; tries < p.H; ++tries) {
        unsigned long long k = rel_load(&p.keys[s]);
        if (k == kRelEmpty) {
            k = atomicCAS(&p.keys[s], kRelEmpty, key);
            if (k == kRelEmpty) {
                atomicAdd(&p.header->pairs, 1u);
                return (long long)s;
            }
        }
        if (k == key) return (long long)s;
        s = (s + 1) & (p.H - 1);
    }
    return -1;
}

// what a lane has gathered for the pair of its own label and the last other label it met
struct RelPending {
    int b;
    long long slot;
    unsigned long long best;
    unsigned int on, contacts;
};

__device__ __forceinline__ void rel_flush(const RelParams& p, int a, const RelPending& q) {
    if (q.b == 0 || q.slot < 0) return;
    if (q.best < rel_load(&p.mins[q.slot])) atomicMin(&p.mins[q.slot], q.best);
    unsigned long long* c = p.counters + 3 * q.slot;
    if (q.on) atomicAdd(&c[a < q.b ? 0 : 1], (unsigned long long)q.on);
    if (q.contacts) atomicAdd(&c[2], (unsigned long long)q.contacts);
}

// ci_probe for an index that may be foreign: the row that owns the occupied linear cell `lin`, -1 when the cell is empty or the
// index does not answer with a row of the list (no read out of bounds)
__device__ __forceinline__ int rel_owner(const RelParams& p, int lin) {
    const uint32_t word = p.bits[lin >> 5], b = (uint32_t)lin & 31u;
    if (!(word >> b & 1u)) return -1;
    const int64_t rank = (int64_t)p.prefix[lin >> 5] + __popc(word & ((1u << b) - 1u));
    if (rank < 0 || rank >= p.N) return -1;
    const int j = p.perm[rank];
    return j >= 0 && j < p.N ? j : -1;
}

// the largest m >= 0 with m * m <= x, 0 <= x <= 225
__device__ __forceinline__ int rel_isqrt(int x) {
    int m = (int)sqrtf((float)x);
    if (m * m > x) --m;
    if ((m + 1) * (m + 1) <= x) ++m;
    return m;
}

// The lanes take the voxels in the order of their CELLS, so that the lanes of a wave scan neighbouring columns and their word loads
// fall into a few cache lines (the list itself is in any order: a wave of 64 listed rows touches 64 lines per load, measured 2.5 to
// 6.5 times slower).  Items 0 .. N - 1 are the ranks of the index: item t is perm[t], the owner of the t-th occupied cell; ranks at
// or past the number of occupied cells are empty.  Items N .. 2N - 1 are the rows again, of which only those that do NOT own their
// cell scan (the owners were a rank).  Every labelled row inside the grid scans exactly once.
__global__ __launch_bounds__(256) void rel_scan_kernel(RelParams p) {
    const int R = p.R, side = 2 * R + 1;
    const int64_t occupied = (int64_t)p.prefix[p.nwords - 1] + __popc(p.bits[p.nwords - 1]);
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < 2 * p.N; x += (int64_t)gridDim.x * 256) {
        int64_t i = x - p.N;
        if (x < p.N) {
            if (x >= occupied) continue;
            i = p.perm[x];
            if (i < 0 || i >= p.N) continue;                                       // a foreign index: no read out of bounds
        }
        const int a = p.labels[i];
        if (a < 1 || a > p.n) continue;
        const int r = p.pos[3 * i], c = p.pos[3 * i + 1], h = p.pos[3 * i + 2];
        const int64_t own = ci_linear(r, c, h, p.gs, p.vh);
        if (own < 0) continue;
        if ((x >= p.N) == (rel_owner(p, (int)own) == i)) continue;                 // owners scan as ranks, the others as rows
        if ((int64_t)__hip_atomic_load(&p.header->pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p.max_pairs) return;   // too many pairs already
        RelPending q{0, -1, kRelEmpty, 0u, 0u};
        for (int dr = -R; dr <= R; ++dr) {
            const int rr = r + dr;
            if (rr < 0 || rr >= p.gs) continue;
            const int mc = rel_isqrt(R * R - dr * dr);
            for (int dc = -mc; dc <= mc; ++dc) {
                const int cc = c + dc;
                if (cc < 0 || cc >= p.gs) continue;
                const int d2c = dr * dr + dc * dc;
                const int mh = rel_isqrt(R * R - d2c);
                const int h0 = max(h - mh, 0), h1 = min(h + mh, p.vh - 1);       // h0 <= h <= h1: at most 31 cells, inside the column
                const int lin0 = (rr * p.gs + cc) * p.vh + h0;                   // < gs * gs * vh < 2^31
                const int w0 = lin0 >> 5, sh = lin0 & 31;
                unsigned long long window = p.bits[w0];
                if (w0 + 1 < p.nwords) window |= (unsigned long long)p.bits[w0 + 1] << 32;
                window = (window >> sh) & ((1ull << (h1 - h0 + 1)) - 1ull);
                while (window) {
                    const int k = __ffsll((long long)window) - 1;
                    window &= window - 1;
                    const int j = rel_owner(p, lin0 + k);                        // (its word is one of the two above: a cache hit)
                    if (j < 0) continue;
                    const int b = p.labels[j];
                    if (b < 1 || b > p.n || b == a) continue;
                    if (b != q.b) {
                        rel_flush(p, a, q);
                        const unsigned long long lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
                        q = RelPending{b, rel_slot(p, lo * ((unsigned long long)p.n + 1ull) + hi), kRelEmpty, 0u, 0u};
                    }
                    const int dh = h0 + k - h;
                    const int d2 = d2c + dh * dh;
                    const unsigned code = (unsigned)(((dr + R) * side + (dc + R)) * side + (dh + R));
                    const unsigned long long packed = (unsigned long long)d2 << 46 | (unsigned long long)i << 15 | code;
                    q.best = min(q.best, packed);
                    if (d2c == 0 && dh == -1) ++q.on;
                    if (d2 >= 1 && d2 <= 3) ++q.contacts;
                }
            }
        }
        rel_flush(p, a, q);
    }
}

// the claimed slots in slot order: key and slot.  Nothing is written at or past max_pairs
__global__ __launch_bounds__(kRelScanThreads) void rel_compact_kernel(const unsigned long long* __restrict__ keys, int64_t H,
                                                                      const int* __restrict__ offsets, int64_t max_pairs,
                                                                      unsigned long long* __restrict__ out_keys, int* __restrict__ out_slots) {
    __shared__ int s_w[kRelScanThreads / kWave];
    const int64_t base = offsets[blockIdx.x];
    int64_t s0;
    int before, total;
    const int f = block_flags<kRelScanThreads, kRelScanPer>(H, RelClaimed{keys}, s_w, &s0, &before, &total);
    int64_t t = base + before;
#pragma unroll
    for (int k = 0; k < kRelScanPer; ++k) {
        if (!(f >> k & 1) || t < 0 || t >= max_pairs) continue;
        out_keys[t] = keys[s0 + k];
        out_slots[t] = (int)(s0 + k);
        ++t;
    }
}

// row t of the table from the t-th smallest key; the count
__global__ __launch_bounds__(256) void rel_rows_kernel(RelParams p, const unsigned long long* __restrict__ keys, const int* __restrict__ slots,
                                                       int64_t* __restrict__ table, int64_t* __restrict__ count) {
    const int64_t P = p.header->pairs;
    if (blockIdx.x == 0 && threadIdx.x == 0) count[0] = P;
    if (P > p.max_pairs) return;
    const int side = 2 * p.R + 1;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < P; t += (int64_t)gridDim.x * 256) {
        const unsigned long long key = keys[t];
        const int64_t s = slots[t];
        int64_t* row = table + t * kRelCols;
        row[0] = (int64_t)(key / ((unsigned long long)p.n + 1ull));
        row[1] = (int64_t)(key % ((unsigned long long)p.n + 1ull));
        if (s < 0 || (unsigned long long)s >= p.H) {                             // a foreign workspace: no read out of bounds
            for (int k = 2; k < kRelCols; ++k) row[k] = -1;
            continue;
        }
        const unsigned long long best = p.mins[s];
        const int64_t i = (int64_t)(best >> 15 & 0x7fffffffull);
        int code = (int)(best & 0x7fffull);
        const int dh = code % side - p.R;
        code /= side;
        const int dc = code % side - p.R, dr = code / side - p.R;
        int j = -1;
        if (i < p.N) {
            const int64_t lin = ci_linear(p.pos[3 * i] + dr, p.pos[3 * i + 1] + dc, p.pos[3 * i + 2] + dh, p.gs, p.vh);
            if (lin >= 0) j = rel_owner(p, (int)lin);
        }
        row[2] = (int64_t)(best >> 46);
        row[3] = i;
        row[4] = j;
        row[5] = (int64_t)p.counters[3 * s];
        row[6] = (int64_t)p.counters[3 * s + 1];
        row[7] = (int64_t)p.counters[3 * s + 2];
    }
}

// workspace of avl_object_relations: header | keys and minima of the H slots (one memset) | their counters | one count per scan
// block | the claimed keys, sorted | their slots, sorted
struct RelWork {
    int64_t H;
    int nblocks;
    RelHeader* header;
    unsigned long long *keys, *mins, *counters, *keys_in, *keys_out;
    int *counts, *slots_in, *slots_out;
    size_t total;
};
static RelWork rel_work(int64_t max_pairs, void* ws) {
    Carver c(ws);
    RelWork w;
    w.H = 2;
    while (w.H < 2 * max_pairs) w.H <<= 1;
    w.nblocks = (int)((w.H + kRelScanBlock - 1) / kRelScanBlock);
    w.header = c.ptr<RelHeader>(sizeof(RelHeader));
    w.keys = c.ptr<unsigned long long>((size_t)w.H * 8);
    w.mins = c.ptr<unsigned long long>((size_t)w.H * 8);
    w.counters = c.ptr<unsigned long long>((size_t)w.H * 24);
    w.counts = c.ptr<int>((size_t)w.nblocks * 4);
    w.keys_in = c.ptr<unsigned long long>((size_t)max_pairs * 8);
    w.keys_out = c.ptr<unsigned long long>((size_t)max_pairs * 8);
    w.slots_in = c.ptr<int>((size_t)max_pairs * 4);
    w.slots_out = c.ptr<int>((size_t)max_pairs * 4);
    w.total = c.total();
    return w;
}

static int rel_check_pairs(const char* who, int64_t max_pairs) {
    AVL_REQUIRE(max_pairs >= 1 && max_pairs <= kRelMaxPairs, "%s: max_pairs = %lld (1 .. 2^28)", who, (long long)max_pairs);
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_object_relations_work_bytes(int64_t max_pairs, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_object_relations_work_bytes: null output");
    const int rc = rel_check_pairs("avl_object_relations_work_bytes", max_pairs);
    if (rc != AVL_OK) return rc;
    *bytes = rel_work(max_pairs, nullptr).total;
    return AVL_OK;
}

int avl_object_relations(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const int32_t* d_grid_pos, const int32_t* d_labels,
                         int32_t n, int radius, int64_t max_pairs, int64_t* d_table, int64_t* d_count, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "avl_object_relations";
    AVL_REQUIRE(d_index, "%s: null d_index", who);
    AVL_REQUIRE(d_table, "%s: null d_table", who);
    AVL_REQUIRE(d_count, "%s: null d_count", who);
    int rc = ci_check_grid(who, N, gs, vh);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(N == 0 || d_grid_pos, "%s: null d_grid_pos", who);
    AVL_REQUIRE(N == 0 || d_labels, "%s: null d_labels", who);
    const CellIndexView v = ci_layout(const_cast<void*>(d_index), N, gs, vh);
    AVL_REQUIRE(index_bytes >= v.total, "%s: the index buffer has %zu bytes, needs %zu", who, index_bytes, v.total);
    AVL_REQUIRE(n >= 0, "%s: n = %d objects (at least 0)", who, (int)n);
    rc = rel_check_pairs(who, max_pairs);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(radius >= 1 && radius <= kRelMaxRadius, "%s: radius %d cells (1 .. %d)", who, radius, kRelMaxRadius);
    const RelWork w = rel_work(max_pairs, ws);
    AVL_REQUIRE(ws && ws_bytes >= w.total, "%s: workspace (ws) of %zu bytes, need %zu", who, ws_bytes, w.total);
    hipStream_t st = as_stream(stream);
    if (N == 0 || n == 0) {
        AVL_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
        return AVL_OK;
    }
    keep_mempool_once();
    AVL_HIP_CHECK(hipMemsetAsync(w.header, 0, sizeof(RelHeader), st));
    AVL_HIP_CHECK(hipMemsetAsync(w.keys, 0xff, (size_t)((char*)w.counters - (char*)w.keys), st));       // keys and minima: all ones
    AVL_HIP_CHECK(hipMemsetAsync(w.counters, 0, (size_t)w.H * 24, st));
    AVL_HIP_CHECK(hipMemsetAsync(w.keys_in, 0xff, (size_t)max_pairs * 8, st));                          // the padding of the sort
    AVL_HIP_CHECK(hipMemsetAsync(w.slots_in, 0xff, (size_t)max_pairs * 4, st));
    RelParams p{};
    p.gs = gs, p.vh = vh, p.R = radius, p.n = n;
    p.N = N, p.nwords = v.nwords, p.max_pairs = max_pairs, p.H = (unsigned long long)w.H;
    p.bits = v.bits, p.prefix = v.prefix, p.perm = v.perm, p.pos = d_grid_pos, p.labels = d_labels;
    p.keys = w.keys, p.mins = w.mins, p.counters = w.counters, p.header = w.header;
    hipLaunchKernelGGL(rel_scan_kernel, dim3(stride_blocks(2 * N)), dim3(256), 0, st, p);
    const dim3 scan_n((unsigned)w.nblocks), scan_t(kRelScanThreads);
    const RelClaimed claimed{w.keys};
    hipLaunchKernelGGL((count_flagged_kernel<kRelScanThreads, kRelScanPer, RelClaimed>), scan_n, scan_t, 0, st, w.H, claimed, w.counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)w.counts, (int64_t)w.nblocks, w.counts,
                       (int*)nullptr, OpSum{}, 0);
    hipLaunchKernelGGL(rel_compact_kernel, scan_n, scan_t, 0, st, (const unsigned long long*)w.keys, w.H, (const int*)w.counts, max_pairs, w.keys_in,
                       w.slots_in);
    AVL_HIP_CHECK(hipGetLastError());
    // every key is below (n + 1)^2 <= 2^bits, and the low `bits` bits of the padding are all ones: it sorts behind every pair
    const int bits = bits_for(((unsigned long long)n + 1ull) * ((unsigned long long)n + 1ull), 64);
    rc = sort_pairs_pooled(who, w.keys_in, w.keys_out, w.slots_in, w.slots_out, max_pairs, bits, st);
    if (rc != AVL_OK) return rc;
    hipLaunchKernelGGL(rel_rows_kernel, dim3(stride_blocks(max_pairs)), dim3(256), 0, st, p, (const unsigned long long*)w.keys_out,
                       (const int*)w.slots_out, d_table, d_count);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
