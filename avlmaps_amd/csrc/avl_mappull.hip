// Resampling a finished voxel map backward: for every cell of the TARGET grid, where its centre came from in map B,
// and the voxel gathered from there.  avl_mapfuse.hip's move is a forward, nearest-cell scatter: under a rotation some cells receive
// two or three voxels and their neighbours none.  Asking from the target's side leaves no such pinholes.  Upstream has no counterpart
// for finished maps.
//
// THE MEMBERS OF A TARGET CELL.  One device function, pl_members, used by the marking pass and by the fill pass, so that both see the
// same list.  The cell c, moved back by the whole-cell shift, stands for its centre as in avl_mapfuse.hip's move (the cell k = 0 is two
// cells wide upstream and has the centre 0); the point goes through the INVERSE transform, which the host inverted once in float64, in
// the move's own grouping ((P0 x + P1 y) + P2 z) + P3, every product and sum rounded once (this file is built with -ffp-contract=off).
// Nearest: the cell of B that upstream's base_pos2grid_id_3d maps the point to, lambda = 1.  Linear: the point is bracketed on every
// axis by the centres of B's lattice -- horizontally 0, +-1.5, +-2.5, .. cells, in height h + 0.5 --, and the eight corners carry the
// products of t or 1 - t.  Corner j has dz = j & 1, dy = j >> 1 & 1, dx = j >> 2 & 1; lambda = (lx * ly) * lz.  A corner is a member
// when lambda > 0 and a selected row of B owns its cell.  The cell exists when the sum of the members' lambdas, added in corner
// order, reaches min_support.  Without a transform nothing floats: the member is the cell itself, moved back by the shift.
//
// THE PLAN.  The selected rows of B go into the cell index (avl_cellindex.h) through a copy of the cells in which every other row is
// (-1, -1, -1); a selected row that does not own its cell shares it: an error.  Pass 1 is dense: one thread per target cell finds its
// members' support, and the wave's ballot is the cell's bit in a bit plane of the index's own layout (bit lin & 31 of word lin >> 5,
// lin = (row * gs + col) * vh + h).  Pass 2 is the index's prefix over the words' popcounts: it numbers the cells in linear order
// and gives n_out, which the host reads back -- it has no bound from n_b.  Pass 3, the second entry point, is dense again: every
// cell whose bit is set finds its members once more and writes them at its rank.
//
// THE ROWS.  The hot kernel, shaped like mf_rows_kernel: a group of L lanes owns an output voxel, a lane four elements per chunk, one
// 16-byte load per member and chunk where D % 4 == 0 and the matrix is 16-byte aligned, scalars otherwise, same bytes.  The eight
// member rows and their float64 weights lambda * w stay in registers across the chunks.  No LDS, no cross-lane step.  Neighbouring
// output voxels share members (up to eight reads of a row of B): what of that the caches absorb is measured, not assumed.
#include "avl_mapfuse.h"
#include "avl_scan.h"

namespace avl {

constexpr int kPlErrShared = 2;                 // the bit that avl_map_fuse_plan sets for two selected rows in one cell
constexpr int kPlNearest = 0, kPlLinear = 1;

struct PlArgs {
    MfTransform P;                              // the inverse transform: target base frame -> B's
    double cs, min_support;
    int gs, vh, sr, sc, sh, mode;
    bool moving;
};

// the scratch array of both plan calls, in int32: 4 n_b + 2 W + W / 1024 + 2 and five roundings to 64, W = ceil(gs gs vh / 32)
struct PlScratch {
    int32_t *masked, *used, *tprefix, *block_counts;
    uint32_t* tbits;
    int64_t nwords, nblocks;
};

static int64_t pl_scratch_need(int64_t n_b, int gs, int vh) {
    const int64_t nwords = ((int64_t)gs * gs * vh + 31) / 32;
    return 4 * n_b + 2 * nwords + nwords / 1024 + 512;
}

static PlScratch pl_scratch(int32_t* base, int64_t n_b, int gs, int vh) {
    PlScratch s{};
    s.nwords = ((int64_t)gs * gs * vh + 31) / 32;
    s.nblocks = (s.nwords + kCiThreads * kCiPer - 1) / (kCiThreads * kCiPer);
    int64_t at = 0;
    const auto piece = [&](int64_t count) {
        int32_t* p = base + at;
        at += (count + 63) / 64 * 64;
        return p;
    };
    s.masked = piece(3 * n_b);
    s.used = piece(n_b);
    s.tbits = reinterpret_cast<uint32_t*>(piece(s.nwords));
    s.tprefix = piece(s.nwords);
    s.block_counts = piece(s.nblocks + 1);
    return s;
}

// masked = the cell of a selected row, (-1, -1, -1) for every other; head[3] = rows that use or weight unselects, head[4] = further rows outside
__global__ __launch_bounds__(256) void pl_select_kernel(const int32_t* __restrict__ cells, const uint8_t* __restrict__ use, const float* __restrict__ w,
                                                        int64_t n, int gs, int vh, int32_t* __restrict__ masked, int32_t* __restrict__ head) {
    const int64_t rounds = (n + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);     // every lane takes part in every ballot
    for (int64_t k = 0; k < rounds; ++k) {
        const int64_t i = (k * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        bool unsel = false, outside = false;
        if (i < n) {
            const bool sel = (!use || use[i]) && mf_weight_ok(w[i]);
            const bool in = mf_lin(cells, i, gs, vh) >= 0;
            unsel = !sel;
            outside = sel && !in;
            const bool take = sel && in;
            masked[3 * i] = take ? cells[3 * i] : -1;
            masked[3 * i + 1] = take ? cells[3 * i + 1] : -1;
            masked[3 * i + 2] = take ? cells[3 * i + 2] : -1;
        }
        mf_count(unsel, head + 3);
        mf_count(outside, head + 4);
    }
}

// a selected row that does not own its cell shares it; head[1] = the selected rows
__global__ __launch_bounds__(256) void pl_shared_kernel(const int32_t* __restrict__ masked, int64_t n, int gs, int vh, const uint32_t* __restrict__ bits,
                                                        const int32_t* __restrict__ prefix, const int32_t* __restrict__ perm, int32_t* __restrict__ head) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int lin = mf_lin(masked, i, gs, vh);
        if (lin >= 0 && ci_probe(bits, prefix, perm, lin) != i) atomicOr(head + 2, kPlErrShared);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) head[1] = (int32_t)n - head[3] - head[4];
}

// the row of B that owns the cell, -1 when it is empty or outside the grid
__device__ __forceinline__ int pl_probe(const PlArgs& g, const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                        const int32_t* __restrict__ perm, int64_t r, int64_t c, int64_t h) {
    if (r < 0 || r >= g.gs || c < 0 || c >= g.gs || h < 0 || h >= g.vh) return -1;
    return ci_probe(bits, prefix, perm, (int)((r * g.gs + c) * g.vh + h));
}

// s = coordinate / cs on the horizontal lattice of centres 0, +-1.5, +-2.5, ..: the lower bracketing centre's k and the fraction t
__device__ __forceinline__ void pl_bracket(double s, int64_t* k0, double* t) {
    const double a = fabs(s);
    int64_t j0 = 0;
    double u;
    if (a < 1.5) {
        u = a / 1.5;
    } else {
        const double b = a - 0.5, f = floor(b);
        j0 = (int64_t)f;
        u = b - f;
    }
    if (s >= 0.0) *k0 = j0, *t = u;
    else if (u == 0.0) *k0 = -j0, *t = 0.0;
    else *k0 = -(j0 + 1), *t = 1.0 - u;
}

// Calls emit(j, row, lambda) for j = 0 .. 7 in corner order, (-1, 0.0) for a corner that is no member, and returns the members' support.
template <typename Emit>
__device__ __forceinline__ double pl_members(const PlArgs& g, const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                             const int32_t* __restrict__ perm, int r, int c, int h, Emit emit) {
    const int64_t r1 = (int64_t)r - g.sr, c1 = (int64_t)c - g.sc, h1 = (int64_t)h - g.sh;
    bool sole = true;                           // one candidate with lambda = 1
    int64_t br = r1, bc = c1, bh = h1;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (g.moving) {
        const int64_t kr = g.gs / 2 - r1, kc = g.gs / 2 - c1;
        const double x = ((double)kr + (kr > 0 ? 0.5 : kr < 0 ? -0.5 : 0.0)) * g.cs;
        const double y = ((double)kc + (kc > 0 ? 0.5 : kc < 0 ? -0.5 : 0.0)) * g.cs;
        const double z = ((double)h1 + 0.5) * g.cs;
        const double x1 = ((g.P.t[0] * x + g.P.t[1] * y) + g.P.t[2] * z) + g.P.t[3];
        const double y1 = ((g.P.t[4] * x + g.P.t[5] * y) + g.P.t[6] * z) + g.P.t[7];
        const double z1 = ((g.P.t[8] * x + g.P.t[9] * y) + g.P.t[10] * z) + g.P.t[11];
        qx = x1 / g.cs, qy = y1 / g.cs, qz = z1 / g.cs;
        const bool ok = fabs(qx) < 2147483648.0 && fabs(qy) < 2147483648.0 && fabs(qz) < 2147483648.0;         // false for a NaN
        if (!ok) br = bc = bh = -1;
        else if (g.mode == kPlNearest) br = mf_index(qx, g.gs), bc = mf_index(qy, g.gs), bh = (int64_t)qz;
        else sole = false;
    }
    if (sole) {
        const int m = pl_probe(g, bits, prefix, perm, br, bc, bh);
        emit(0, m, m >= 0 ? 1.0 : 0.0);
#pragma unroll
        for (int j = 1; j < 8; ++j) emit(j, -1, 0.0);
        return m >= 0 ? 1.0 : 0.0;
    }
    int64_t kx, ky;
    double tx, ty;
    pl_bracket(qx, &kx, &tx);
    pl_bracket(qy, &ky, &ty);
    const double sz = qz - 0.5, fz = floor(sz), tz = sz - fz;
    const int64_t h0 = (int64_t)fz;
    double support = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int dz = j & 1, dy = j >> 1 & 1, dx = j >> 2 & 1;
        const double lx = dx ? tx : 1.0 - tx, ly = dy ? ty : 1.0 - ty, lz = dz ? tz : 1.0 - tz;
        const double l = (lx * ly) * lz;
        int m = -1;
        if (l > 0.0) m = pl_probe(g, bits, prefix, perm, g.gs / 2 - (kx + dx), g.gs / 2 - (ky + dy), h0 + dz);
        if (m >= 0) support = support + l;      // from +0.0: the first member's lambda as it is
        emit(j, m, m >= 0 ? l : 0.0);
    }
    return support;
}

// pass 1: a target cell's bit; head[5] = the cells with members whose support stays below min_support.  One thread per cell (the
// grid covers the cells, fewer than 2^31, in workgroups of 256: no loop, which keeps the scalar registers free for the transform); a
// workgroup is a multiple of the wave, so lane 0 and lane 32 of a wave own the first cells of two consecutive words.
__global__ __launch_bounds__(256) void pl_mark_kernel(PlArgs g, const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                                      const int32_t* __restrict__ perm, int cells, uint32_t* __restrict__ tbits,
                                                      int32_t* __restrict__ head) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;             // below 2^31 + 256
    const int lin = at < cells ? (int)at : -1;
    bool exists = false, below = false;
    if (lin >= 0) {
        const int h = lin % g.vh, c = lin / g.vh % g.gs, r = lin / g.vh / g.gs;
        const double support = pl_members(g, bits, prefix, perm, r, c, h, [](int, int, double) {});
        exists = support > 0.0 && support >= g.min_support;
        below = support > 0.0 && !exists;
    }
    const unsigned long long word = __ballot(exists);
    if (lane == 0 && lin >= 0) tbits[lin >> 5] = (uint32_t)word;
    if (lane == 32 && lin >= 0) tbits[lin >> 5] = (uint32_t)(word >> 32);
    mf_count(below, head + 5);
}

// pass 2, the cell index's prefix passes over the target's bit plane: a thread's kCiPer consecutive words
__device__ __forceinline__ int pl_block_scan(const uint32_t* __restrict__ tbits, int64_t nwords, int* lds, int64_t* w0, int* total) {
    *w0 = (int64_t)blockIdx.x * (kCiThreads * kCiPer) + threadIdx.x * kCiPer;
    int s = 0;
#pragma unroll
    for (int k = 0; k < kCiPer; ++k)
        if (*w0 + k < nwords) s += __popc(tbits[*w0 + k]);
    return block_excl_scan<kCiThreads / kWave>(s, OpSum{}, 0, lds, total);
}

__global__ __launch_bounds__(kCiThreads) void pl_count_kernel(const uint32_t* __restrict__ tbits, int64_t nwords, int32_t* __restrict__ counts) {
    __shared__ int s_w[kCiThreads / kWave];
    int64_t w0;
    int total;
    pl_block_scan(tbits, nwords, s_w, &w0, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kCiThreads) void pl_prefix_kernel(const uint32_t* __restrict__ tbits, int64_t nwords, const int32_t* __restrict__ offsets,
                                                               int32_t* __restrict__ tprefix) {
    __shared__ int s_w[kCiThreads / kWave];
    int64_t w0;
    int total;
    int run = offsets[blockIdx.x] + pl_block_scan(tbits, nwords, s_w, &w0, &total);
#pragma unroll
    for (int k = 0; k < kCiPer; ++k)
        if (w0 + k < nwords) {
            tprefix[w0 + k] = run;
            run += __popc(tbits[w0 + k]);
        }
}

// pass 3: every cell whose bit is set writes its cell, members and lambdas at its rank; used[m] = 1 for every member row
__global__ __launch_bounds__(256) void pl_fill_kernel(PlArgs g, const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                                      const int32_t* __restrict__ perm, int64_t cells, const uint32_t* __restrict__ tbits,
                                                      const int32_t* __restrict__ tprefix, int64_t n_out, int32_t* __restrict__ cells_out,
                                                      int32_t* __restrict__ members, double* __restrict__ lam, int32_t* __restrict__ used,
                                                      int32_t* __restrict__ occupied) {
    for (int64_t lin = (int64_t)blockIdx.x * 256 + threadIdx.x; lin < cells; lin += (int64_t)gridDim.x * 256) {
        const uint32_t w = tbits[lin >> 5], b = (uint32_t)lin & 31u;
        if (!(w >> b & 1u)) continue;
        const int64_t v = (int64_t)tprefix[lin >> 5] + __popc(w & ((1u << b) - 1u));
        if (v < 0 || v >= n_out) continue;      // a plan of other arguments: nothing is written out of bounds
        const int h = (int)(lin % g.vh), c = (int)(lin / g.vh % g.gs), r = (int)(lin / g.vh / g.gs);
        int32_t* __restrict__ mv = members + 8 * v;
        double* __restrict__ lv = lam + 8 * v;
        pl_members(g, bits, prefix, perm, r, c, h, [&](int j, int m, double l) {
            mv[j] = m;
            lv[j] = l;
            if (m >= 0) used[m] = 1;
        });
        cells_out[3 * v] = r, cells_out[3 * v + 1] = c, cells_out[3 * v + 2] = h;
        if (occupied) occupied[lin] = (int32_t)v;
    }
}

// counts[3] = the selected rows of B that no target cell uses
__global__ __launch_bounds__(256) void pl_unused_kernel(const int32_t* __restrict__ masked, const int32_t* __restrict__ used, int64_t n,
                                                        int32_t* __restrict__ counts) {
    const int64_t rounds = (n + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);
    for (int64_t k = 0; k < rounds; ++k) {
        const int64_t i = (k * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        mf_count(i < n && masked[3 * i] >= 0 && !used[i], counts + 3);
    }
}

__global__ void pl_counts_kernel(const int32_t* __restrict__ head, int32_t* __restrict__ counts) {
    counts[0] = head[3], counts[1] = head[4], counts[2] = head[5], counts[3] = 0;
}

template <int L>
__global__ __launch_bounds__(256) void pl_rows_kernel(int64_t n_out, const int32_t* __restrict__ members, const double* __restrict__ lam,
                                                      const float* __restrict__ feat_b, const float* __restrict__ w_b, const uint8_t* __restrict__ rgb_b,
                                                      int64_t n_b, int D, bool vec_b, bool vec_o, float* __restrict__ feat_out,
                                                      float* __restrict__ weight_out, uint8_t* __restrict__ rgb_out) {
    constexpr int kPerBlock = 256 / L;
    const int sub = threadIdx.x % L;
    const int64_t step = (int64_t)gridDim.x * kPerBlock;
    for (int64_t v = (int64_t)blockIdx.x * kPerBlock + threadIdx.x / L; v < n_out; v += step) {
        // the members, their weights omega = lambda * w and both sums, in corner order
        int m[8];
        double om[8];
        double W = 0.0, S = 0.0;                // from +0.0: the first positive term as it is
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            m[j] = members[8 * v + j];
            if (m[j] >= n_b) m[j] = -1;
            const double l = lam[8 * v + j];
            om[j] = m[j] >= 0 ? l * (double)w_b[m[j]] : 0.0;
            if (m[j] >= 0) W = W + om[j], S = S + l;
        }
        const bool any = S > 0.0;
        float* __restrict__ ro = feat_out + (size_t)v * D;
        for (int d = 4 * sub; d < D; d += 4 * L) {
            MfAcc acc{0.0, 0.0, 0.0, 0.0, false};
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (m[j] >= 0) acc.add(om[j], mf_load4(feat_b + (size_t)m[j] * D, d, D, vec_b));
            float4 o;
            o.x = any ? (float)(acc.x / W) : 0.0f;
            o.y = any ? (float)(acc.y / W) : 0.0f;
            o.z = any ? (float)(acc.z / W) : 0.0f;
            o.w = any ? (float)(acc.w / W) : 0.0f;
            if (vec_o) {
                *reinterpret_cast<float4*>(ro + d) = o;
            } else {
                ro[d] = o.x;
                if (d + 1 < D) ro[d + 1] = o.y;
                if (d + 2 < D) ro[d + 2] = o.z;
                if (d + 3 < D) ro[d + 3] = o.w;
            }
        }
        if (sub == 0) {
            MfAcc acc{0.0, 0.0, 0.0, 0.0, false};
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (m[j] >= 0) {
                    const uint8_t* __restrict__ px = rgb_b + 3 * (size_t)m[j];
                    acc.add(om[j], make_float4((float)px[0], (float)px[1], (float)px[2], 0.0f));
                }
            weight_out[v] = any ? (float)(W / S) : 0.0f;
            rgb_out[3 * v] = any ? (uint8_t)(int)(acc.x / W) : 0;
            rgb_out[3 * v + 1] = any ? (uint8_t)(int)(acc.y / W) : 0;
            rgb_out[3 * v + 2] = any ? (uint8_t)(int)(acc.z / W) : 0;
        }
    }
}

// the checks that both plan calls share; fills *g
static int pl_check(const char* who, int64_t n_b, const double* h_P, const int32_t* h_shift, int gs, double cs, int vh, int mode, double min_support,
                    PlArgs* g) {
    const int rc = ci_check_grid(who, n_b, gs, vh);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(cs > 0.0 && cs < __builtin_inf(), "%s: cs = %g (> 0 and finite)", who, cs);
    AVL_REQUIRE(mode == kPlNearest || mode == kPlLinear, "%s: mode %d (0 = nearest, 1 = linear)", who, mode);
    AVL_REQUIRE(min_support > 0.0 && min_support <= 1.0, "%s: min_support = %g (0 < min_support <= 1)", who, min_support);
    *g = PlArgs{};
    if (h_P) {
        for (int k = 0; k < 16; ++k) AVL_REQUIRE(h_P[k] - h_P[k] == 0.0, "%s: the inverse transform is not finite (element %d)", who, k);
        AVL_REQUIRE(h_P[12] == 0.0 && h_P[13] == 0.0 && h_P[14] == 0.0 && h_P[15] == 1.0, "%s: the bottom row of the inverse transform is not 0 0 0 1", who);
        for (int k = 0; k < 12; ++k) g->P.t[k] = h_P[k];
    }
    g->cs = cs, g->min_support = min_support, g->gs = gs, g->vh = vh, g->mode = mode, g->moving = h_P != nullptr;
    g->sr = h_shift ? h_shift[0] : 0, g->sc = h_shift ? h_shift[1] : 0, g->sh = h_shift ? h_shift[2] : 0;
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_map_pull_plan(const int32_t* d_cells_b, const uint8_t* d_use_b, const float* d_w_b, int64_t n_b, const double* h_P, const int32_t* h_shift,
                      int gs, double cs, int vh, int mode, double min_support, void* d_index, size_t index_bytes, int32_t* d_scratch,
                      int64_t scratch_i32, int32_t* d_head, void* stream) {
    PlArgs g;
    int rc = pl_check("avl_map_pull_plan", n_b, h_P, h_shift, gs, cs, vh, mode, min_support, &g);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_index && d_scratch && d_head, "avl_map_pull_plan: null pointer");
    AVL_REQUIRE((d_cells_b && d_w_b) || n_b == 0, "avl_map_pull_plan: null pointer for map B");
    AVL_REQUIRE(scratch_i32 >= pl_scratch_need(n_b, gs, vh), "avl_map_pull_plan: the scratch array has %lld int32, needs %lld", (long long)scratch_i32,
                (long long)pl_scratch_need(n_b, gs, vh));
    const size_t index_need = ci_layout(d_index, n_b, gs, vh).total;
    AVL_REQUIRE(index_bytes >= index_need, "avl_map_pull_plan: the index buffer has %zu bytes, needs %zu", index_bytes, index_need);
    const PlScratch s = pl_scratch(d_scratch, n_b, gs, vh);
    const int64_t cells = (int64_t)gs * gs * vh;
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(d_head, 0, 8 * sizeof(int32_t), st));
    if (n_b) hipLaunchKernelGGL(pl_select_kernel, dim3(stride_blocks(n_b)), dim3(256), 0, st, d_cells_b, d_use_b, d_w_b, n_b, gs, vh, s.masked, d_head);
    rc = avl_cell_index_build(s.masked, n_b, gs, vh, d_index, index_bytes, stream);
    if (rc != AVL_OK) return rc;
    const CellIndexView ix = ci_layout(d_index, n_b, gs, vh);
    if (n_b)
        hipLaunchKernelGGL(pl_shared_kernel, dim3(stride_blocks(n_b)), dim3(256), 0, st, (const int32_t*)s.masked, n_b, gs, vh, (const uint32_t*)ix.bits,
                           (const int32_t*)ix.prefix, (const int32_t*)ix.perm, d_head);
    hipLaunchKernelGGL(pl_mark_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, g, (const uint32_t*)ix.bits, (const int32_t*)ix.prefix,
                       (const int32_t*)ix.perm, (int)cells, s.tbits, d_head);
    hipLaunchKernelGGL(pl_count_kernel, dim3((unsigned)s.nblocks), dim3(kCiThreads), 0, st, (const uint32_t*)s.tbits, s.nwords, s.block_counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)s.block_counts, s.nblocks, s.block_counts,
                       d_head, OpSum{}, 0);
    hipLaunchKernelGGL(pl_prefix_kernel, dim3((unsigned)s.nblocks), dim3(kCiThreads), 0, st, (const uint32_t*)s.tbits, s.nwords,
                       (const int32_t*)s.block_counts, s.tprefix);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_map_pull_fill(int64_t n_b, const double* h_P, const int32_t* h_shift, int gs, double cs, int vh, int mode, double min_support,
                      const void* d_index, size_t index_bytes, int32_t* d_scratch, int64_t scratch_i32, const int32_t* d_head, int64_t n_out,
                      int32_t* d_cells_out, int32_t* d_members, double* d_lam, int32_t* d_occupied, int32_t* d_counts, void* stream) {
    PlArgs g;
    const int rc = pl_check("avl_map_pull_fill", n_b, h_P, h_shift, gs, cs, vh, mode, min_support, &g);
    if (rc != AVL_OK) return rc;
    const int64_t cells = (int64_t)gs * gs * vh;
    AVL_REQUIRE(n_out >= 0 && n_out <= cells, "avl_map_pull_fill: %lld output voxels on a grid of %lld cells", (long long)n_out, (long long)cells);
    AVL_REQUIRE(d_index && d_scratch && d_head && d_counts, "avl_map_pull_fill: null pointer");
    AVL_REQUIRE(n_out == 0 || (d_cells_out && d_members && d_lam), "avl_map_pull_fill: null pointer for the plan's arrays");
    AVL_REQUIRE(scratch_i32 >= pl_scratch_need(n_b, gs, vh), "avl_map_pull_fill: the scratch array has %lld int32, needs %lld", (long long)scratch_i32,
                (long long)pl_scratch_need(n_b, gs, vh));
    const CellIndexView ix = ci_layout(const_cast<void*>(d_index), n_b, gs, vh);
    AVL_REQUIRE(index_bytes >= ix.total, "avl_map_pull_fill: the index buffer has %zu bytes, needs %zu", index_bytes, ix.total);
    const PlScratch s = pl_scratch(d_scratch, n_b, gs, vh);
    hipStream_t st = as_stream(stream);
    if (d_occupied) AVL_HIP_CHECK(hipMemsetAsync(d_occupied, 0xFF, (size_t)cells * sizeof(int32_t), st));
    if (n_b) AVL_HIP_CHECK(hipMemsetAsync(s.used, 0, (size_t)n_b * sizeof(int32_t), st));
    hipLaunchKernelGGL(pl_counts_kernel, dim3(1), dim3(1), 0, st, d_head, d_counts);
    if (n_out)
        hipLaunchKernelGGL(pl_fill_kernel, dim3(stride_blocks(cells)), dim3(256), 0, st, g, (const uint32_t*)ix.bits, (const int32_t*)ix.prefix,
                           (const int32_t*)ix.perm, cells, (const uint32_t*)s.tbits, (const int32_t*)s.tprefix, n_out, d_cells_out, d_members, d_lam,
                           s.used, d_occupied);
    if (n_b) hipLaunchKernelGGL(pl_unused_kernel, dim3(stride_blocks(n_b)), dim3(256), 0, st, (const int32_t*)s.masked, (const int32_t*)s.used, n_b, d_counts);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_map_pull_rows(int64_t n_out, const int32_t* d_members, const double* d_lam, const float* d_feat_b, const float* d_w_b, const uint8_t* d_rgb_b,
                      int64_t n_b, int D, float* d_feat_out, float* d_weight_out, uint8_t* d_rgb_out, void* stream) {
    AVL_REQUIRE(n_b >= 0 && n_b < INT_MAX && n_out >= 0 && n_out < INT_MAX, "avl_map_pull_rows: %lld output voxels of %lld rows (each 0 .. 2^31 - 2)",
                (long long)n_out, (long long)n_b);
    AVL_REQUIRE(D >= 1 && D <= kMfMaxDim, "avl_map_pull_rows: D = %d (1 .. %d)", D, kMfMaxDim);
    if (n_out == 0) return AVL_OK;
    AVL_REQUIRE(d_members && d_lam && d_feat_out && d_weight_out && d_rgb_out, "avl_map_pull_rows: null pointer");
    AVL_REQUIRE(n_b == 0 || (d_feat_b && d_w_b && d_rgb_b), "avl_map_pull_rows: null pointer for map B");
    AVL_REQUIRE(reinterpret_cast<uintptr_t>(d_lam) % 8 == 0, "avl_map_pull_rows: the lambdas are not 8-byte aligned");
    const bool quad = D % 4 == 0;
    const bool vec_b = quad && reinterpret_cast<uintptr_t>(d_feat_b) % 16 == 0, vec_o = quad && reinterpret_cast<uintptr_t>(d_feat_out) % 16 == 0;
    const int quads = (D + 3) / 4;
    hipStream_t st = as_stream(stream);
#define AVL_PL_LAUNCH(L)                                                                                                                          \
    hipLaunchKernelGGL(pl_rows_kernel<L>, dim3(stride_blocks(n_out* L)), dim3(256), 0, st, n_out, d_members, d_lam, d_feat_b, d_w_b, d_rgb_b, n_b, D, \
                       vec_b, vec_o, d_feat_out, d_weight_out, d_rgb_out)
    if (quads > 32) AVL_PL_LAUNCH(64);
    else if (quads > 16) AVL_PL_LAUNCH(32);
    else if (quads > 8) AVL_PL_LAUNCH(16);
    else if (quads > 4) AVL_PL_LAUNCH(8);
    else if (quads > 2) AVL_PL_LAUNCH(4);
    else if (quads > 1) AVL_PL_LAUNCH(2);
    else AVL_PL_LAUNCH(1);
#undef AVL_PL_LAUNCH
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
