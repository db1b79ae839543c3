// Multi-source travel-distance field on the free space of a 2-D obstacle map for gfx950, and the decay map built on it.
//
// Upstream has no counterpart: avlmaps/robot/habitat_lang_robot.py:229-240 decays with the Euclidean distance transform of the
// category mask (csrc/avl_edt2d.hip reproduces that chain), which does not know about walls.  This file is its counterpart on
// the free space of the obstacle crop.
//
// Definition.  free (H, W) uint8, nonzero = free; sources (H, W) uint8, nonzero = source, a source may lie on an
// obstacle cell.  A step u -> v between 8-neighbours is legal when v is free, u is free or a source, and -- for a diagonal step --
// both cells that share an edge with u and with v are free (no corner cutting).  A walk of a straight and b diagonal steps has
// length a + b * sqrt(2); the field of a cell is the pair (a, b) of the shortest legal walk from any source to it, (0, 0) on a
// source, (-1, -1) where no walk ends.  sqrt(2) is irrational, so different pairs differ in length: the minimum is unique.
//
// Order.  Pairs are compared exactly in integers (travel_less in avl_travel_tile.h, with its bounds).
//
// State.  One 64-bit word per cell, a in the high half and b in the low half; all ones = unreached, which unpacks to (-1, -1).
// A candidate is "neighbour + step", a plain 64-bit addition: b never carries into a.
//
// Work.  The tile scheme of avl_travel_tile.h, described there at travel_tile_relax: rounds of 32 x 32 tiles that relax in LDS,
// write back what changed and wake the tiles that read it.  This family is the plain variant, travel_tile_relax<false, false>:
// every step costs 1 and the passability byte holds the source bit.
//
// Convergence.  Every stored word is (0, 0) on a source or was produced as "a stored neighbour + a legal step": by induction the
// length of a real legal walk from a source, so never below the definition's minimum.  Words only decrease.  A cell whose word
// changes wakes every tile that can read it (its own through the sweep loop or the cap mark, the neighbours through the halo
// mark), so when no tile is active every cell equals the minimum over its legal incoming steps: the Bellman fixed point, which
// with strictly positive step lengths is the shortest-walk field itself, whatever order the tiles ran in.  The optimal pair of
// a cell whose shortest walk has k steps is in place after at most k rounds, and a walk without repeated cells has fewer than
// H * W steps: the host gives up with an error after H * W + 1 rounds, which cannot happen unless the device misbehaves.
#include <algorithm>
#include <cmath>

#include "avl_common.h"
#include "avl_decay2d.h"
#include "avl_travel_tile.h"
#include "avl_wave.h"

namespace avl {

// pass = free | source << 1 per cell, state = (0, 0) on sources and unreached elsewhere; the tile of every source and its eight
// neighbours (a source on a tile border is their halo) start active
__global__ __launch_bounds__(256) void travel_init_kernel(const uint8_t* __restrict__ free_u8, int64_t ld_free,
                                                          const uint8_t* __restrict__ src_u8, int64_t ld_src, int H, int W,
                                                          uint8_t* __restrict__ pass, unsigned long long* __restrict__ state,
                                                          unsigned* __restrict__ flags, unsigned* __restrict__ hdr) {
    const int tw = travel_tiles(W), th = travel_tiles(H);
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
        travel_init_cell(i, r, c, free_u8[(int64_t)r * ld_free + c] != 0, src_u8[(int64_t)r * ld_src + c] != 0, th, tw, pass, state, flags, hdr);
    }
}

// One round: the shared body with unit steps (its legal-step rule is travel_legal_in<kTravelHalo> on the loaded pass bytes).
// cur / next: the active marks of this round and of the coming one.
__global__ __launch_bounds__(kTravelThreads) void travel_round_kernel(const uint8_t* __restrict__ pass, unsigned long long* state, int H,
                                                                      int W, unsigned* __restrict__ cur, unsigned* __restrict__ next,
                                                                      unsigned* __restrict__ activated) {
    __shared__ TravelTileLds lds;
    if (!travel_take_mark(cur, &lds.active, &lds.dirty)) return;
    const int tile_r = blockIdx.x / travel_tiles(W), tile_c = blockIdx.x - tile_r * travel_tiles(W);
    travel_tile_relax<false, false>(lds, pass, nullptr, 0, state, H, W, tile_r, tile_c, 0, next, activated);
}

// the two int32 planes, the number of reached cells, and the host's counters into d_stats = [rounds, tile runs, reached, any source]
__global__ __launch_bounds__(256) void travel_unpack_kernel(const unsigned long long* __restrict__ state, int64_t n,
                                                            int32_t* __restrict__ straight, int32_t* __restrict__ diagonal,
                                                            long long rounds, long long tile_runs, int any_source,
                                                            unsigned long long* __restrict__ stats) {
    unsigned long long reached = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long s = state[i];
        straight[i] = (int32_t)(unsigned)(s >> 32);
        diagonal[i] = (int32_t)(unsigned)s;
        reached += s != kTravelUnreached;
    }
    reached = wave_sum(reached);
    if ((threadIdx.x & (kWave - 1)) == 0 && reached) atomicAdd(&stats[2], reached);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[0] = (unsigned long long)rounds;
        stats[1] = (unsigned long long)tile_runs;
        stats[3] = (unsigned long long)any_source;
    }
}

// d = double(a) + double(b) * sqrt(2), unfused; t = decay_value(d), 0 on unreached cells; [min, max] of the window by bit pattern
__global__ __launch_bounds__(256) void travel_decay_kernel(const int32_t* __restrict__ straight, const int32_t* __restrict__ diagonal,
                                                           int64_t n, double cell_size, double decay_rate, double* __restrict__ out,
                                                           unsigned long long* __restrict__ minmax) {
    __shared__ double s_red[2 * 256 / kWave];
    double mn = INFINITY, mx = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = straight[i], b = diagonal[i];
        double v = 0.0;
        if (a >= 0 && b >= 0) v = decay_value((double)a + (double)b * 1.4142135623730951, cell_size, decay_rate);
        out[i] = v;
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    block_minmax_atomic<256>(mn, mx, minmax, s_red);
}

int travel_check_shape(const char* what, int H, int W) {
    AVL_REQUIRE(H > 0 && W > 0 && H <= kTravelMaxSide && W <= kTravelMaxSide, "%s: bad shape %d x %d (sides 1 .. %d)", what, H, W,
                kTravelMaxSide);
    return AVL_OK;
}

TravelLayout travel_layout(int H, int W) {
    const size_t tiles = (size_t)travel_tiles(H) * (size_t)travel_tiles(W);
    Carver c;
    TravelLayout l;
    l.hdr = c.take(kTravelHdrWords * sizeof(unsigned));
    l.flags = c.take(2 * tiles * sizeof(unsigned));
    l.pass = c.take((size_t)H * W);
    l.state = c.take((size_t)H * W * sizeof(unsigned long long));
    l.total = c.total() + 256;                        // the entry point aligns the base itself
    return l;
}

int travel_unpack(const unsigned long long* state, int64_t n, int32_t* d_straight, int32_t* d_diagonal, int64_t rounds, int64_t tile_runs,
                  bool any_source, int64_t* d_stats, hipStream_t st) {
    hipLaunchKernelGGL(travel_unpack_kernel, dim3(stride_blocks(n)), dim3(256), 0, st, state, n, d_straight, d_diagonal, (long long)rounds,
                       (long long)tile_runs, (int)any_source, reinterpret_cast<unsigned long long*>(d_stats));
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_travel2d_workspace_bytes(int H, int W, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_travel2d_workspace_bytes: null output");
    int rc = travel_check_shape("avl_travel2d_workspace_bytes", H, W);
    if (rc != AVL_OK) return rc;
    *bytes = travel_layout(H, W).total;
    return AVL_OK;
}

int avl_travel2d(const uint8_t* d_free, int64_t ld_free, const uint8_t* d_sources, int64_t ld_src, int H, int W, int32_t* d_straight,
                 int32_t* d_diagonal, int64_t* d_stats, void* ws, size_t ws_bytes, void* stream) {
    int rc = travel_check_shape("avl_travel2d", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_free && d_sources, "avl_travel2d: null free or source image");
    AVL_REQUIRE(d_straight && d_diagonal && d_stats, "avl_travel2d: null output plane or stats pointer");
    AVL_REQUIRE(ld_free >= W, "avl_travel2d: free rows of %lld cells cannot hold %d columns", (long long)ld_free, W);
    AVL_REQUIRE(ld_src >= W, "avl_travel2d: source rows of %lld cells cannot hold %d columns", (long long)ld_src, W);
    const TravelLayout l = travel_layout(H, W);
    AVL_REQUIRE(ws && ws_bytes >= l.total, "avl_travel2d: workspace of %zu bytes, need %zu", ws_bytes, l.total);
    hipStream_t st = as_stream(stream);
    char* base = (char*)align256_ptr(ws);
    unsigned* hdr = (unsigned*)(base + l.hdr);
    unsigned* flags = (unsigned*)(base + l.flags);
    uint8_t* pass = (uint8_t*)(base + l.pass);
    unsigned long long* state = (unsigned long long*)(base + l.state);
    const unsigned tiles = (unsigned)(travel_tiles(W) * travel_tiles(H));      // at most 512 * 512
    const int64_t n = (int64_t)H * W;

    AVL_HIP_CHECK(hipMemsetAsync(hdr, 0, l.pass - l.hdr, st));              // the header and both mark buffers
    AVL_HIP_CHECK(hipMemsetAsync(d_stats, 0, 4 * sizeof(int64_t), st));
    hipLaunchKernelGGL(travel_init_kernel, dim3(stride_blocks(n)), dim3(256), 0, st, d_free, ld_free, d_sources, ld_src, H, W, pass, state,
                       flags, hdr);
    AVL_HIP_CHECK(hipGetLastError());

    // a shortest walk has fewer than H * W steps and every round moves every pending walk on by a step or more
    const int64_t max_rounds = n + 1;
    int64_t rounds = 0, tile_runs = 0;
    unsigned host[kTravelHdrWords];
    rc = travel_run_rounds(
        "avl_travel2d", max_rounds, hdr, flags, tiles, st,
        [&](int64_t, unsigned* cur, unsigned* next, unsigned* activated) {
            hipLaunchKernelGGL(travel_round_kernel, dim3(tiles), dim3(kTravelThreads), 0, st, (const uint8_t*)pass, state, H, W, cur, next, activated);
        },
        &rounds, &tile_runs, host);
    if (rc != AVL_OK) return rc;
    return travel_unpack(state, n, d_straight, d_diagonal, rounds, tile_runs, host[kTravelHdrAny] != 0, d_stats, st);
}

int avl_travel_decay_2d(const int32_t* d_straight, const int32_t* d_diagonal, int H, int W, double cell_size, double decay_rate,
                        int normalize, double* d_out_f64, int32_t* d_flags, void* ws, size_t ws_bytes, void* stream) {
    int rc = travel_check_shape("avl_travel_decay_2d", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_straight && d_diagonal && d_out_f64 && d_flags, "avl_travel_decay_2d: null plane, output or flag pointer");
    AVL_REQUIRE(std::isfinite(decay_rate) && decay_rate >= 0.0, "avl_travel_decay_2d: decay_rate must be finite and >= 0");
    AVL_REQUIRE(std::isfinite(cell_size) && cell_size > 0.0, "avl_travel_decay_2d: cell_size must be finite and > 0");
    AVL_REQUIRE(ws && ws_bytes >= 256 + 2 * sizeof(double), "avl_travel_decay_2d: workspace of %zu bytes, need %zu", ws_bytes,
                256 + 2 * sizeof(double));
    hipStream_t st = as_stream(stream);
    double* minmax = (double*)align256_ptr(ws);
    AVL_HIP_CHECK(hipMemsetAsync(d_flags, 0, sizeof(int32_t), st));
    rc = decay_minmax_reset(minmax, st);
    if (rc != AVL_OK) return rc;
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(travel_decay_kernel, dim3(stride_blocks(n)), dim3(256), 0, st, d_straight, d_diagonal, n, cell_size, decay_rate,
                       d_out_f64, reinterpret_cast<unsigned long long*>(minmax));
    AVL_HIP_CHECK(hipGetLastError());
    if (!normalize) return AVL_OK;
    return decay_normalize(d_out_f64, minmax, n, d_flags, st);
}

}  // extern "C"
