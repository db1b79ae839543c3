// Cost-weighted travel field on a 2-D obstacle map for gfx950, and the layered costmap that prices its cells.
//
// Upstream has no counterpart: its only answer to "keep away from walls" is to dilate the obstacle map by a fixed number of cells
// (avlmaps/map/map.py, Map._dilate_map), which closes narrow doors instead of making them expensive.  This file is the weighted
// sibling of avl_travel.hip: the same tile scheme, workspace and host loop (avl_travel_tile.h), with one more operand, the price
// of the cell a step enters.
//
// Definition.  free, sources, cost (H, W) uint8, each with its own row length.  A cell is passable when
// free != 0 && cost != 0: price 0 on a free cell means lethal.  The legal-step rule is 4.26's with "passable" in place of "free",
// the no-corner-cutting test on the two edge-sharing cells included; a source may lie on an impassable cell.  A step u -> v costs
// cost[v], the price of the cell entered: it adds (cost[v], 0) when straight and (0, cost[v]) when diagonal.  The price of a walk
// is A + B * sqrt(2) with A the summed price of its straight steps and B that of its diagonal steps; the field of a cell is the
// pair (A, B) of the cheapest legal walk from any source, (0, 0) on a source, (-1, -1) where no walk ends.  A and B are integers
// and sqrt(2) is irrational, so different pairs differ in price and the minimum is unique.  With cost == 1 everywhere this is
// avl_travel2d's field.
//
// Bounds.  H * W <= 2^22 (kCostMaxCells), on top of the side limit of avl_travel.hip.  Every stored word is the price of a walk
// without repeated cells: a candidate that returned to a cell would be dearer than the word that cell already holds (prices are
// positive), and words only decrease.  Such a walk has fewer than H * W steps of price <= 255 each, so A, B < 2^22 * 2^8 = 2^30:
// the low half of the packed word never carries into the high half, and travel_less stays inside its bounds.
//
// State and work: avl_travel.hip's word and the shared tile body, here the priced variant travel_tile_relax<true, false>.  The only
// new operand of a round is the thread's own four cell prices, held in registers: candidate = neighbour + cost[v] * (diagonal ? 1 :
// 2^32).  No price plane in LDS.  The initialisation folds cost == 0 into the passability byte, so the legal-step rule
// (travel_legal_in<kTravelHalo>) never looks at a price.
//
// Convergence.  avl_travel.hip's argument holds verbatim for positive prices: every stored word is (0, 0) on a source or "a stored
// neighbour + a legal step", so the price of a real legal walk and never below the minimum; words only decrease; a cell whose word
// changes wakes every tile that can read it; when no tile is active every cell equals the minimum over its legal incoming steps,
// the Bellman fixed point, which with strictly positive step prices is the cheapest-walk field.  The optimal pair of a cell whose
// cheapest walk has k steps is in place after at most k rounds, k < H * W: the host gives up after H * W + 1 rounds.
//
// The workspace is avl_travel2d's, travel_layout() itself: the same header, marks, passability bytes and state words; the prices
// are read from the caller's plane.
//
// The costmap (avl_costmap2d) is element-wise: per cell the layers' tables are looked up at the squared distance and summed.
#include <algorithm>
#include <cmath>

#include "avl_common.h"
#include "avl_travel_tile.h"

namespace avl {

constexpr int64_t kCostMaxCells = 1ll << 22;     // H * W: keeps A, B < 2^30, see the head of the file
constexpr int kCostMaxLayers = 8;

// pass = (free && cost != 0) | source << 1 per cell, state = (0, 0) on sources and unreached elsewhere; the tile of every source
// and its eight neighbours start active
__global__ __launch_bounds__(256) void cost_init_kernel(const uint8_t* __restrict__ free_u8, int64_t ld_free,
                                                        const uint8_t* __restrict__ cost_u8, int64_t ld_cost,
                                                        const uint8_t* __restrict__ src_u8, int64_t ld_src, int H, int W,
                                                        uint8_t* __restrict__ pass, unsigned long long* __restrict__ state,
                                                        unsigned* __restrict__ flags, unsigned* __restrict__ hdr) {
    const int tw = travel_tiles(W), th = travel_tiles(H);
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
        const bool passable = free_u8[(int64_t)r * ld_free + c] != 0 && cost_u8[(int64_t)r * ld_cost + c] != 0;
        travel_init_cell(i, r, c, passable, src_u8[(int64_t)r * ld_src + c] != 0, th, tw, pass, state, flags, hdr);
    }
}

// One round: the shared body with the entered cell's price in the candidate.
__global__ __launch_bounds__(kTravelThreads) void cost_round_kernel(const uint8_t* __restrict__ pass, const uint8_t* __restrict__ cost_u8,
                                                                    int64_t ld_cost, unsigned long long* state, int H, int W,
                                                                    unsigned* __restrict__ cur, unsigned* __restrict__ next,
                                                                    unsigned* __restrict__ activated) {
    __shared__ TravelTileLds lds;
    if (!travel_take_mark(cur, &lds.active, &lds.dirty)) return;
    const int tile_r = blockIdx.x / travel_tiles(W), tile_c = blockIdx.x - tile_r * travel_tiles(W);
    travel_tile_relax<true, false>(lds, pass, cost_u8, ld_cost, state, H, W, tile_r, tile_c, 0, next, activated);
}

struct CostLayers {
    avl_cost_layer layer[kCostMaxLayers];
};

// cost = 0 where not free; else per layer t = table[min(d2, n - 1)] with d2 = rint(d * d); any t == 255 -> 0 (lethal), else
// min(254, 1 + sum t).  d2 is exact: avl_edt2d stores the correctly rounded square root d = sqrt(m) (1 + e), |e| <= 2^-53, of an
// integer m <= 2 * 16384^2 = 2^29 < 2^32, so the rounded product d * d lies within m * 3 * 2^-53 < 2^-20 of m and rint() returns m.
// The product stands alone (the file is compiled with -ffp-contract=off).  !(x < n - 1) also sends a NaN to the last entry: the
// index is inside the table whatever the plane holds.
__global__ __launch_bounds__(256) void costmap_kernel(const uint8_t* __restrict__ free_u8, int64_t ld_free, int H, int W, CostLayers layers,
                                                      int n_layers, uint8_t* __restrict__ out) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
        unsigned v = 0;
        if (free_u8[(int64_t)r * ld_free + c] != 0) {
            unsigned sum = 1;
            bool lethal = false;
            for (int l = 0; l < n_layers; ++l) {
                const double d = layers.layer[l].d_distance[i];
                const double x = d * d;
                const int64_t last = (int64_t)layers.layer[l].n_table - 1;
                const int64_t d2 = !(x < (double)last) ? last : std::max<int64_t>((int64_t)rint(x), 0);
                const unsigned t = layers.layer[l].d_table[d2];
                lethal = lethal || t == 255u;
                sum += t;
            }
            v = lethal ? 0u : (sum < 254u ? sum : 254u);
        }
        out[i] = (uint8_t)v;
    }
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_costfield2d(const uint8_t* d_free, int64_t ld_free, const uint8_t* d_cost, int64_t ld_cost, const uint8_t* d_sources,
                    int64_t ld_src, int H, int W, int32_t* d_straight, int32_t* d_diagonal, int64_t* d_stats, void* ws, size_t ws_bytes,
                    void* stream) {
    int rc = travel_check_shape("avl_costfield2d", H, W);
    if (rc != AVL_OK) return rc;
    const int64_t n = (int64_t)H * W;
    AVL_REQUIRE(n <= kCostMaxCells, "avl_costfield2d: %d x %d = %lld cells, at most 2^22 (the sums of prices must stay below 2^30)", H, W,
                (long long)n);
    AVL_REQUIRE(d_free && d_cost && d_sources, "avl_costfield2d: null free, cost or source image");
    AVL_REQUIRE(d_straight && d_diagonal && d_stats, "avl_costfield2d: null output plane or stats pointer");
    AVL_REQUIRE(ld_free >= W, "avl_costfield2d: free rows of %lld cells cannot hold %d columns", (long long)ld_free, W);
    AVL_REQUIRE(ld_cost >= W, "avl_costfield2d: cost rows of %lld cells cannot hold %d columns", (long long)ld_cost, W);
    AVL_REQUIRE(ld_src >= W, "avl_costfield2d: source rows of %lld cells cannot hold %d columns", (long long)ld_src, W);
    const TravelLayout l = travel_layout(H, W);
    AVL_REQUIRE(ws && ws_bytes >= l.total, "avl_costfield2d: workspace of %zu bytes, need %zu", ws_bytes, l.total);
    hipStream_t st = as_stream(stream);
    char* base = (char*)align256_ptr(ws);
    unsigned* hdr = (unsigned*)(base + l.hdr);
    unsigned* flags = (unsigned*)(base + l.flags);
    uint8_t* pass = (uint8_t*)(base + l.pass);
    unsigned long long* state = (unsigned long long*)(base + l.state);
    const unsigned tiles = (unsigned)(travel_tiles(W) * travel_tiles(H));

    AVL_HIP_CHECK(hipMemsetAsync(hdr, 0, l.pass - l.hdr, st));              // the header and both mark buffers
    AVL_HIP_CHECK(hipMemsetAsync(d_stats, 0, 4 * sizeof(int64_t), st));
    hipLaunchKernelGGL(cost_init_kernel, dim3(stride_blocks(n)), dim3(256), 0, st, d_free, ld_free, d_cost, ld_cost, d_sources, ld_src, H,
                       W, pass, state, flags, hdr);
    AVL_HIP_CHECK(hipGetLastError());

    // a cheapest walk has fewer than H * W steps and every round moves every pending walk on by a step or more
    const int64_t max_rounds = n + 1;
    int64_t rounds = 0, tile_runs = 0;
    unsigned host[kTravelHdrWords];
    rc = travel_run_rounds(
        "avl_costfield2d", max_rounds, hdr, flags, tiles, st,
        [&](int64_t, unsigned* cur, unsigned* next, unsigned* activated) {
            hipLaunchKernelGGL(cost_round_kernel, dim3(tiles), dim3(kTravelThreads), 0, st, (const uint8_t*)pass, d_cost, ld_cost, state, H, W,
                               cur, next, activated);
        },
        &rounds, &tile_runs, host);
    if (rc != AVL_OK) return rc;
    return travel_unpack(state, n, d_straight, d_diagonal, rounds, tile_runs, host[kTravelHdrAny] != 0, d_stats, st);
}

int avl_costmap2d(const uint8_t* d_free, int64_t ld_free, int H, int W, const avl_cost_layer* h_layers, int n_layers, uint8_t* d_cost_out,
                  void* stream) {
    int rc = travel_check_shape("avl_costmap2d", H, W);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_free && d_cost_out, "avl_costmap2d: null free image or output");
    AVL_REQUIRE(ld_free >= W, "avl_costmap2d: free rows of %lld cells cannot hold %d columns", (long long)ld_free, W);
    AVL_REQUIRE(n_layers >= 0 && n_layers <= kCostMaxLayers, "avl_costmap2d: %d layers (0 .. %d)", n_layers, kCostMaxLayers);
    AVL_REQUIRE(n_layers == 0 || h_layers, "avl_costmap2d: null layer array");
    CostLayers layers = {};
    for (int l = 0; l < n_layers; ++l) {
        AVL_REQUIRE(h_layers[l].d_distance && h_layers[l].d_table, "avl_costmap2d: layer %d has a null distance plane or table", l);
        AVL_REQUIRE(h_layers[l].n_table >= 1, "avl_costmap2d: layer %d has a table of %d entries (at least 1)", l, (int)h_layers[l].n_table);
        layers.layer[l] = h_layers[l];
    }
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(costmap_kernel, dim3(stride_blocks(n)), dim3(256), 0, as_stream(stream), d_free, ld_free, H, W, layers, n_layers,
                       d_cost_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
