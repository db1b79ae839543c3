// The cell index of a voxel list, shared by the sources that probe it (avl_audit.hip builds it and walks depth rays through it,
// avl_sight.hip walks cell-to-cell sight lines through it): the ONE layout of the index buffer, the linear cell and the probe.
// The index itself is described at the top of avl_audit.hip (THE CELL INDEX) and in DESIGN.md 4.21.
#pragma once
#include <algorithm>
#include <climits>

#include "avl_common.h"

namespace avl {

constexpr int kCiMaxSide = 16384;               // gs, as the carver's
constexpr int kCiThreads = 256;
constexpr int kCiPer = 4;                       // words per thread of the prefix passes: a block owns 1024 words

struct CellIndexView {
    uint32_t* bits;
    int32_t* prefix;
    int32_t* perm;
    int32_t* counts;
    int64_t nwords, nblocks;
    size_t total;
};

// the ONE layout of the index buffer (the size query passes a null base)
static CellIndexView ci_layout(void* base, int64_t N, int gs, int vh) {
    CellIndexView v{};
    const int64_t cells = (int64_t)gs * gs * vh;
    v.nwords = (cells + 31) / 32;
    v.nblocks = (v.nwords + kCiThreads * kCiPer - 1) / (kCiThreads * kCiPer);
    Carver c(base ? align256_ptr(base) : nullptr);
    v.bits = c.ptr<uint32_t>((size_t)v.nwords * 4);
    v.prefix = c.ptr<int32_t>((size_t)v.nwords * 4);
    v.perm = c.ptr<int32_t>((size_t)std::max<int64_t>(N, 1) * 4);
    v.counts = c.ptr<int32_t>((size_t)v.nblocks * 4);
    v.total = c.total() + 256;                  // the slack of a base that is not 256-aligned
    return v;
}

__device__ __forceinline__ int64_t ci_linear(int r, int c, int h, int gs, int vh) {
    const bool in = r >= 0 && r < gs && c >= 0 && c < gs && h >= 0 && h < vh;
    return in ? ((int64_t)r * gs + c) * vh + h : -1;    // < 2^31 (checked by the entry points)
}

// the voxel row that owns linear cell `lin` (inside the grid), -1 when it is empty
__device__ __forceinline__ int ci_probe(const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix,
                                        const int32_t* __restrict__ perm, int lin) {
    const uint32_t w = bits[lin >> 5], b = (uint32_t)lin & 31u;
    if (!(w >> b & 1u)) return -1;
    return perm[prefix[lin >> 5] + __popc(w & ((1u << b) - 1u))];
}

// the limits of the layout: every entry point that takes an index checks them first
static int ci_check_grid(const char* who, int64_t N, int gs, int vh) {
    AVL_REQUIRE(N >= 0 && N < INT_MAX, "%s: %lld voxels (0 .. 2^31 - 2)", who, (long long)N);
    AVL_REQUIRE(gs >= 1 && gs <= kCiMaxSide && vh >= 1 && (int64_t)gs * gs * vh < INT_MAX, "%s: grid %d x %d x %d (gs 1 .. %d, vh >= 1, gs * gs * vh < 2^31)",
                who, gs, gs, vh, kCiMaxSide);
    return AVL_OK;
}

}  // namespace avl
