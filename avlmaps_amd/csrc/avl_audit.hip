// The visibility audit of a voxel map for gfx950: for every voxel the last frame whose depth rays ended in it, and how many rays of
// later frames passed through its cell on their way to something further away.  The 3-D half of the free-space carver
// (avl_explore.hip): the same rays, walked through (row, col, height) cells and probed against the map's voxel list.
//
// Upstream has no counterpart: its maps are static (avlmaps/map/vlmap.py only ever loads what the builder wrote).  Everything
// below is this project's own definition, written out in DESIGN.md 4.21; every output is an integer maximum or an integer sum, so a
// scalar restatement (tests/_audit_ref.py) is compared with np.array_equal.
//
// THE CELL INDEX.  A lookup from cell (row, col, h) of a gs x gs x vh grid to the voxel row that owns it, in one caller-owned
// buffer laid out by ci_layout() (avl_cellindex.h, with the probe; avl_sight.hip reads the same index):
//   bits    one bit per cell, uint32 words, linear cell (row * gs + col) * vh + h; set with atomicOr
//   prefix  per word, the number of set bits in the words before it (count per 1024 words, avl_scan.h's scan_counts_kernel over the
//           counts, one more pass that writes the words' own exclusive prefix)
//   perm    perm[rank] = the voxel row of the rank-th set bit; several rows of one cell fold with atomicMax: the largest row owns it
//   counts  the per-block counts of the scan
// 4 bytes per 32 cells twice over plus 4 bytes per voxel: 15.5 MB at gs = 1000, vh = 30 and 2 M voxels, where a dense int32 id
// grid is 120 MB.  A probe is one bit test; on a set bit rank = prefix[w] + popc(word & below) and the row is perm[rank].  Rows
// outside the grid set no bit: no probe finds them.
//
// ONE RAY.  Steps 1 - 8 are the sight ray of avl_sightray.h, the carver's: the pixel lattice, the depth, bp_backproject, validity,
// far / hit, bp_transform, the height slab with its t0 and t1, the end points A = X(t0) and B = X(t1) in all three coordinates
// (X(0) = O, X(1) = P exactly) and the finiteness of their x and y.  Then
//    9  the cell of a point: row and col as the carver's (ray_cell_rc), hu = int(z / cs) truncating, h = min(max(hu, 0), vh - 1);
//       a = cell(A), b = cell(B)
//   10  also skipped whole: the z of A or B not finite; a outside [0, gs)^2; |b.row| or |b.col| above 2^28
//   11  has_end = !far && t1 == 1;  is_hit = has_end && 0 <= hu(P) < vh && b inside [0, gs)^2  (the builder's in-range rule)
//   12  the walk: d = |b - a| per axis, s the signs, n = max(d); cells k = 0 .. n; between two cells every axis x with error
//       e_x (starting at 2 d_x - n) does `if e_x > 0: x += s_x, e_x -= 2 n`, then `e_x += 2 d_x`.  DESIGN states this with a driving
//       axis that always steps; an axis with d_x == n has e_x == n > 0 before every step and -n + 2 n after it, so the one rule
//       steps it every time and the kernel needs no per-axis case (the steps of one move commute: the cell is their sum).  The
//       walk stops at the first cell outside [0, gs)^2; h cannot leave [0, vh).
//   13  a visit of a cell that voxel i owns:  k == n && is_hit: last_hit[i] = max(last_hit[i], id).  !has_end, or has_end and
//       k < n - end_margin: through[i] += 1, unless `after` is given and id <= after[i].
// Both folds commute: rays, frames, launches and calls may come in any order and continue each other.
//
// Launch shape: the carver's.  A thread owns a ray, lanes run along an image row, blockIdx.y is the frame, up to kRayFrames poses
// travel in the kernel arguments, nothing is allocated per call.  The through-add is pre-aggregated once per wave (audit_add: the
// lanes on the first adding lane's voxel share one atomic, 2.15 -> 0.85 ms for pass B of 64 frames); last_hit is
// read first and the atomicMax issued only when it would change it.
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_cellindex.h"
#include "avl_scan.h"
#include "avl_sightray.h"

namespace avl {

constexpr int kAuditThreads = 256;
constexpr int kAuditMaxCell = 1 << 28;          // |b.row|, |b.col|: 2 d and 2 n stay inside int32

__global__ __launch_bounds__(256) void ci_set_kernel(const int32_t* __restrict__ pos, int64_t N, int gs, int vh, uint32_t* __restrict__ bits) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const int64_t lin = ci_linear(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], gs, vh);
        if (lin >= 0) atomicOr(bits + (lin >> 5), 1u << (lin & 31));
    }
}

// a thread's kCiPer consecutive words: their popcounts summed, the block's exclusive scan of the sums
__device__ __forceinline__ int ci_block_scan(const uint32_t* __restrict__ bits, int64_t nwords, int* lds, int64_t* w0, int* total) {
    *w0 = (int64_t)blockIdx.x * (kCiThreads * kCiPer) + threadIdx.x * kCiPer;
    int s = 0;
#pragma unroll
    for (int k = 0; k < kCiPer; ++k)
        if (*w0 + k < nwords) s += __popc(bits[*w0 + k]);
    return block_excl_scan<kCiThreads / kWave>(s, OpSum{}, 0, lds, total);
}

__global__ __launch_bounds__(kCiThreads) void ci_count_kernel(const uint32_t* __restrict__ bits, int64_t nwords, int32_t* __restrict__ counts) {
    __shared__ int s_w[kCiThreads / kWave];
    int64_t w0;
    int total;
    ci_block_scan(bits, nwords, s_w, &w0, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kCiThreads) void ci_prefix_kernel(const uint32_t* __restrict__ bits, int64_t nwords, const int32_t* __restrict__ offsets,
                                                               int32_t* __restrict__ prefix) {
    __shared__ int s_w[kCiThreads / kWave];
    int64_t w0;
    int total;
    int run = offsets[blockIdx.x] + ci_block_scan(bits, nwords, s_w, &w0, &total);
#pragma unroll
    for (int k = 0; k < kCiPer; ++k)
        if (w0 + k < nwords) {
            prefix[w0 + k] = run;
            run += __popc(bits[w0 + k]);
        }
}

__global__ __launch_bounds__(256) void ci_perm_kernel(const int32_t* __restrict__ pos, int64_t N, int gs, int vh, const uint32_t* __restrict__ bits,
                                                      const int32_t* __restrict__ prefix, int32_t* __restrict__ perm) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const int64_t lin = ci_linear(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], gs, vh);
        if (lin < 0) continue;
        const uint32_t w = bits[lin >> 5], b = (uint32_t)lin & 31u;
        atomicMax(perm + prefix[lin >> 5] + __popc(w & ((1u << b) - 1u)), (int32_t)i);        // the largest row of a cell owns it
    }
}

__global__ __launch_bounds__(256) void ci_lookup_kernel(const int32_t* __restrict__ cells, int64_t M, int gs, int vh, const uint32_t* __restrict__ bits,
                                                        const int32_t* __restrict__ prefix, const int32_t* __restrict__ perm, int32_t* __restrict__ out) {
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
        const int64_t lin = ci_linear(cells[3 * m], cells[3 * m + 1], cells[3 * m + 2], gs, vh);
        out[m] = lin < 0 ? -1 : ci_probe(bits, prefix, perm, (int)lin);
    }
}

__device__ __forceinline__ void audit_add(unsigned* __restrict__ through, int i) {
#ifdef AVL_AUDIT_PLAIN_ADD
    atomicAdd(through + i, 1u);     // the B side of tools/probe_audit.py's A/B (tools/build_variant.py), never in the shipped library
#else
    // The lanes that add to the voxel of the wave's first adding lane share one atomic -- near the camera neighbouring rays all
    // cross the same few voxels -- and every other lane adds for itself: one round, no loop over the wave's distinct voxels, which
    // far from the camera are as many as its lanes.  The same integer either way.  Called from divergent code: the builtin and the
    // ballot see the lanes that are adding in this step
    const int lead = __builtin_amdgcn_readfirstlane(i);
    const unsigned long long same = __ballot(i == lead);
    if (i != lead) atomicAdd(through + i, 1u);
    else if ((same & ((1ull << (threadIdx.x & (kWave - 1))) - 1ull)) == 0) atomicAdd(through + lead, (unsigned)__popcll(same));
#endif
}

struct AuditParams {
    RayParams ray;
    int vh, end_margin;
    const uint32_t* bits;
    const int32_t* prefix;
    const int32_t* perm;
};

__global__ __launch_bounds__(kAuditThreads) void audit_kernel(AuditParams p, RayBatch batch, const void* __restrict__ depth,
                                                             int32_t* __restrict__ last_hit, unsigned* __restrict__ through,
                                                             const int32_t* __restrict__ after) {
    const RayFrame& fr = batch.f[blockIdx.y];
    const int id = fr.id;
    const int ray = blockIdx.x * kAuditThreads + threadIdx.x;
    if (ray >= p.ray.nv * p.ray.nu) return;
    SightRay s;
    ray_origin(fr, s);
    size_t pix;
    double p0, p1, p2;
    ray_pixel(p.ray, depth, ray, blockIdx.y, pix, p0, p1, p2);                  // (1 - 2)
    if (!(sight_ray(p.ray, fr, p0, p1, p2, s) && isfinite(s.az) && isfinite(s.bz))) return;       // (3 - 8)
    int r = ray_cell_rc(p.ray, s.ax), c = ray_cell_rc(p.ray, s.ay);             // (9)
    int h = min(max(py_int(s.az / p.ray.cs), 0), p.vh - 1);
    const int br = ray_cell_rc(p.ray, s.bx), bc = ray_cell_rc(p.ray, s.by);
    const int bhu = py_int(s.bz / p.ray.cs), bh = min(max(bhu, 0), p.vh - 1);
    const int gs = p.ray.gs;
    if (!(r >= 0 && r < gs && c >= 0 && c < gs)) return;                        // (10)
    if (br > kAuditMaxCell || br < -kAuditMaxCell || bc > kAuditMaxCell || bc < -kAuditMaxCell) return;
    const bool has_end = !s.far && s.ends;                                      // (11)
    const bool is_hit = has_end && bhu >= 0 && bhu < p.vh && br >= 0 && br < gs && bc >= 0 && bc < gs;
    const int dr = abs(br - r), dc = abs(bc - c), dh = abs(bh - h);             // (12)
    const int sr = br > r ? 1 : -1, sc = bc > c ? 1 : -1, sh = bh > h ? 1 : -1;
    const int n = max(dr, max(dc, dh));
    int er = 2 * dr - n, ec = 2 * dc - n, eh = 2 * dh - n;
    const int through_below = has_end ? n - p.end_margin : INT_MAX;            // k < this counts as through (k <= n < INT_MAX)
    for (int k = 0; k <= n; ++k) {
        if (!(r >= 0 && r < gs && c >= 0 && c < gs)) break;
        const int i = ci_probe(p.bits, p.prefix, p.perm, (r * gs + c) * p.vh + h);
        if (i >= 0) {                                                           // (13)
            if (last_hit && k == n && is_hit) {
                if (id > __hip_atomic_load(last_hit + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(last_hit + i, id);
            }
            if (through && k < through_below && (!after || id > after[i])) audit_add(through, i);
        }
        if (er > 0) {
            r += sr;
            er -= 2 * n;
        }
        er += 2 * dr;
        if (ec > 0) {
            c += sc;
            ec -= 2 * n;
        }
        ec += 2 * dc;
        if (eh > 0) {
            h += sh;
            eh -= 2 * n;
        }
        eh += 2 * dh;
    }
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_cell_index_work_bytes(int64_t N, int gs, int vh, size_t* bytes) {
    AVL_REQUIRE(bytes, "avl_cell_index_work_bytes: null output");
    const int rc = ci_check_grid("avl_cell_index_work_bytes", N, gs, vh);
    if (rc != AVL_OK) return rc;
    *bytes = ci_layout(nullptr, N, gs, vh).total;
    return AVL_OK;
}

int avl_cell_index_build(const int32_t* d_grid_pos, int64_t N, int gs, int vh, void* d_index, size_t index_bytes, void* stream) {
    const int rc = ci_check_grid("avl_cell_index_build", N, gs, vh);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(d_index && (d_grid_pos || N == 0), "avl_cell_index_build: null pointer");
    const CellIndexView v = ci_layout(d_index, N, gs, vh);
    AVL_REQUIRE(index_bytes >= v.total, "avl_cell_index_build: the index buffer has %zu bytes, needs %zu", index_bytes, v.total);
    hipStream_t st = as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(v.bits, 0, (size_t)v.nwords * 4, st));
    AVL_HIP_CHECK(hipMemsetAsync(v.perm, 0xFF, (size_t)std::max<int64_t>(N, 1) * 4, st));          // -1 below every row: atomicMax's identity
    if (N) hipLaunchKernelGGL(ci_set_kernel, dim3(stride_blocks(N)), dim3(256), 0, st, d_grid_pos, N, gs, vh, v.bits);
    hipLaunchKernelGGL(ci_count_kernel, dim3((unsigned)v.nblocks), dim3(kCiThreads), 0, st, (const uint32_t*)v.bits, v.nwords, v.counts);
    hipLaunchKernelGGL((scan_counts_kernel<1024, int, int, OpSum>), dim3(1), dim3(1024), 0, st, (const int*)v.counts, v.nblocks, v.counts,
                       (int*)nullptr, OpSum{}, 0);
    hipLaunchKernelGGL(ci_prefix_kernel, dim3((unsigned)v.nblocks), dim3(kCiThreads), 0, st, (const uint32_t*)v.bits, v.nwords, (const int32_t*)v.counts,
                       v.prefix);
    if (N)
        hipLaunchKernelGGL(ci_perm_kernel, dim3(stride_blocks(N)), dim3(256), 0, st, d_grid_pos, N, gs, vh, (const uint32_t*)v.bits,
                           (const int32_t*)v.prefix, v.perm);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_cell_index_lookup(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const int32_t* d_cells, int64_t M, int32_t* d_out,
                          void* stream) {
    const int rc = ci_check_grid("avl_cell_index_lookup", N, gs, vh);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(M >= 0 && M < INT_MAX, "avl_cell_index_lookup: %lld cells (0 .. 2^31 - 2)", (long long)M);
    AVL_REQUIRE(d_index, "avl_cell_index_lookup: null index");
    const CellIndexView v = ci_layout(const_cast<void*>(d_index), N, gs, vh);
    AVL_REQUIRE(index_bytes >= v.total, "avl_cell_index_lookup: the index buffer has %zu bytes, needs %zu", index_bytes, v.total);
    if (M == 0) return AVL_OK;
    AVL_REQUIRE(d_cells && d_out, "avl_cell_index_lookup: null pointer");
    hipLaunchKernelGGL(ci_lookup_kernel, dim3(stride_blocks(M)), dim3(256), 0, as_stream(stream), d_cells, M, gs, vh, (const uint32_t*)v.bits,
                       (const int32_t*)v.prefix, (const int32_t*)v.perm, d_out);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_audit_rays(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const void* d_depth, int depth_is_u16, double depth_div,
                   int F, int H, int W, const double* h_calib_inv, const double* h_transforms, const int32_t* h_frame_ids, double cs, int stride,
                   double h_min, double h_max, double min_depth, double max_depth, int end_margin, int32_t* d_last_hit, uint32_t* d_through,
                   const int32_t* d_after, void* stream) {
    int rc = ci_check_grid("avl_audit_rays", N, gs, vh);
    if (rc != AVL_OK) return rc;
    const double h_band[2] = {h_min, h_max};
    AuditParams p{};
    rc = ray_params("avl_audit_rays", depth_is_u16, depth_div, F, H, W, h_calib_inv, gs, 0, cs, stride, h_band, min_depth, max_depth, &p.ray);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(end_margin >= 0, "avl_audit_rays: end_margin %d < 0", end_margin);
    AVL_REQUIRE(d_index, "avl_audit_rays: null index");
    const CellIndexView v = ci_layout(const_cast<void*>(d_index), N, gs, vh);
    AVL_REQUIRE(index_bytes >= v.total, "avl_audit_rays: the index buffer has %zu bytes, needs %zu", index_bytes, v.total);
    if (F == 0 || (!d_last_hit && !d_through)) return AVL_OK;
    AVL_REQUIRE(d_depth && h_calib_inv && h_transforms && h_frame_ids, "avl_audit_rays: null pointer");
    if ((rc = ray_frame_ids("avl_audit_rays", h_frame_ids, F)) != AVL_OK) return rc;
    p.vh = vh;
    p.end_margin = end_margin;
    p.bits = v.bits;
    p.prefix = v.prefix;
    p.perm = v.perm;
    const int rays = p.ray.nv * p.ray.nu;
    if (rays == 0) return AVL_OK;
    const unsigned blocks = (unsigned)((rays + kAuditThreads - 1) / kAuditThreads);
    const size_t frame_bytes = (size_t)H * W * (depth_is_u16 ? sizeof(uint16_t) : sizeof(float));
    hipStream_t st = as_stream(stream);
    ray_launches(F, h_transforms, h_frame_ids, [&](const RayBatch& b, int n, int f0) {
        hipLaunchKernelGGL(audit_kernel, dim3(blocks, (unsigned)n), dim3(kAuditThreads), 0, st, p, b,
                           (const void*)((const char*)d_depth + (size_t)f0 * frame_bytes), d_last_hit, (unsigned*)d_through, d_after);
    });
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

}  // extern "C"
