// Ground-truth label map for gfx950: per-voxel class votes from the semantic frames of a scene, the majority label of every voxel,
// the label-valued top-down pool and the confusion matrix a VLMap is scored with.
//
// Stands in for (upstream reference, path:line):
//   avlmaps/dataloader/habitat_dataloader.py:85-107   get_obstacles_cropped_no_floor, get_gt_semantic_cropped: read a gt_cropped
//                                                     nothing upstream ever sets ("TODO: implement loading GT map option", :85)
//   avlmaps/map/gtmap.py:18-30,41-71                  GTMap loads a grid_gt_1.npy no program of the tree writes
//   avlmaps/utils/visualize_utils.py:77-83            pool_3d_label_to_2d, for ONE boolean mask
// Upstream has NO vote pass to mirror: dataset/README.md:78 says the semantic frames "can be used for creating a GT semantic map"
// and stops there.  The definition below is this project's own, written so that every output is an integer with one value: a
// scalar restatement (tests/_gtmap_ref.py) is compared with np.array_equal.
//
// avl_gt_vote, per pixel of the lattice stride / 2, stride / 2 + stride, ... in both image directions, in this order (float64,
// unfused: the file is compiled with -ffp-contract=off, the only fma() are bp_backproject's and bp_transform's, K1's own code):
//    1  z = depth[v, u] (float32 metres, or uint16 / depth_div); p = bp_backproject(Kinv, u + 0.5, v + 0.5, z) (avl_sightray.h's
//       ray_pixel, the carver's and the audit's); dropped unless
//       p.z > min_depth && p.z < max_depth                          (the builder's rule, oracle/avl_oracle.c:63; drops NaN and inf)
//    2  g = bp_transform(T, p); row = int(gs / 2 - int(g.x / cs)), col = int(gs / 2 - int(g.y / cs)), h = int(g.z / cs), all
//       truncating toward zero (base_pos2grid_id_3d); dropped outside [0, gs) x [0, gs) x [0, vh)       1 - 2 count in stats[0]
//    3  o = semantic[v, u]; with a table: dropped when o < 0 || o >= n_obj, else c = obj2cls[o]; without: c = o; dropped when
//       c < 0 || c >= C                                                                                  counts in stats[1]
//    4  r = occupied_ids[row, col, h]; dropped when r < 0: the map has no such voxel (the builder samples pixels, this pass does
//       not)                                                                                             counts in stats[2]
//       r >= N sets bit 0 of the error flag and the pixel is dropped (counted nowhere)
//    5  votes[r * C + c] += 1                                                                            counts in stats[3]
// The class is looked up before the voxel, so an unlabelled pixel never reads the voxel index (120 MB at gs = 1000, vh = 30).
// Counters are uint32: a voxel needs more than 4.29e9 pixel hits to wrap (2 M frames of 720 x 1080 that all look at one voxel);
// not guarded.  Every fold is an integer sum: nothing depends on the order of pixels, frames, launches or calls.
//
// Launch shape (the carver's, avl_explore.hip): a thread owns a pixel, lanes run along an image row, blockIdx.y is the frame, the
// pose is wave-uniform and comes from the kernel arguments (up to kRayFrames frames per launch; a longer batch takes several
// launches).  A block walks tiles of 256 pixels in a grid-stride loop (about 8 blocks per CU over the launch's frames).  The vote is
// one vector atomic whose result is not used.  The four statistics are counted per wave with ballots (scalar adds, once per tile),
// per block in LDS, and added with one 64-bit atomic per block and non-zero count: every block of every frame adds to the same four
// words, and with one atomic per WAVE those four words set the kernel's time (0.25 ms per 720 x 1080 frame).  Lanes
// of a wave that hit the same vote counter are NOT combined first.
//
// avl_gt_labels: a group of G lanes owns a row of votes; lane l reads classes l, l + G, ... (ascending, so its own best is its lowest
// class at its maximum), then log2(G) xor-shuffle steps fold (max, lowest class at max, sum).  G = the smallest power of two >= C,
// at most 16, for C <= 64: C = 40 gives G = 16, three loads per lane, a wave reads 4 rows = 640 contiguous bytes; C > 64: G = 64,
// one wave per row, 256 contiguous bytes per load.  Every byte of the votes is read once.
//
// avl_pool_labels_2d: a thread owns a cell of the window and walks its column from vh - 1 down; consecutive lanes take
// consecutive columns (vh-strided reads of the index: its layout).  A gather, no atomics.
//
// avl_label_confusion: Cg * Cp <= kConfLdsCounters: a block counts its contiguous share of the pairs (fewer than 2^32) in private
// uint32 LDS counters and flushes every non-zero one with a 64-bit global atomic; above: 64-bit global atomics directly.
#include <algorithm>
#include <climits>
#include <cmath>

#include "avl_sightray.h"
#include "avl_wave.h"

namespace avl {

constexpr int kVoteThreads = 256;
constexpr int kVoteBlocksPerCu = 8;             // blocks of a launch per CU, all frames together
constexpr int kGtMaxSide = 16384;               // gs
constexpr int kGtMaxClasses = 4096;             // C of avl_gt_vote / avl_gt_labels
constexpr int64_t kGtMaxVotes = (int64_t)1 << 40;      // N * C, and gs * gs * vh
constexpr int kConfLdsCounters = 16384;         // 64 KB of uint32 counters per block
constexpr int kConfMaxClasses = 65536;
constexpr int64_t kConfMaxCounters = (int64_t)1 << 28;
constexpr int64_t kConfBlockItems = (int64_t)1 << 30;  // a block's LDS counters are uint32: it takes fewer than 2^32 pairs

struct VoteParams {
    RayParams ray;
    long long n_voxels;
    int vh, n_obj, n_classes;
};

// (the poses travel as avl_sightray.h's RayBatch, 16 * 104 bytes of kernel arguments: 8 more per frame than the 96 of a bare pose,
// for a frame id that the vote does not read)
__global__ __launch_bounds__(kVoteThreads) void gt_vote_kernel(VoteParams p, RayBatch batch, const void* __restrict__ depth,
                                                               const int32_t* __restrict__ semantic, const int32_t* __restrict__ obj2cls,
                                                               const int32_t* __restrict__ occupied, uint32_t* __restrict__ votes,
                                                               unsigned long long* __restrict__ stats, int* __restrict__ err_flag) {
    __shared__ unsigned block_counts[4];
    if (threadIdx.x < 4) block_counts[threadIdx.x] = 0;
    __syncthreads();
    const double* T = batch.f[blockIdx.y].t;
    const int pixels = p.ray.nv * p.ray.nu, tiles = (pixels + kVoteThreads - 1) / kVoteThreads;
    unsigned n0 = 0, n1 = 0, n2 = 0, n3 = 0;                                   // wave-uniform: what this wave's pixels came to
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {              // (block-uniform trip count: the ballots below see whole waves)
        const int pixel = tile * kVoteThreads + threadIdx.x;
        int outcome = -1;                                                       // 0 .. 3: the statistic this pixel counts in
        if (pixel < pixels) {
            size_t pix;
            double p0, p1, p2;
            ray_pixel(p.ray, depth, pixel, blockIdx.y, pix, p0, p1, p2);
            outcome = 0;
            if (p2 > p.ray.min_depth && p2 < p.ray.max_depth) {                 // (1)
                double g0, g1, g2;
                bp_transform(T, p0, p1, p2, g0, g1, g2);                        // (2)
                const int row = ray_cell_rc(p.ray, g0), col = ray_cell_rc(p.ray, g1);
                const int h = py_int(g2 / p.ray.cs);
                if (row >= 0 && row < p.ray.gs && col >= 0 && col < p.ray.gs && h >= 0 && h < p.vh) {
                    outcome = 1;
                    int c = semantic[pix];                                      // (3)
                    if (obj2cls) c = (c >= 0 && c < p.n_obj) ? obj2cls[c] : -1;
                    if (c >= 0 && c < p.n_classes) {
                        outcome = 2;
                        const int r = occupied[((size_t)row * p.ray.gs + col) * p.vh + h];  // (4)
                        if (r >= p.n_voxels) {
                            outcome = -1;
                            if (err_flag) atomicOr(err_flag, 1);
                        } else if (r >= 0) {
                            outcome = 3;
                            atomicAdd(votes + (size_t)r * p.n_classes + c, 1u);     // (5)
                        }
                    }
                }
            }
        }
        n0 += (unsigned)__popcll(__ballot(outcome == 0));
        n1 += (unsigned)__popcll(__ballot(outcome == 1));
        n2 += (unsigned)__popcll(__ballot(outcome == 2));
        n3 += (unsigned)__popcll(__ballot(outcome == 3));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {                                     // wave -> block in LDS, block -> one 64-bit atomic per non-zero count
        if (n0) atomicAdd(block_counts + 0, n0);
        if (n1) atomicAdd(block_counts + 1, n1);
        if (n2) atomicAdd(block_counts + 2, n2);
        if (n3) atomicAdd(block_counts + 3, n3);
    }
    __syncthreads();
    if (threadIdx.x < 4 && block_counts[threadIdx.x]) atomicAdd(stats + threadIdx.x, (unsigned long long)block_counts[threadIdx.x]);
}

__global__ __launch_bounds__(256) void gt_labels_kernel(const uint32_t* __restrict__ votes, long long N, int C, int G,
                                                        int32_t* __restrict__ label, uint32_t* __restrict__ support) {
    const int lane = threadIdx.x & (G - 1);
    const int rows_per_block = 256 / G;
    for (long long row0 = (long long)blockIdx.x * rows_per_block; row0 < N; row0 += (long long)gridDim.x * rows_per_block) {
        const long long row = row0 + threadIdx.x / G;                           // (a wave's rows are all inside or it has lanes that idle)
        uint32_t best = 0, sum = 0;
        int best_c = INT_MAX;
        if (row < N) {
            const uint32_t* v = votes + (size_t)row * C;
            for (int c = lane; c < C; c += G) {
                const uint32_t x = v[c];
                sum += x;
                if (x > best || best_c == INT_MAX) {
                    best = x;
                    best_c = c;
                }
            }
        }
        for (int m = G >> 1; m > 0; m >>= 1) {                                  // (xor with m < G stays inside the aligned group)
            const uint32_t ob = (uint32_t)__shfl_xor((int)best, m, kWave), os = (uint32_t)__shfl_xor((int)sum, m, kWave);
            const int oc = __shfl_xor(best_c, m, kWave);
            sum += os;
            if (ob > best || (ob == best && oc < best_c)) {
                best = ob;
                best_c = oc;
            }
        }
        if (row < N && lane == 0) {
            label[row] = best == 0 ? -1 : best_c;
            support[row] = sum;
        }
    }
}

__global__ __launch_bounds__(256) void pool_labels_kernel(const int32_t* __restrict__ label, long long N, const int32_t* __restrict__ occupied,
                                                          int gs, int vh, int r0, int c0, int Hw, int Ww, int32_t* __restrict__ out,
                                                          int* __restrict__ err_flag) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= Hw || c >= Ww) return;
    const int32_t* col = occupied + ((size_t)(r0 + r) * gs + (c0 + c)) * vh;
    int res = -1;
    for (int h = vh - 1; h >= 0; --h) {
        const int id = col[h];
        if (id < 0) continue;
        if (id >= N) {
            if (err_flag) atomicOr(err_flag, 1);
            continue;
        }
        const int l = label[id];
        if (l >= 0) {
            res = l;
            break;
        }
    }
    out[(size_t)r * Ww + c] = res;
}

template <bool LDS>
__global__ __launch_bounds__(256) void confusion_kernel(const int32_t* __restrict__ gt, const int32_t* __restrict__ pred, long long n,
                                                        long long per_block, int Cg, int Cp, unsigned long long* __restrict__ conf,
                                                        unsigned long long* __restrict__ skipped, int* __restrict__ err_flag) {
    extern __shared__ uint32_t counters[];
    const int cells = Cg * Cp;
    if (LDS) {
        for (int i = threadIdx.x; i < cells; i += 256) counters[i] = 0;
        __syncthreads();
    }
    const long long lo = (long long)blockIdx.x * per_block, hi = lo + per_block < n ? lo + per_block : n;
    unsigned long long s0 = 0, s1 = 0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const int g = gt[i], q = pred[i];
        if (g < 0) {
            ++s0;
        } else if (q < 0) {
            ++s1;
        } else if (g >= Cg || q >= Cp) {
            if (err_flag) atomicOr(err_flag, 1);
        } else if (LDS) {
            atomicAdd(counters + g * Cp + q, 1u);
        } else {
            atomicAdd(conf + (size_t)g * Cp + q, 1ull);
        }
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (s0) atomicAdd(skipped + 0, s0);
        if (s1) atomicAdd(skipped + 1, s1);
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += 256) {
            const uint32_t k = counters[i];
            if (k) atomicAdd(conf + i, (unsigned long long)k);
        }
    }
}

}  // namespace avl

using namespace avl;

extern "C" {

int avl_gt_vote(const void* d_depth, int depth_is_u16, double depth_div, const int32_t* d_semantic, int F, int H, int W,
                const double* h_calib_inv, const double* h_transforms, int gs, double cs, int vh, int stride, double min_depth,
                double max_depth, const int32_t* d_obj2cls, int n_obj, int n_classes, const int32_t* d_occupied_ids, int64_t n_voxels,
                uint32_t* d_votes, uint64_t* d_stats, int32_t* d_err_flag, void* stream) {
    VoteParams p{};
    const int rc = ray_params("avl_gt_vote", depth_is_u16, depth_div, F, H, W, h_calib_inv, gs, kGtMaxSide, cs, stride, nullptr, min_depth,
                              max_depth, &p.ray);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(vh >= 1 && (int64_t)gs * gs * vh < kGtMaxVotes, "avl_gt_vote: voxel height %d (>= 1, gs * gs * vh < 2^40)", vh);
    AVL_REQUIRE(n_classes >= 1 && n_classes <= kGtMaxClasses, "avl_gt_vote: %d classes (1 .. %d)", n_classes, kGtMaxClasses);
    AVL_REQUIRE(n_voxels >= 0 && n_voxels * n_classes < kGtMaxVotes, "avl_gt_vote: %lld voxels x %d classes (N * C < 2^40)",
                (long long)n_voxels, n_classes);
    AVL_REQUIRE(d_obj2cls ? n_obj >= 1 : n_obj == 0, "avl_gt_vote: object table of %d entries (>= 1 with a table, 0 without)", n_obj);
    if (F == 0) return AVL_OK;
    AVL_REQUIRE(d_depth && d_semantic && h_calib_inv && h_transforms && d_occupied_ids && d_stats && (d_votes || n_voxels == 0),
                "avl_gt_vote: null pointer");
    p.n_voxels = n_voxels;
    p.vh = vh;
    p.n_obj = n_obj;
    p.n_classes = n_classes;
    const int pixels = p.ray.nv * p.ray.nu;
    if (pixels == 0) return AVL_OK;
    const int tiles = (pixels + kVoteThreads - 1) / kVoteThreads;
    const size_t frame_px = (size_t)H * W, depth_bytes = frame_px * (depth_is_u16 ? sizeof(uint16_t) : sizeof(float));
    hipStream_t st = as_stream(stream);
    ray_launches(F, h_transforms, nullptr, [&](const RayBatch& b, int n, int f0) {
        // about kVoteBlocksPerCu blocks per CU over the launch's frames: a block walks several tiles and adds its statistics once
        const unsigned blocks = (unsigned)std::max(1, std::min(tiles, (num_cus() * kVoteBlocksPerCu + n - 1) / n));
        hipLaunchKernelGGL(gt_vote_kernel, dim3(blocks, (unsigned)n), dim3(kVoteThreads), 0, st, p, b,
                           (const void*)((const char*)d_depth + (size_t)f0 * depth_bytes), d_semantic + (size_t)f0 * frame_px, d_obj2cls,
                           d_occupied_ids, d_votes, (unsigned long long*)d_stats, (int*)d_err_flag);
    });
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_gt_labels(const uint32_t* d_votes, int64_t n_voxels, int n_classes, int32_t* d_label, uint32_t* d_support, void* stream) {
    AVL_REQUIRE(n_classes >= 1 && n_classes <= kGtMaxClasses, "avl_gt_labels: %d classes (1 .. %d)", n_classes, kGtMaxClasses);
    AVL_REQUIRE(n_voxels >= 0 && n_voxels * n_classes < kGtMaxVotes, "avl_gt_labels: %lld voxels x %d classes (N * C < 2^40)",
                (long long)n_voxels, n_classes);
    if (n_voxels == 0) return AVL_OK;
    AVL_REQUIRE(d_votes && d_label && d_support, "avl_gt_labels: null pointer");
    int G = kWave;
    if (n_classes <= kWave) {
        G = 1;
        while (G < n_classes && G < 16) G *= 2;
    }
    const int64_t rows_per_block = 256 / G;
    const int64_t want = (n_voxels + rows_per_block - 1) / rows_per_block;
    const unsigned blocks = (unsigned)std::min<int64_t>(want, (int64_t)num_cus() * 16);
    hipLaunchKernelGGL(gt_labels_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_votes, (long long)n_voxels, n_classes, G, d_label,
                       d_support);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_pool_labels_2d(const int32_t* d_label, int64_t n_voxels, const int32_t* d_occupied_ids, int gs, int vh, int r0, int r1, int c0,
                       int c1, int32_t* d_out, int32_t* d_err_flag, void* stream) {
    AVL_REQUIRE(gs >= 1 && gs <= kGtMaxSide, "avl_pool_labels_2d: grid size %d (1 .. %d)", gs, kGtMaxSide);
    AVL_REQUIRE(vh >= 1 && (int64_t)gs * gs * vh < kGtMaxVotes, "avl_pool_labels_2d: voxel height %d (>= 1, gs * gs * vh < 2^40)", vh);
    AVL_REQUIRE(0 <= r0 && r0 <= r1 && r1 < gs && 0 <= c0 && c0 <= c1 && c1 < gs,
                "avl_pool_labels_2d: window rows %d .. %d, columns %d .. %d of a grid of %d", r0, r1, c0, c1, gs);
    AVL_REQUIRE(n_voxels >= 0 && n_voxels <= INT_MAX, "avl_pool_labels_2d: %lld voxels", (long long)n_voxels);
    AVL_REQUIRE((d_label || n_voxels == 0) && d_occupied_ids && d_out, "avl_pool_labels_2d: null pointer");
    const int Hw = r1 - r0 + 1, Ww = c1 - c0 + 1;
    hipLaunchKernelGGL(pool_labels_kernel, dim3((unsigned)((Ww + 63) / 64), (unsigned)((Hw + 3) / 4)), dim3(256), 0, as_stream(stream), d_label,
                       (long long)n_voxels, d_occupied_ids, gs, vh, r0, c0, Hw, Ww, d_out, (int*)d_err_flag);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_label_confusion(const int32_t* d_gt, const int32_t* d_pred, int64_t n, int n_gt_classes, int n_pred_classes, uint64_t* d_conf,
                        uint64_t* d_skipped, int32_t* d_err_flag, void* stream) {
    AVL_REQUIRE(n_gt_classes >= 1 && n_pred_classes >= 1 && n_gt_classes <= kConfMaxClasses && n_pred_classes <= kConfMaxClasses &&
                    (int64_t)n_gt_classes * n_pred_classes <= kConfMaxCounters,
                "avl_label_confusion: a %d x %d matrix (sides 1 .. %d, at most 2^28 counters)", n_gt_classes, n_pred_classes, kConfMaxClasses);
    AVL_REQUIRE(n >= 0 && n < kGtMaxVotes, "avl_label_confusion: %lld pairs (< 2^40)", (long long)n);
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_gt && d_pred && d_conf && d_skipped, "avl_label_confusion: null pointer");
    const int cells = n_gt_classes * n_pred_classes;
    int64_t per_block = std::max<int64_t>(4096, (n + (int64_t)num_cus() * 4 - 1) / ((int64_t)num_cus() * 4));
    per_block = std::min(per_block, kConfBlockItems);
    const unsigned blocks = (unsigned)((n + per_block - 1) / per_block);
    hipStream_t st = as_stream(stream);
    if (cells <= kConfLdsCounters)
        hipLaunchKernelGGL(confusion_kernel<true>, dim3(blocks), dim3(256), (size_t)cells * sizeof(uint32_t), st, d_gt, d_pred, (long long)n,
                           (long long)per_block, n_gt_classes, n_pred_classes, (unsigned long long*)d_conf, (unsigned long long*)d_skipped,
                           (int*)d_err_flag);
    else
        hipLaunchKernelGGL(confusion_kernel<false>, dim3(blocks), dim3(256), 0, st, d_gt, d_pred, (long long)n, (long long)per_block,
                           n_gt_classes, n_pred_classes, (unsigned long long*)d_conf, (unsigned long long*)d_skipped, (int*)d_err_flag);
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

int avl_label_confusion_limits(int* h_lds_counters) {
    AVL_REQUIRE(h_lds_counters, "avl_label_confusion_limits: null pointer");
    *h_lds_counters = kConfLdsCounters;
    return AVL_OK;
}

}  // extern "C"
