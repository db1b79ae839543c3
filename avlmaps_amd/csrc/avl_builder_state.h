// The voxel map builder's state and the records its kernels exchange, shared by avl_builder.hip (the frame path), avl_finalize.hip
// (finalisation and map I/O) and avl_replay.hip (the exact-colour replay): plain structs that the three files read directly, and
// the few host functions that cross them.
#pragma once
#include "avl_common.h"

namespace avl {

// one frame of a batch (avl_builder_integrate_batch): what differs between the frames of one launch
struct BatchEntry {
    double t[16];                 // pc_transform of the frame
    const float* depth;
    const int32_t* samples;
    const uint8_t* rgb;
    const float* feat;
    unsigned long long frame_key; // key_bias | frame_idx << 32
};

struct FrameParams {
    double kinv[9];   // inv(calib)            (mapping_utils.py:237)
    double k[9];      // calib                 (vlmap_builder.py:98)
    double kf[9];     // get_sim_cam_mat(Hf,Wf)(mapping_utils.py:591-596)
    double t[16];     // pc_transform          (vlmap_builder.py:133)
    double min_depth, max_depth, two_sigma_sq;
    double cs, half_gs;
    double pcd_min[3];   // global mode: lower corner of the pass-1 bounding box (vlmap_builder_multi_floor.py:117)
    double depth_div;    // uint16 depth images: metres = value / depth_div (multi-floor: / 1000.0, :105)
    int H, W, Hf, Wf, n0, n1, n2, P;   // grid: n0 rows x n1 cols x n2 heights (mobile-base mode: gs, gs, vh)
    const BatchEntry* batch;   // nullptr: single frame (pointers / transform passed directly); else P = B * P_frame samples
    int P_frame;
    int mode;            // 0 = mobile-base map (vlmap_builder.py), 1 = global multi-floor map (vlmap_builder_multi_floor.py)
    int depth_u16;
    long long capacity;
    const struct PreRec* pre;   // the stateless half of K1 for THIS frame, computed by the previous launch (PreGather); nullptr: compute here
};

// The frame loop in C (avl_builder_integrate_frames) knows frame i + 1 while it launches frame i, and the first half of K1 --
// sample index -> depth -> back-projection, pose, cell, the two pinhole projections, the colour gather, the weight -- depends on
// nothing the builder holds: only from the cell's slot onwards does a sample touch the map.  A few workgroups in FRONT of frame
// i's launch run that half for frame i + 1 (bp_voxelize_body<.., 2>) and leave 24 bytes per sample; K1 of frame i + 1
// (bp_voxelize_body<.., 1>) then starts its chain with one coalesced load and goes straight to the slot: four of the chain's
// hops (sample index, depth, geometry, colour) move out of the dependent path into the shadow of the previous frame.
// Single float32-depth frames of one avl_builder_integrate_frames call; the same arithmetic, operation for operation.
struct PreRec {
    double alpha;     // 0 if the sample dropped out
    int32_t cell;     // -1 if the sample dropped out
    int32_t fpix;
    uint32_t rgbv;
    uint32_t flags;   // bit 0: outside the pass-1 bounding box (global mode), bit 1: projected outside the RGB image
};
static_assert(sizeof(PreRec) == 24, "PreRec");

struct PreGather {
    PreRec* out;              // nullptr: nothing to prepare
    const float* depth;
    const int32_t* samples;
    const uint8_t* rgb;
};

// per-frame sample records (structure of arrays, sized for the largest P seen)
struct Recs {
    double* alpha;
    int32_t* slot;    // -1 = the sample updates no voxel
    int32_t* fpix;    // py*Wf + px into the (Hf, Wf, D) feature map
    uint32_t* rgb;    // r | g<<8 | b<<16
    int32_t* next;    // next sample of the same voxel in this frame, -1 = end
    uint8_t* owner;   // 1 = this sample found its voxel's list empty: it is the list's TAIL and its wave fuses the list
};
// The owners of a BATCHED launch compacted per K2 workgroup (no atomics: a ballot and four LDS words): entry 256 b + k is owner k of
// workgroup b, ocnt[b] of them.  K3 then runs kFuseWaves waves per K2 workgroup over them instead of one wave per SAMPLE, most of
// which load a flag and leave: half the workgroups to dispatch, +3 % / +6 % at 16 / 64 frames per launch.  Single-frame launches keep
// the wave-per-sample form (the compacted one measured 11.2 -> 12.0 us there), and these pointers stay out of their kernel arguments.
struct OwnerList {
    double* o_alpha;
    int32_t* o_s;
    int32_t* o_slot;
    int32_t* o_fpix;
    uint32_t* o_rgb;
    int32_t* ocnt;
};

constexpr unsigned long long kNoKey = ~0ull;   // slot_key of a voxel whose first-touch sample is not known yet

// optional per-sample log for the exact sequential replay of weight / grid_rgb at finalisation (position = key order)
// One 32-byte record per sample = one memory sector: the replay walks a voxel's samples through an index list, i.e. every entry is
// a random access -- with alpha / key / colour in three arrays that was three sectors per entry (replay_chain_kernel 1.63 ms for the
// 27 M active samples of a 10 000-frame build).  The slots stay in an array of their own: the compaction and the sort read only them.
struct alignas(32) LogRec {
    double alpha;
    unsigned long long key;
    uint32_t rgb;
    uint32_t pad[3];
};
static_assert(sizeof(LogRec) == 32, "one sector per replay-log record");
struct ReplayLog {
    uint32_t* slot;            // 0xFFFFFFFF = sample did not update a voxel
    LogRec* rec;
};

// per-voxel state of the replay when it runs as a chain over ranks (replay_chain_kernel, avl_replay.hip)
struct ReplayState {
    double w;
    float c[3];
    uint32_t started;
};
static_assert(sizeof(ReplayState) == 24, "ReplayState is exchanged between ranks as 3 x int64");

}  // namespace avl

struct LogSegments;   // the replay log sorted by voxel (avl_replay.hip)
struct avl_builder {
    int n0, gs, vh, D;   // grid n0 x gs x vh (n0 == gs for the square mobile-base map)
    double cs;
    int64_t capacity;
    size_t ncell;
    int32_t* cell_slot = nullptr;
    int32_t* slot_cell = nullptr;
    unsigned long long* slot_key = nullptr;
    double* sum_feat = nullptr;
    double* sum_w4 = nullptr;
    float* first_feat = nullptr;
    double* first_alpha = nullptr;
    int32_t* head = nullptr;                 // lists of the launch being linked
    int32_t* head_alt = nullptr;             // deferred fuse: lists of the frame whose K3 is still pending (the two swap per frame)
    uint8_t* dirty = nullptr;                // slot fused since the last clearing finalize (incremental checkpoints)
    unsigned long long* counters = nullptr;  // [0] slots handed out, [1] samples fused, [2] per-frame voxel groups fused
    int* err_flags = nullptr;
    char* recs_mem = nullptr;
    avl::OwnerList owners{};                 // batched launches only (see struct OwnerList)
    avl::Recs recs{}, recs_alt{};            // recs_alt: records of the pending frame (deferred fuse), swapped like head
    int recs_cap = 0;
    // deferred fuse (avl_builder_set_deferred_fuse): K3 of a frame runs inside the NEXT frame's launch
    int deferred = 0;
    struct Pending {
        int P = 0;                           // 0: nothing pending
        unsigned long long frame_key = 0;
        const float* feat = nullptr;
    } pend;
    unsigned long long key_bias = 0;  // set after import_map so that imported voxels order before new ones
    avl::ReplayLog log{};
    long long log_cap = 0, log_used = 0;
    char* rs_mem = nullptr;     // scratch of the log's slot-sorted form (LogSegments), allocated WITH the log: the first finalisation /
    size_t rs_bytes = 0;        // merge of a build does not grow a pool by a GB inside its timed path (22 ms at 78 M samples)
    size_t rs_tmp_bytes = 0;
    avl::BatchEntry* d_table = nullptr;
    int table_cap = 0;
    int64_t vox_bound = 0;       // host-side upper bound on the voxel counter (every fused sample may create one voxel)
    int64_t max_capacity = 0;    // 0: the capacity is fixed; else the accumulators double up to this many voxels
    // the slot-sorted replay log of the last avl_builder_replay_chain call: the round-4 merge calls it twice per merge (voxels that
    // depend on no other rank, then the ones whose predecessor's state had to arrive first) and sorts the log once
    LogSegments* ls_cache = nullptr;
    long long ls_log_used = -1;
    int64_t ls_n = -1;

    // next frame's stateless half of K1 in the C frame loop (PreGather): two buffers of recs_cap records, the one K1 reads and the one
    // being written
    avl::PreRec* pre_buf[2] = {nullptr, nullptr};
    struct PreHeld {           // what pre_buf[buf] holds: the frame with exactly these inputs and parameters
        avl::FrameParams fp{};
        const int32_t* samples = nullptr;
        const void* depth = nullptr;
        const uint8_t* rgb = nullptr;
        int buf = 0;
        bool valid = false;
    } pre_held;
    struct PreNext {           // set by avl_builder_integrate_frames for the launch being issued: the frame after it
        const int32_t* samples = nullptr;
        const float* depth = nullptr;
        const uint8_t* rgb = nullptr;
        const double* h_pc_transform = nullptr;
    } pre_next;
};

namespace avl {

// avl_builder.hip
int flush_pending(avl_builder* b, hipStream_t st);              // deferred fuse: run the K3 that is still owed
int grow_builder(avl_builder* b, int64_t want, hipStream_t st);  // double the per-slot arrays, up to max_capacity
// avl_replay.hip
void drop_log_segments(avl_builder* b, hipStream_t st);         // forget the cached voxel-sorted log (stale once a frame is fused)
size_t replay_sort_tmp_bytes(int64_t n);                        // rocPRIM's storage for sorting a log of n samples; 0: query failed
// exact sequential weight / grid_rgb of the n rows of a finalisation (row r = slot perm[r], keys_sorted = its first-touch keys)
int replay_rgb(avl_builder* b, int64_t n, const int32_t* perm, const unsigned long long* keys_sorted, float* d_weight,
               uint8_t* d_grid_rgb, hipStream_t st);

}  // namespace avl
