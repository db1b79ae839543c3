/*
 * avlmaps_hip.h -- C ABI of libavlmaps_hip.so: the MI355X (gfx950) implementation of the AVLMaps
 * map-creation / landmark-indexing hot path.
 *
 * The upstream reference is pure Python and has no FFI layer; each entry point below replaces a
 * span of reference Python (cited as path:line relative to the upstream repo root) and is what a
 * ctypes binding inside the reference would call.
 *
 * Conventions
 *   - every function returns an int status (AVL_OK == 0); avl_last_error() returns a thread-local
 *     human-readable message for the last failure on the calling thread.
 *   - pointers named d_* are DEVICE pointers (HIP), pointers named h_* are HOST pointers.
 *     Small fixed-size parameter blocks (3x3 / 4x4 float64 matrices) are always host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     asynchronous with respect to the host unless stated otherwise.
 *   - caller-owned buffers in, library-owned state only behind opaque handles, nothing allocated
 *     by the library crosses the boundary.
 *   - one handle is used by one host thread at a time; one process (or thread) per GPU.
 */
#ifndef AVLMAPS_HIP_H
#define AVLMAPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVL_API __attribute__((visibility("default")))

enum {
    AVL_OK = 0,
    AVL_ERR_INVALID = 1,   /* bad argument                                   */
    AVL_ERR_HIP = 2,       /* a HIP runtime call failed                      */
    AVL_ERR_CAPACITY = 3,  /* voxel capacity exhausted (builder)             */
    AVL_ERR_NO_DEVICE = 4, /* no usable gfx950 device                        */
    AVL_ERR_STATE = 5      /* call not valid in the handle's current state   */
};

/* ------------------------------------------------------------------------------------------------
 * library / device plumbing
 * ------------------------------------------------------------------------------------------------ */
AVL_API const char* avl_last_error(void);
AVL_API int avl_version(void);                       /* major*10000 + minor*100 + patch */
AVL_API int avl_device_count(int* h_count);
AVL_API int avl_set_device(int device);
AVL_API int avl_get_device(int* h_device);           /* the calling THREAD's current device (HIP keeps it per thread) */
AVL_API int avl_device_name(int device, char* h_buf, size_t buf_len);
AVL_API int avl_device_sync(void);
AVL_API int avl_stream_create(void** h_stream_out);
AVL_API int avl_stream_destroy(void* stream);
AVL_API int avl_stream_sync(void* stream);
/* device memory helpers so that hosts without a GPU array library can drive the ABI */
AVL_API int avl_malloc(void** h_ptr_out, size_t bytes);
AVL_API int avl_free(void* d_ptr);
/* page-locked host memory (hipHostMalloc): device-to-host copies into it run at PCIe rate (~50 GB/s) instead of the ~6 GB/s of a
 * pageable destination; used as the staging buffer of the checkpoint rows */
/* Host only (no GPU needed): advance a NumPy legacy Mersenne-twister state (np.random.get_state(): key[624], pos) as n_shuffles
 * calls of np.random.shuffle on an array of n_items elements would (vlmap_builder.py:275-277 shuffles arange(H*W) once per
 * frame) -- the draws only, nothing is permuted.  A rank of a sharded build fast-forwards past the frames of the ranks before
 * it with this, so that a seeded N-rank run samples the pixels of the seeded single-process run. */
AVL_API int avl_mt19937_skip_shuffles(uint32_t* h_key624, int* h_pos, int64_t n_items, int64_t n_shuffles);
/* Host only: h_out[k] = perm[k * rate] of the permutation np.random.shuffle(np.arange(n_items)) produces from this state
 * (vlmap_builder.py:275-277: shuffle_mask[::depth_sample_rate]); the state advances exactly as the shuffle advances it.
 * h_scratch: n_items int32 of work space, h_out: ceil(n_items / rate) int32.  Same result as NumPy, about twice as fast (int32
 * indices, branch-free rejection): the serial part of a pixel-faithful build. */
AVL_API int avl_mt19937_shuffle_sample(uint32_t* h_key624, int* h_pos, int64_t n_items, int64_t rate, int32_t* h_scratch, int32_t* h_out);
AVL_API int avl_host_alloc(void** h_ptr_out, size_t bytes);
AVL_API int avl_host_free(void* h_ptr);
AVL_API int avl_memset(void* d_ptr, int value, size_t bytes, void* stream);
AVL_API int avl_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);
AVL_API int avl_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);
AVL_API int avl_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes, void* stream);
/* Stable argsort of n NON-NEGATIVE integer keys smaller than 2^bits: d_perm[i] = position of the i-th smallest key, ties in
 * position order (an LSD radix sort over the low `bits` bits only).  d_keys int32 or int64 (key_bytes 4 / 8), d_perm int64[n].
 * The multi-GPU merge plan sorts 3-bit destination ranks and 22-bit row numbers held in int64 tensors (avlmaps_amd/parallel.py:
 * the bookkeeping around vlmap_builder.py:163-170's voxel ids); a generic 64-bit sort makes eight passes where one or three do. */
AVL_API int avl_argsort_bits_work_bytes(int64_t n, int key_bytes, int bits, size_t* h_bytes);
AVL_API int avl_argsort_bits(int64_t n, const void* d_keys, int key_bytes, int bits, int64_t* d_perm, void* d_work, size_t work_bytes,
                             void* stream);
/* The reverse: row d_rows[i] of d_dst (n_dst rows) = row i of d_src; rows distinct, 16-byte multiples at 16-byte aligned bases.
 * A row index outside [0, n_dst) is skipped and sets bit 0 of *d_err_flag (nullable).  The owner side of the multi-GPU merge places
 * the finished float32 rows it received at their final positions with it (avlmaps_amd/parallel.py). */
AVL_API int avl_scatter_rows(const void* d_src, int64_t row_bytes, const int64_t* d_rows, int64_t n, void* d_dst, int64_t n_dst,
                             int32_t* d_err_flag, void* stream);
/* dst row i = src row d_rows[i] (rows of row_bytes bytes, int64 indices): packs the rows an incremental checkpoint has to
 * write (the changed and the new voxels, avl_builder_finalize_ex's d_row_dirty) so that only they cross PCIe -- the reference
 * rewrites the whole map file every 100 frames (vlmap_builder.py:180-183). */
AVL_API int avl_gather_rows(const void* d_src, int64_t row_bytes, const int64_t* d_rows, int64_t n, void* d_dst, void* stream);
/* Read-only streaming probe over a caller buffer of `rows` x `row_floats` float32.
 * pattern bit 0: 0 = plain coalesced 16-byte grid-stride reads, 1 = the similarity kernels' row-line walk;
 * pattern bit 1: 0 = best GB/s of `iters` individually synchronised passes (burst rate),
 *                2 = mean GB/s of `iters` back-to-back passes (sustained rate at the package's power operating point);
 * pattern bits 2-3 (row-line walk only): workgroups per CU, 0 = two (default), 4 = one, 8 = three.
 * Used by bench.py to report the box's practical HBM read ceiling next to the 8 TB/s spec peak.  Synchronous. */
AVL_API int avl_hbm_read_probe(const void* d_buf, int64_t rows, int row_floats, int pattern, int iters, float* h_best_gbs,
                               void* stream);
/* HIP-event timing on `stream` (bench.py measures kernels on the stream they are launched on) */
AVL_API int avl_event_create(void** h_event_out);
AVL_API int avl_event_destroy(void* event);
AVL_API int avl_event_record(void* event, void* stream);
AVL_API int avl_event_sync(void* event);
/* work submitted to `stream` after this call waits (on the device, the host does not block) until `event` has completed: the
 * hand-over between the copy stream of the builder's pinned frame staging (avlmaps_amd/device.py FrameStager: depth / rgb / sample
 * list of frame i + k cross PCIe while frame i is fused) and the stream the frame kernels run on */
AVL_API int avl_stream_wait_event(void* stream, void* event);
AVL_API int avl_event_elapsed_ms(void* start, void* stop, float* h_ms);

/* ------------------------------------------------------------------------------------------------
 * (1) voxel x query similarity + row argmax
 *     replaces  avlmaps/utils/clip_utils.py:227-229   scores_list = map_feats @ text_feats.T
 *               avlmaps/map/vlmap.py:123-124          max_ids = np.argmax(scores_mat, axis=1)
 *               avlmaps/utils/index_utils.py:153-161  (same pair, obstacle classes)
 *     The score is the reference's RAW dot product (no normalisation).  Ties in the argmax resolve
 *     to the lowest query index, like np.argmax.
 * ------------------------------------------------------------------------------------------------ */
enum {
    AVL_SIM_AUTO = 0,      /* SPLIT_F16 when the shape allows it (D % 64 == 0, 16-byte aligned rows), else EXACT        */
    AVL_SIM_EXACT = 1,     /* float32 products and accumulation (an fmaf chain): v_mfma_f32_32x32x2_f32 on the matrix
                              cores when the shape allows it, otherwise the vector-ALU kernel (any N, D, Q, strides)     */
    AVL_SIM_SPLIT_F16 = 2, /* fp16 hi/lo split, 3 MFMA per product, fp32 accumulate: |err| <~ 1e-6*|a||q|, HBM-bound.
                              Range-guarded: a row whose largest |element| is outside [2^-7, 2^15) -- where the unscaled
                              fp16 pair would lose bits or saturate -- or non-finite is recomputed in float32 by a
                              follow-up kernel (np.argmax semantics for NaN rows), so every row is float32-class.       */
    AVL_SIM_EXACT_VALU = 3,/* force the vector-ALU float32 kernel                                                        */
    AVL_SIM_PREPARED = 4,  /* d_feat was converted by avl_sim_prepare_map: SPLIT_F16 without the on-the-fly split        */
    AVL_SIM_PREPARED24 = 5 /* d_feat is the compact 3-byte form of avl_sim_prepare_map24 (avl_sim_scores_prepared24, or
                              avl_sim_scores_blocks with d_feat = d_map24, ld_feat = D and its d_row_scale)               */
};

/* One-off, IN-PLACE conversion of a device-resident float32 map (N, D; D % 64 == 0, 16-byte aligned rows) into the split
 * layout the matrix-core kernel consumes directly: every group of 8 floats (32 bytes) becomes fp16 hi[8] | fp16 lo[8]
 * (same 4 bytes per element, same row stride).  Meant for a map that is indexed many times (VLMap keeps its private device
 * copy in this form).  The float32 values are not recoverable exactly.
 *   d_row_scale != NULL (N floats, out): every row is first scaled by the power of two that brings its largest |element| into
 *     [2^14, 2^15) and 2^-s is stored here; pass it to avl_sim_scores_prepared.  Rows of any magnitude (a voxel observed once
 *     from 5 m away stores feat * exp(-r^2/1.2) ~ 1e-9, vlmap_builder.py:166-168) keep the full ~22 bits: this is the form
 *     VLMap uses.  Rows containing NaN / inf are left unscaled and score NaN (argmax 0).
 *   d_row_scale == NULL: no scaling; avl_sim_scores(..., AVL_SIM_PREPARED) then gives scores bit-identical to the on-the-fly
 *     split of the raw map (without its range guard: meant for maps known to be LSeg-scale). */
AVL_API int avl_sim_prepare_map(float* d_feat, int64_t N, int D, int64_t ld_feat, float* d_row_scale, void* stream);

/*
 * d_feat     (N, D) float32 row-major with row stride ld_feat (elements)  -- VLMap.grid_feat
 * d_queries  (Q, D) float32 row-major with row stride ld_q                -- text_feats
 * d_scores   (N, Q) float32 row-major, or NULL to skip materialising scores_mat
 * d_argmax   (N,) int32, or NULL
 * d_best     (N,) float32 score of the argmax column, or NULL
 * precision  one of AVL_SIM_*
 */
AVL_API int avl_sim_scores(const float* d_feat, int64_t N, int D, int64_t ld_feat, const float* d_queries, int Q,
                           int64_t ld_q, float* d_scores, int32_t* d_argmax, float* d_best, int precision,
                           void* stream);

/* Scratch of the matrix-core paths: the prepared query image (avl_sim_workspace_bytes: depends on D, Q only) and, for
 * the raw split path, one range-guard word per 32 voxel rows (avl_sim_workspace_bytes_n = image + guard words).  Pass a
 * buffer of that size (it also covers avl_sim_scores_blocks' gathered queries) to avl_sim_scores_ws to keep every allocation off the hot path (benchmark / graph capture); with a
 * smaller or NULL workspace the library allocates from the stream-ordered pool. */
AVL_API int avl_sim_workspace_bytes(int D, int Q, size_t* h_bytes);
AVL_API int avl_sim_workspace_bytes_n(int64_t N, int D, int Q, size_t* h_bytes);
AVL_API int avl_sim_scores_ws(const float* d_feat, int64_t N, int D, int64_t ld_feat, const float* d_queries, int Q,
                              int64_t ld_q, float* d_scores, int32_t* d_argmax, float* d_best, int precision,
                              void* d_workspace, size_t workspace_bytes, void* stream);
/* Block-structured query sets: h_col_begin / h_col_end (Q host ints) give every query's non-zero column window [begin, end)
 * (a superset is fine).  Queries with the same window (rounded out to 128 columns) are scored against just those columns of
 * the map, one launch group per window: on a fused visual | audio map (BASELINE config 5: 512 + 1024 columns, every query
 * living in one modality block) the map is still read once overall but the matrix cores do half the work.  Results equal the
 * dense call (same products; zero products dropped); argmax ties still resolve to the lowest query index.  d_row_scale: see
 * avl_sim_scores_prepared (NULL unless precision == AVL_SIM_PREPARED on a scaled map, or AVL_SIM_PREPARED24: then d_feat is the
 * compact map of avl_sim_prepare_map24 and ld_feat == D).  Falls back to the dense path when the windows do not split the
 * queries or the shape does not allow it. */
AVL_API int avl_sim_scores_blocks(const float* d_feat, const float* d_row_scale, int64_t N, int D, int64_t ld_feat,
                                  const float* d_queries, int Q, int64_t ld_q, const int32_t* h_col_begin,
                                  const int32_t* h_col_end, float* d_scores, int32_t* d_argmax, float* d_best, int precision,
                                  void* d_workspace, size_t workspace_bytes, void* stream);
/* Scores of a map prepared WITH row scaling (d_row_scale from avl_sim_prepare_map; NULL = prepared without). */
AVL_API int avl_sim_scores_prepared(const float* d_feat, const float* d_row_scale, int64_t N, int D, int64_t ld_feat,
                                    const float* d_queries, int Q, int64_t ld_q, float* d_scores, int32_t* d_argmax,
                                    float* d_best, void* d_workspace, size_t workspace_bytes, void* stream);

/* COMPACT resident copy of a map that is indexed many times (VLMap.compact_map, its default when D % 128 == 0): 3 bytes per element
 * instead of 4 -- fp16 hi (round to nearest) and one byte per element holding the residual x - hi in units of ulp(hi) / 256, every row
 * scaled by a power of two (d_row_scale out, N floats).  Row layout (round 4; opaque to callers, it only has to come from this
 * function): a plane of hi values [0, 2 D) -- column c at byte 2 c -- then a plane of residual bytes [2 D, 3 D), column c at
 * 128 (c >> 7) + 64 ((c >> 5) & 1) + 32 ((c >> 6) & 1) + (c & 31): every load of the kernels' walk is a whole cache line shared by the
 * two halves of a wave (the first layout interleaved hi[32] | residuals[32] per 96 bytes and requested every third line twice).
 * d_map24: N * D * 3 bytes, out of place (the float32 map is left alone).  A query pass then reads a quarter less HBM; the
 * residuals are rebuilt as fp16 in registers (five vector-ALU instructions per two elements) and the arithmetic is the same three
 * fp16 MFMAs.  Accuracy: 19 significant bits per element (hi's 11 + 8: the residual's exponent is implied by hi) instead of 22 --
 * max |score - float64| 2.3e-6 on LSeg-scale rows against 1.4e-6 for the 4-byte forms (tests/test_sim_gpu.py): still float32-class.
 * Elements below 2^-11 of their row's maximum keep hi only.  D % 128 == 0.  Every matrix-core kernel reads this form: the
 * resident-query kernel (D <= 512, up to ~78 queries per pass: 0.70 -> 0.57 ms at 2 M x 512 x 64), the K-swap kernel (D <= 1024),
 * the streamed kernels (up to 128 queries per pass) and the column-block launches of avl_sim_scores_blocks (precision
 * AVL_SIM_PREPARED24; BASELINE config 5's fused 1536-column map is 9.2 GB instead of 12.3 GB per pass). */
AVL_API int avl_sim_prepare_map24(const float* d_feat, int64_t N, int D, int64_t ld_feat, void* d_map24, float* d_row_scale,
                                  void* stream);
AVL_API int avl_sim_scores_prepared24(const void* d_map24, const float* d_row_scale, int64_t N, int D, const float* d_queries,
                                      int Q, int64_t ld_q, float* d_scores, int32_t* d_argmax, float* d_best,
                                      void* d_workspace, size_t workspace_bytes, void* stream);

/* Host-buffer convenience wrapper (synchronous): copies in, runs, copies out. */
AVL_API int avl_sim_scores_host(const float* h_feat, int64_t N, int D, const float* h_queries, int Q,
                                float* h_scores, int32_t* h_argmax, float* h_best, int precision);

/* mask[i] = (argmax[i] == cat_id) as uint8 -- avlmaps/map/vlmap.py:124 */
AVL_API int avl_mask_from_argmax(const int32_t* d_argmax, int64_t N, int32_t cat_id, uint8_t* d_mask, void* stream);
/* the same mask bit-packed: d_bits (ceil(N / 64),) uint64, word w bit i = (argmax[64 w + i] == cat_id), i.e. the byte / bit order of
 * np.unpackbits(bitorder="little"); bits beyond N are 0.  1 bit instead of 4 bytes per voxel has to reach the host. */
AVL_API int avl_mask_bits_from_argmax(const int32_t* d_argmax, int64_t N, int32_t cat_id, uint64_t* d_bits, void* stream);

/* index and value of the maximum of a float32 vector, first maximum wins -- the navigator's
 * heatmap argmax, avlmaps/robot/habitat_lang_robot.py:427-430.  Synchronous (returns host scalars).
 * NaN is ignored: with at least one value that is not NaN the index is np.nanargmax's (not np.argmax's, which returns the first
 * NaN); an all-NaN vector returns index 0. */
AVL_API int avl_argmax_f32(const float* d_vals, int64_t N, int64_t* h_index, float* h_value, void* stream);

/* the k largest values with their indices, descending, ties in ascending index order (np.argsort(-v, kind="stable")[:k]): for
 * every k, +0 and -0 tie and NaN of either sign comes last.  h_index (k,) int64 and h_value (k,) float32 are host buffers.
 * Synchronous. */
AVL_API int avl_topk_f32(const float* d_vals, int64_t N, int k, int64_t* h_index, float* h_value, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (2) map builder: depth back-projection + voxelisation + weighted feature fusion
 *     replaces  avlmaps/map/vlmap_builder.py:129-178 (per-frame body of create_mobile_base_map)
 *               avlmaps/utils/mapping_utils.py:226-251 depth2pc, :305-315 transform_pc,
 *               :345-349 base_pos2grid_id_3d, :599-605 project_point
 *     State lives on the device behind the handle; avl_builder_finalize reproduces the reference's
 *     arrays (grid_feat, grid_pos, weight, grid_rgb, occupied_ids) in the reference's voxel-id order.
 * ------------------------------------------------------------------------------------------------ */
typedef struct avl_builder avl_builder;

/* gs, cs, vh: grid size, cell size (m), cells in height (= int(camera_height / cs), vlmap_builder.py:201)
 * D: feature dimension; capacity: maximum number of occupied voxels the handle can hold. */
AVL_API int avl_builder_create(avl_builder** h_out, int gs, double cs, int vh, int D, int64_t capacity);
/* Rectangular grid n0 rows x n1 cols x n2 heights (the global multi-floor map: grid_size[[0, 2, 1]],
 * vlmap_builder_multi_floor.py:222-224). */
AVL_API int avl_builder_create_grid(avl_builder** h_out, int n0, int n1, int n2, double cs, int D, int64_t capacity);
AVL_API int avl_builder_destroy(avl_builder* b);
AVL_API int avl_builder_reset(avl_builder* b, void* stream);
/* The reference doubles its arrays whenever max_id reaches their length (_reserve_map_space, vlmap_builder.py:286-311).
 * max_capacity > capacity: the per-voxel accumulators double (realloc + device copy, between launches) up to max_capacity
 * voxels instead of failing with AVL_ERR_CAPACITY; 0 (the default after create) keeps the capacity fixed. */
AVL_API int avl_builder_set_max_capacity(avl_builder* b, int64_t max_capacity);
AVL_API int avl_builder_capacity(avl_builder* b, int64_t* h_capacity);
/* Deferred fuse: frame-by-frame integration in ONE launch per frame instead of two dependent ones.  With on != 0,
 * avl_builder_integrate_frame / _frame_global run the geometry + list linking of the frame they are given next to the feature
 * fusion of the PREVIOUS frame (disjoint state, same kernel); the frame's own fusion rides in the next call's launch or in
 * avl_builder_flush.  The map that results is the same, bit for bit (the samples of a voxel are summed in ascending sample
 * order in either mode; only a voxel that receives more than 64 samples in ONE launch may differ in the last feature bit, as
 * it may between two runs of any mode).  What changes for the caller: the d_feat buffer of a
 * frame is read by the launch of the NEXT integrate / flush / finalize / num_* / export call, so it must stay valid and
 * unmodified until that call has been enqueued (all on one stream).  d_depth, d_sample_idx and d_rgb are consumed by the
 * call they are passed to, as before.  Every entry point that reads the map flushes first; batched calls flush and then run
 * the three-launch path.  The reference's loop (vlmap_builder.py:102-183) has the same shape: features of frame i are
 * produced, then fused, one frame at a time. */
AVL_API int avl_builder_set_deferred_fuse(avl_builder* b, int on, void* stream);
AVL_API int avl_builder_flush(avl_builder* b, void* stream);
/* Give back what the builder's finalisation / replay / merge temporaries left cached: the slot-sorted replay log kept between the
 * two replay calls of a merge, and everything above keep_bytes in the device's stream-ordered pool (hipMemPoolTrimTo).  The
 * library keeps AVLMAPS_MEMPOOL_KEEP_MB (default 1024) MB of that pool between calls; call this after the last merge / final
 * save of a build that shares the GPU with a feature extractor.  Synchronises the stream. */
AVL_API int avl_builder_release_scratch(avl_builder* b, int64_t keep_bytes, void* stream);

/* Optional: keep a 24-byte log entry per sampled pixel (up to max_samples in total) so that avl_builder_finalize can
 * REPLAY the reference's sequential weight / grid_rgb updates exactly -- float32 weight accumulation and the truncating
 * uint8 colour store of vlmap_builder.py:166-178, including the dtype switch at _reserve_map_space (:286-311).
 * Without the log, finalize returns float32(sum alpha) and the once-truncated weighted mean colour.
 * Call on a fresh (or reset) builder.  Not used after avl_builder_import_map. */
AVL_API int avl_builder_enable_replay_log(avl_builder* b, int64_t max_samples);

/*
 * Fuse one RGB-D frame.
 *   d_depth        (H, W) float32 metres
 *   h_calib        3x3 float64 row-major camera matrix  (map_config.cam_calib_mat)
 *   h_calib_inv    3x3 float64 = numpy.linalg.inv(calib) as the reference computes it (mapping_utils.py:237)
 *   h_pc_transform 4x4 float64 row-major camera->map transform (vlmap_builder.py:133)
 *   d_sample_idx   (P,) int32 flattened pixel indices in the reference's sampling order
 *                  (shuffle_mask[::depth_sample_rate], vlmap_builder.py:275-277), BEFORE depth masking
 *   d_feat         (Hf, Wf, D) float32 CHANNELS-LAST pixel features (the reference holds (1, D, Hf, Wf))
 *   d_rgb          (H, W, 3) uint8
 *   frame_idx      position of the frame in the sequence (defines first-touch order across frames)
 *   min_depth/max_depth  strict bounds on camera-frame z (0.1, 6: vlmap_builder.py:129)
 *   sigma_sq       0.6 (vlmap_builder.py:157)
 */
AVL_API int avl_builder_integrate_frame(avl_builder* b, const float* d_depth, int H, int W, const double* h_calib,
                                        const double* h_calib_inv, const double* h_pc_transform,
                                        const int32_t* d_sample_idx, int P, const float* d_feat, int Hf, int Wf,
                                        const uint8_t* d_rgb, int64_t frame_idx, double min_depth,
                                        double max_depth, double sigma_sq, void* stream);

/*
 * Fuse B consecutive frames (frame_idx0 .. frame_idx0 + B - 1) with ONE launch pair.  Same semantics and results as B calls
 * of avl_builder_integrate_frame; the samples of a voxel coming from different frames share one list, so the voxel row is
 * read-modified-written once per batch instead of once per frame, and the per-launch latencies are amortised.
 * All frames share H, W, P, Hf, Wf and the camera matrix.  h_*_ptrs are HOST arrays of B DEVICE pointers
 * (depth (H,W) f32, samples (P,) i32, feat (Hf,Wf,D) f32 channels-last, rgb (H,W,3) u8); h_pc_transforms is (B, 16) float64.
 * The per-frame device buffers must stay valid until the launches have run (stream order).
 */
AVL_API int avl_builder_integrate_batch(avl_builder* b, int B, const float* const* h_depth_ptrs, int H, int W,
                                        const double* h_calib, const double* h_calib_inv, const double* h_pc_transforms,
                                        const int32_t* const* h_sample_ptrs, int P, const float* const* h_feat_ptrs, int Hf,
                                        int Wf, const uint8_t* const* h_rgb_ptrs, int64_t frame_idx0, double min_depth,
                                        double max_depth, double sigma_sq, void* stream);

/*
 * The frame-by-frame loop itself (vlmap_builder.py:102-183's `for frame_i in ...`), for callers whose frames are already resident:
 * exactly n_frames calls of avl_builder_integrate_frame -- one launch pair per frame, or one launch with deferred fuse; NOT a
 * batch: no two frames share a launch or a list -- issued from C.  A call through a language binding costs more host time than the
 * frame's kernels take (12.4 us per ctypes call against 11.9 us of pipe_kernel, tools/probe_frame_loop.py).  Arguments as for
 * avl_builder_integrate_batch; with deferred fuse the LAST frame's features are still to be fused when the call returns.
 * Every frame of the call must be resident when it is made (as for a batch): while frame i is launched, a few workgroups of the
 * same launch already read frame i + 1's sample indices, depth and colour image and run the half of its back-projection that
 * does not depend on the map (geometry, projections, colour gather, weight), so that frame i + 1's dependent chain starts at the
 * voxel-hash lookup.  Same arithmetic, same maps; the frames of one launch still share nothing.
 */
AVL_API int avl_builder_integrate_frames(avl_builder* b, int n_frames, const float* const* h_depth_ptrs, int H, int W,
                                        const double* h_calib, const double* h_calib_inv, const double* h_pc_transforms,
                                        const int32_t* const* h_sample_ptrs, int P, const float* const* h_feat_ptrs, int Hf,
                                        int Wf, const uint8_t* const* h_rgb_ptrs, int64_t frame_idx0, double min_depth,
                                        double max_depth, double sigma_sq, void* stream);

/*
 * Global (multi-floor) variant of the frame fusion: replaces vlmap_builder_multi_floor.py:137-199.
 *   voxel index = np.round((p_global - pcd_min) / cs) per axis, (row, height, col) = (x, y, z) (:146);
 *   d_depth is float32 metres, or uint16 with metres = value / depth_div (depth PNGs / 1000.0, :105);
 *   h_transform = camera_pose_tf @ habitat2cam_rot_tf (:141); h_pcd_min = lower bounding-box corner from pass 1.
 * Samples that fall outside the grid are dropped (the reference wraps negative indices or raises).
 */
AVL_API int avl_builder_integrate_frame_global(avl_builder* b, const void* d_depth, int depth_is_u16, double depth_div, int H,
                                               int W, const double* h_calib, const double* h_calib_inv,
                                               const double* h_transform, const int32_t* d_sample_idx, int P,
                                               const float* d_feat, int Hf, int Wf, const uint8_t* d_rgb, int64_t frame_idx,
                                               double min_depth, double max_depth, double sigma_sq, const double* h_pcd_min,
                                               void* stream);

/* Pass 1 of the global builder (vlmap_builder_multi_floor.py:97-118): fold the transformed, depth-masked sampled points of
 * one frame into h_minmax = [min x, min y, min z, max x, max y, max z] (in/out; start from +inf / -inf).  Synchronous. */
AVL_API int avl_points_bbox(const void* d_depth, int depth_is_u16, double depth_div, int H, int W, const double* h_calib_inv,
                            const double* h_transform, const int32_t* d_sample_idx, int P, double min_depth, double max_depth,
                            double* h_minmax, void* stream);

/* Seed an EMPTY builder from a finished map so that more frames can be fused on top (the reference's resume path,
 * vlmap_builder.py:212-222): d_grid_feat (n,D) f32, d_grid_pos (n,3) i32, d_weight (n,) f32, d_grid_rgb (n,3) u8 or NULL.
 * Voxel ids 0..n-1 are kept; new voxels are appended after them.  The accumulators grow to n first when the handle may
 * (avl_builder_set_max_capacity): a map that outgrew gs*gs voxels resumes like upstream's.  n == 0 only marks the builder as
 * continuing a map (the other ranks of a resumed multi-GPU build: same first-touch key space as the rank that imported).
 * Synchronous. */
AVL_API int avl_builder_import_map(avl_builder* b, int64_t n, const float* d_grid_feat, const int32_t* d_grid_pos,
                                   const float* d_weight, const uint8_t* d_grid_rgb, void* stream);

/* number of occupied voxels so far (synchronises the stream) */
AVL_API int avl_builder_num_voxels(avl_builder* b, int64_t* h_n, void* stream);
/* number of sampled points that updated a voxel so far (synchronises the stream) */
AVL_API int avl_builder_num_points(avl_builder* b, int64_t* h_n, void* stream);
/* number of (frame, voxel) groups fused so far = voxel rows read-modified-written (synchronises the stream) */
AVL_API int avl_builder_num_groups(avl_builder* b, int64_t* h_n, void* stream);

/*
 * Produce the reference's arrays.  Slot ids are assigned in first-touch order (a deterministic prefix
 * scan over each frame's sample list), so row r of every output IS the reference's voxel id r:
 *   d_grid_feat (n, D) f32, d_grid_pos (n, 3) i32, d_weight (n,) f32, d_grid_rgb (n, 3) u8,
 *   d_occupied_ids (gs, gs, vh) i32 (-1 = empty) -- any of them may be NULL.
 * n must equal avl_builder_num_voxels().  Synchronous.
 */
AVL_API int avl_builder_finalize(avl_builder* b, int64_t n, float* d_grid_feat, int32_t* d_grid_pos, float* d_weight,
                                 uint8_t* d_grid_rgb, int32_t* d_occupied_ids, void* stream);

/* avl_builder_finalize plus, for incremental checkpoints: d_row_dirty (n,) uint8 (nullable) receives 1 for every output row whose
 * voxel was fused since the flags were last cleared, and clear_dirty != 0 clears them.  Voxel ids never change once assigned
 * (new voxels are appended), so a checkpoint only has to rewrite the dirty rows and append rows >= the previous n -- upstream
 * rewrites the whole file every 100 frames (vlmap_builder.py:180-183). */
AVL_API int avl_builder_finalize_ex(avl_builder* b, int64_t n, float* d_grid_feat, int32_t* d_grid_pos, float* d_weight,
                                    uint8_t* d_grid_rgb, int32_t* d_occupied_ids, uint8_t* d_row_dirty, int clear_dirty,
                                    void* stream);

/*
 * Multi-GPU merge support (frames sharded over ranks; the exchange itself runs in the host layer over
 * RCCL, see avlmaps_amd/parallel.py).  Export the raw per-voxel accumulators of the first n slots:
 *   d_cell        (n,)   int32   linear cell index (row*gs + col)*vh + h
 *   d_first_key   (n,)   uint64  first-touch key (frame_idx << 32 | position in the frame's sample list)
 *   d_sum_feat    (n, D) float64 sum_i alpha_i * f_i
 *   d_sum_w4      (n, 4) float64 [sum alpha, sum alpha*r, sum alpha*g, sum alpha*b]
 *   d_first_feat  (n, D) float32 feature of the first-touch point
 *   d_first_alpha (n,)   float64 alpha of the first-touch point
 * Any output may be NULL.
 */
AVL_API int avl_builder_export_raw(avl_builder* b, int64_t n, int32_t* d_cell, uint64_t* d_first_key,
                                   double* d_sum_feat, double* d_sum_w4, float* d_first_feat,
                                   double* d_first_alpha, void* stream);

/*
 * Stateless finalisation of raw accumulators (the arrays of avl_builder_export_raw, possibly merged
 * across ranks and re-ordered by first-touch key): applies the reference's first-touch weighting
 *   grid_feat = (sum_feat - a1*(1-a1)*first_feat) / sum_alpha      (vlmap_builder.py:166-174 closed form)
 * and writes grid_feat (n,D) f32, grid_pos (n,3) i32, weight (n,) f32, grid_rgb (n,3) u8 in the given row
 * order, and occupied_ids[cell] = row index (d_occupied_ids (gs,gs,vh) must be pre-filled with -1).
 * Any output may be NULL.
 */
AVL_API int avl_finalize_raw(int64_t n, int D, int gs, int vh, const int32_t* d_cell, const double* d_sum_feat,
                             const double* d_sum_w4, const float* d_first_feat, const double* d_first_alpha,
                             float* d_grid_feat, int32_t* d_grid_pos, float* d_weight, uint8_t* d_grid_rgb,
                             int32_t* d_occupied_ids, void* stream);

/*
 * Multi-GPU merge on the device (avlmaps_amd/parallel.py drives the RCCL calls).  After the ranks have agreed
 * on the union of occupied cells and all-reduced (MIN) the first-touch keys, every rank scatters its accumulators into a
 * zero-initialised dense (M, ld_acc >= D + 4) float64 buffer that is then sum-reduced ONCE:
 *   row d_row_of_slot[s] <- [sum_feat[s] + (own ? a1^2 : a1) first_feat[s]  |  sum alpha, sum alpha * (r, g, b)]
 * where sum_feat[s] sums alpha f over every sample of the slot EXCEPT its local first touch (a1, first_feat) and
 * own = (this rank's first-touch key of the voxel == d_global_key[row]): the owner of the global first touch contributes it
 * with the reference's weight a1^2 (vlmap_builder.py:166-174), every other rank with a1, so no first_feat / first_alpha
 * exchange is needed.
 * n must equal avl_builder_num_voxels().  d_row_of_slot (n,) int64, d_global_key (M,) uint64.
 */
AVL_API int avl_builder_scatter_merge(avl_builder* b, int64_t n, const int64_t* d_row_of_slot, const uint64_t* d_global_key,
                                      double* d_acc, int64_t ld_acc, void* stream);
/* Finalise n rows of reduced accumulators laid out as above (d_acc points at the first of them, d_cell (n,) are their linear
 * cells): grid_feat = acc[:, :D] / sum alpha etc.; output row r is voxel id row0 + r (occupied_ids[cell] = row0 + r), so one
 * rank can finalise one block of a reduce-scattered map.  Any output may be NULL; d_occupied_ids must be pre-filled with -1. */
AVL_API int avl_finalize_merged(int64_t n, int64_t row0, int D, int gs, int vh, const int32_t* d_cell, const double* d_acc,
                                int64_t ld_acc, float* d_grid_feat, int32_t* d_grid_pos, float* d_weight, uint8_t* d_grid_rgb,
                                int32_t* d_occupied_ids, void* stream);
/* Exact sequential weight / grid_rgb across ranks (needs the replay log): the per-voxel state {float64 weight, float32 rgb[3],
 * uint32 started} = 24 bytes, d_state (M, 24 B) zero-initialised on the first rank, is continued with this rank's log for its
 * own voxels (row d_row_of_slot[s]; a NEGATIVE index leaves slot s out of this call: the round-4 merge replays the voxels that do not
 * depend on another rank first and the others once their predecessor's state has arrived) and handed to the next rank, in rank
 * order (contiguous frame shards).  grow_key = first-touch
 * key of the voxel with global id gs*gs - 1 (after it the reference's arrays have been re-allocated with other dtypes,
 * vlmap_builder.py:286-311), or ~0 if the map is smaller.  avl_replay_state_apply writes weight / grid_rgb from the final state. */
AVL_API int avl_builder_replay_chain(avl_builder* b, int64_t n, const int64_t* d_row_of_slot, uint64_t grow_key, void* d_state,
                                     void* stream);
/* The log sorted by voxel is kept between avl_builder_replay_chain calls until the next frame is fused (a merge calls it twice);
 * this drops it, so that a caller timing a merge twice on the same map pays for the sort both times (bench.py). */
AVL_API int avl_builder_drop_replay_cache(avl_builder* b, void* stream);
/* build that voxel-sorted log NOW (n = avl_builder_num_voxels) instead of inside the next avl_builder_replay_chain / finalize; a no-op without
 * a replay log */
AVL_API int avl_builder_replay_prepare(avl_builder* b, int64_t n, void* stream);
/* ------------------------------------------------------------------------------------------------
 * The local steps of the multi-GPU merge plan (avlmaps_amd/parallel.py, plan_merge_directory): which final row -- the reference's
 * voxel id, vlmap_builder.py:163-170 -- every voxel of every rank gets.  torch.distributed carries the collectives between them;
 * each entry point replaces the 20-40 small tensor operations a rank ran between two collectives by a radix sort over the bits
 * the keys have and one or two kernels (no host synchronisation inside).  At most 64 ranks.  d_work: caller-owned scratch of
 * avl_merge_work_bytes(max(n, R)) bytes.
 *   avl_merge_partition  local voxels -> directory ranks: d_ordd[n] = the slots grouped by directory rank (stable), d_cell_sorted[n] =
 *                        their cells in that order (what the first all_to_all sends), d_head[ws + 3] = [voxels per directory
 *                        rank | n | smallest first-touch key | largest]
 *   avl_merge_dir_scan   directory side, the R cells that arrived (grouped by source rank; d_rc[ws] = how many from each): d_perm[R] =
 *                        their (cell, source rank) order, d_first[R] = "first entry of its cell" in that order, and in ARRIVAL order
 *                        d_prev_r / d_next_r[R] = the neighbouring contributors of the entry's cell (-1: none), d_reply[R] = both
 *                        packed for the way back ((prev + 1) | (next + 1) << 16), d_m3r / d_m4r[R] = the masks of the two later
 *                        round trips; d_cnt[2 ws + 1] = [m3r per source | m4r per source | distinct cells]
 *   avl_merge_classify   back home, d_back[n] = the replies in sending order: d_prev / d_next[n] per slot, d_is_new[n] per slot,
 *                        d_m3 / d_m4[n] in sending order, d_cnt[1 + 4 ws] = [new voxels | m3 per directory rank | m4 per directory
 *                        rank | voxels per prev rank | voxels per next rank]
 *   avl_merge_rows_new   after the count all_gather (c = this rank's new voxels, base = its first final row): d_idx_new[c] = the new
 *                        voxels' slots in first-touch-key order (radix sort over key_bits), d_row[n] = base + position for them and
 *                        -1 for the others, d_send3[n3] = the rows of the new voxels other ranks share, in sending order (d_m3)
 *   avl_merge_dir_rows   directory side: d_recv3 = the rows that arrived for the d_m3r entries (arrival order); every entry of a cell
 *                        inherits the row of the cell's first contributor; d_send4[n4] = those rows for the d_m4r entries
 *   avl_merge_rows_other home: d_recv4[n4] = the rows of this rank's voxels whose first touch another rank holds (d_m4, sending
 *                        order) -> d_row
 *                        (scratch of these three: avl_merge_rows_work_bytes(max(n, R)))
 * ------------------------------------------------------------------------------------------------ */
AVL_API int avl_merge_work_bytes(int64_t n, size_t* h_bytes);
AVL_API int avl_merge_rows_work_bytes(int64_t n, size_t* h_bytes);
AVL_API int avl_merge_rows_new(int64_t n, int64_t c, const uint8_t* d_is_new, const int64_t* d_key, int key_bits, int64_t base,
                               const int64_t* d_ordd, const uint8_t* d_m3, int64_t n3, int64_t* d_row, int64_t* d_idx_new, int64_t* d_send3,
                               void* d_work, size_t work_bytes, void* stream);
AVL_API int avl_merge_dir_rows(int64_t R, const int64_t* d_recv3, const uint8_t* d_m3r, const uint8_t* d_first, const int64_t* d_perm,
                               const uint8_t* d_m4r, int64_t n4, int64_t* d_send4, void* d_work, size_t work_bytes, void* stream);
AVL_API int avl_merge_rows_other(int64_t n, const uint8_t* d_m4, const int64_t* d_ordd, const int64_t* d_recv4, int64_t n4, int64_t* d_row,
                                 void* d_work, size_t work_bytes, void* stream);
AVL_API int avl_merge_partition(int64_t n, const int32_t* d_cell, const int64_t* d_key, int ws, int64_t* d_ordd, int32_t* d_cell_sorted,
                                int64_t* d_head, void* d_work, size_t work_bytes, void* stream);
AVL_API int avl_merge_dir_scan(int64_t R, const int32_t* d_recv, const int64_t* d_rc, int ws, int cell_bits, int64_t* d_perm, uint8_t* d_first,
                               int64_t* d_prev_r, int64_t* d_next_r, int32_t* d_reply, uint8_t* d_m3r, uint8_t* d_m4r, int64_t* d_cnt,
                               void* d_work, size_t work_bytes, void* stream);
AVL_API int avl_merge_classify(int64_t n, const int32_t* d_back, const int64_t* d_ordd, const int32_t* d_cell_sorted, int ws, int64_t* d_prev,
                               int64_t* d_next, uint8_t* d_is_new, uint8_t* d_m3, uint8_t* d_m4, int64_t* d_cnt, void* stream);

/* The 64-byte side record every local voxel sends to the owner of its final row (avlmaps_amd/parallel.py: MixedExchange):
 * [row | cell << 32 | single << 63, sum_w4 (4 x f64), replay state (3 x i64)].
 *   avl_merge_side_pack    sender: record i (final-row order) from voxel d_order[i]: d_rows_sorted[i], d_single_sorted[i] (by position),
 *                          d_cell / d_w4 (n x 4) / d_state (n x 3, nullable = zeros; sent only where d_next[voxel] < 0,
 *                          d_next nullable = everywhere) (by voxel) -> d_side (n x 8 int64)
 *   avl_merge_side_unpack  owner: R records that arrived -> d_rows[i] = row - r0 (clamped into the block), d_own_cell[row] = cell,
 *                          d_state[row] = the state of the voxel's LAST contributor (`started` != 0); d_own_cell (n_own) and
 *                          d_state (n_own x 3) are zeroed by the caller.  A row outside [r0, r0 + n_own) is skipped and sets
 *                          bit 0 of *d_err_flag (nullable).
 * The reference has no such step (one process, one map: vlmap_builder.py:136-178); it is part of the N-rank merge of north_star. */
AVL_API int avl_merge_side_pack(int64_t n, const int64_t* d_order, const int64_t* d_rows_sorted, const uint8_t* d_single_sorted,
                                const int32_t* d_cell, const double* d_w4, const int64_t* d_state, const int64_t* d_next, int64_t* d_side,
                                void* stream);
AVL_API int avl_merge_side_unpack(int64_t R, const int64_t* d_side, int64_t r0, int64_t n_own, int64_t* d_rows, int32_t* d_own_cell,
                                  int64_t* d_state, int* d_err_flag, void* stream);

/* The N-rank merge of the map build, second form ("gather plan"; avlmaps_amd/merge2.py carries the collectives, csrc/avl_merge2.hip
 * holds the kernels).  The reference has no such step (one process, one map: vlmap_builder.py:102-183 is the loop being sharded); a
 * voxel's final row is the reference's voxel id = its position in first-touch order (vlmap_builder.py:163-170).
 *   avl_merge2_prepare  a rank's own list, sorted by first-touch key (keys below 2^key_bits): d_key_sorted, d_cell_sorted, d_perm (n x i32:
 *                     position in that order -> voxel slot), d_hdr[4] = n, smallest key, largest key, flags (the header every rank
 *                     all_gathers first).
 *   avl_merge2_plan   EVERY rank, after the all_gather of the ranks' key-sorted (first-touch key, cell) lists: d_gathered holds ws chunks
 *                     of nmax + (nmax + 1) / 2 int64 words each -- [keys (nmax x i64) | cells (nmax x i32)], h_n_all[p] entries valid in
 *                     chunk p; keys must be ordered by rank (contiguous frame shards), so that the concatenation is in key order and a
 *                     voxel's row is the number of first contributors before it; cells below 2^cell_bits; d_perm: this rank's own
 *                     avl_merge2_prepare permutation.  Work buffer: avl_merge2_work_bytes(sum n, n of this rank, ws, nchunk).  Results (byte offsets into
 *                     d_work returned in h_off[11]): 0 row (n x i32, final row of own voxel s), 1 prev, 2 next (n x i32: the
 *                     neighbouring contributors of the voxel in rank order, -1 = none), 3 order (n x i32: own voxels in final-row
 *                     order), 4 sidx (n x i32: single-rank voxels before position i of that order), 5 selA, 6 selB (n x i64:
 *                     avl_builder_replay_chain selections: s where prev < 0 / prev >= 0, else -1), 7 idx_prev, 8 idx_next
 *                     (n x i32: own voxels grouped by prev / next rank, final-row order inside a group, voxels without one last;
 *                     only with want_replay_lists), 9 rowcell (M x i32: cell of every final row), 10 the device copy of h_res.
 *                     h_res[2 + 3 ws^2] (host; the call synchronises once to deliver it): M, the first-touch key of row grow_row
 *                     (-1 if M <= grow_row), then three ws x ws tables [sender p][receiver q]: voxels of p whose row q owns, the
 *                     single-rank ones among them, voxels of q whose previous contributor is p.
 *                     With nchunk > 0 (<= avl_merge2_max_chunks; chunk_rows * nchunk must cover ceil(sum n / ws) rows) h_res continues
 *                     with nchunk x two ws x ws tables: the first two tables restricted to rows [q per + c chunk_rows, q per + (c + 1)
 *                     chunk_rows) of every owner q's block (per = ceil(M / ws)) -- the sizes of an exchange done chunk by chunk.
 *   avl_builder_m2_pack   sender, ONE exchange (the whole payload or one chunk of it): the n voxels of the call in destination order --
 *                     wave w serves rank q with h_cum[q] <= w < h_cum[q + 1] and is voxel h_lo[q] + (w - h_cum[q]) of d_order (the
 *                     rank's final-row order; h_dlo[q] single-rank voxels precede h_lo[q] there) -> the send buffer (int64 words):
 *                     64-byte side records at word h_side_off[q] ([row - h_row0[q] | list index << 32 | single << 63 | direct << 62,
 *                     sum_w4 (4 x f64), 3 zero words]), finished float32 rows of single-rank voxels at h_done_off[q] (row stride
 *                     (D + 1) / 2 words), float64 partial rows of shared voxels at h_part_off[q].  d_own_feat (nullable): this rank's
 *                     block of grid_feat (first row own_r0) -- single-rank voxels whose row it owns are written there directly (`direct`).
 *   avl_merge2_side_state  after the replay: words 5..7 of the call's side records (same h_cum / h_lo) = the replay state (d_state n x 3
 *                     i64, nullable) where this rank is the voxel's last contributor (d_next < 0), zeros elsewhere.
 *   avl_merge2_state_gather / _scatter   the 24-byte replay states of the listed voxels <-> a contiguous hop buffer.
 *   avl_merge2_fold   owner: the block [r0, r0 + n_own) from what the peers sent (h_side / h_done / h_part: per peer the device
 *                     addresses of its three lists, h_count[p] records; the rank's own lists stay in its send buffer): contributors
 *                     summed in rank order, grid_feat / grid_pos / weight / grid_rgb / cell of the block written.  d_work: 256-aligned scratch of
 *                     avl_merge2_fold_work_bytes (which record of peer p belongs to row r, sum alpha and a to-do flag per row).  Bits of *d_err_flag: 1 = a record outside the
 *                     block, 2 = a row nobody sent, 4 = a single-rank record next to other contributors. */
AVL_API int avl_merge2_load(void);   /* load the merge's code object now (avl_builder_create does): not inside the first merge */
AVL_API int avl_merge2_prepare_work_bytes(int64_t n, size_t* h_bytes);
AVL_API int avl_merge2_prepare(int64_t n, const int64_t* d_key, const int32_t* d_cell, int key_bits, int64_t flags, int64_t* d_key_sorted,
                               int32_t* d_cell_sorted, int32_t* d_perm, int64_t* d_hdr, void* d_work, size_t work_bytes, void* stream);
AVL_API int avl_merge2_max_chunks(int ws, int* h_max);    /* how many chunks of an owner's block the plan can size (tables in LDS) */
AVL_API int avl_merge2_work_bytes(int64_t n_entries, int64_t n_own, int ws, int nchunk, size_t* h_bytes);
AVL_API int avl_merge2_plan(int ws, int rank, const int64_t* h_n_all, int64_t nmax, const int64_t* d_gathered, const int32_t* d_perm,
                            int cell_bits, int64_t grow_row, int want_replay_lists, int64_t chunk_rows, int nchunk, void* d_work,
                            size_t work_bytes, int64_t* h_off, int64_t* h_res, void* stream);
AVL_API int avl_builder_m2_pack(avl_builder* b, int64_t n, int ws, int rank, int64_t own_r0, const int64_t* h_cum, const int64_t* h_lo,
                                const int64_t* h_dlo, const int64_t* h_row0, const int64_t* h_side_off, const int64_t* h_done_off,
                                const int64_t* h_part_off, const int32_t* d_order, const int32_t* d_row, const int32_t* d_prev,
                                const int32_t* d_next, const int32_t* d_sidx, int64_t* d_send, float* d_own_feat, void* stream);
AVL_API int avl_merge2_side_state(int64_t n, int ws, const int64_t* h_cum, const int64_t* h_lo, const int64_t* h_side_off,
                                  const int32_t* d_order, const int32_t* d_next, const int64_t* d_state, int64_t* d_send, void* stream);
AVL_API int avl_merge2_state_gather(int64_t k, const int32_t* d_idx, const int64_t* d_state, int64_t* d_out, void* stream);
AVL_API int avl_merge2_state_scatter(int64_t k, const int32_t* d_idx, const int64_t* d_in, int64_t* d_state, void* stream);
AVL_API int avl_merge2_fold(int64_t n_own, int64_t r0, int ws, int D, int gs, int vh, const void* const* h_side, const void* const* h_done,
                            const void* const* h_part, const int64_t* h_count, const int32_t* d_rowcell, int have_log, float* d_grid_feat,
                            int32_t* d_grid_pos, float* d_weight, uint8_t* d_grid_rgb, int32_t* d_cell, void* d_work, size_t work_bytes,
                            int32_t* d_err_flag, void* stream);
AVL_API int avl_merge2_fold_work_bytes(int64_t n_own, int ws, size_t* h_bytes);

/* Shared rows of a rank's block of the merged map: row d_rows[i] of d_out (n_out x D float32) = (float)(d_acc[i, :] / d_w4[d_rows[i], 0]),
 * i < k -- the division of finalize (vlmap_builder.py:172-174's running mean in closed form) applied to the float64 sums several
 * ranks contributed to (avlmaps_amd/parallel.py).  An index outside [0, n_out) is skipped and sets bit 0 of *d_err_flag (nullable). */
AVL_API int avl_rows_div_f32(int64_t k, int D, const double* d_acc, const int64_t* d_rows, const double* d_w4, float* d_out, int64_t n_out,
                             int32_t* d_err_flag, void* stream);
AVL_API int avl_replay_state_apply(int64_t n, const void* d_state, float* d_weight, uint8_t* d_grid_rgb, void* stream);
/* Mixed payload of the row-sharded merge (round 4).  A voxel only ONE rank touched is finished where its accumulators live:
 * d_out[i, :D] = (float)((a1^2 first_feat[s] + sum_feat[s]) / sum alpha), s = d_slots[i] -- the float64 expression of the
 * single-process finalisation (vlmap_builder.py:166-178 closed form), so the row is bit-identical to the single-process map and
 * travels as 4 B per element.  Voxels several ranks touched ship float64 partial sums: d_out[i, :D] = sum_feat[s] +
 * (d_own[i] ? a1^2 : a1) first_feat[s] (d_own[i] != 0: this rank holds the voxel's global first touch).  d_slots (k,) int32 distinct slots. */
AVL_API int avl_builder_export_rows_f32(avl_builder* b, int64_t k, const int32_t* d_slots, float* d_out, int64_t ld, void* stream);
AVL_API int avl_builder_export_rows_f64(avl_builder* b, int64_t k, const int32_t* d_slots, const uint8_t* d_own, double* d_out,
                                        int64_t ld, void* stream);
/* grid_pos / weight / grid_rgb / occupied_ids of n merged rows from their linear cells and their [sum alpha, sum alpha * (r, g, b)]
 * float64 quadruples d_w4 (n, 4) alone (avl_finalize_merged without the feature part); output row r is voxel id row0 + r. */
AVL_API int avl_finalize_side(int64_t n, int64_t row0, int gs, int vh, const int32_t* d_cell, const double* d_w4, int32_t* d_grid_pos,
                              float* d_weight, uint8_t* d_grid_rgb, int32_t* d_occupied_ids, void* stream);
/* Row-sharded merge (parallel.merge_accumulator_sharded; SURVEY.md 8e "reduce-scatter by voxel range"): rank r owns the final
 * rows [row0, row0 + nrows) and receives from every peer only that peer's contributions to them -- n rows of `cols` = D + 4
 * float64 with their final row index d_rows (n,) int64, a peer holds a voxel at most once so the indices of one call are
 * distinct.  d_dst[d_rows[i] - row0, :cols] += d_src[i, :cols].  Calls in peer order give a reproducible sum.  Synchronous
 * (reports an out-of-range row as AVL_ERR_INVALID). */
AVL_API int avl_rows_add_f64(int64_t n, int cols, const int64_t* d_rows, int64_t row0, int64_t nrows, const double* d_src,
                             int64_t ld_src, double* d_dst, int64_t ld_dst, void* stream);
/* The same fold without the host round trip: an out-of-range row index sets *d_err_flag (device int32, zeroed by the caller) to 1
 * and is skipped; the caller reads the flag once after the last peer (the round-4 merge folds up to ws lists per exchange). */
AVL_API int avl_rows_add_f64_async(int64_t n, int cols, const int64_t* d_rows, int64_t row0, int64_t nrows, const double* d_src,
                                   int64_t ld_src, double* d_dst, int64_t ld_dst, int32_t* d_err_flag, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (3) nearest-target distance-decay heatmap
 *     replaces  avlmaps/utils/visualize_utils.py:29-49 get_heatmap_from_mask_3d
 *     heat[i] = 1 for mask[i] != 0, else clip(1 - min_t ||pos_t - pos_i|| / cell_size * decay, 0, 1)
 * ------------------------------------------------------------------------------------------------ */
AVL_API int avl_heatmap_from_mask(const int32_t* d_grid_pos, const uint8_t* d_mask, int64_t N, double cell_size,
                                  double decay_rate, float* d_heat, void* stream);
/* The same heat for a map that is queried again and again (AVLMap.index_object on one map, many object names): a PLAN holds what
 * depends on the voxel positions only -- the bounding box, the voxels in CELL order (one radix sort) and the zeroed bit-grid
 * buffers -- so that a call is a memset, a scatter of the targets and the window scan walked in cell order (the lanes of a wave
 * are then spatial neighbours and their column loads coalesce: the scan is 3x faster than in voxel-id order, and no host
 * round trip for the bounding box remains).  Results are the same bits as avl_heatmap_from_mask.  d_grid_pos is caller-owned
 * and must outlive the plan; one plan = one device = one host thread at a time.  AVL_ERR_INVALID when the bounding box has
 * >= 2^32 cells (use the stateless call). */
typedef struct avl_heat_plan avl_heat_plan;
AVL_API int avl_heat_plan_create(avl_heat_plan** h_out, const int32_t* d_grid_pos, int64_t N, void* stream);
AVL_API int avl_heat_plan_destroy(avl_heat_plan* plan);
AVL_API int avl_heatmap_from_mask_planned(avl_heat_plan* plan, const uint8_t* d_mask, double cell_size, double decay_rate,
                                          float* d_heat, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (4) top-down 2-D products of the voxel map (the consumers that loop over all N voxels in Python upstream).
 *     All take device pointers; images are row-major uint8 with 1 = true.  Synchronous (they report index errors).
 *     Voxel positions index the image like NumPy does: negative values wrap once, anything else out of range is the
 *     reference's IndexError -> AVL_ERR_INVALID.
 * ------------------------------------------------------------------------------------------------ */
/* avlmaps/utils/visualize_utils.py:77-83 pool_3d_label_to_2d: mask2d[row, col] |= mask[i].  d_mask2d (gs, gs) is cleared first. */
AVL_API int avl_pool_label_2d(const int32_t* d_grid_pos, const uint8_t* d_mask, int64_t N, int gs, uint8_t* d_mask2d, void* stream);
/* avlmaps/map/map.py:106-113 generate_rgb_topdown_map: rgb2d[row, col] = grid_rgb[i], the LAST voxel (largest i) of a
 * column wins as in the sequential loop; untouched cells are 0.  d_rgb2d (gs, gs, 3). */
AVL_API int avl_rgb_topdown(const int32_t* d_grid_pos, const uint8_t* d_grid_rgb, int64_t N, int gs, uint8_t* d_rgb2d, void* stream);
/* avlmaps/map/map.py:79-95 generate_obstacle_map: free[r, c] = no voxel id > 0 among heights [h_begin, h_end) of
 * occupied_ids (n0, n1, vh) -- the index range of `(heights > h_min) & (heights < h_max)`, which the host evaluates in
 * float64 exactly as upstream.  Asynchronous. */
AVL_API int avl_obstacle_map(const int32_t* d_occupied_ids, int n0, int n1, int vh, int h_begin, int h_end, uint8_t* d_free,
                             void* stream);
/* avlmaps/utils/index_utils.py:163-177 (body of get_dynamic_obstacles_map_3d after the argmax): voxels whose class
 * d_class[i] (the similarity kernel's argmax, still on the device) has h_class_is_obstacle[class] != 0 mark
 * (row - rmin, col - cmin) of the (H, W) crop; out_free = !(marked & (cropped_free == 0)). */
AVL_API int avl_obstacle_scatter(const int32_t* d_grid_pos, const int32_t* d_class, int64_t N, const uint8_t* h_class_is_obstacle,
                                 int Q, int rmin, int cmin, int H, int W, const uint8_t* d_cropped_free, uint8_t* d_out_free,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * (6) sliding-window merge of the pixel-feature extractor's output (device-resident, channels-last)
 *     replaces  avlmaps/utils/lseg_utils.py:61-102 (window accumulation, count normalisation, crop, and the per-frame
 *               device-to-host copy of the (1, D, Hf, Wf) result)
 *     d_win     (G, D, crop, crop) row-major: the model's output for the batch of G windows, float32 (is_f16 = 0) or float16
 *     h_origin  (G, 2) host int32: (h0, w0) of every window on the padded canvas, in the reference's loop order (idh major)
 *     d_out     (height, width, D) float32 channels-last -- the layout avl_builder_integrate_frame gathers from:
 *               out[y, x, :] = (sum over the windows g covering (y, x), in window order, of win[g, :, y - h0, x - w0]) / count
 *     G <= 64.  Every pixel of (height, width) must be covered by a window (AVL_ERR_INVALID otherwise).
 * ------------------------------------------------------------------------------------------------ */
AVL_API int avl_lseg_merge_windows(const void* d_win, int is_f16, int G, int D, int crop, const int32_t* h_origin, int height,
                                   int width, float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (7) 2-D goal fields of the area, sound and image queries, and their lift to the voxels (csrc/avl_field2d.hip)
 *     Cells are (row, col) int32 pairs of the full (gs, gs) map; the host converts poses to cells (the Habitat dataloader path,
 *     float64) once per loaded map.  Given the same peaks every result is the reference's bits (correctly rounded sqrt and
 *     divisions, no FMA contraction).  decay_rate must be finite and >= 0.  All calls are asynchronous.
 * ------------------------------------------------------------------------------------------------ */
/* avlmaps/map/avlmap.py:78-96 index_area_2d before its normalisation (one scipy EDT per pose upstream):
 *   field[r, c] = max(0, max over poses i with 0 <= cell_i < gs of clip(peak_i - decay * ||(r, c) - cell_i||, 0, 1))  (float64)
 * d_cells (P, 2) int32, d_peaks (P,) float64 (the min-max normalised frame scores); poses outside the grid are skipped.
 * d_minmax (2,) float64 device receives [min, max] of the whole field. */
AVL_API int avl_field_area(const int32_t* d_cells, const double* d_peaks, int64_t P, int gs, double decay_rate, double* d_field,
                           double* d_minmax, void* stream);
/* avlmaps/map/avlmap.py:111-131 index_sound_2d before its normalisation (one scipy EDT per segment upstream): for every
 * segment s in order, with d = the distance from the cell to the nearest of its locations,
 *   field = f32(field + max(p_s - (p_s * d) * decay, 0))   (the term in float64, the sum in float32; field starts at 0)
 * Locations of segment s are d_cells[d_offsets[s] .. d_offsets[s + 1]) of the (L, 2) int32 array, d_offsets (S + 1,) int64
 * non-decreasing (clamped to [0, L]); every location must lie inside the grid; d_peaks (S,) float32 >= 0.
 * d_minmax (2,) float32 device receives [min, max] of the whole field. */
AVL_API int avl_field_sound(const int64_t* d_offsets, const int32_t* d_cells, int64_t L, const float* d_peaks, int64_t S, int gs,
                            double decay_rate, float* d_field, float* d_minmax, void* stream);
/* avlmaps/map/avlmap.py:97,100-109 and :132,135-144 (min-max normalisation + the Python loop over occupied_ids): for every voxel
 *   heat[i] = f32((field[row_i, col_i] - min) / (max - min)), or 0 when grid_pos[i] lies outside the (gs, gs, vh) grid
 * is_f64 = 1: a float64 field and d_minmax (avl_field_area), normalised in float64; 0: float32 (avl_field_sound).
 * max == min gives NaN as upstream; the caller checks d_minmax. */
AVL_API int avl_field_lift(const void* d_field, int is_f64, const void* d_minmax, int gs, int vh, const int32_t* d_grid_pos, int64_t N,
                           float* d_heat, void* stream);
/* the normalised 2-D map itself (the return value of index_area_2d / index_sound_2d): d_out (gs, gs) of the field's type */
AVL_API int avl_field_normalize(const void* d_field, int is_f64, const void* d_minmax, int gs, void* d_out, void* stream);
/* avlmaps/map/avlmap.py:154-161 index_image after localisation: sim[i] = clip(1 - decay * ||grid_pos[i, :2] - (row, col)||, 0, 1)
 * in float64, d_sim (N,) float64 */
AVL_API int avl_planar_decay(const int32_t* d_grid_pos, int64_t N, int64_t row, int64_t col, double decay_rate, double* d_sim,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * (7b) cross-modal goals: the product of per-voxel heats and its first maximum in one pass (csrc/avl_goal.hip)
 *     replaces  avlmaps/robot/habitat_lang_robot.py:377-430 as generated robot code uses them: get_map_3d(..) * get_major_map_3d(..)
 *               * ... on (N,) host arrays (:377-425), then get_max_pos_3d = grid_pos[np.argmax(heat)] (:427-430)
 *     A term is one factor of the product, evaluated at voxel i with grid_pos[i] = (r, c, h) and widened to float64 exactly:
 *       AVL_GOAL_DENSE_F32 / _F64  d_data[i], (N,) float32 / float64: the object heat, or any heat the caller made
 *       AVL_GOAL_FIELD_F32 / _F64  the value avl_field_lift gives this voxel, bit for bit: d_data the (gs, gs) field, d_aux its
 *                                  (2,) [min, max], both float32 / float64 (avl_field_sound / avl_field_area); 0 outside (gs, gs, vh)
 *       AVL_GOAL_CONES             max over the n_points points j of clip(peak_j - decay * ||(r, c) - cell_j||, 0, 1) in float64:
 *                                  d_data (n_points, 2) int32 cells, d_aux (n_points,) float64 peaks.  One point with peak 1 is
 *                                  avl_planar_decay bit for bit (avlmap.py:154-161); several are get_distribution_map_3d
 *                                  (habitat_lang_robot.py:207-227, distances in cells)
 *     heat[i] = ((t_0 * t_1) * t_2) * ... in float64, left to right (the order NumPy multiplies the arrays in).
 * ------------------------------------------------------------------------------------------------ */
enum {
    AVL_GOAL_DENSE_F32 = 0,
    AVL_GOAL_DENSE_F64 = 1,
    AVL_GOAL_FIELD_F32 = 2,
    AVL_GOAL_FIELD_F64 = 3,
    AVL_GOAL_CONES = 4
};
#define AVL_GOAL_MAX_TERMS 8
typedef struct avl_goal_term {
    int32_t kind;         /* AVL_GOAL_* */
    int32_t gs;           /* field: the grid size, >= 1 */
    int32_t vh;           /* field: the grid height, >= 0 */
    int32_t reserved;     /* 0 */
    const void* d_data;   /* dense: the values; field: the field; cones: the cells */
    const void* d_aux;    /* field: [min, max]; cones: the peaks; dense: unused */
    int64_t n_points;     /* cones: the number of points, >= 1 */
    double decay;         /* cones: the decay per cell, finite and >= 0 */
} avl_goal_term;
/* h_terms: K terms on the host, 1 <= K <= AVL_GOAL_MAX_TERMS.  d_out (N,) float64 receives the product, or NULL: then nothing
 * of size N is written.  h_index / h_value / h_pos3 (each may be NULL) receive the first index of the maximum product, the product
 * there and grid_pos of that voxel: what np.argmax and habitat_lang_robot.py:427-430 return.  The order is (product descending,
 * index ascending); a NaN product never wins, and when every product is NaN the call fails with AVL_ERR_INVALID.  With any of the
 * three host outputs the call is synchronous and N == 0 is AVL_ERR_INVALID (there is no goal); with none of them it only enqueues
 * the product.  Arguments are checked before any device work. */
AVL_API int avl_goal_fuse(const avl_goal_term* h_terms, int K, const int32_t* d_grid_pos, int64_t N, double* d_out, int64_t* h_index,
                          double* h_value, int32_t* h_pos3, void* stream);

/* The same product over 2-D windows: avlmaps/robot/habitat_lang_robot.py:357-375 get_map(..) * get_major_map(..) * ... on (h, w)
 * host arrays, then get_max_pos (:419-425), np.argmax + np.unravel_index.  A term is an (h, w) window of a row-major float32 or
 * float64 device image: d_data points at the window's first value, ld is the image's row length in values. */
typedef struct avl_window_term {
    const void* d_data;   /* the window's first value */
    int64_t ld;           /* values per image row, >= w */
    int32_t is_f64;       /* 1: float64, 0: float32 (widened exactly) */
    int32_t reserved;     /* 0 */
} avl_window_term;
/* h_terms: K windows on the host, 1 <= K <= AVL_GOAL_MAX_TERMS, multiplied left to right in float64.  d_out (h, w) float64 receives
 * the product, or NULL.  h_index / h_value (each may be NULL) receive row * w + col of the first maximum in raster order and the
 * product there; with either of them the call is synchronous.  A NaN product never wins; all NaN is AVL_ERR_INVALID.  Arguments are
 * checked before any device work. */
AVL_API int avl_product_argmax_2d(const avl_window_term* h_terms, int K, int h, int w, double* d_out, int64_t* h_index, double* h_value,
                                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * (8) visibility-graph navigation on the 2-D obstacle map (csrc/avl_nav.hip)
 *     The obstacle map is (H, W) uint8, nonzero = free, 0 = obstacle (Map.obstacles_cropped).  Obstacle pixel (r, c) is the point
 *     (r, c); the obstacle set is the union of the segments between 8-adjacent obstacle pixels and the convex hulls of the obstacle
 *     corners of every 2 x 2 window holding 3 or 4 (DESIGN.md "Navigation").  Path vertices are the obstacle pixels whose obstacle
 *     8-neighbours (at least one) lie within 135 degrees, in raster order; their ids are their positions in that list.
 *     The graph stays on the device behind the opaque handle until avl_nav_destroy.  H, W <= 32768; at most 65 536 vertices.
 * ------------------------------------------------------------------------------------------------ */
/* avlmaps/utils/navigation_utils.py:77-127 build_visgraph_with_obs_map (cv2.findContours + pyvisgraph's VisGraph.build) and
 * avlmaps/navigator/navigator.py:11-15 Navigator.build_visgraph: uploads h_obs, finds the vertices and fills the symmetric
 * V x V visibility bitset.  Synchronous.  More than 65 536 vertices: AVL_ERR_CAPACITY and no handle. */
AVL_API int avl_nav_create(const uint8_t* h_obs, int H, int W, void* stream, void** h_graph);
AVL_API int avl_nav_destroy(void* graph);
AVL_API int avl_nav_num_vertices(void* graph, int64_t* h_V);
/* the vertex list, (V, 2) int32 (row, col) on the host (synchronous) */
AVL_API int avl_nav_vertices(void* graph, int32_t* h_verts, void* stream);
/* the visibility bitset on the host, (V, ceil(V / 64)) uint64 words: bit b % 64 of word (a, b / 64) = vertices a and b see each
 * other (the diagonal is 0); synchronous */
AVL_API int avl_nav_export_visibility(void* graph, uint64_t* h_bits, void* stream);
/* avlmaps/utils/navigation_utils.py:130-197 plan_to_pos_v2 from the pyvisgraph shortest_path call on, and navigator.py:17-30
 * Navigator.plan_to: the visibility of the start (sr, sc) and the goal (gr, gc) -- float64 points inside the map -- to every vertex
 * and to each other, then the float64 shortest path from the start over the graph (edge length sqrt(dr * dr + dc * dc)).
 * Node ids in h_path: vertices 0 .. V-1, V = the start, V + 1 = the goal; the path runs start -> goal, ties between predecessors
 * go to the smallest id.  A visible edge is used only where it leaves each vertex end outside the angular span of that vertex's
 * obstacle neighbours and not along a wall whose neighbours lie on both sides of it.  *h_dist = the path length, +inf and *h_len = 0 when the goal is unreachable.  cap = the capacity of
 * h_path (V + 2 always suffices).  Synchronous. */
AVL_API int avl_nav_plan(void* graph, double sr, double sc, double gr, double gc, double* h_dist, int32_t* h_path, int* h_len,
                         int cap, void* stream);
/* the last plan's internals, for tests and tools (each pointer may be NULL): h_dist (V + 2,) float64 distances from the start,
 * h_pred (V + 2,) int32 predecessors (-1 for the start and unreached nodes), h_qbits (2, ceil(V / 64)) uint64 vertex visibility
 * of the start and of the goal, h_sg the start-goal visibility.  Synchronous. */
AVL_API int avl_nav_last_plan(void* graph, double* h_dist, int32_t* h_pred, uint64_t* h_qbits, int32_t* h_sg, void* stream);

/* Many goals from one start (DESIGN.md 4.6 "Many goals").  (The prefix is avl_navmany_, not avl_nav_: the set of avl_nav_*
 * declarations is pinned by tests/test_navigator_host.py and stays the single-plan interface.)  These entry points work on the avl_nav_create handle and keep buffers of
 * their own on it (grown on demand, freed by avl_nav_destroy): single plans and batches may interleave on one graph, and
 * avl_nav_last_plan keeps describing the last avl_nav_plan.  At most 2^20 points per call; M = 0 is valid and touches no output
 * array.  Every point must be finite and inside [0, H - 1] x [0, W - 1] (AVL_ERR_INVALID otherwise, as in avl_nav_plan).
 * Synchronous.
 *
 * avl_navmany_snap: navigation_utils._in_obstacle + _nearest_free for M points, h_pts (M, 2) float64 (row, col).  A point is inside
 * the obstacle set when its int() cell is an obstacle, or when that cell is free, the other three cells of the 2 x 2 window below
 * and right of it are obstacles and the point lies strictly beyond the hypotenuse ((r - int r) + (c - int c) > 1, not on a grid
 * line).  Such a point moves to the free cell with the smallest (r - pr) * (r - pr) + (c - pc) * (c - pc), evaluated in float64
 * without contraction; ties go to the first cell in raster order (smallest row, then smallest column), which is np.argmin over
 * np.where.  h_out (M, 2) float64 gets the cell (h_moved[k] = 1) or the point unchanged (h_moved[k] = 0).  The search goes outward
 * ring by ring from the point's cell and stops once no cell further out can beat or tie the best.  A map without a free cell:
 * AVL_ERR_STATE. */
AVL_API int avl_navmany_snap(void* graph, const double* h_pts, int64_t M, double* h_out, uint8_t* h_moved, void* stream);
/* avl_navmany_plan: the start's visibility row and the shortest-path tree from (sr, sc) over the V vertices (the relaxation and the
 * predecessor rule of avl_nav_plan, no goal node taking part), then every goal of h_goals (M, 2) float64 against the tree:
 *   h_dist[k] = min(fl(D[u] + |u g_k|) over the vertices u that see g_k, with D[u] finite and the edge usable at u; |s g_k| when the
 *               start sees the goal); +inf when nothing reaches the goal;
 *   h_via[k]  = the node the goal hangs on: the SMALLEST vertex id that attains the minimum, V (the start) only when no vertex does;
 *               -1 for an unreachable goal;
 *   *h_best   = the SMALLEST k with the smallest finite h_dist[k]; -1 when there is none (also for M = 0).
 * h_dist[k] and the path of goal k equal avl_nav_plan's for the same start and goal, bit for bit. */
AVL_API int avl_navmany_plan(void* graph, double sr, double sc, const double* h_goals, int64_t M, double* h_dist, int32_t* h_via,
                             int64_t* h_best, void* stream);
/* the node ids start .. goal k of the last avl_navmany_plan, read from the tree's predecessors and via[k] (no second relaxation):
 * V = the start, V + 1 = the goal, as in avl_nav_plan.  *h_len = 0 for an unreachable goal.  AVL_ERR_STATE before the first batch,
 * AVL_ERR_INVALID for k outside the batch or a buffer that is too small (V + 2 always suffices). */
AVL_API int avl_navmany_path(void* graph, int64_t k, int32_t* h_path, int* h_len, int cap, void* stream);
/* the pruning of the last avl_navmany_plan, for tools/probe_plan_many.py ("the share of walks that pruning skipped"):
 * h_counts[0] = goal-vertex walks started, h_counts[1] = goal-vertex pairs with a finite candidate distance (the walks an unpruned
 * kernel would start).  Counting is off until avl_navmany_count_walks(graph, 1): a batch then costs nothing for it.
 * avl_navmany_stats after a batch that did not count: AVL_ERR_STATE. */
AVL_API int avl_navmany_count_walks(void* graph, int on);
AVL_API int avl_navmany_stats(void* graph, uint64_t* h_counts);

/* ------------------------------------------------------------------------------------------------
 * (9) 2-D image morphology on top-down masks (csrc/avl_morph2d.hip): the SciPy / OpenCV calls of the planner's map smoothing.
 *     All pointers are device pointers unless named h_*; images are row-major, uint8 (nonzero = true on input, 0 / 1 on output)
 *     or float64.  All calls are asynchronous on `stream`; no call works in place.
 * ------------------------------------------------------------------------------------------------ */
enum { AVL_MORPH_DILATE = 0, AVL_MORPH_ERODE = 1 };
enum { AVL_MORPH_CROSS = 0, AVL_MORPH_BOX = 1 };
/* scipy.ndimage.binary_dilation / binary_erosion(x, structure, iterations) with border_value = 0 and no mask, as called in
 * avlmaps/map/vlmap.py:168,171 (cross = generate_binary_structure(2, 1), the default) and avlmaps/map/map.py:175-179
 * (box = np.ones((3, 3))).  k iterations = one pass with the L1 diamond / the Chebyshev square of radius k; cells outside the image
 * count as 0 for both ops, so erosion eats k cells inwards from every edge.  1 <= iterations <= 127, else AVL_ERR_INVALID.
 * d_tmp (H * W bytes) is needed for iterations > 4 only. */
AVL_API int avl_morph_binary(const uint8_t* d_in, int H, int W, int op, int structure, int iterations, uint8_t* d_out, uint8_t* d_tmp,
                             void* stream);
/* scipy.ndimage.gaussian_filter(x.astype(float), sigma, truncate=t) (vlmap.py:169, map.py:173): mode 'reflect', axis 0 first, then
 * axis 1, float64, SciPy's summation order for a symmetric kernel -- the result has SciPy's bits.  h_weights: the 2 * radius + 1
 * weights of _gaussian_kernel1d on the host (radius = int(t * sigma + 0.5) <= 32).  d_in is uint8 (in_is_u8 != 0) or float64.
 * d_out_f64 (H, W) and d_out_gt_u8 (H, W) = value > threshold may each be NULL, not both; d_tmp: H * W float64. */
AVL_API int avl_gauss2d_f64(const void* d_in, int in_is_u8, int H, int W, const double* h_weights, int radius, double* d_out_f64,
                            uint8_t* d_out_gt_u8, double threshold, double* d_tmp, void* stream);
/* cv2.resize(x, (2 * W, 2 * H)) with the default INTER_LINEAR (map.py:172): destination index i samples the source at
 * (i + 0.5) / 2 - 0.5 -- fraction 0.75 for even i, 0.25 for odd i -- with source indices clamped at both ends.
 * d_in (H, W) uint8 or float64 -> d_out (2 * H, 2 * W) float64. */
AVL_API int avl_resize2x_up_f64(const void* d_in, int in_is_u8, int H, int W, double* d_out, void* stream);
/* cv2.resize(x, (W, H)) of a (2 * H, 2 * W) image (map.py:180): the mean of every 2 x 2 block.  -> d_out (H, W) float64. */
AVL_API int avl_resize2x_down_f64(const void* d_in, int in_is_u8, int H, int W, double* d_out, void* stream);
/* avlmaps/map/map.py:169-181 Map._dilate_map on a (H, W) binary image: x2 up-sampling, gaussian(sigma, truncate 3), > 0.5, 3 x 3 box
 * dilation with 2 * dilate_iter iterations, x1/2 down-sampling.  d_out_f64 (H, W) is upstream's return value, d_out_zero_u8 (H, W)
 * is `result == 0`, what VLMap.customize_obstacle_map keeps (vlmap.py:156); each may be NULL, not both.  dilate_iter = 0 is SciPy's
 * "repeat until nothing changes": one set cell after the threshold fills the image.  0 <= dilate_iter <= 63, radius
 * int(3 * sigma + 0.5) <= 32.  ws: avl_dilate_map_work_bytes(H, W) bytes of device memory. */
AVL_API int avl_dilate_map_work_bytes(int H, int W, size_t* bytes);
AVL_API int avl_dilate_map(const uint8_t* d_binary_u8, int H, int W, int dilate_iter, double sigma, double* d_out_f64,
                           uint8_t* d_out_zero_u8, void* ws, size_t ws_bytes, void* stream);
/* avlmaps/map/vlmap.py:166-171 VLMap.get_pos: the crop [r0:r1, c0:c1] of a mask with rows of ld cells (the pooled (gs, gs) mask of
 * avl_pool_label_2d), then binary_closing(iterations=3), gaussian_filter(sigma=0.8, truncate=3), > 0.5, binary_dilation -- all with
 * the crop's borders.  d_out_u8 (r1 - r0, c1 - c0).  ws: avl_mask_foreground_work_bytes(r1 - r0, c1 - c0) bytes of device memory. */
AVL_API int avl_mask_foreground_work_bytes(int H, int W, size_t* bytes);
AVL_API int avl_mask_foreground(const uint8_t* d_mask2d_u8, int64_t ld, int r0, int r1, int c0, int c1, uint8_t* d_out_u8, void* ws,
                                size_t ws_bytes, void* stream);

/* scipy.ndimage.gaussian_filter(x.astype(np.float32), sigma, truncate=t) as avlmaps/robot/habitat_lang_robot.py:231-232 calls it
 * on the predicted mask: SciPy filters a float32 array in float32 storage -- every line is accumulated in double in the order of
 * avl_gauss2d_f64, and the intermediate (after axis 0) and the result are rounded to float32.  The result has SciPy's float32 bits.
 * d_in: uint8 (in_is_u8 != 0, nonzero = 1.0f) or float32, rows of ld values (a window of a larger image: ld > W); h_weights as for
 * avl_gauss2d_f64.  d_out_f32 (H, W) and d_out_gt_u8 (H, W) = stored value > threshold may each be NULL, not both; d_tmp: H * W
 * float32. */
AVL_API int avl_gauss2d_f32(const void* d_in, int in_is_u8, int64_t ld, int H, int W, const double* h_weights, int radius, float* d_out_f32,
                            uint8_t* d_out_gt_u8, double threshold, float* d_tmp, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (10) exact 2-D Euclidean distance transform and the decay maps of the 2-D goal queries (csrc/avl_edt2d.hip)
 *     Images are row-major uint8 with rows of ld cells (a window of a larger image: ld > W), 1 <= H, W <= 16384 -- beyond that the
 *     squared distance leaves 32 bits: AVL_ERR_INVALID before any device work.  Results are float64 (H, W), contiguous.  All calls
 *     are asynchronous.  d_found (1 int32, device) receives 1 when the image has a cell to measure to and 0 when it has none; the
 *     result is then meaningless and the caller reports it (SciPy measures to an imaginary cell outside the image there).
 *     ws: avl_edt2d_work_bytes(H, W) bytes of device memory.
 * ------------------------------------------------------------------------------------------------ */
AVL_API int avl_edt2d_work_bytes(int H, int W, size_t* bytes);
/* scipy.ndimage.distance_transform_edt(image) (habitat_lang_robot.py:233, visualize_utils.py:98): per cell the distance to the
 * nearest zero cell, 0 on zero cells, SciPy's bits (the minimum of the exact integer squared distances, one correctly rounded
 * sqrt).  invert != 0 measures to the nearest NON-zero cell instead: distance_transform_edt(image == 0). */
AVL_API int avl_edt2d(const uint8_t* d_image_u8, int64_t ld, int H, int W, int invert, double* d_out_f64, int32_t* d_found, void* ws,
                      size_t ws_bytes, void* stream);
/* habitat_lang_robot.py:233-236 (and :284-287, :298-301, :315-318) and visualize_utils.py:98-100 on a mask (nonzero = target):
 *   d = distance_transform_edt(mask == 0);  t = 1 - (d / cell_size) * decay_rate;  t < 0 -> 0;
 *   normalize != 0:  (t - min t) / (max t - min t)
 * in NumPy's float64 operation order.  cell_size = 1 is the robot's expression (a division by 1.0 is the identity), cell_size = cs
 * is get_heatmap_from_mask_2d.  d_minmax (2 float64, device; required with normalize, else optional) receives [min t, max t]:
 * max == min gives NaN as upstream, the caller checks.  decay_rate finite and >= 0, cell_size finite and > 0. */
AVL_API int avl_mask_decay_2d(const uint8_t* d_mask_u8, int64_t ld, int H, int W, double cell_size, double decay_rate, int normalize,
                              double* d_out_f64, double* d_minmax, int32_t* d_found, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (11) object islands of a 2-D mask: labels, table, outer contours, nearest pair of two contours (csrc/avl_islands.hip)
 *     The island step of navigation_utils.py:10-36 (get_segment_islands_pos) and the distance matrix of map.py:351-364
 *     (find_middle_bewteen_contours).  Images are row-major (H, W), 1 <= H, W <= 16384 and H * W <= 2^28: AVL_ERR_INVALID before
 *     any device work otherwise.  All calls are asynchronous; every result is unique (the bytes do not depend on scheduling).
 * ------------------------------------------------------------------------------------------------ */
AVL_API int avl_label_islands_work_bytes(int H, int W, size_t* bytes);
/* 8-connected components of the non-zero cells of a uint8 mask with rows of ld cells: d_labels (H, W) int32, background 0, islands
 * 1 .. n in raster order of their first pixel = scipy.ndimage.label(mask, np.ones((3, 3))); *d_n (1 int32, device) = n. */
AVL_API int avl_label_islands(const uint8_t* d_mask_u8, int64_t ld, int H, int W, int32_t* d_labels, int32_t* d_n, void* ws, size_t ws_bytes,
                              void* stream);
/* d_table (n, 8) int32, row k - 1 for label k: area, rmin, rmax, cmin, cmax, first_row, first_col, 0.  n is avl_label_islands' count
 * (at most ceil(H / 2) * ceil(W / 2)); n = 0 does nothing. */
AVL_API int avl_island_table(const int32_t* d_labels, int H, int W, int32_t n, int32_t* d_table, void* stream);
/* The outer boundary of every island by Moore tracing from (first_row, first_col): neighbour order W NW N NE E SE S SW, the scan
 * restarting at (d + 5) % 8, stop at the first return to the start or when no neighbour is found, at most 4 * H * W + 8 steps.
 * d_points == NULL (and d_offsets == NULL): the count pass, the number of points of island k goes to d_table[k - 1][7].
 * Otherwise the write pass: island k's (row, col) int32 pairs go to d_points[d_offsets[k - 1] ...]; d_points holds n_points pairs
 * and nothing is written past an island's counted length or past n_points. */
AVL_API int avl_trace_islands(const int32_t* d_labels, int H, int W, int32_t n, int32_t* d_table, const int64_t* d_offsets, int32_t* d_points,
                              int64_t n_points, void* stream);
AVL_API int avl_nearest_pair_work_bytes(int64_t na, int64_t nb, size_t* bytes);
/* d_a (na, 2), d_b (nb, 2) int32 points, 1 <= na, nb <= 2^24, |coordinate| <= 2^15.  d_out3 (3 int64, device) = i, j, d2: the pair
 * with the smallest squared distance, among equals the smallest i * nb + j =
 * np.unravel_index(np.argmin(np.linalg.norm(a[:, None] - b[None], axis=2)), (na, nb)).  The matrix is never built. */
AVL_API int avl_nearest_pair_i32(const int32_t* d_a, int64_t na, const int32_t* d_b, int64_t nb, int64_t* d_out3, void* ws, size_t ws_bytes,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * (12) headless rendering of a per-voxel heat (csrc/avl_render.hip)
 *     d_table is the colour map as data: (256, 3) uint8 RGB, 768 bytes of device memory.  d_heat is (N,) float32 or float64
 *     (heat_is_f64 = 0 | 1); a heat that is NaN or outside [0, 1] has no defined uint8 cast: AVL_ERR_INVALID, nothing is clamped.
 *     The blend is NumPy 2's:  float64(float32(table[idx]) * float32(t)) + float64(rgb) * (1 - t),  idx = (heat * 255).astype(uint8)
 *     with the product in the heat's own dtype.  0 <= transparency <= 1.  Images are row-major (rows, columns, 3) uint8; every image
 *     is unique (its bytes do not depend on scheduling).  N < 2^31.
 * ------------------------------------------------------------------------------------------------ */
/* avlmaps/utils/visualize_utils.py:59-64 convert_heatmap_to_rgb per voxel: d_out_f64 (N, 3) float64 is the expression itself,
 * d_out_u8 (N, 3) its truncating .astype(np.uint8) (visualize_utils.py:111); either may be NULL, not both.  Synchronous. */
AVL_API int avl_render_colorize(const void* d_heat, int heat_is_f64, const uint8_t* d_grid_rgb, const uint8_t* d_table, int64_t N,
                                double transparency, double* d_out_f64, uint8_t* d_out_u8, void* stream);
AVL_API int avl_render_topdown_work_bytes(int H, int W, size_t* bytes);
/* avlmaps/utils/visualize_utils.py:117-128 visualize_heatmap_2d on the window rows [rmin, rmax], columns [cmin, cmax] (inclusive) of
 * the (gs, gs) map, without a dense heat image: per cell the colour of the voxel with the largest h (avlmaps/map/map.py:106-113 with the
 * height test upstream meant) blended with table[idx(the largest heat of the column)].  d_out (rmax - rmin + 1, cmax - cmin + 1, 3);
 * cells without a voxel get h_background3.  Positions wrap and fail like avl_rgb_topdown's.  ws: avl_render_topdown_work_bytes of the
 * window's shape.  Synchronous. */
AVL_API int avl_render_topdown(const int32_t* d_grid_pos, const void* d_heat, int heat_is_f64, const uint8_t* d_grid_rgb,
                               const uint8_t* d_table, int64_t N, int gs, int rmin, int rmax, int cmin, int cmax, double transparency,
                               const uint8_t* h_background3, uint8_t* d_out, void* ws, size_t ws_bytes, void* stream);
AVL_API int avl_render_view_work_bytes(int W, int H, size_t* bytes);
/* avlmaps/utils/visualize_utils.py:10-26 visualize_rgb_map_3d without a window: a z-buffered splat of the voxels from a pinhole
 * camera.  h_T34: 3 x 4 float64, row-major, from cell coordinates (row, col, h, 1) to the camera frame (x right, y down, z forward,
 * in cells).  Per voxel, in float64 and this order: p = T (row, col, h, 1) as a left-to-right sum of four products per row; culled
 * unless z > znear; u = fx * x / z + cx, v = fy * y / z + cy; half = min(0.5 * fx / z, 0.5 * smax); pixels floor(u - half) ..
 * floor(u + half) by floor(v - half) .. floor(v + half), clipped to the image.  A pixel shows d_color_u8 (N, 3) of the voxel with
 * the smallest (float32(z), id), or h_background3.  1 <= W, H <= 8192, znear >= 0, 1 <= smax <= 8192.  d_out (H, W, 3).
 * Asynchronous. */
AVL_API int avl_render_view(const int32_t* d_grid_pos, const uint8_t* d_color_u8, int64_t N, const double* h_T34, double fx, double fy,
                            double cx, double cy, int W, int H, double znear, double smax, const uint8_t* h_background3, uint8_t* d_out,
                            void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (13) image localization geometry (csrc/avl_pnp.hip, csrc/avl_pnp_math.h)
 *     Float64 throughout.  Correspondences are d_points (M, 3) in the reference camera's frame and d_pixels (M, 2) in the query
 *     image, used as given (no half-pixel shift).  The query camera is the reference's SIMPLE_PINHOLE: f = K[0,0], cx = K[0,2],
 *     cy = K[1,2].  A pose is a row-major 3 x 4 [R|t], query camera from reference camera.  With (x, y, z) = R X + t, each row the
 *     left-to-right sum ((r0 X + r1 Y) + r2 Z) + t, a correspondence is an inlier when z > 0, x y z are finite and
 *     ((f (x / z) + cx) - u)^2 + ((f (y / z) + cy) - v)^2 <= max_error^2; a NaN anywhere is an outlier.  M <= 2^24.
 * ------------------------------------------------------------------------------------------------ */
/* the number of correspondences the RANSAC and scoring kernels stage in LDS at a time (larger M takes several stages) */
AVL_API int avl_pnp_lds_stage(void);
/* avlmaps/utils/localization_utils.py:461-473 with avlmaps/utils/mapping_utils.py:226-251 (depth2pc) evaluated at the matched pixels
 * only: d_kp_ref (M, 2) (x, y) in the reference image is truncated toward zero like astype(np.int32); the point is
 * ((Kinv[i,0] (x + 0.5) + Kinv[i,1] (y + 0.5)) + Kinv[i,2]) * depth[y, x], h_Kinv9 = inv(K_ref) row-major; it is kept when
 * 0.1 < p_z < 10.  d_depth (H, W) float32 or float64 (depth_is_f64) metres.  d_points (M, 3) / d_pixels (M, 2) receive the kept
 * points and their d_kp_query rows, compacted in input order; *h_count = M'.  d_counter2: two int32 of device scratch (M' and the
 * error word, read back in one copy).  A key point that is not finite or truncates outside the image (negative included: NumPy would
 * wrap it, no matcher produces it) is AVL_ERR_INVALID, the reference's IndexError; nothing is clamped.  Synchronous. */
AVL_API int avl_loc_lift(const void* d_depth, int depth_is_f64, int H, int W, const double* h_Kinv9, const double* d_kp_ref,
                         const double* d_kp_query, int64_t M, double* d_points, double* d_pixels, int32_t* d_counter2, int64_t* h_count,
                         void* stream);
AVL_API int avl_pnp_ransac_work_bytes(int n_hyp, size_t* bytes);
/* avlmaps/utils/localization_utils.py:478-498, the estimation half of pycolmap.absolute_pose_estimation: n_hyp P3P hypotheses.
 * Hypothesis h draws three distinct indices from the counter hash of (seed, h, draw) documented at the top of csrc/avl_pnp.hip
 * (d_triples (n_hyp, 3) int32, or NULL), solves Grunert's P3P for up to four poses (none for repeated or collinear points or when
 * no root is real and positive) and counts the inliers of each over all M correspondences.  d_hyp_counts (n_hyp,) int32: the best
 * count of each hypothesis (ties: the smallest solution index; 0 without a solution).  d_pose12 / d_count: the hypothesis with the
 * largest count, ties to the smallest h; [I|0] and 0 when no hypothesis has a solution.  ws (avl_pnp_ransac_work_bytes) holds the
 * (n_hyp, 3, 4) float64 best pose of every hypothesis afterwards, [I|0] where there is none.  3 <= M.  Asynchronous. */
AVL_API int avl_pnp_ransac(const double* d_points, const double* d_pixels, int64_t M, double f, double cx, double cy, double max_error,
                           uint32_t seed, int n_hyp, int32_t* d_triples, int32_t* d_hyp_counts, double* d_pose12, int32_t* d_count,
                           void* ws, size_t ws_bytes, void* stream);
/* inlier counts d_counts (P,) int32 of caller-supplied poses d_poses (P, 3, 4), and the uint8 inlier mask of pose 0 (d_mask0 (M,), or
 * NULL): the inlier test of avl_pnp_ransac, the same device function.  Asynchronous. */
AVL_API int avl_pnp_score(const double* d_points, const double* d_pixels, int64_t M, const double* d_poses, int P, double f, double cx,
                          double cy, double max_error, int32_t* d_counts, uint8_t* d_mask0, void* stream);
/* avlmaps/utils/localization_utils.py:486-498, the refinement half (refine_focal_length False): Levenberg-Marquardt on the inliers
 * of d_pose12 (fixed for the whole refinement), minimising the plain sum of squared pixel residuals over the update
 * R <- exp([w]x) R, t <- t + dt, in ONE launch that iterates on the device until the step norm |(w, dt)| < step_tol or max_iter
 * steps were tried.  The normal equations are summed in a fixed order.  d_out13: the refined 3 x 4 pose and the final cost;
 * d_out3 int32: steps tried, the inlier count of the refined pose over all M, the number of correspondences refined on; d_mask
 * (M,) uint8: the inlier mask of the refined pose.  Fewer than 3 inliers: the pose is returned as given.  Asynchronous. */
AVL_API int avl_pnp_refine(const double* d_points, const double* d_pixels, int64_t M, const double* d_pose12, double f, double cx,
                           double cy, double max_error, int max_iter, double step_tol, double* d_out13, int32_t* d_out3, uint8_t* d_mask,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * (14) the audio side of the sound map (csrc/avl_audio.hip)
 *     A recording is mono float32 in device memory, 1 <= n <= 2^31 - 1 samples.  Null pointers and ranges are rejected before any
 *     device work.  All three calls are asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------------ */
/* d_pcm: n interleaved frames of `channels` int16 (1 <= channels <= 8); d_audio_f32 (n,):
 * np.mean(pcm.astype(np.float32) / 32768, axis=1) in float32.  The sum of at most eight multiples of 2^-15 is exact in every
 * order, so the only rounding is the division by `channels`; one and two channels are exact. */
AVL_API int avl_audio_decode_pcm16(const int16_t* d_pcm, int64_t n, int channels, float* d_audio_f32, void* stream);
AVL_API int avl_audio_segment_work_bytes(int64_t n, size_t* h_bytes);
/* avlmaps/utils/audio_utils.py:515-546 segment_audio_with_silence on a whole recording.  Sample i is loud iff
 * d_audio[i] > threshold (float32; NaN is never loud; a NaN threshold is AVL_ERR_INVALID).  A loud sample starts a segment iff it is
 * the first loud sample or lies gap or more samples after the previous loud one; gap >= 1.  Segment k is (l, r): its start and the
 * last loud sample before the next start (or the last loud sample of all); the track upstream cuts is audio[l:r], r excluded, so a
 * lone loud sample gives l == r.  d_segments (cap, 2) int64 receives the first min(count, cap) pairs in ascending order and
 * d_count[0] (int64) the true count, which may exceed cap (cap = 0 only counts; d_segments may then be NULL).  d_ws:
 * avl_audio_segment_work_bytes(n).  Five launches, none waits on another, no atomics. */
AVL_API int avl_audio_segment(const float* d_audio, int64_t n, float threshold, int64_t gap, int64_t* d_segments, int64_t cap,
                              int64_t* d_count, void* d_ws, size_t ws_bytes, void* stream);
/* avlmaps/utils/audio_utils.py:569-583 get_five_second_contexts_audio(track, [2.5], sr) of audio_mapping_utils.py:85's scaled
 * tracks, for every segment at once: d_ranges (S, 2) int64 (start, stop) with 0 <= start <= stop <= n (the caller checks its host
 * copy; the kernel clamps, so a bad range reads nothing out of bounds), d_out (S, L) float32:
 * out[k, j] = audio[start_k + j] * scale for j < min(stop_k - start_k, L), +0 elsewhere.  1 <= L <= 2^31 - 1, S * L <= 2^40;
 * S = 0 does nothing. */
AVL_API int avl_audio_pack(const float* d_audio, int64_t n, const int64_t* d_ranges, int64_t S, int64_t L, float scale, float* d_out,
                           void* stream);
/* (csrc/avl_resample.hip)  avlmaps/utils/audio_mapping_utils.py:238, librosa.load(path, sr=sample_rate), in two steps: the PCM
 * widths avl_audio_decode_pcm16 does not read, and the change of rate.
 * d_pcm: n interleaved frames of `channels` samples (1 <= channels <= 8), width = 3: packed little-endian 24-bit, read byte by
 * byte (no alignment); width = 4: int32 (also a 24-bit sample left-justified in 32 bits).  d_out (n,):
 * float32((sum_c float64(s[i, c]) / 2^(8 width - 1)) / channels): an exact float64 sum, one float64 division, one rounding. */
AVL_API int avl_audio_decode_pcm(const void* d_pcm, int64_t n, int channels, int width, float* d_out, void* stream);
/* Rational resampling by up / down (reduced by the caller, 1 <= up, down <= 4096) with the FIR d_taps[0 .. n_taps), n_taps odd and
 * at most 81 921, half = (n_taps - 1) / 2; the taps are data (ops.resample_taps designs scipy.signal.resample_poly's default).
 * d_out (n_out,), n_out == ceil(n * up / down) <= 2^31 - 1:
 *     out[m] = float32(sum_k d_taps[m * down + half - k * up] * float64(d_audio[k]))
 * over every 0 <= k < n whose tap index lies in [0, n_taps), added in ascending k with separate float64 multiplies and adds:
 * scipy.signal.resample_poly(x, up, down) with a float64 accumulator.  One launch, no atomics. */
AVL_API int avl_audio_resample(const float* d_audio, int64_t n, int up, int down, const double* d_taps, int64_t n_taps, float* d_out,
                               int64_t n_out, void* stream);
/* outputs per tile of avl_audio_resample, and how many taps / input samples it stages in LDS before it reads them from global memory */
AVL_API int avl_audio_resample_limits(int* h_tile, int* h_lds_taps, int* h_lds_window);

/* ------------------------------------------------------------------------------------------------
 * (15) observed free space and the frontier of the 2-D map (csrc/avl_explore.hip)
 *     d_first_seen is a (gs, gs) int32 map in device memory: the smallest frame id whose sight rays crossed the cell inside the
 *     height band, -1 where no ray ever did (the device map has the host's encoding: the fold is a minimum of the bits as unsigned
 *     integers).  1 <= gs <= 16384.  Both calls are asynchronous; every result is unique (an integer minimum: the bytes do not
 *     depend on the order of rays, frames, launches or calls).
 * ------------------------------------------------------------------------------------------------ */
/* Takes the place of avlmaps/utils/mapping_utils.py:403-454 (get_frustum_4pts, generate_mask), in the base-frame conventions of
 * the builder instead of theirs.  d_depth: F frames of (H, W), float32 metres or uint16 (metres = value / depth_div), as
 * avl_points_bbox takes them; h_calib_inv: inv(K), 3 x 3 row-major; h_transforms: F camera -> map transforms, 4 x 4 row-major
 * (VLMapBuilder.frame_transforms); h_frame_ids: F ids >= 0.  One ray per pixel of the lattice stride / 2, stride / 2 + stride, ...
 * in both image directions, defined operation by operation at the top of csrc/avl_explore.hip: the point of avl_builder's K1
 * (skipped unless p_z > min_depth, pulled back to max_depth when p_z >= max_depth), the part of the segment from the camera to
 * it whose height lies in [h_min, h_max], and an all-octant integer Bresenham between the cells of its two ends (cells by
 * base_pos2grid_id_3d's rule) that marks every cell it visits inside the grid -- but not the end cell of a ray that ends on a
 * surface inside the band.  The camera's own cell is marked once per frame.  d_first_seen is updated in place: continuing a map in
 * a second call is part of the contract.  F = 0 does nothing.  h_min <= h_max, 0 <= min_depth < max_depth, stride >= 1. */
AVL_API int avl_carve_free_space(const void* d_depth, int depth_is_u16, double depth_div, int F, int H, int W, const double* h_calib_inv,
                                 const double* h_transforms, const int32_t* h_frame_ids, int gs, double cs, int stride, double h_min,
                                 double h_max, double min_depth, double max_depth, int32_t* d_first_seen, void* stream);
/* d_out_u8 (H, W): 1 where a cell is explored and free (both non-zero) and at least one of its 4 neighbours inside the image is
 * unknown, i.e. not explored and free; else 0.  A cell that holds an obstacle (free == 0) is known whether or not a ray crossed
 * it.  1 <= H, W <= 16384. */
AVL_API int avl_frontier_mask(const uint8_t* d_free_u8, const uint8_t* d_explored_u8, int H, int W, uint8_t* d_out_u8, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (16) the ground-truth label map and the scores of a map against it (csrc/avl_gtmap.hip)
 *     Every result is an integer with one value: no output depends on the order of pixels, frames, launches or calls.  All calls
 *     are asynchronous on `stream`, check their arguments before any device work and allocate nothing.  d_err_flag (nullable) is
 *     a device int32 the caller zeroes: bit 0 is set when data on the device is out of range (each call says which).
 *     Upstream has NO vote pass to mirror (dataset/README.md:78 says the semantic frames "can be used for creating a GT semantic
 *     map" and stops; gtmap.py loads a grid_gt_1.npy no program writes): the definitions below are this project's own, written
 *     out operation by operation at the top of csrc/avl_gtmap.hip and in DESIGN.md 4.16.
 * ------------------------------------------------------------------------------------------------ */
/* Produces what avlmaps/map/gtmap.py:18-30 loads and avlmaps/dataloader/habitat_dataloader.py:85-107 reads (gt_cropped), from the
 * semantic frames.  d_depth: F frames of (H, W), float32 metres or uint16 (metres = value / depth_div), and d_semantic: F frames
 * of (H, W) int32 object ids, as avl_carve_free_space takes its depth; h_calib_inv: inv(K) 3 x 3 row-major; h_transforms: F
 * camera -> map transforms, 4 x 4 row-major (VLMapBuilder.frame_transforms).  Per pixel of the lattice stride / 2,
 * stride / 2 + stride, ... in both directions: (1) the point of avl_builder's K1, dropped unless min_depth < p_z < max_depth; (2)
 * its cell (row, col, h) by base_pos2grid_id_3d's rule, dropped outside (gs, gs, vh) -- (1) and (2) count in d_stats[0]; (3) its
 * class c = d_obj2cls[o] for the object id o (dropped when o is outside [0, n_obj)), or c = o when d_obj2cls is NULL (n_obj = 0);
 * dropped when c is outside [0, n_classes) -- counts in d_stats[1]; (4) its voxel r = d_occupied_ids[row, col, h] ((gs, gs, vh)
 * int32), dropped when r < 0 -- counts in d_stats[2]; r >= n_voxels sets bit 0 of *d_err_flag and the pixel is dropped; (5)
 * d_votes[r * n_classes + c] += 1 (uint32, (n_voxels, n_classes) row-major, updated in place; a counter wraps after 2^32 hits)
 * -- counts in d_stats[3].  d_stats: uint64[4], updated in place.  Continuing d_votes and d_stats in a second call is part of
 * the contract.  1 <= n_classes <= 4096, gs <= 16384, n_voxels * n_classes < 2^40, stride >= 1, 0 <= min_depth < max_depth. */
AVL_API int avl_gt_vote(const void* d_depth, int depth_is_u16, double depth_div, const int32_t* d_semantic, int F, int H, int W,
                        const double* h_calib_inv, const double* h_transforms, int gs, double cs, int vh, int stride, double min_depth,
                        double max_depth, const int32_t* d_obj2cls, int n_obj, int n_classes, const int32_t* d_occupied_ids,
                        int64_t n_voxels, uint32_t* d_votes, uint64_t* d_stats, int32_t* d_err_flag, void* stream);
/* The majority label of every voxel (the per-voxel form of the grid gtmap.py:18-30 loads).  d_label (n_voxels,) int32: the lowest
 * class whose count is the maximum of the voxel's row of d_votes, -1 when the row is all zero; d_support (n_voxels,) uint32: the
 * row's sum, wrapping like the counters.  d_votes is read once. */
AVL_API int avl_gt_labels(const uint32_t* d_votes, int64_t n_voxels, int n_classes, int32_t* d_label, uint32_t* d_support, void* stream);
/* avlmaps/utils/visualize_utils.py:77-83 pool_3d_label_to_2d for labels instead of one mask: d_out (r1 - r0 + 1, c1 - c0 + 1) int32
 * over the window of rows r0 .. r1 and columns c0 .. c1 (inclusive) of the (gs, gs, vh) voxel index; out[r, c] is the label of
 * the highest h whose voxel exists (id >= 0) and has d_label[id] >= 0, -1 when the column has none.  An id >= n_voxels sets bit 0
 * of *d_err_flag and counts as no voxel. */
AVL_API int avl_pool_labels_2d(const int32_t* d_label, int64_t n_voxels, const int32_t* d_occupied_ids, int gs, int vh, int r0, int r1,
                               int c0, int c1, int32_t* d_out, int32_t* d_err_flag, void* stream);
/* The confusion matrix of two label arrays of n entries (voxels, or the cells of two avl_pool_labels_2d maps; gtmap.py:41-71 and
 * habitat_dataloader.py:85-107 only ever look at the ground truth, nothing upstream compares it with a map).  d_conf
 * (n_gt_classes, n_pred_classes) uint64 row-major and d_skipped uint64[2], both updated in place: gt[i] < 0 counts in
 * d_skipped[0]; otherwise pred[i] < 0 counts in d_skipped[1]; otherwise gt[i] >= n_gt_classes or pred[i] >= n_pred_classes sets
 * bit 0 of *d_err_flag; otherwise d_conf[gt[i], pred[i]] += 1.  Sides 1 .. 65536, at most 2^28 counters, n < 2^40. */
AVL_API int avl_label_confusion(const int32_t* d_gt, const int32_t* d_pred, int64_t n, int n_gt_classes, int n_pred_classes,
                                uint64_t* d_conf, uint64_t* d_skipped, int32_t* d_err_flag, void* stream);
/* the largest n_gt_classes * n_pred_classes avl_label_confusion counts in block-private LDS counters; above it: global atomics */
AVL_API int avl_label_confusion_limits(int* h_lds_counters);

/* ------------------------------------------------------------------------------------------------
 * (17) Pillow's 8-bit image resize and CLIP's preprocess (csrc/avl_resize.hip)
 *     d_in is a batch of B equally sized images, (B, H, W, C) uint8 in device memory, 1 <= B <= 65535, 1 <= H, W <= 16384,
 *     1 <= C <= 4.  A pass along an axis is given by two tables in device memory (ops.resize_coeffs builds them; they are
 *     Pillow's precompute_coeffs and normalize_coeffs_8bpc): d_k (out_size, ksize) int32 coefficients scaled by 2^22 and d_b
 *     (out_size, 2) int32 (first input index, number of taps <= ksize); per channel
 *         out = clamp((2^21 + sum over i of in[first + i] * k[i]) >> 22, 0, 255)      int32, arithmetic shift
 *     which needs 255 * sum|k| + 2^21 < 2^31 of every row (the caller's to check: the tables are not read on the host).  The
 *     horizontal pass (d_kh, d_bh: W -> ow) runs first and is rounded to uint8, the vertical one (d_kv, d_bv: H -> oh) reads its
 *     bytes: PIL.Image.resize((ow, oh)) for the box, bilinear and bicubic filters, bit for bit.  Both tables of a pass NULL: the
 *     axis keeps its size (ow == W, oh == H).  Only the window of out_h x out_w pixels at (top, left) of the resized image is
 *     computed, and only the input rows and columns that reach it are read.  An index of a table that leaves the image is
 *     clamped.  Arguments are checked before any device work; both calls are asynchronous on `stream` and allocate nothing.
 * ------------------------------------------------------------------------------------------------ */
/* the workspace of the two calls below: the horizontal pass's bytes, needed (and read) only when there is a vertical pass */
AVL_API int avl_resize_work_bytes(int B, int H, int C, int out_w, int vertical, size_t* h_bytes);
/* Stands in for PIL.Image.resize (the resize inside avlmaps/utils/clip_utils.py:96-130's preprocess, and any other use of it).
 * d_out (B, out_h, out_w, C) uint8. */
AVL_API int avl_resize_u8(const uint8_t* d_in, int B, int H, int W, int C, const int32_t* d_kh, const int32_t* d_bh, int ksize_h, int ow,
                          const int32_t* d_kv, const int32_t* d_bv, int ksize_v, int oh, int top, int left, int out_h, int out_w,
                          uint8_t* d_out, void* d_ws, size_t ws_bytes, void* stream);
/* Replaces avlmaps/utils/clip_utils.py:96-130's preprocess(Image.fromarray(img)) per image on the host (OpenAI CLIP's
 * _transform: Resize, CenterCrop, ToTensor, Normalize) for a batch: the resize and window of avl_resize_u8 with C = 3, then
 * d_out[b, c, y, x] = d_table[v * 3 + c] for the byte v, channel-planar (B, 3, out_h, out_w).  d_table (256, 3) holds float32
 * (out_f16 = 0) or float16 (out_f16 = 1) values, which are moved as bit patterns: the caller's table is ToTensor and Normalize. */
AVL_API int avl_clip_preprocess(const uint8_t* d_in, int B, int H, int W, const int32_t* d_kh, const int32_t* d_bh, int ksize_h, int ow,
                                const int32_t* d_kv, const int32_t* d_bv, int ksize_v, int oh, int top, int left, int out_h, int out_w,
                                const void* d_table, int out_f16, void* d_out, void* d_ws, size_t ws_bytes, void* stream);
/* output columns per workgroup of the horizontal pass, and how many coefficients of such a tile / bytes of an input row it stages in
 * LDS before it reads them from global memory */
AVL_API int avl_resize_limits(int* h_tile_w, int* h_lds_coefs, int* h_lds_span);

/* ------------------------------------------------------------------------------------------------
 * (18) object instances in 3-D: connected components of the masked voxels of a voxel list (csrc/avl_instances.hip)
 *     Upstream has no counterpart: avlmaps/map/map.py:146-151 and avlmaps/map/vlmap_3d.py:75-100, the nearest lines, stop at a
 *     category's voxel mask.  d_grid_pos is the map's (N, 3) int32 cell list (row, col, height) in any order, 0 <= N < 2^31.  Two
 *     masked voxels are adjacent when their cells differ by at most 1 on every axis and on at most 1 / 2 / 3 axes (connectivity
 *     6 / 18 / 26); voxels of one cell belong together; unmasked voxels take part in nothing.  Every result is unique: a minimum,
 *     a maximum or an integer sum, whose bytes do not depend on scheduling.  Arguments are checked before any device work.
 * ------------------------------------------------------------------------------------------------ */
/* The workspace of avl_label_voxels, a function of N alone: 28 bytes per voxel, whatever the bounding box.  Upstream has no
 * counterpart. */
AVL_API int avl_label_voxels_work_bytes(int64_t N, size_t* bytes);
/* d_labels (N,) int32: 0 where d_mask (N,) uint8 is 0, else the voxel's instance, 1 .. n in lexicographic (row, col, height) order of
 * the instances' first cells = scipy.ndimage.label(dense, generate_binary_structure(3, 1 | 2 | 3)) of dense[row, col, height] read
 * back at the voxels; *d_n (1 int32, device) = n.  Coordinates are any int32 for which every side of the MASKED voxels' bounding box
 * is at most 2^20 cells: the box is read back after its pass (the call synchronises `stream` once) and a larger one returns
 * AVL_ERR_INVALID.  N = 0 and a mask without a voxel give n = 0.  Upstream has no counterpart (a host user would scatter into a
 * dense array and label that). */
AVL_API int avl_label_voxels(const int32_t* d_grid_pos, const uint8_t* d_mask, int64_t N, int connectivity, int32_t* d_labels, int32_t* d_n,
                             void* ws, size_t ws_bytes, void* stream);
/* d_table (n, 12) int64, row k - 1 for label k: count, rmin, rmax, cmin, cmax, hmin, hmax, sum_row, sum_col, sum_height, first, best.
 * first = the smallest voxel index at the instance's first cell; best = the voxel index of its largest d_scores (N,) float32, the
 * smallest index among equals (+0 and -0 are equal; a NaN score leaves best undefined), -1 when d_scores is NULL.
 * d_best_score (n,) float32 = d_scores[best], 0 without scores.  The centre of an instance is sum / count.  n is avl_label_voxels'
 * count; n = 0 does nothing.  Asynchronous.  Upstream has no counterpart. */
AVL_API int avl_voxel_instance_table(const int32_t* d_grid_pos, const int32_t* d_labels, const float* d_scores, int64_t N, int32_t n,
                                     int64_t* d_table, float* d_best_score, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (19) open-set queries: exact column order statistics of the score matrix and "above the column's own threshold"
 *     (csrc/avl_colselect.hip).  d_scores is a row-major float32 matrix (N, Q) with row stride ld >= Q elements, 1 <= N < 2^31.
 *     The order is np.sort's: -inf < ... < -0 = +0 < ... < +inf < NaN, every NaN counts as one largest value, a selected zero
 *     comes back as +0.  Every result is a count, a minimum or an element of the matrix: the bytes do not depend on scheduling.
 *     Arguments are checked before any device work.
 * ------------------------------------------------------------------------------------------------ */
/* The workspace of avl_colselect_f32: one size for any number of slots (their groups of 64 use it one after the other).
 * Replaces map/clip_map.py:62-75, which partitions a host copy of every column (np.percentile). */
AVL_API int avl_colselect_workspace_bytes(int n_slots, size_t* bytes);
/* Slot s = (h_columns[s], h_ks[s]), host tables of n_slots entries with 0 <= column < Q and 0 <= k < N; a column may appear in
 * several slots.  Per slot, to device arrays of n_slots entries: d_v_k = the k-th smallest value of the column (k = 0: the minimum),
 * d_v_next = the (k+1)-th smallest (= d_v_k when k = N - 1), d_count_lt / d_count_le = the number of elements before / up to the
 * run of values equal to v_k in the sorted column (NaN = NaN there), d_nan_count = the column's NaNs.  A most-significant-digit
 * radix select: five streaming passes over the matrix per 64 slots, a fixed number of launches.  Asynchronous; the host tables
 * are read before the call returns.  Replaces map/clip_map.py:62-75 (np.percentile of every column on the host): the quantile is
 * v_k + (v_next - v_k) * t in float64, computed by the caller. */
AVL_API int avl_colselect_f32(const float* d_scores, int64_t N, int Q, int64_t ld, const int32_t* h_columns, const int64_t* h_ks,
                              int n_slots, float* d_v_k, float* d_v_next, int64_t* d_count_lt, int64_t* d_count_le, int64_t* d_nan_count,
                              void* ws, size_t ws_bytes, void* stream);
/* One pass over the same matrix (N >= 0) against d_thresholds (Q,) float64: d_bits (N, ceil(Q / 64)) uint64, bit c % 64 of word
 * c / 64 of row r set iff (double)d_scores[r * ld + c] > d_thresholds[c] (NaN on either side: not set; bits past column Q - 1 are 0);
 * d_counts (Q,) int64 = the set bits of every column; d_mask (N,) uint8 = column mask_column's bits as the
 * 0 / 1 voxel mask the other entry points take, or NULL with mask_column = -1.  Asynchronous.  Replaces map/clip_map.py:62-75
 * (mask = column > threshold, per category, on the host). */
AVL_API int avl_cols_above_f32(const float* d_scores, int64_t N, int Q, int64_t ld, const double* d_thresholds, int mask_column,
                               uint64_t* d_bits, int64_t* d_counts, uint8_t* d_mask, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (20) the visibility audit of a voxel map: a device cell index of the voxel list, and the 3-D sight-ray pass that records for
 *     every voxel the last frame that hit it and the rays that passed through it (csrc/avl_audit.hip).
 *     Upstream has no counterpart: its maps are static (avlmaps/map/vlmap.py loads what the builder wrote and never revises it).
 *     The grid is gs x gs x vh cells with 1 <= gs <= 16384, vh >= 1 and gs * gs * vh < 2^31; 0 <= N < 2^31 - 1 voxels.  Every
 *     result is an integer maximum or an integer sum: the bytes do not depend on the order of rays, frames, launches or calls.
 *     All calls are asynchronous on `stream`, check their arguments before any device work and allocate nothing.
 * ------------------------------------------------------------------------------------------------ */
/* The size of the index buffer of avl_cell_index_build: an occupancy bitmap (one bit per cell), the exclusive prefix of its words'
 * popcounts, a rank -> voxel permutation and the scan's block counts -- 8 bytes per 32 cells and 4 per voxel.  Upstream has no
 * counterpart. */
AVL_API int avl_cell_index_work_bytes(int64_t N, int gs, int vh, size_t* bytes);
/* Builds the lookup cell (row, col, h) -> voxel row of d_grid_pos (N, 3) int32 into d_index (index_bytes >= the size above).  Rows
 * outside the grid are ignored; of several rows in one cell the largest row index owns it.  N = 0 gives an empty index.  The
 * buffer is read by the two calls below with the same N, gs and vh.  Upstream has no counterpart. */
AVL_API int avl_cell_index_build(const int32_t* d_grid_pos, int64_t N, int gs, int vh, void* d_index, size_t index_bytes, void* stream);
/* d_out (M,) int32: the voxel row that owns each of the M cells of d_cells (M, 3) int32, -1 where the cell is empty or outside the
 * grid.  0 <= M < 2^31 - 1; M = 0 does nothing.  Upstream has no counterpart. */
AVL_API int avl_cell_index_lookup(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const int32_t* d_cells, int64_t M,
                                  int32_t* d_out, void* stream);
/* Folds the sight rays of F depth frames into d_last_hit (N,) int32 (-1 = never) and d_through (N,) uint32; each may be NULL.
 * Depth, calibration, transforms, frame ids, stride, height band and depth range are avl_carve_free_space's, and so is a ray up to
 * its segment inside the band; from there it is walked through (row, col, h) cells (h = int(z / cs) clamped to [0, vh)) by the
 * integer walk written out at the top of csrc/avl_audit.hip, from the cell of its start to the cell of its end, stopping at the
 * first cell outside [0, gs)^2.  With i the voxel that owns a visited cell: the END cell of a ray that ends on a surface which
 * the builder would fuse (not far, not cut by the band, 0 <= int(z / cs) < vh, inside the grid) does d_last_hit[i] =
 * max(d_last_hit[i], id); a cell more than end_margin steps before such an end, or any cell of a ray without a surface at its
 * end, does d_through[i] += 1 -- only where id > d_after[i] when d_after (N,) int32 is given.  d_through does not saturate (it
 * would take 2^32 rays through one voxel).  Both folds commute: calls continue each other in any order.  F = 0, or both outputs
 * NULL, does nothing.  end_margin >= 0.  Upstream has no counterpart. */
AVL_API int avl_audit_rays(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const void* d_depth, int depth_is_u16,
                           double depth_div, int F, int H, int W, const double* h_calib_inv, const double* h_transforms,
                           const int32_t* h_frame_ids, double cs, int stride, double h_min, double h_max, double min_depth, double max_depth,
                           int end_margin, int32_t* d_last_hit, uint32_t* d_through, const int32_t* d_after, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (21) cell-to-cell line of sight through a voxel map (csrc/avl_sight.hip), on the cell index of (20).  Cells are
 *     (row, col, h) int32.  The sight line from eye cell e to target cell t is the integer walk written out at the top of
 *     csrc/avl_audit.hip (step 12) from e to t, cells k = 0 .. n with n = max |t - e| over the axes.  It is NOT symmetric:
 *     (0,0,0) -> (2,1,0) passes (1,0,0), the reverse passes (1,1,0); the direction is always eye -> target.  Cell k is a blocker
 *     when 1 <= k < n - end_margin, the index has an owner row for it, and d_transparent (N,) uint8 is NULL or 0 at that row.  The
 *     eye's own cell never blocks and the target cell is never tested.  A pair is visible when it has no blocker and invalid when
 *     either end lies outside [0, gs)^2 x [0, vh).  Lines run between cell centres: there is no sub-cell geometry, and no field
 *     of view or heading of a camera.  Both calls are asynchronous on `stream`, check their arguments before any device work and
 *     allocate nothing; every result is an integer and does not depend on the launch geometry.  Upstream has no counterpart.
 * ------------------------------------------------------------------------------------------------ */
/* d_blocker (M,) int32 of the M pairs d_eyes[m] -> d_targets[m] (both (M, 3) int32): -1 visible, -2 invalid, else the voxel row of
 * the first blocker along the walk (the one with the smallest k).  0 <= M < 2^31 - 1; M = 0 does nothing.  end_margin >= 0. */
AVL_API int avl_los_pairs(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const int32_t* d_eyes, const int32_t* d_targets,
                          int64_t M, const uint8_t* d_transparent, int end_margin, int32_t* d_blocker, void* stream);
/* Every eye of d_eyes (E, 3) against every target of d_targets (T, 3): d_visible[e] (E,) uint32 = the number of targets that are
 * valid, in range -- dr^2 + dc^2 + dh^2 <= max_range2 in int64, equality included; max_range2 < 0: unlimited -- and visible from
 * eye e; d_first[e] (E,) int32, or NULL, = the smallest such target index, -1 when there is none.  An eye outside the grid gets 0
 * and -1.  0 <= E < 2^31, 0 <= T <= 65536; E = 0 does nothing, T = 0 writes zeros and -1s. */
AVL_API int avl_los_count(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const int32_t* d_eyes, int64_t E,
                          const int32_t* d_targets, int64_t T, const uint8_t* d_transparent, int end_margin, int64_t max_range2,
                          uint32_t* d_visible, int32_t* d_first, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (22) registration of depth frames to a voxel map: correlative scan matching on the cell index of (20) (csrc/avl_match.hip,
 *     DESIGN.md 4.23).  The hit points of F depth frames (min_depth < z < max_depth, the builder's rule) are turned into map cells
 *     (row, col, h) under their prior transforms, once per angle of a table of K planar rotations (cos, sin) about a pivot, and
 *     score[v, k, di + R, dj + R] counts the points of volume v whose cell shifted by (di, dj) is occupied, for every shift of the
 *     window [-R, R]^2.  joint != 0: one volume (V = 1) of all frames, rotated about (pivot_x, pivot_y); joint == 0: a volume per
 *     frame (V = F), each rotated about its own origin (T[0, 3], T[1, 3]).  Only points with h_lo <= h <= h_hi (cells) take part.
 *     The definition, operation by operation, is written out at the top of csrc/avl_match.hip.  Planar only: no pitch, roll or
 *     height is searched, and a shift is a whole number of cells.  1 <= K <= 1024, 0 <= R <= 64, V * K * (2R + 1)^2 < 2^31,
 *     fewer than 2^31 - 1 lattice pixels per volume, (gs + 2R)^2 * vh < 2^32.  Both calls check their arguments before any device
 *     work; avl_match_frames is asynchronous on `stream` and allocates nothing.  Upstream has no counterpart.
 * ------------------------------------------------------------------------------------------------ */
/* The size of the workspace of avl_match_frames for F frames of H x W pixels sampled every `stride`: the K point lists of every
 * volume, 4 bytes per lattice pixel, frame and angle.  Upstream has no counterpart. */
AVL_API int avl_match_ws_bytes(int F, int H, int W, int stride, int K, int R, int joint, size_t* bytes);
/* d_scores (V, K, 2R + 1, 2R + 1) uint32, d_valid (V,) uint32 = the points of a volume inside the depth range and the height band,
 * d_best (V, 4) int32 = (k, di, dj, score) of the winner: the largest score, then the smallest di^2 + dj^2, then the smallest
 * |k - k0|, then the smallest k, di, dj; (k0, 0, 0, 0) for a volume without a valid point.  Depth, calibration and transforms are
 * avl_audit_rays's; h_angles (K, 2) float64 on the host.  split: over how many blocks at most a volume's list of points is spread
 * in the scoring kernel, 1 .. 65536, or 0 to have it chosen (from the arguments alone, not from the device); it changes the
 * launch, never a byte of the results.  d_ws: ws_bytes >= the size above.  F = 0 does nothing and touches no pointer.  Upstream
 * has no counterpart. */
AVL_API int avl_match_frames(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const void* d_depth, int depth_is_u16,
                             double depth_div, int F, int H, int W, const double* h_calib_inv, const double* h_transforms, double cs,
                             int stride, double min_depth, double max_depth, const double* h_angles, int K, int R, int h_lo, int h_hi,
                             int joint, double pivot_x, double pivot_y, int k0, int split, uint32_t* d_scores, int32_t* d_best,
                             uint32_t* d_valid, void* d_ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (23) the scene inventory: the objects of ALL categories in one labelling, the score of every voxel's own class, and the score
 *     rows pooled per object (csrc/avl_objects.hip).  Upstream has no counterpart: avlmaps/map/map.py:146-151 and
 *     avlmaps/map/vlmap_3d.py:75-100, the nearest lines, stop at ONE category's voxel mask.  The table of the objects is (18)'s
 *     avl_voxel_instance_table, called with these labels.  Arguments are checked before any device work.
 * ------------------------------------------------------------------------------------------------ */
/* The workspace of avl_label_classes, a function of N alone:
 *     256 + 2 * align256(8 N) + 3 * align256(4 N) + align256(4 * ceil(N / 1024)) bytes, align256(b) = b rounded up to 256
 * (a header, the cell keys and their sorted copy, two index arrays, the parents, the scan's block counts): 28 bytes per voxel,
 * whatever the bounding box and the class ids.  Upstream has no counterpart (nearest: map/map.py:146-151). */
AVL_API int avl_label_classes_work_bytes(int64_t N, size_t* bytes);
/* avl_label_voxels for all classes at once.  d_classes (N,) int32: a voxel with a negative class takes part in nothing; two others
 * are adjacent when their cells are (as in avl_label_voxels, connectivity 6 / 18 / 26) AND their classes are equal; voxels of one
 * cell with the same class belong together, with different classes they do not.  d_labels (N,) int32: 0 or the voxel's object,
 * 1 .. n in lexicographic order of (first cell (row, col, height), class); *d_n (1 int32, device) = n.  That is
 * scipy.ndimage.label run once per class on the class's dense array, all components then sorted by (first cell, class); with one
 * class it is avl_label_voxels on the mask d_classes >= 0, byte for byte.  Class ids are any int32 >= 0.  Every side of the
 * participating voxels' bounding box is at most 2^20 cells: the box is read back after its pass (the call synchronises `stream`
 * once) and a larger one returns AVL_ERR_INVALID.  Every output is an integer that does not depend on the order in which atomics
 * land.  Upstream has no counterpart (nearest: map/vlmap_3d.py:75-100, one category's 3-D index). */
AVL_API int avl_label_classes(const int32_t* d_grid_pos, const int32_t* d_classes, int64_t N, int connectivity, int32_t* d_labels,
                              int32_t* d_n, void* ws, size_t ws_bytes, void* stream);
/* d_out[i] = (float)d_rows[i * ld + d_cols[i]] for the row-major float32 matrix d_rows (N, C) with row stride ld >= C elements, and
 * 0.0f where d_cols[i] lies outside 0 .. C - 1: with d_cols the row argmax, every voxel's score of its own class.  0 <= N < 2^31,
 * C >= 1; N = 0 does nothing.  Asynchronous.  Upstream has no counterpart (nearest: map/vlmap.py:123, np.argmax of the rows). */
AVL_API int avl_pick_columns(const float* d_rows, int64_t N, int C, int64_t ld, const int32_t* d_cols, float* d_out, void* stream);
/* The workspace of avl_pool_rows for N rows of C columns and n objects:
 *     4 * align256(4 N) + 2 * align256(4 (n + 1)) + align256(8 C * (floor(N / 256) + n)) bytes
 * (labels as sort keys and their sorted copy, the row indices and their sorted copy, the objects' first members and first chunks,
 * one float64 row per chunk).  Upstream has no counterpart (nearest: map/map.py:146-151). */
AVL_API int avl_pool_rows_work_bytes(int64_t N, int C, int32_t n, size_t* bytes);
/* d_sums (n, C) float64, row k - 1 = the sum of the rows of d_rows (N, C) float32 (row stride ld >= C) whose d_labels (N,) int32 is
 * k; labels outside 1 .. n take part in nothing, an object without a member gets zeros.  The order of the additions is pinned, so
 * the bytes are the same on every run: the members of an object in ascending row index, cut into chunks of 256 consecutive
 * members; a chunk's partial is the sequential float64 sum of its rows in that order, starting from 0.0; the object's sum is the
 * sequential float64 sum of its partials in chunk order, starting from 0.0.  No floating-point atomics.  0 <= N < 2^31,
 * 0 <= n < 2^31 - 1, C >= 1; n = 0 does nothing.  Asynchronous.  Upstream has no counterpart (nearest: map/vlmap.py:92-102, the
 * score matrix itself). */
AVL_API int avl_pool_rows(const float* d_rows, int64_t N, int C, int64_t ld, const int32_t* d_labels, int32_t n, double* d_sums,
                          void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (24) object relations: for every pair of objects of a labelled voxel list that come within `radius` cells of each other, their
 *     nearest gap, where it is, who rests on whom and how much they touch (csrc/avl_relations.hip), on the cell
 *     index of (20) and the labels of (23) or (18).  Upstream has no counterpart: avlmaps/map/map.py:183-240, the nearest lines,
 *     relate the 2-D islands of ONE category's top-down mask.  Arguments are checked before any device work.  Every result is an
 *     integer minimum or an integer sum: nothing depends on the order in which atomics land, and the bytes are the same on
 *     every run.
 * ------------------------------------------------------------------------------------------------ */
/* The workspace of avl_object_relations, a function of max_pairs alone (1 <= max_pairs <= 2^28).  With H the smallest power of two
 * >= 2 * max_pairs (at least 2) and align256(b) = b rounded up to 256:
 *     256 + 2 * align256(8 H) + align256(24 H) + align256(4 * ceil(H / 1024)) + 2 * align256(8 max_pairs) + 2 * align256(4 max_pairs)
 * bytes (a header, the keys and the packed minima of the pair table's H slots, their three counters, the scan's block counts, the
 * claimed keys and their sorted copy, their slots and their sorted copy).  Upstream has no counterpart (nearest: map/map.py:183). */
AVL_API int avl_object_relations_work_bytes(int64_t max_pairs, size_t* bytes);
/* d_index: the avl_cell_index_build index of the same d_grid_pos (N, 3) int32 on the gs x gs x vh grid; d_labels (N,) int32, a value
 * outside 1 .. n takes part in nothing; R = radius, 1 <= R <= 15.  Every voxel row i with label a in 1 .. n and its cell inside
 * the grid scans every offset d = (dr, dc, dh) with dr^2 + dc^2 + dh^2 <= R^2, d = 0 included; an offset whose cell
 * cell(i) + d lies outside the grid is skipped (each of row, col and height is checked, not the linear cell).  With j the owner of
 * that cell in the index (the largest row of the cell; an empty cell gives no event) and b = d_labels[j]: when b lies in 1 .. n and
 * b != a, the unordered pair (min(a, b), max(a, b)) exists and the event (i, d, j) belongs to it.  A pair collects
 *     d2        the minimum of |d|^2 over its events;
 *     i, j      the witness: among the events with |d|^2 = d2 the one with the smallest scanning row i, then the smallest offset
 *               code ((dr + R)(2R + 1) + (dc + R))(2R + 1) + (dh + R); i scans, j is seen;
 *     lo_on_hi  the events with d = (0, 0, -1) whose scanning voxel has the lower label: a voxel of the lower-numbered object with
 *               a cell of the higher-numbered one directly beneath it (larger height is up);
 *     hi_on_lo  the same with the roles exchanged;
 *     contacts  the events with 0 < |d|^2 <= 3 (the 26-neighbourhood), from either side.
 * Several rows in one cell make the scan ASYMMETRIC: a row that does not own its cell scans but is never seen; two rows of
 * different objects in one cell give d2 = 0.  d_table (max_pairs, 8) int64: its first P rows are
 * [lo, hi, d2, i, j, lo_on_hi, hi_on_lo, contacts], sorted by (lo, hi); d_count[0] (1 int64, device) = P, exact when
 * P <= max_pairs.  With more pairs d_count[0] is some value above max_pairs and the table's content is unspecified: that is not
 * an error code, the caller looks at the count.  Rows P .. max_pairs - 1 are not written.  Pairs live in a hash table of the
 * workspace (64-bit keys lo * (n + 1) + hi claimed by compare-and-swap; d2, i and the code packed as d2 << 46 | i << 15 | code
 * under one 64-bit atomic minimum, which is why R stops at 15 and N at 2^31 - 2); integer minima and sums only, so nothing depends
 * on the order in which atomics land.  0 <= N <= 2^31 - 2, the grid as in (20), index_bytes >= avl_cell_index_work_bytes(N, gs, vh),
 * n >= 0, ws_bytes >= the size above; N = 0 or n = 0 writes P = 0.  Asynchronous on `stream`; the sort's temporary storage comes
 * from the stream's memory pool.  Upstream has no counterpart (nearest: map/map.py:183-240, get_nearest_pos and the left / right /
 * between helpers on one category's 2-D islands). */
AVL_API int avl_object_relations(const void* d_index, size_t index_bytes, int64_t N, int gs, int vh, const int32_t* d_grid_pos,
                                 const int32_t* d_labels, int32_t n, int radius, int64_t max_pairs, int64_t* d_table, int64_t* d_count,
                                 void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (25) travel-distance fields on the free space of a 2-D obstacle map and their decay maps (csrc/avl_travel.hip).
 *     Upstream has no counterpart: avlmaps/robot/habitat_lang_robot.py:229-240 decays with the Euclidean distance of (10).
 *     d_free (H, W) uint8, nonzero = free; d_sources (H, W) uint8, nonzero = source (a source may lie on an obstacle cell); rows of
 *     ld_free / ld_src cells (a window of a larger image: ld > W).  A step u -> v between 8-neighbours is legal when v is free, u is
 *     free or a source and, for a diagonal step, both cells that share an edge with u and with v are free.  The field of a cell is
 *     the pair (a, b) of straight and diagonal steps of the shortest legal walk (length a + b sqrt(2)) from any source: (0, 0) on a
 *     source, (-1, -1) where no walk ends.  Pairs are compared exactly in integers, so the planes are the same on every run.
 *     1 <= H, W <= 16384, the sides of (10); every argument is checked before any device work.
 * ------------------------------------------------------------------------------------------------ */
/* 256 + align256(256) + align256(8 T) + align256(H W) + align256(8 H W) bytes with T = ceil(H / 32) * ceil(W / 32) tiles (a header,
 * two mark words per tile, a passability byte and a 64-bit state word per cell). */
AVL_API int avl_travel2d_workspace_bytes(int H, int W, size_t* bytes);
/* d_straight, d_diagonal: (H, W) int32, contiguous.  d_stats: 4 int64 on the device = [rounds that had an active tile, tile runs,
 * reached cells, 1 when a source exists else 0]; without a source both planes are -1 everywhere, which is not an error code.  The
 * call launches rounds in batches of 8 and SYNCHRONISES the stream after each batch to read how many tiles are still active; the
 * last launch (the planes and the stats) is asynchronous.  AVL_ERR_STATE ("did not converge") after H * W + 1 rounds. */
AVL_API int avl_travel2d(const uint8_t* d_free, int64_t ld_free, const uint8_t* d_sources, int64_t ld_src, int H, int W,
                         int32_t* d_straight, int32_t* d_diagonal, int64_t* d_stats, void* ws, size_t ws_bytes, void* stream);
/* The decay map of a travel field, NumPy's float64 operation order of avl_mask_decay_2d:
 *   d = double(a) + double(b) * 1.4142135623730951 (unfused);  t = 1 - (d / cell_size) * decay_rate;  t < 0 -> 0;  unreached -> 0;
 *   normalize != 0:  (t - min t) / (max t - min t) over the whole (H, W) window.
 * d_flags (1 int32, device): 1 when normalize was asked for and max t > min t does not hold (the output is then NaN or inf as in
 * NumPy, the caller reports it), else 0.  ws: at least 272 bytes of device memory (an avl_travel2d workspace serves).
 * decay_rate finite and >= 0, cell_size finite and > 0.  Asynchronous. */
AVL_API int avl_travel_decay_2d(const int32_t* d_straight, const int32_t* d_diagonal, int H, int W, double cell_size, double decay_rate,
                                int normalize, double* d_out_f64, int32_t* d_flags, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (26) rooms and doorways: label growth along the travel field, room seeds, the room and door tables and the lift of a label image
 *     onto voxels (csrc/avl_rooms.hip).  Upstream has no counterpart.  Images are row-major, 1 <= H, W <= 16384 as in
 *     (25); every argument is checked before any device work; every result is integers and the same bytes on every run.
 * ------------------------------------------------------------------------------------------------ */
AVL_API int avl_grow_labels_workspace_bytes(int H, int W, size_t* bytes);
/* d_free as in (25); d_seeds (H, W) int32 with rows of ld_seeds cells, a seed is > 0 and is a label, it may lie on an obstacle cell.
 * First the travel field of (25) from the sources seeds > 0 (avl_travel2d itself: d_straight, d_diagonal, d_stats[0 .. 3]), then the
 * label rounds on the fixed field: d_owner (H, W) int32 = the seed on a source, 0 where the field does not reach, else the smallest
 * label over the tight predecessors (the step u -> c is legal and field[u] + step == field[c]).  d_stats: 8 int64 on the device;
 * [4] label rounds that had an active tile, [5] label tile runs, [6] 1 when a negative seed was seen (it counts as no seed), [7] 0.
 * SYNCHRONISES the stream after each batch of 8 rounds of either phase; the last launch is asynchronous.  AVL_ERR_STATE after
 * H * W + 1 rounds of a phase. */
AVL_API int avl_grow_labels(const uint8_t* d_free, int64_t ld_free, const int32_t* d_seeds, int64_t ld_seeds, int H, int W, int32_t* d_straight,
                            int32_t* d_diagonal, int32_t* d_owner, int64_t* d_stats, void* ws, size_t ws_bytes, void* stream);
AVL_API int avl_room_seeds_workspace_bytes(int H, int W, size_t* bytes);
/* d_clearance (H, W) float64 (avl_edt2d of the free map).  core = clearance > radius; d_seeds (H, W) int32 = the 8-connected islands
 * of core in avl_label_islands' numbering, those with fewer than min_seed_cells cells dropped and the rest renumbered 1 .. K in their
 * old order; *d_k (1 int32, device) = K.  H * W <= 2^28 as in (11).  SYNCHRONISES the stream once (the island count). */
AVL_API int avl_room_seeds(const double* d_clearance, int H, int W, double radius, int64_t min_seed_cells, int32_t* d_seeds, int32_t* d_k,
                           void* ws, size_t ws_bytes, void* stream);
/* d_table (K, 10) int64, row k - 1 for label k of d_labels (H, W) int32: cells, rmin, rmax, cmin, cmax, sum of rows, sum of columns,
 * seed cells (d_seeds == k), centre row, centre col.  The centre is the room's cell with the largest clearance, the smallest raster
 * index among equals.  A label without a cell: 0 cells, -1 in the box and the centre.  K = 0 does nothing.  Asynchronous. */
AVL_API int avl_room_table(const int32_t* d_labels, const int32_t* d_seeds, const double* d_clearance, int H, int W, int32_t K,
                           int64_t* d_table, void* stream);
AVL_API int avl_room_doors_workspace_bytes(int32_t K, size_t* bytes);
/* Accumulates the contacts of d_labels per unordered pair of labels 1 .. K and sorts the pairs by (i, j) inside ws.  A contact is a
 * pair of 4-adjacent cells (u, v), v right of or below u, both labels nonzero and different.  d_count: 2 int64 on the device =
 * [pairs D, 1 when the pair table overflowed (the result is then incomplete and the caller reports it)].  Asynchronous. */
AVL_API int avl_room_doors(const int32_t* d_labels, const double* d_clearance, int H, int W, int32_t K, int64_t* d_count, void* ws,
                           size_t ws_bytes, void* stream);
/* d_table (D, 10) int64 from the workspace avl_room_doors filled, sorted by (i, j): i, j, contacts, rmin, rmax, cmin, cmax over all
 * cells of all contacts, door row, door col, 0.  The door cell has the largest clearance among the cells of the pair's contacts, the
 * smallest raster index among equals.  D = 0 does nothing.  Asynchronous. */
AVL_API int avl_room_door_table(const void* ws, size_t ws_bytes, int32_t K, int W, int64_t D, int64_t* d_table, void* stream);
/* d_out[n] = d_labels[row - rmin, col - cmin] for d_grid_pos (N, 3) int32 = (row, col, height), 0 outside the (H, W) crop. */
AVL_API int avl_lift_labels_2d(const int32_t* d_labels, int H, int W, const int32_t* d_grid_pos, int64_t N, int rmin, int cmin,
                               int32_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (27) 2-D viewsheds on the explored map: the unknown cells a candidate cell would see, per 45-degree sector, and the cells a set
 *     of eyes sees (csrc/avl_viewshed.hip).  d_free_u8, d_explored_u8: (H, W) uint8 masks as in avl_frontier_mask;
 *     a cell is opaque when free == 0 and unknown when free != 0 and explored == 0; opaque cells block, with opaque_unknown != 0
 *     unknown cells block as well.  d_eyes: (E, 2) int32 (row, col).  Target t is visible from eye e when both lie inside the
 *     image, t != e, dr^2 + dc^2 <= radius^2 (equality counts) and no cell strictly between them on the sight line e -> t -- the
 *     walk of (21) without the height axis, rows before columns, not symmetric -- is blocking.  The eye's own cell never blocks,
 *     the target cell is never tested, and an eye may stand on any cell.  Sides 1 .. 16384, 1 <= radius <= 127 cells,
 *     0 <= E < 2^31.  Both calls are asynchronous on `stream`, check their arguments before any device work and allocate nothing;
 *     every result is an integer and does not depend on the launch geometry.  Upstream has no counterpart.
 * ------------------------------------------------------------------------------------------------ */
/* d_gain (E, 8) int32: per eye and sector k = [k * 45, (k + 1) * 45) degrees of atan2(dr, dc) the number of visible targets that
 * are unknown; a row of -1 for an eye outside the image.  The sector in integers: if dc > 0 and dr >= 0 it is 0 when dr < dc, else
 * 1; otherwise replace (dr, dc) by (-dc, dr), add 2 and repeat.  E = 0 does nothing and touches no pointer. */
AVL_API int avl_viewshed_gain(const uint8_t* d_free_u8, const uint8_t* d_explored_u8, int H, int W, const int32_t* d_eyes, int64_t E,
                              int radius, int opaque_unknown, int32_t* d_gain, void* stream);
/* d_seen (H, W) uint8: 1 on every cell, of any class, that is visible from at least one of the M eyes and on the eyes' own cells;
 * eyes outside the image contribute nothing.  accumulate == 0: the mask is zeroed first (also with M = 0); accumulate != 0: the
 * ones are OR-ed into what d_seen holds. */
AVL_API int avl_viewshed_seen(const uint8_t* d_free_u8, const uint8_t* d_explored_u8, int H, int W, const int32_t* d_eyes, int64_t M,
                              int radius, int opaque_unknown, int accumulate, uint8_t* d_seen, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (28) cost-weighted travel fields and the layered costmap that prices their cells (csrc/avl_costfield.hip).
 *     Upstream has no counterpart: it dilates the obstacle map by a fixed number of cells (Map._dilate_map).
 *     d_free, d_sources as in (25); d_cost (H, W) uint8 with rows of ld_cost cells, the price of entering a cell.  A cell is passable
 *     when free != 0 and cost != 0 (price 0 on a free cell is lethal); the legal-step rule is that of (25) with "passable" in place
 *     of "free", and a source may lie on an impassable cell.  A step u -> v adds (cost[v], 0) when straight and (0, cost[v]) when
 *     diagonal; the field of a cell is the pair (A, B) of the cheapest legal walk (price A + B sqrt(2)) from any source: (0, 0) on a
 *     source, (-1, -1) where no walk ends.  Pairs are compared exactly in integers, so the planes are the same on every run; with
 *     cost == 1 everywhere they are avl_travel2d's.  1 <= H, W <= 16384 and H * W <= 2^22, which keeps A, B < 2^30; every argument
 *     is checked before any device work.
 * ------------------------------------------------------------------------------------------------ */
/* d_straight, d_diagonal, d_stats and the synchronisation are avl_travel2d's: rounds in batches of 8, the stream SYNCHRONISED after
 * each batch, the last launch asynchronous, AVL_ERR_STATE ("did not converge") after H * W + 1 rounds.  The workspace is
 * avl_travel2d's as well: ws_bytes >= avl_travel2d_workspace_bytes(H, W) serves (the same layout; the prices are read from d_cost). */
AVL_API int avl_costfield2d(const uint8_t* d_free, int64_t ld_free, const uint8_t* d_cost, int64_t ld_cost, const uint8_t* d_sources,
                            int64_t ld_src, int H, int W, int32_t* d_straight, int32_t* d_diagonal, int64_t* d_stats, void* ws,
                            size_t ws_bytes, void* stream);
/* One layer of avl_costmap2d: d_distance (H, W) float64, contiguous -- an avl_edt2d plane: the EDT of the free map (clearance) or
 * of an inverted mask (nearness to things to avoid); d_table: n_table >= 1 uint8 prices on the device, indexed by the SQUARED
 * distance in cells, the last entry serving every larger one. */
typedef struct avl_cost_layer {
    const double* d_distance;
    const uint8_t* d_table;
    int32_t n_table;
} avl_cost_layer;
/* d_cost_out (H, W) uint8, contiguous: 0 where d_free == 0; else with t_l = d_table_l[min(d2_l, n_table_l - 1)],
 * d2_l = (int64) rint(d_l * d_l) (exact for avl_edt2d planes): 0 when any t_l == 255 (lethal), else min(254, 1 + sum t_l).
 * h_layers: n_layers (0 .. 8) layers in HOST memory, read before the call returns.  No workspace.  Asynchronous. */
AVL_API int avl_costmap2d(const uint8_t* d_free, int64_t ld_free, int H, int W, const avl_cost_layer* h_layers, int n_layers,
                          uint8_t* d_cost_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (29) K travel-distance fields of (25) on one free map in one batch, the set-to-set arrivals read from their planes, and the sound
 *     field that decays around walls (csrc/avl_travel_many.hip).  Upstream has no counterpart.
 *     Sets are CSR: d_offsets (K + 1) int64 from 0 to L, d_cells (L, 2) int32 (row, col), both on the device; set k is
 *     cells[offsets[k] .. offsets[k + 1]).  A set may repeat a cell and its cells may lie on obstacles; a cell outside the map is
 *     passed over.  1 <= K <= 1024, sides as in (25), K * ceil(H / 32) * ceil(W / 32) <= 2^28; int64 indexing throughout; every
 *     argument is checked before any device work.
 * ------------------------------------------------------------------------------------------------ */
/* Field k is avl_travel2d's field whose sources are the cells of set k: the same step rule, pair order and planes, byte for byte.
 * d_straight, d_diagonal: (K, H, W) int32, contiguous.  d_stats: 2 + K int64 on the device = [rounds that had an active (field,
 * tile) pair, pair runs, reached cells of field 0 .. K - 1].  The batch runs as many rounds as its slowest field; rounds in batches
 * of 8, the stream SYNCHRONISED after each batch, the last launch asynchronous, AVL_ERR_STATE ("did not converge") after H * W + 1
 * rounds.  Workspace: ws_bytes >= K * avl_travel2d_workspace_bytes(H, W); there is no size query of its own.  The layout is
 *   256 + align256(256) + align256(8 K T) + align256(H W) + align256(8 K H W) bytes, T = ceil(H / 32) * ceil(W / 32)
 * (a header, two mark words per (field, tile) pair, ONE free plane for all fields, a 64-bit state word per field and cell), which
 * is at most K times the single field's figure because align256(K x) <= K align256(x). */
AVL_API int avl_travel2d_many(const uint8_t* d_free, int64_t ld_free, int H, int W, const int64_t* d_offsets, const int32_t* d_cells, int K,
                              int64_t L, int32_t* d_straight, int32_t* d_diagonal, int64_t* d_stats, void* ws, size_t ws_bytes, void* stream);
/* Arrivals of K fields (the planes of avl_travel2d_many on d_free) at M target sets (CSR as above, 1 <= M <= 1024, L < 2^31).  For a
 * target cell t, arrive_k(t) is (0, 0) when t's pair in field k is (0, 0); otherwise the exact minimum over the eight neighbours u
 * of t of pair_k(u) + step(u -> t), over the u whose pair is reached and, for a diagonal step, with both cells that share an edge
 * with u and t free; t itself need not be free (the mirror image of "a source may lie on an obstacle").  For a free t this is
 * pair_k(t).  Outputs (K, M) int32: d_a, d_b the minimum over the set's cells; d_cell the index into d_cells of the first cell in
 * CSR order that attains it; d_from the index of the winning neighbour in the order E, NE, N, NW, W, SW, S, SE, the first among
 * ties, -1 when the target is a source.  -1 in all four where no cell of the set is arrived at.  No workspace.  Asynchronous. */
AVL_API int avl_travel_arrive(const uint8_t* d_free, int64_t ld_free, int H, int W, const int32_t* d_straight, const int32_t* d_diagonal,
                              int K, const int64_t* d_offsets, const int32_t* d_cells, int M, int64_t L, int32_t* d_a, int32_t* d_b,
                              int32_t* d_cell, int32_t* d_from, void* stream);
/* avl_field_sound of (9) with the travel distance.  d_straight, d_diagonal (K, H, W): the field of segment s = 0 .. K - 1;
 * d_peaks (K) float32 >= 0.  For every cell, segments in order:  d = double(a) + double(b) * 1.4142135623730951 (unfused);
 * t = p - (p * d) * decay_rate in float64, < 0 -> 0, unreached -> 0;  acc = float(double(acc) + t).  first != 0: acc starts from 0;
 * first == 0: from what d_field (H, W) float32 holds, so that many segments go through in chunks.  A segment with p == 0 adds
 * exactly +0.  d_minmax (2) float32: [min, max] of the field after this call.  Asynchronous. */
AVL_API int avl_travel_sound2d(const int32_t* d_straight, const int32_t* d_diagonal, int K, int H, int W, const float* d_peaks,
                               double decay_rate, int first, float* d_field, float* d_minmax, void* stream);
/* d_out = (d_field - min) / (max - min) in float32, avl_field_normalize's expression on an (H, W) field.  Asynchronous. */
AVL_API int avl_travel_sound_normalize(const float* d_field, const float* d_minmax, int H, int W, float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (30) comparing two voxel maps of one place: the join of two voxel lists by cell, the dot products of every joined pair of feature
 *     rows and the status of every voxel (csrc/avl_mapdiff.hip), on the cell index of (20).  Upstream has no
 *     counterpart: its maps are static.  Every output is sized by the number of voxels and allocated by the caller; the only
 *     workspace is the index that avl_cell_index_build made, so there is no size query.  Every result has one value: the join is
 *     integer, the sums are added in a fixed order, the status is a float64 predicate in a fixed grouping.  All calls are asynchronous
 *     on `stream`, check their arguments before any device work and allocate nothing.
 * ------------------------------------------------------------------------------------------------ */
/* For each of the n_a cells (row, col, h) of d_cells (n_a, 3) int32, moved by h_shift (3 int32 in HOST memory, NULL = no shift): the
 * nearest occupied cell of the index of the OTHER map (d_index of N_b voxels on gs x gs x vh, as avl_cell_index_build made it)
 * within Chebyshev radius 0 <= radius <= 2.  The winner minimises the pair (squared cell distance, linear cell (row * gs + col) * vh
 * + h of the hit), compared in that order.  d_match (n_a) int32: the row of the other map that owns the winning cell (the largest
 * row of the cell, as everywhere on this index), -1 where no cell within the radius is occupied or the moved cell lies outside the
 * grid; d_d2 (n_a) int32: the squared cell distance 0 .. 12, -1 with it.  Cells outside the grid count as empty.  0 <= n_a <
 * 2^31 - 1; n_a = 0 does nothing, N_b = 0 gives -1 everywhere. */
AVL_API int avl_map_match_cells(const void* d_index, size_t index_bytes, int64_t N_b, int gs, int vh, const int32_t* d_cells, int64_t n_a,
                                const int32_t* h_shift, int radius, int32_t* d_match, int32_t* d_d2, void* stream);
/* d_sums (n_a, 3) float64: for every i with m = d_match[i] in 0 .. N_b - 1 the sums (a.b, a.a, b.b) of a = d_feat_a[i, :] and b =
 * d_feat_b[m, :], float32 rows of D contiguous elements, 1 <= D <= 8192; three zeros for every other i.  The order of the additions is
 * part of the contract: lane l = 0 .. 63 owns the elements d with (d / 4) % 64 == l and adds their products, each formed exactly in
 * float64, in ascending d into one float64 accumulator per sum that starts at +0.0, each addition rounded once and none fused with
 * its product; the 64 lane values are then combined by the xor butterfly with offsets 32, 16, 8, 4, 2, 1 (v = v + partner).  The
 * bytes do not depend on the run, on n_a, on the alignment of the matrices or on which load path served them. */
AVL_API int avl_row_dots_f32(const float* d_feat_a, int64_t n_a, const float* d_feat_b, int64_t N_b, int D, const int32_t* d_match,
                             double* d_sums, void* stream);
/* d_status (n) uint8 from d_match (n) and d_sums (n, 3) = (ab, aa, bb):  2 (no match) where d_match[i] < 0;  0 (same) where
 * aa > 0 && bb > 0 && ab > 0 && ab * ab >= t2 * (aa * bb) in float64 with the products in exactly that grouping;  1 (changed)
 * otherwise.  t2 is the square of the cosine threshold, 0 < t2 <= 1.  With d_through (n) int32 (may be NULL) a voxel without a match
 * whose d_through[i] < min_rays gets 3 (unseen) instead of 2.  d_counts (4) int32 receives the number of voxels of each status (it is
 * set, not added to).  n = 0 writes four zeros. */
AVL_API int avl_map_diff_status(const int32_t* d_match, const double* d_sums, int64_t n, double t2, const int32_t* d_through, int min_rays,
                                uint8_t* d_status, int32_t* d_counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (31) fusing a revisit into the map: the cells of map B moved into map A's grid under a 4 x 4 transform, the join of both voxel
 *     lists by cell, and the weighted mean of the joined rows (csrc/avl_mapfuse.hip).  The arithmetic is the
 *     builder's running mean in closed form (vlmap_builder.py:172-178: feat = (feat * w + new * a) / (w + a)) applied to finished
 *     maps: sum(w_i f_i) / sum(w_i).  Every output is allocated by the caller and sized by n_a, n_b and D as stated below; the
 *     scratch is the cell index of (20), the workspace of avl_argsort_bits and one int32 array, so there is no size query.  Every
 *     result has one value: the move is float64 with every product and sum rounded once, the plan is integer, a fused element is a
 *     float64 sum in member order.  All calls are asynchronous on `stream`, check their arguments before any device work and
 *     allocate nothing.
 * ------------------------------------------------------------------------------------------------ */
/* Moves the n cells (row, col, h) of d_cells (n, 3) int32 on the gs x gs x vh grid of cell size cs.  A cell stands for the centre of
 * the interval of base coordinates that base_pos2grid_id_3d (mapping_utils.py:345-349) maps to it: with k = gs / 2 - index (integer
 * division) for row and col, x = (k + 0.5 * sign(k)) * cs -- the cell k = 0 is two cells wide upstream (truncation toward zero) and
 * its centre is 0 --, and z = (h + 0.5) * cs.  h_T (16 float64 in HOST memory, row-major 4 x 4, finite, bottom row 0 0 0 1; NULL =
 * identity): x' = ((T00 * x + T01 * y) + T02 * z) + T03 and likewise y' and z', every product and sum rounded once in float64, none
 * fused.  The moved cell is upstream's (int)(gs / 2.0 - (int)(x' / cs)), (int)(gs / 2.0 - (int)(y' / cs)), (int)(z' / cs): float64
 * divides, truncation toward zero.  h_shift (3 int32 in HOST memory, NULL = none) is then added in index space.  d_inside (n) uint8:
 * 0 where a moved coordinate is not finite, a quotient is not below 2^31 in magnitude or a final index leaves the grid; d_out (n, 3)
 * int32 holds the final cell where d_inside is 1 and (-1, -1, -1) elsewhere.  With h_T = NULL the call is integer only: the cell
 * plus the shift.  1 <= gs <= 16384, vh >= 1, gs * gs * vh < 2^31, cs > 0 and finite, 0 <= n < 2^31 - 1; n = 0 does nothing. */
AVL_API int avl_map_move_cells(const int32_t* d_cells, int64_t n, const double* h_T, const int32_t* h_shift, int gs, double cs, int vh,
                               int32_t* d_out, uint8_t* d_inside, void* stream);
/* Joins map A's cells d_cells_a (n_a, 3) and map B's moved cells d_cells_b (n_b, 3) by cell.  A row of B is SELECTED when d_use_b
 * (n_b uint8, NULL = all ones) is non-zero, its weight d_w_b (float32) is finite and > 0, d_inside_b (n_b uint8, NULL = all ones) is
 * non-zero and its cell lies inside the grid.  A row of A is selected when d_use_a is non-zero and its weight is finite and > 0; a
 * selected row of A outside the grid sets bit 0 of the error word and is dropped, two selected rows of A in one cell set bit 1.
 * The output voxels: first every selected row of A in row order, then every cell that only selected rows of B reach, ordered by the
 * smallest such row.
 *   d_head (4) int32: n_out, the selected rows of A, the selected rows of B, the error word;
 *   d_a_row (n_a + n_b) int32: the first n_out hold the A row of an output voxel or -1;
 *   d_b_start (n_a + n_b + 1) int32 and d_b_rows (n_b) int32: the CSR of the selected rows of B of every output voxel, ascending
 *     (entries of d_b_start past n_out hold the number of selected rows, entries of d_b_rows past that number -1);
 *   d_out_of_a (n_a), d_out_of_b (n_b) int32: the output voxel of every input row, -1 for a row that is not selected;
 *   d_counts (6) int32: rows of A not selected; rows of B whose use or weight unselects them; further rows of B outside; rows of B
 *     in a cell of a selected row of A; new cells; rows of B in a new cell beyond its first.  [1] .. [5] add up to n_b.
 * Scratch: d_index, index_bytes >= avl_cell_index_work_bytes(max(n_a, n_b), gs, vh), built twice here; d_sort_work, sort_work_bytes
 * >= avl_argsort_bits_work_bytes(n_b, 4, bits) with bits = the bit length of n_a + n_b; d_scratch: 9 * max(n_a, n_b) + 1024 int32 at
 * an 8-byte aligned address (scratch_i32 = its length).  0 <= n_a, n_b and n_a + n_b < 2^31 - 1; the grid as in (20). */
AVL_API int avl_map_fuse_plan(const int32_t* d_cells_a, const uint8_t* d_use_a, const float* d_w_a, int64_t n_a, const int32_t* d_cells_b,
                              const uint8_t* d_inside_b, const uint8_t* d_use_b, const float* d_w_b, int64_t n_b, int gs, int vh, void* d_index,
                              size_t index_bytes, void* d_sort_work, size_t sort_work_bytes, int32_t* d_scratch, int64_t scratch_i32,
                              int32_t* d_head, int32_t* d_a_row, int32_t* d_b_start, int32_t* d_b_rows, int32_t* d_out_of_a,
                              int32_t* d_out_of_b, int32_t* d_counts, void* stream);
/* The n_out fused voxels of a plan.  The members of voxel v: row d_a_row[v] of A when >= 0, then the rows d_b_rows[d_b_start[v] ..
 * d_b_start[v + 1]) of B in that order; a member index outside its map is skipped.  In float64, with g = g_a or g_b (> 0, finite)
 * by side: w_i = (double)weight_i * g; W = w_0 + w_1 + .. in member order; per element d, acc = w_0 * (double)f_0[d] + w_1 *
 * (double)f_1[d] + .. in member order, every product and every addition rounded once, none fused, the first product taken as it
 * is (a sole -0.0 stays -0.0).  d_feat_out[v, d] = (float)(acc / W), d_weight_out[v] = (float)W, d_rgb_out[v, c] = (uint8)(int)(acc_c
 * / W) with acc_c the same sum over (double)rgb_i[c]: truncated, as upstream's uint8 store truncates.  A voxel with one member and
 * g = 1 comes back bit for bit.  The elements are independent: rows are read and written 16 bytes at a time where D % 4 == 0 and
 * the matrix is 16-byte aligned and by scalars otherwise, chosen per matrix, same bytes.  d_grid_pos_out (n_out, 3): the cell of
 * the first member (d_cells_b are the MOVED cells).  d_occupied (gs, gs, vh) int32, NULL = not wanted: set to -1 and then to v at
 * the cell of voxel v.  A voxel without a member gets zeros and no cell.  Matrices are (rows, D) float32 contiguous, 1 <= D <= 8192;
 * 0 <= n_out <= n_a + n_b < 2^31 - 1; n_out = 0 only clears d_occupied. */
AVL_API int avl_map_fuse_rows(int64_t n_out, const int32_t* d_a_row, const int32_t* d_b_start, const int32_t* d_b_rows, const float* d_feat_a,
                              const float* d_w_a, const uint8_t* d_rgb_a, const int32_t* d_cells_a, int64_t n_a, const float* d_feat_b,
                              const float* d_w_b, const uint8_t* d_rgb_b, const int32_t* d_cells_b, int64_t n_b, int D, double g_a, double g_b,
                              int gs, int vh, float* d_feat_out, float* d_weight_out, uint8_t* d_rgb_out, int32_t* d_grid_pos_out,
                              int32_t* d_occupied, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (32) resampling a finished voxel map backward: for every cell of the target grid the rows of map B that its centre came from,
 *     and the voxel gathered from them (csrc/avl_mappull.hip).  (31)'s move is a forward, nearest-cell scatter that
 *     leaves pinholes under a rotation; this is the inverse mapping.  Upstream has no counterpart: its maps are static and it never
 *     resamples one.  The plan is two calls around one read-back of n_out, which has no bound from n_b.  The scratch is the cell
 *     index of (20) and one int32 array whose length is stated below, so there is no size query.  Every result has one value: the
 *     pulled-back point is float64 with every product and sum rounded once, the members and their order are fixed, an element is a
 *     float64 sum in corner order.  All calls are asynchronous on `stream`, check their arguments before any device work and
 *     allocate nothing.
 * ------------------------------------------------------------------------------------------------ */
/* Passes 1 and 2 of the plan.  Map B has n_b cells d_cells_b (n_b, 3) int32 on the gs x gs x vh grid of cell size cs.  A row is
 * SELECTED when d_use_b (n_b uint8, NULL = all ones) is non-zero, its weight d_w_b (float32) is finite and > 0 and its cell lies
 * inside the grid; two selected rows in one cell set bit 1 of the error word.
 * THE MEMBERS of target cell c = (row, col, h):  c' = c - h_shift (3 int32 in HOST memory, NULL = none).  With h_P = NULL the sole
 * member is the selected row of B in cell c', lambda = 1: integers only, whatever the mode.  Otherwise p is the centre of c' by
 * avl_map_move_cells' rule (k = gs / 2 - index, x = (k + 0.5 * sign(k)) * cs, z = (h + 0.5) * cs) and q = P p with h_P (16 float64
 * in HOST memory, row-major 4 x 4, finite, bottom row 0 0 0 1) the INVERSE of the transform from B's base frame to the target's:
 * qx = ((P00 * x + P01 * y) + P02 * z) + P03 and likewise qy, qz, every product and sum rounded once in float64, none fused; then
 * sx = qx / cs, sy = qy / cs, sz = qz / cs, true float64 divides.  A cell whose quotients are not all below 2^31 in magnitude has
 * no member.
 *   mode 0 (nearest): the sole member is the selected row in cell ((int)(gs / 2.0 - (int)sx), (int)(gs / 2.0 - (int)sy), (int)sz),
 *     upstream's base_pos2grid_id_3d, lambda = 1.
 *   mode 1 (linear): each axis is bracketed by the centres of B's lattice.  Horizontally the centres are 0, +-1.5, +-2.5, .. (the
 *     cell k = 0 is two cells wide): with a = |s|, j0 = 0 and u = a / 1.5 where a < 1.5, else j0 = floor(a - 0.5) and u = (a - 0.5)
 *     - j0; for s >= 0 k0 = j0 and t = u; for s < 0 k0 = -j0 and t = 0 where u == 0, else k0 = -(j0 + 1) and t = 1 - u.  In
 *     height s = sz - 0.5, h0 = floor(s), t = s - h0.  Corner j = 0 .. 7 has dz = j & 1, dy = j >> 1 & 1, dx = j >> 2 & 1, the
 *     cell (gs / 2 - (k0x + dx), gs / 2 - (k0y + dy), h0 + dz) and lambda = (lx * ly) * lz with l = t for d = 1 and 1 - t for
 *     d = 0.  A corner is a member when lambda > 0 and a selected row owns its cell.
 * The support of c is the sum of its members' lambdas, added in corner order.  The target cell EXISTS when its support is > 0 and
 * >= min_support (0 < min_support <= 1, compared in float64).  The existing cells are numbered in ascending linear cell order
 * (row * gs + col) * vh + h, whatever the order of B's rows.
 *   d_head (8) int32: n_out; the selected rows of B; the error word; rows of B that use or weight unselects; further rows of B
 *     outside the grid; target cells with a member whose support is below min_support; two zeros.
 * Scratch: d_index, index_bytes >= avl_cell_index_work_bytes(n_b, gs, vh); d_scratch of scratch_i32 >= 4 * n_b + 2 * W + W / 1024 +
 * 512 int32 with W = ceil(gs * gs * vh / 32).  Both are read by avl_map_pull_fill and stay untouched until then.  The grid as in
 * (20), cs > 0 and finite, 0 <= n_b < 2^31 - 1; n_b = 0 gives n_out = 0. */
AVL_API int avl_map_pull_plan(const int32_t* d_cells_b, const uint8_t* d_use_b, const float* d_w_b, int64_t n_b, const double* h_P,
                              const int32_t* h_shift, int gs, double cs, int vh, int mode, double min_support, void* d_index,
                              size_t index_bytes, int32_t* d_scratch, int64_t scratch_i32, int32_t* d_head, void* stream);
/* Pass 3 of the plan, after the caller has read n_out = d_head[0] back: the same n_b, h_P, h_shift, grid, mode, min_support, d_index,
 * d_scratch and d_head as in avl_map_pull_plan.  For the v-th existing cell in linear order: d_cells_out (n_out, 3) int32 its cell;
 * d_members (n_out, 8) int32 the row of B of corner j, -1 where the corner is no member; d_lam (n_out, 8) float64 the member's
 * lambda, 0 where there is none (nearest mode and h_P = NULL: the sole member in column 0).  d_occupied (gs, gs, vh) int32, NULL =
 * not wanted: set to -1 and then to v at the cell of voxel v.  d_counts (4) int32: rows of B that use or weight unselects; further
 * rows outside the grid; target cells below the support; selected rows of B that are a member of no existing cell.  A cell whose
 * rank is not below n_out is skipped: nothing is written out of bounds.  0 <= n_out <= gs * gs * vh. */
AVL_API int avl_map_pull_fill(int64_t n_b, const double* h_P, const int32_t* h_shift, int gs, double cs, int vh, int mode, double min_support,
                              const void* d_index, size_t index_bytes, int32_t* d_scratch, int64_t scratch_i32, const int32_t* d_head,
                              int64_t n_out, int32_t* d_cells_out, int32_t* d_members, double* d_lam, int32_t* d_occupied,
                              int32_t* d_counts, void* stream);
/* The n_out voxels of a plan.  The members of voxel v are the rows m_j = d_members[v, j] in 0 .. n_b - 1, in the order j = 0 .. 7.
 * In float64: omega_j = d_lam[v, j] * (double)d_w_b[m_j]; Omega = the sum of omega_j and Lambda = the sum of d_lam[v, j] over the
 * members in that order; per element d, acc = omega_0 * (double)f_0[d] + omega_1 * (double)f_1[d] + .. in that order, every
 * product and every addition rounded once, none fused, the first product taken as it is (a sole -0.0 stays -0.0).
 * d_feat_out[v, d] = (float)(acc / Omega); d_weight_out[v] = (float)(Omega / Lambda), the lambda-weighted mean of the members'
 * weights; d_rgb_out[v, c] = (uint8)(int)(acc_c / Omega) with acc_c the same sum over (double)rgb_j[c], truncated.  A voxel with
 * one member of lambda 1 comes back bit for bit.  Rows are read and written 16 bytes at a time where D % 4 == 0 and the matrix is
 * 16-byte aligned and by scalars otherwise, chosen per matrix, same bytes.  A voxel without a member gets zeros.  d_feat_b (n_b, D)
 * and d_feat_out (n_out, D) float32 contiguous, 1 <= D <= 8192; 0 <= n_out, n_b < 2^31 - 1; n_out = 0 does nothing. */
AVL_API int avl_map_pull_rows(int64_t n_out, const int32_t* d_members, const double* d_lam, const float* d_feat_b, const float* d_w_b,
                              const uint8_t* d_rgb_b, int64_t n_b, int D, float* d_feat_out, float* d_weight_out, uint8_t* d_rgb_out,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AVLMAPS_HIP_H */
