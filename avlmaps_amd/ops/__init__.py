"""Python face of the hot-path kernels (thin: argument marshalling only, all compute in HIP), one module per kernel family.
This file only gathers their names: everything `avlmaps_amd.ops` offers is listed here, defined in the module it is imported from."""
from .. import _lib  # noqa: F401
from ..device import DeviceArray, DeviceView, as_device, _is_torch  # noqa: F401
from .sim import (  # noqa: F401
    argmax_f32, mask_bool_from_argmax, mask_from_argmax, PRECISION, prepare_map, PreparedMap, query_col_support, sim_scores,
    _sim_scores_compact, _sim_workspace, topk_f32, _WS_CACHE,
)
from .builder import (  # noqa: F401
    BatchPlan, export_raw_torch, finalize_merged, finalize_raw, _global_depth, points_bbox, VoxelAccumulator,
)
from .heat import (  # noqa: F401
    _fingerprint, heatmap_from_mask, HeatPlan, _host_heat_plan, _HOST_PLANS,
)
from .map2d import (  # noqa: F401
    obstacle_map, obstacle_scatter, pool_label_2d, rgb_topdown,
)
from .render import (  # noqa: F401
    _background3, colorize_heat, _heat_arg, jet_table, RENDER_MAX_SIDE, render_topdown, render_view, _rgb_arg, _table_arg,
)
from .image2d import (  # noqa: F401
    binary_morph, dilate_map, distance_transform_edt, EDT_MAX_SIDE, _edt_workspace, gaussian_filter2d,
    gaussian_filter2d_f32, gaussian_weights, mask_decay_2d, mask_foreground, mask_smooth_2d, _MORPH_OPS, _MORPH_STRUCTURES,
    product_argmax_2d, ProductResult, resize2x_down, resize2x_up, _smooth_mask_window, Window, _WindowTermC,
)
from .fields import (  # noqa: F401
    area_field, _check_decay, field_lift, field_normalize, GOAL_CONES, GOAL_DENSE_F32, GOAL_DENSE_F64, GOAL_FIELD_F32,
    GOAL_FIELD_F64, goal_fuse, GOAL_MAX_TERMS, goal_terms_array, GoalField, GoalResult, GoalTerm, _GoalTermC, planar_decay,
    sound_field,
)
from .nav import (  # noqa: F401
    nav_graph, NAV_MANY_MAX, NAV_MAX_SIDE, NAV_MAX_VERTICES, NavGraph, NavPlanMany, unpack_rows,
)
from .islands import (  # noqa: F401
    contour_nearest_pair, ISLAND_TABLE_COLS, Islands, ISLANDS_MAX_SIDE, label_islands, NEAREST_PAIR_MAX_COORD, _points_i32,
    trace_islands,
)
from .localize import (  # noqa: F401
    _camera3, _corr_args, Correspondences, _f64_2d, loc_lift, _mix32, PNP_DEFAULT_HYPOTHESES, pnp_lds_stage, PNP_MAX_ERROR,
    PNP_MAX_ITERATIONS, pnp_ransac, pnp_refine, pnp_sample_indices, pnp_score, PNP_STEP_TOLERANCE, PnpRansacResult,
    PnpRefineResult, retrieve_frame,
)
from .audio import (  # noqa: F401
    _audio_f32, _audio_len, AUDIO_MAX_CHANNELS, AUDIO_MAX_SAMPLES, AudioSegments, _check_ranges, context_ranges, decode_pcm,
    decode_pcm16, _device_taps, pack_tracks, resample_audio, RESAMPLE_LDS_TAPS, RESAMPLE_LDS_WINDOW, resample_limits,
    RESAMPLE_MAX_RATIO, resample_ratio, _RESAMPLE_TAPS, resample_taps, _RESAMPLE_TAPS_KEPT, RESAMPLE_TILE, segment_audio,
)
from .explore import (  # noqa: F401
    carve_free_space, EXPLORE_MAX_SIDE, frontier_mask, _mask_dtype_check, NEVER_SEEN,
)
from .gtmap import (  # noqa: F401
    check_label_flag, CONFUSION_MAX_CLASSES, CONFUSION_MAX_COUNTERS, _counter_arg, _counter_check, _counter_result,
    _dtype_of, gt_labels, GT_MAX_CLASSES, GT_MAX_VOTES, gt_vote, _ids_i32, label_confusion, label_confusion_limits,
    map_scores, MapScores, obj2cls_table, pool_labels_2d, UNLABELLED,
)
from .resize import (  # noqa: F401
    clip_preprocess, clip_preprocess_plan, clip_table, CLIP_MEAN, CLIP_STD, resize_coeffs, RESIZE_LDS_COEFS, RESIZE_LDS_SPAN,
    resize_limits, RESIZE_MAX_BATCH, RESIZE_MAX_CHANNELS, RESIZE_MAX_SIDE, RESIZE_TILE_W, resize_u8,
)
from .instances import (  # noqa: F401
    Instance3D, INSTANCE_TABLE_COLS, INSTANCES_MAX_BOX_SIDE, label_voxels, VoxelInstances,
)
from .select import (  # noqa: F401
    cols_above, COLSELECT_SLOTS, column_order_stats, column_quantiles, ColumnOrderStats, quantile_index, quantile_lerp,
)
from .audit import (  # noqa: F401
    AUDIT_MAX_SIDE, audit_rays, cell_index, CellIndex, lookup_cells, NEVER_HIT,
)
from .sight import (  # noqa: F401
    line_of_sight, LOS_INVALID, LOS_MAX_TARGETS, LOS_VISIBLE, visible_counts,
)
from .match import (  # noqa: F401
    match_angles, match_frames, MATCH_MAX_ANGLES, MATCH_MAX_RADIUS, MATCH_MAX_SPLIT, MatchResult,
)
from .objects import (  # noqa: F401
    label_voxel_classes, Object3D, pick_columns, POOL_CHUNK, pool_rows, vote_rows, VoxelObjects,
)
from .relations import (  # noqa: F401
    object_relations, ObjectRelations, RELATION_TABLE_COLS, RELATIONS_MAX_PAIRS, RELATIONS_MAX_RADIUS,
)
from .travel import (  # noqa: F401
    travel_decay_2d, travel_field, TRAVEL_MAX_SIDE, TRAVEL_NEIGHBOURS, TRAVEL_SWEEPS, TRAVEL_TILE, TravelField, UNREACHED,
)
from .rooms import (  # noqa: F401
    DOOR_TABLE_COLS, grow_labels, LabelGrowth, lift_labels_2d, ROOM_TABLE_COLS, room_seeds, room_tables, ROOMS_MAX,
    RoomSegmentation, _seed_image, segment_rooms,
)
from .viewshed import (  # noqa: F401
    best_heading, octant_of, viewshed_gain, VIEWSHED_MAX_RADIUS, viewshed_seen,
)
from .costmap import (  # noqa: F401
    build_costmap, cost_field, COST_LETHAL, COST_MAX, COST_MAX_CELLS, COST_MAX_LAYERS, CostField, distance_to_mask, drop_collinear,
    inflation_table, penalty_table,
)
from .travelmany import (  # noqa: F401
    sound_travel_field, sound_travel_normalize, travel_arrivals, travel_fields, TRAVEL_MANY_MAX_FIELDS, TRAVEL_MANY_MAX_PAIRS,
    TravelArrivals, TravelFields,
)
from .mapdiff import (  # noqa: F401
    cosine_of, DIFF_CHANGED, DIFF_MAX_DIM, DIFF_MAX_RADIUS, DIFF_NO_MATCH, DIFF_SAME, DIFF_STREAM_ROWS, DIFF_UNSEEN, diff_status,
    DiffSide, map_diff, MapDiff, match_cells, row_dots,
)
from .mapfuse import (  # noqa: F401
    check_gain, check_transform, FUSE_COUNTS, FUSE_ERR_OUTSIDE, FUSE_ERR_SHARED, FUSE_MAX_DIM, fuse_maps, fuse_plan, fuse_rows, FusedMap,
    FusePlan, move_cells,
)
from .mappull import (  # noqa: F401
    check_interp, check_min_support, inverse_transform, PULL_COUNTS, PULL_INTERP, PULL_MAX_DIM, pull_map, pull_plan, pull_rows, PulledMap,
    PullPlan,
)
# the shared marshalling layer; its one device predicate keeps both of the names it had here
from ._args import (  # noqa: F401
    _dev_u8, _image_any, _image_shape, _image_u8, _is_dev, _is_dev as _on_device, _result,
)
