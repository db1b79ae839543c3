"""The surface of the avlmaps_amd.ops package without a GPU and without the library: every name the single-module ops.py offered is
still an attribute of the package, each function and class is defined in exactly one family module, the package's __init__ only
imports, and importing it neither imports torch nor loads the library."""
import ast
import inspect
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
OPS = ROOT / "avlmaps_amd" / "ops"

# dir(avlmaps_amd.ops) of the last single-module ops.py, without dunders and without the imports C, np, Path and annotations
NAMES = """
    AUDIO_MAX_CHANNELS AUDIO_MAX_SAMPLES AudioSegments BatchPlan CONFUSION_MAX_CLASSES CONFUSION_MAX_COUNTERS
    Correspondences DeviceArray DeviceView EDT_MAX_SIDE EXPLORE_MAX_SIDE GOAL_CONES GOAL_DENSE_F32 GOAL_DENSE_F64
    GOAL_FIELD_F32 GOAL_FIELD_F64 GOAL_MAX_TERMS GT_MAX_CLASSES GT_MAX_VOTES GoalField GoalResult GoalTerm HeatPlan
    ISLANDS_MAX_SIDE ISLAND_TABLE_COLS Islands MapScores NAV_MANY_MAX NAV_MAX_SIDE NAV_MAX_VERTICES NEAREST_PAIR_MAX_COORD
    NEVER_SEEN NavGraph NavPlanMany PNP_DEFAULT_HYPOTHESES PNP_MAX_ERROR PNP_MAX_ITERATIONS PNP_STEP_TOLERANCE PRECISION
    PnpRansacResult PnpRefineResult PreparedMap ProductResult RENDER_MAX_SIDE RESAMPLE_LDS_TAPS RESAMPLE_LDS_WINDOW
    RESAMPLE_MAX_RATIO RESAMPLE_TILE UNLABELLED VoxelAccumulator Window _GoalTermC _HOST_PLANS _MORPH_OPS _MORPH_STRUCTURES
    _RESAMPLE_TAPS _RESAMPLE_TAPS_KEPT _WS_CACHE _WindowTermC _audio_f32 _audio_len _background3 _camera3 _check_decay
    _check_ranges _corr_args _counter_arg _counter_check _counter_result _dev_u8 _device_taps _dtype_of _edt_workspace
    _f64_2d _fingerprint _global_depth _heat_arg _host_heat_plan _ids_i32 _image_any _image_shape _image_u8 _is_dev
    _is_torch _lib _mask_dtype_check _mix32 _on_device _points_i32 _result _rgb_arg _sim_scores_compact _sim_workspace
    _table_arg area_field argmax_f32 as_device binary_morph carve_free_space check_label_flag colorize_heat context_ranges
    contour_nearest_pair decode_pcm decode_pcm16 dilate_map distance_transform_edt export_raw_torch field_lift
    field_normalize finalize_merged finalize_raw frontier_mask gaussian_filter2d gaussian_filter2d_f32 gaussian_weights
    goal_fuse goal_terms_array gt_labels gt_vote heatmap_from_mask jet_table label_confusion label_confusion_limits
    label_islands loc_lift map_scores mask_bool_from_argmax mask_decay_2d mask_foreground mask_from_argmax nav_graph
    obj2cls_table obstacle_map obstacle_scatter pack_tracks planar_decay pnp_lds_stage pnp_ransac pnp_refine
    pnp_sample_indices pnp_score points_bbox pool_label_2d pool_labels_2d prepare_map product_argmax_2d query_col_support
    render_topdown render_view resample_audio resample_limits resample_ratio resample_taps resize2x_down resize2x_up
    retrieve_frame rgb_topdown segment_audio sim_scores sound_field topk_f32 trace_islands unpack_rows
""".split()


def _definitions(path):
    """names of the functions and classes a module defines at its top level"""
    return [n.name for n in ast.parse(path.read_text()).body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef))]


def test_the_package_keeps_the_surface_one_definition_each_and_a_bare_import():
    from avlmaps_amd import ops
    assert len(NAMES) == len(set(NAMES)) == 164
    missing = [n for n in NAMES if not hasattr(ops, n)]
    assert not missing, missing

    # __init__ only imports (after its docstring)
    body = ast.parse((OPS / "__init__.py").read_text()).body
    assert all(isinstance(n, (ast.Import, ast.ImportFrom)) for n in body[1:]) and isinstance(body[0], ast.Expr)
    assert not any(a.name == "*" for n in body[1:] for a in n.names)

    # every function / class of the package among the names is defined in exactly one submodule, the one it says it lives in
    defined = {}
    for path in sorted(OPS.glob("*.py")):
        for name in _definitions(path):
            defined.setdefault(name, []).append(path.stem)
    assert "__init__" not in {m for mods in defined.values() for m in mods}
    assert {n: m for n, m in defined.items() if len(m) != 1} == {}
    own = 0
    for n in NAMES:
        obj = getattr(ops, n)
        if (inspect.isfunction(obj) or inspect.isclass(obj)) and obj.__module__.startswith("avlmaps_amd.ops"):
            assert defined.get(obj.__name__) == [obj.__module__.rsplit(".", 1)[1]], (n, obj.__module__, defined.get(obj.__name__))
            own += 1
    assert own == 121          # 104 functions + 21 classes, less the four (DeviceArray, DeviceView, as_device, _is_torch) of avlmaps_amd.device

    # a bare import in a fresh interpreter: no torch, no library
    code = ("import sys; import avlmaps_amd.ops; from avlmaps_amd import _lib; "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert _lib._lib is None, 'the library was loaded'")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
