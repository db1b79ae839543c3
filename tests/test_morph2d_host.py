"""CPU-side checks of the 2-D morphology layer: the C ABI entries and their ctypes signatures, the host-side gaussian weights against
SciPy's own, Map._dilate_map without OpenCV, compat.install re-pointing upstream's Map._dilate_map, and the apps' new flags."""
import ctypes as C
import inspect
import sys
import textwrap

import numpy as np
import pytest

MORPH_SYMBOLS = ("avl_morph_binary", "avl_gauss2d_f64", "avl_resize2x_up_f64", "avl_resize2x_down_f64", "avl_dilate_map_work_bytes",
                 "avl_dilate_map", "avl_mask_foreground_work_bytes", "avl_mask_foreground")


@pytest.fixture(scope="module")
def lib():
    from avlmaps_amd import _lib
    from avlmaps_amd.build import build
    build()
    return _lib.load()


def test_ctypes_signatures_exist(lib):
    from avlmaps_amd import _lib, ops
    for name in MORPH_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None and len(fn.argtypes) == len(_lib._SIGS[name][1])
    assert len(lib.avl_morph_binary.argtypes) == 9 and len(lib.avl_gauss2d_f64.argtypes) == 11
    assert len(lib.avl_dilate_map.argtypes) == 10 and len(lib.avl_mask_foreground.argtypes) == 10
    for name in ("binary_morph", "gaussian_filter2d", "dilate_map", "mask_foreground", "resize2x_up", "resize2x_down"):
        assert callable(getattr(ops, name))
        assert "device" in inspect.signature(getattr(ops, name)).parameters


def test_arguments_are_validated_before_any_device_work(lib):
    """argument checks come first, so they are testable without a GPU"""
    n = C.c_size_t(0)
    assert lib.avl_dilate_map_work_bytes(1000, 1000, C.byref(n)) == 0
    assert n.value >= 4 * 1000 * 1000 * 8 + 2 * 4 * 1000 * 1000                   # the float64 intermediate and two byte images at 2x
    assert lib.avl_mask_foreground_work_bytes(300, 400, C.byref(n)) == 0 and n.value >= 300 * 400 * 10
    assert lib.avl_dilate_map_work_bytes(0, 5, C.byref(n)) != 0
    one = C.c_void_p(256)                                                         # never dereferenced: every call below is refused
    assert lib.avl_morph_binary(one, 8, 8, 0, 0, 128, C.c_void_p(512), None, None) != 0 and b"iterations" in lib.avl_last_error()
    assert lib.avl_morph_binary(one, 8, 8, 0, 0, 0, C.c_void_p(512), None, None) != 0
    assert lib.avl_morph_binary(one, 8, 8, 2, 0, 1, C.c_void_p(512), None, None) != 0 and b"op" in lib.avl_last_error()
    assert lib.avl_morph_binary(one, 8, 8, 0, 0, 6, C.c_void_p(512), None, None) != 0 and b"d_tmp" in lib.avl_last_error()
    w = np.ones(3)
    assert lib.avl_gauss2d_f64(one, 1, 8, 8, w.ctypes.data, 33, C.c_void_p(512), None, 0.5, C.c_void_p(1024), None) != 0
    assert lib.avl_gauss2d_f64(one, 1, 8, 8, w.ctypes.data, 1, None, None, 0.5, C.c_void_p(1024), None) != 0
    assert lib.avl_dilate_map(one, 8, 8, 64, 1.0, C.c_void_p(512), None, C.c_void_p(1024), 1 << 20, None) != 0
    assert lib.avl_dilate_map(one, 8, 8, 3, 1.0, C.c_void_p(512), None, C.c_void_p(1024), 16, None) != 0 and b"workspace" in lib.avl_last_error()
    assert lib.avl_mask_foreground(one, 100, 5, 5, 0, 10, C.c_void_p(512), C.c_void_p(1024), 1 << 20, None) != 0
    assert lib.avl_mask_foreground(one, 100, 0, 5, 0, 101, C.c_void_p(512), C.c_void_p(1024), 1 << 20, None) != 0


@pytest.mark.parametrize("sigma", [0.5, 0.8, 1.0, 2.0, 2.3, 7.9])
@pytest.mark.parametrize("truncate", [3, 4.0])
def test_gaussian_weights_equal_scipys(sigma, truncate):
    from scipy.ndimage._filters import _gaussian_kernel1d
    from avlmaps_amd import ops
    w, radius = ops.gaussian_weights(sigma, truncate)
    assert radius == int(truncate * float(sigma) + 0.5) and w.dtype == np.float64 and w.shape == (2 * radius + 1,)
    assert np.array_equal(w, _gaussian_kernel1d(sigma, 0, radius))
    assert np.array_equal(w, w[::-1])                                              # symmetric: SciPy takes its symmetric summation branch


def test_dilate_map_does_not_import_cv2():
    from avlmaps_amd.map.map import Map
    from avlmaps_amd.map.vlmap import VLMap
    for fn in (Map._dilate_map, VLMap.customize_obstacle_map, VLMap.get_pos):
        src = inspect.getsource(fn)
        assert "import cv2" not in src and "scipy" not in src.split('"""')[2], fn.__name__
    assert "dilate_map" in inspect.getsource(Map._dilate_map)
    assert list(inspect.signature(Map._dilate_map).parameters) == ["binary_map", "dilate_iter", "gaussian_sigma"]
    assert inspect.signature(Map._dilate_map).parameters["dilate_iter"].default == 0
    assert isinstance(Map.__dict__["_dilate_map"], staticmethod)
    m = Map.__new__(Map)
    m.obstacles_cropped, m.obstacles_new_cropped = "raw", "custom"
    assert m.get_obstacle_cropped() == "raw" and m.get_customized_obstacle_cropped() == "custom"


def test_no_cpu_fallback_for_the_morphology(lib):
    from avlmaps_amd import _lib, ops
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.AvlError):
        ops.dilate_map(np.zeros((4, 4), bool), 1, 1.0)
    with pytest.raises(_lib.AvlError):
        ops.mask_foreground(np.zeros((4, 4), bool))


def test_compat_install_repoints_dilate_map(tmp_path):
    from avlmaps_amd import compat
    name = "fake_avlmaps_morph_pkg"
    root = tmp_path / name
    for sub in ("", "map"):
        (root / sub).mkdir(parents=True, exist_ok=True)
        (root / sub / "__init__.py").write_text("")
    (root / "map" / "map.py").write_text(textwrap.dedent("""
        class Map:
            def generate_obstacle_map(self, h_min=0, h_max=1.5):
                return 'upstream-obstacles'
            @staticmethod
            def _dilate_map(binary_map, dilate_iter=0, gaussian_sigma=1.0):
                return 'upstream-cv2'
    """))
    sys.path.insert(0, str(tmp_path))
    try:
        import importlib
        mp = importlib.import_module(f"{name}.map.map")
        counts = compat.install(name)
        assert counts["map.map.Map._dilate_map"] == 1 and counts["map.map.Map.generate_obstacle_map"] == 1
        assert isinstance(mp.Map.__dict__["_dilate_map"], staticmethod)
        assert "avl_dilate_map" in mp.Map._dilate_map.__doc__ and "avl_dilate_map" in mp.Map()._dilate_map.__doc__
        compat.uninstall(name)
        assert mp.Map._dilate_map(None) == "upstream-cv2" and mp.Map()._dilate_map(None) == "upstream-cv2"
    finally:
        compat.uninstall(name)
        sys.path.remove(str(tmp_path))
        for m in [m for m in sys.modules if m == name or m.startswith(name + ".")]:
            del sys.modules[m]


def test_plan_path_obstacle_flags():
    from avlmaps_amd.apps import generate_obstacle_map, plan_path
    from avlmaps_amd.apps.common import load_config
    base = ["--data-dir", "x", "--query", "sofa", "--start", "1", "2"]
    a = plan_path.parse_args(base)
    assert not a.customize_obstacles and plan_path.obstacle_overrides(a) == {}
    a = plan_path.parse_args(base + ["--customize-obstacles"])
    assert a.customize_obstacles and plan_path.obstacle_overrides(a) == {}
    cfg = load_config(None, overrides={f"map_config.{k}": v for k, v in plan_path.obstacle_overrides(a).items()})
    assert cfg.map_config.dilate_iter == 3 and cfg.map_config.gaussian_sigma == 1.0            # upstream's vlmaps.yaml:14-15
    a = plan_path.parse_args(base + ["--customize-obstacles", "--potential-obstacles", "chair, wall,other", "--obstacles", "wall",
                                     "--dilate-iter", "2", "--gaussian-sigma", "0.5"])
    ov = plan_path.obstacle_overrides(a)
    assert ov == {"potential_obstacle_names": ["chair", "wall", "other"], "obstacle_names": ["wall"], "dilate_iter": 2, "gaussian_sigma": 0.5}
    cfg = load_config(None, overrides={f"map_config.{k}": v for k, v in ov.items()})
    assert cfg.map_config.obstacle_names == ["wall"] and cfg.map_config.dilate_iter == 2
    with pytest.raises(SystemExit):
        plan_path.parse_args(base + ["--obstacles", "wall"])                                   # belongs to --customize-obstacles
    g = generate_obstacle_map.parse_args(["--data-dir", "x", "--obstacles", "wall,table"])
    assert plan_path.obstacle_overrides(g) == {"obstacle_names": ["wall", "table"]}
