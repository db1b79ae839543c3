"""The host side of the image resize and of CLIP's preprocess (ops/resize.py, csrc/avl_resize.hip's argument checks), without a GPU:
the NumPy twin of _resize_ref.py is tied to PIL.Image.resize byte for byte, the golden file to the Pillow installed here, and
ops.resize_coeffs, the crop plan and the normalisation table to the twin."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _resize_ref as R  # noqa: E402

FILTER_NAMES = ("box", "bilinear", "bicubic")


def pil_resize(img, oh, ow, filter):
    Image = pytest.importorskip("PIL.Image")
    f = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[filter]
    return np.asarray(Image.fromarray(img).resize((ow, oh), f))


def test_twin_equals_pillow_on_every_case():
    pytest.importorskip("PIL")
    n = 0
    for (H, W, oh, ow, filters) in R.RESIZE_CASES:
        for f in filters:
            for shape in ((H, W), (H, W, 3)):
                for img in R.make_images(n, shape):
                    assert np.array_equal(R.resize_ref(img, (oh, ow), f), pil_resize(img, oh, ow, f)), (H, W, oh, ow, f, shape)
                    win = R.inner_window(oh, ow)
                    assert np.array_equal(R.resize_ref(img, (oh, ow), f, win),
                                          pil_resize(img, oh, ow, f)[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
                    n += 1
    for (H, W) in R.CLIP_CASES + (R.WORKLOAD,):
        oh, ow, top, left = R.plan_ref(H, W)
        for img in R.make_images(n, (H, W, 3)):
            want = pil_resize(img, oh, ow, "bicubic")[top:top + 224, left:left + 224]
            assert np.array_equal(R.resize_ref(img, (oh, ow), "bicubic", (top, left, 224, 224)), want), (H, W)
            n += 1
    assert n == 2 * (2 * 7 + 8)


def test_golden_file_equals_this_pillow(golden):
    PIL = pytest.importorskip("PIL")
    g = golden("g14_resize.npz")
    meta = g["meta"]
    assert len(meta) == 28 and str(g["pillow_version"])
    for i, (oh, ow, f, top, left, h, w) in enumerate(meta.tolist()):
        got = pil_resize(g[f"in_{i}"], oh, ow, FILTER_NAMES[f])[top:top + h, left:left + w]
        assert np.array_equal(got, g[f"out_{i}"]), (i, PIL.__version__, str(g["pillow_version"]))
        assert np.array_equal(R.resize_ref(g[f"in_{i}"], (oh, ow), FILTER_NAMES[f], (top, left, h, w)), g[f"out_{i}"]), i


def test_resize_coeffs_equal_the_twin():
    from avlmaps_amd import ops
    sizes = {(W, ow) for (H, W, oh, ow, _) in R.RESIZE_CASES} | {(H, oh) for (H, W, oh, ow, _) in R.RESIZE_CASES}
    sizes |= {(720, 224), (1080, 336), (37, 224), (53, 320), (1, 224), (151, 338), (224, 1), (16384, 3), (3, 1000)}
    for (a, b) in sorted(sizes):
        for f in FILTER_NAMES:
            k, bounds = ops.resize_coeffs(a, b, f)
            kr, br = R.coeffs_ref(a, b, f)
            assert k.dtype == np.int32 and bounds.dtype == np.int32 and k.shape == kr.shape and bounds.shape == (b, 2)
            assert np.array_equal(k, kr) and np.array_equal(bounds, br), (a, b, f)
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= a).all() and (bounds[:, 1] <= k.shape[1]).all()
            # what the kernel's span staging relies on (it falls back to global reads otherwise): both ends are monotone
            assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(axis=1)) >= 0).all()
            assert 255 * int(np.abs(k.astype(np.int64)).sum(axis=1).max()) + (1 << 21) < 1 << 31
    assert ops.resize_coeffs(1080, 336)[0].shape[1] == 15 and ops.resize_coeffs(720, 224)[0].shape[1] == 15
    assert int(ops.resize_coeffs(720, 224)[1][:, 1].max()) == 13
    with pytest.raises(ValueError):
        ops.resize_coeffs(10, 5, "lanczos")
    with pytest.raises(ValueError):
        ops.resize_coeffs(0, 5)
    with pytest.raises(ValueError):
        ops.resize_coeffs(5, ops.RESIZE_MAX_SIDE + 1)


def test_accumulator_bound_is_checked_before_any_upload(monkeypatch):
    from avlmaps_amd.ops import resize

    def huge(in_size, out_size, filter="bicubic"):
        k = np.full((out_size, 3), 1 << 22, np.int32)         # 255 * 3 * 2^22 + 2^21 >= 2^31
        return k, np.zeros((out_size, 2), np.int32)
    monkeypatch.setattr(resize, "resize_coeffs", huge)
    with pytest.raises(ValueError, match="overflows"):
        resize._resize_tables(9, 4, "bicubic", None)
    assert resize._resize_tables(9, 9, "bicubic", None) is None


def test_crop_plan():
    from avlmaps_amd import ops
    cases = {(720, 1080): (224, 336, 0, 56), (1080, 720): (336, 224, 56, 0), (224, 224): (224, 224, 0, 0),
             (224, 225): (224, 225, 0, 0),           # (225 - 224) / 2 = 0.5 rounds to the even 0
             (224, 227): (224, 227, 0, 2),           # 1.5 rounds to the even 2
             (225, 224): (225, 224, 0, 0), (227, 224): (227, 224, 2, 0), (37, 53): (224, 320, 0, 48), (100, 151): (224, 338, 0, 57),
             (1, 1): (224, 224, 0, 0), (480, 640): (224, 298, 0, 37)}
    for (h, w), want in cases.items():
        assert ops.clip_preprocess_plan(h, w) == want == R.plan_ref(h, w), (h, w)
    assert ops.clip_preprocess_plan(100, 151, n_px=32) == (32, 48, 0, 8)
    with pytest.raises(ValueError):
        ops.clip_preprocess_plan(0, 5)


def test_normalisation_table():
    from avlmaps_amd import ops
    t = ops.clip_table()
    v = np.arange(256, dtype=np.float32)
    for c in range(3):
        want = (v / np.float32(255) - np.float32(ops.CLIP_MEAN[c])) / np.float32(ops.CLIP_STD[c])
        assert want.dtype == np.float32 and np.array_equal(t[:, c], want)
    assert t.shape == (256, 3) and t.dtype == np.float32 and np.array_equal(t, R.table_ref())
    h = ops.clip_table(dtype=np.float16)
    assert h.dtype == np.float16 and np.array_equal(h, t.astype(np.float16)) and np.array_equal(h, R.table_ref(dtype=np.float16))
    assert ops.CLIP_MEAN == R.CLIP_MEAN and ops.CLIP_STD == R.CLIP_STD
    other = ops.clip_table((0.5, 0.5, 0.5), (0.5, 0.25, 2.0))
    assert other[255, 0] == np.float32(1.0) and other[0, 1] == np.float32(-2.0)
    with pytest.raises(TypeError):
        ops.clip_table(dtype=np.float64)
    with pytest.raises(ValueError):
        ops.clip_table(std=(1.0, 0.0, 1.0))


def test_compared_with_the_real_preprocess_when_it_is_installed():
    """torchvision's Resize / CenterCrop / ToTensor / Normalize, which is what clip._transform composes (never run where neither
    package is installed: DESIGN 4.18 says so)"""
    T = pytest.importorskip("torchvision.transforms")
    Image = pytest.importorskip("PIL.Image")
    tf = T.Compose([T.Resize(224, interpolation=T.InterpolationMode.BICUBIC), T.CenterCrop(224), T.ToTensor(),
                    T.Normalize(R.CLIP_MEAN, R.CLIP_STD)])
    for (H, W) in R.CLIP_CASES:
        img = R.make_images(H * W, (H, W, 3))[0]
        assert np.array_equal(tf(Image.fromarray(img)).numpy(), R.clip_preprocess_ref(img)), (H, W)


def test_argument_checks_before_device_work():
    from avlmaps_amd import _lib
    lib = _lib.load()
    err = lib.avl_last_error
    fake, n = C.c_void_p(4096), C.c_size_t(0)
    assert lib.avl_resize_limits(None, None, None) != 0 and b"null" in err()
    assert lib.avl_resize_work_bytes(1, 8, 3, 8, 1, None) != 0 and b"null" in err()
    assert lib.avl_resize_work_bytes(0, 8, 3, 8, 1, C.byref(n)) == 1 and b"B=" in err()
    assert lib.avl_resize_work_bytes(65536, 8, 3, 8, 1, C.byref(n)) == 1
    assert lib.avl_resize_work_bytes(1, 16385, 3, 8, 1, C.byref(n)) == 1 and b"sides" in err()
    assert lib.avl_resize_work_bytes(1, 8, 5, 8, 1, C.byref(n)) == 1 and b"C=" in err()
    assert lib.avl_resize_work_bytes(1, 8, 3, 0, 1, C.byref(n)) == 1 and b"out_w" in err()
    assert lib.avl_resize_work_bytes(2, 10, 3, 7, 1, C.byref(n)) == 0 and n.value >= 2 * 10 * 24
    assert lib.avl_resize_work_bytes(2, 10, 3, 7, 0, C.byref(n)) == 0 and n.value <= 512

    def rs(d_in=fake, B=1, H=8, W=8, Cn=3, kh=fake, bh=fake, ksh=5, ow=4, kv=fake, bv=fake, ksv=5, oh=4, top=0, left=0, h=4, w=4,
           out=fake, ws=fake, nws=1 << 20):
        return lib.avl_resize_u8(d_in, B, H, W, Cn, kh, bh, ksh, ow, kv, bv, ksv, oh, top, left, h, w, out, ws, nws, None)
    assert rs(d_in=None) != 0 and b"null" in err()
    assert rs(out=None) != 0 and b"null" in err()
    assert rs(B=0) == 1 and rs(H=0) == 1 and rs(W=16385) == 1 and b"sides" in err()
    assert rs(Cn=0) == 1 and rs(Cn=5) == 1 and b"C=" in err()
    assert rs(bh=None) == 1 and b"both" in err()
    assert rs(kv=None) == 1 and b"both" in err()
    assert rs(kh=None, bh=None) == 1 and b"width" in err()            # no pass, but ow != W
    assert rs(kv=None, bv=None) == 1 and b"height" in err()
    assert rs(ow=0) == 1 and rs(oh=16385) == 1 and b"resized" in err()
    assert rs(ksh=0) == 1 and b"ksize_h" in err()
    assert rs(ksv=65538) == 1 and b"ksize_v" in err()
    for bad in (dict(top=-1), dict(left=-1), dict(h=0), dict(w=0), dict(top=1), dict(left=1), dict(h=5), dict(w=5),
                dict(top=2 ** 31 - 1), dict(w=2 ** 31 - 1)):
        assert rs(**bad) == 1 and b"window" in err(), bad
    assert rs(kh=C.c_void_p(4098)) == 1 and b"aligned" in err()
    assert rs(ws=None) == 1 and b"workspace" in err()
    assert rs(nws=16) == 1 and b"workspace" in err()

    def cp(table=fake, f16=0, out=fake, **kw):
        a = dict(d_in=fake, B=1, H=8, W=8, kh=fake, bh=fake, ksh=5, ow=4, kv=fake, bv=fake, ksv=5, oh=4, top=0, left=0, h=4, w=4)
        a.update(kw)
        return lib.avl_clip_preprocess(a["d_in"], a["B"], a["H"], a["W"], a["kh"], a["bh"], a["ksh"], a["ow"], a["kv"], a["bv"], a["ksv"],
                                       a["oh"], a["top"], a["left"], a["h"], a["w"], table, f16, out, fake, 1 << 20, None)
    assert cp(table=None) != 0 and b"null" in err()
    assert cp(d_in=None) != 0 and b"null" in err()
    assert cp(f16=2) == 1 and b"out_f16" in err()
    assert cp(out=C.c_void_p(4098)) == 1 and b"aligned" in err()
    assert cp(out=C.c_void_p(4097), f16=1) == 1 and b"aligned" in err()
    assert cp(left=1) == 1 and b"window" in err()


def test_ops_reject_bad_arguments_without_a_gpu():
    from avlmaps_amd import ops
    img = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(TypeError):
        ops.resize_u8(img.astype(np.float32), (4, 4))
    with pytest.raises(ValueError):
        ops.resize_u8(np.zeros((2, 2, 2, 2, 2), np.uint8), (4, 4))
    with pytest.raises(ValueError):
        ops.resize_u8(np.zeros((8, 9, 5), np.uint8), (4, 4))
    with pytest.raises(ValueError):
        ops.resize_u8(img, (4, 4), window=(0, 0, 5, 4))
    with pytest.raises(ValueError):
        ops.resize_u8(img, (0, 4))
    with pytest.raises(ValueError):
        ops.resize_u8(img, (4, 4), filter="hamming")
    with pytest.raises(ValueError):
        ops.clip_preprocess(np.zeros((8, 9), np.uint8))
    with pytest.raises(ValueError):
        ops.clip_preprocess(np.zeros((8, 9, 4), np.uint8))
    with pytest.raises(ValueError):
        ops.clip_preprocess(np.zeros((1, 200, 3), np.uint8))          # 1 x 200 resizes to 224 x 44 800
    with pytest.raises(TypeError):
        ops.clip_preprocess(img, dtype=np.float64)
    assert ops.resize_limits() == (ops.RESIZE_TILE_W, ops.RESIZE_LDS_COEFS, ops.RESIZE_LDS_SPAN)


def test_create_map_cli_accepts_area(capsys):
    from avlmaps_amd.apps import create_map
    with pytest.raises(SystemExit):
        create_map.main(["--data-dir", "s", "--area", "--area-model", "hash", "--area-batch", "0"])
    assert "--area-batch must be at least 1" in capsys.readouterr().err       # everything before it was parsed
    with pytest.raises(SystemExit):
        create_map.main(["--data-dir", "s", "--area", "--area-model", "resnet"])
    assert "--area-model" in capsys.readouterr().err


def test_hash_batch_encoder_and_upstream_shaped_names():
    from avlmaps_amd.apps.common import HashBatchImageEncoder
    from avlmaps_amd.utils import clip_utils
    x = np.random.default_rng(5).standard_normal((3, 3, 224, 224)).astype(np.float32)
    enc = HashBatchImageEncoder()
    f = enc(x)
    assert f.shape == (3, 768) and f.dtype == np.float32 and np.allclose(np.linalg.norm(f.astype(np.float64), axis=1), 1.0, atol=1e-6)
    code = x.astype(np.float64).reshape(3, 3, 4, 56, 4, 56).mean(axis=(3, 5)).reshape(3, 48)
    want = code @ enc.proj
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(f - want).max() <= 2.0 ** -23
    for name in ("ClipPreprocess", "get_img_feats", "get_imgs_feats", "get_imgs_feats_batch"):
        assert callable(getattr(clip_utils, name))
    p = clip_utils.ClipPreprocess()
    assert p.n_px == 224 and p.mean == R.CLIP_MEAN and p.std == R.CLIP_STD
