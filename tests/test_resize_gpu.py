"""Pillow's 8-bit resize and CLIP's preprocess on the GPU (csrc/avl_resize.hip through ops.resize_u8 and ops.clip_preprocess), and the
batched area map on top of them.

Oracles: the NumPy twin of _resize_ref.py, which test_resize_host.py ties to PIL.Image.resize byte for byte, and Pillow's own
bytes in tests/golden/g14_resize.npz.  The arithmetic is integer and the normalisation a table, so every comparison of pixels is
np.array_equal over the whole output.  Shapes are the smallest at which the kernel can go wrong: fewer columns than a tile of 64,
a tile and a bit, rows that are no multiple of 4, windows that start and end inside a tile, either pass alone, neither, a
coefficient table beyond the LDS budget, spans that start at every byte alignment (C = 1, 3, 4), and once the workload's own shape."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(Path(__file__).resolve().parent))
import _resize_ref as R  # noqa: E402

FILTER_NAMES = ("box", "bilinear", "bicubic")


@pytest.fixture(scope="module")
def ops():
    from avlmaps_amd import _lib, ops
    _lib.load()
    _lib.require_gpu()
    return ops


def as_input(ops, a, route):
    """the same pixels as a host array, a DeviceArray or a torch tensor on the GPU"""
    if route % 3 == 0:
        return a
    if route % 3 == 1:
        return ops.DeviceArray.from_numpy(a)
    import torch
    return torch.from_numpy(a).cuda()


def test_kernel_equals_pillows_bytes_in_the_golden_file(ops, golden):
    g = golden("g14_resize.npz")
    for i, (oh, ow, f, top, left, h, w) in enumerate(g["meta"].tolist()):
        got = ops.resize_u8(as_input(ops, g[f"in_{i}"], i), (oh, ow), FILTER_NAMES[f], window=(top, left, h, w))
        assert got.dtype == np.uint8 and np.array_equal(got, g[f"out_{i}"]), (i, oh, ow, FILTER_NAMES[f])


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}x{c[3]}")
def test_resize_u8_equals_the_twin(ops, case):
    H, W, oh, ow, filters = case
    route = 0
    for f in filters:
        for Cn in (1, 3, 4):
            imgs = R.make_images(H * 7 + Cn, (H, W, Cn)) + R.make_images(W * 5 + Cn, (H, W, Cn))[:1]      # three distinct images
            want = [R.resize_ref(a, (oh, ow), f) for a in imgs]
            win = R.inner_window(oh, ow)
            for k, a in enumerate(imgs[:2]):                                   # B = 1: a random and a 0 / 255 image
                got = ops.resize_u8(as_input(ops, a[:, :, 0] if Cn == 1 else a, route), (oh, ow), f)
                route += 1
                assert got.shape == ((oh, ow) if Cn == 1 else (oh, ow, Cn))
                assert np.array_equal(got.reshape(oh, ow, Cn), want[k]), (f, Cn, k)
                got = ops.resize_u8(as_input(ops, a, route), (oh, ow), f, window=win)
                route += 1
                assert np.array_equal(got, want[k][win[0]:win[0] + win[2], win[1]:win[1] + win[3]]), (f, Cn, k, win)
            got = ops.resize_u8(as_input(ops, np.stack(imgs), route), (oh, ow), f, window=win, device=True)       # B = 3
            route += 1
            assert isinstance(got, ops.DeviceArray) and got.shape == (3, win[2], win[3], Cn)
            assert np.array_equal(got.numpy(), np.stack([x[win[0]:win[0] + win[2], win[1]:win[1] + win[3]] for x in want])), (f, Cn)
    if W == 2000:         # the table is the one beyond the LDS budget, and its rows pass the accumulator check with room to spare
        k, _ = ops.resize_coeffs(W, ow)
        assert ops.RESIZE_TILE_W * k.shape[1] > ops.RESIZE_LDS_COEFS and k.shape[1] == 261
        assert 255 * int(np.abs(k.astype(np.int64)).sum(axis=1).max()) + (1 << 21) < 1 << 31


@pytest.mark.parametrize("hw", R.CLIP_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_clip_preprocess_equals_the_twin(ops, hw):
    H, W = hw
    imgs = R.make_images(H * 1000 + W, (H, W, 3)) + R.make_images(H + W, (H, W, 3))[:1]
    want32 = np.stack([R.clip_preprocess_ref(a) for a in imgs])
    want16 = np.stack([R.clip_preprocess_ref(a, dtype=np.float16) for a in imgs])
    assert want32.dtype == np.float32 and want16.dtype == np.float16
    for k in range(2):                                                          # B = 1, both kinds of image, every route in
        got = ops.clip_preprocess(as_input(ops, imgs[k], k + H))
        assert isinstance(got, ops.DeviceArray) and got.shape == (1, 3, 224, 224) and got.dtype == np.float32
        assert np.array_equal(got.numpy(), want32[k:k + 1]), k
    got = ops.clip_preprocess(as_input(ops, np.stack(imgs), 2 + H), device=False)                  # B = 3
    assert got.dtype == np.float32 and np.array_equal(got, want32)
    got = ops.clip_preprocess(as_input(ops, np.stack(imgs), 1 + H), dtype=np.float16, device=False)
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), want16.view(np.uint16))
    t = ops.clip_preprocess(np.stack(imgs), as_torch=True)
    assert t.is_cuda and tuple(t.shape) == (3, 3, 224, 224) and np.array_equal(t.cpu().numpy(), want32)
    # the uint8 pixels under the table, with a window that starts and ends inside a tile
    oh, ow, top, left = R.plan_ref(H, W)
    win = (top + 5, left + 70, 46, 83)
    got = ops.resize_u8(imgs[1], (oh, ow), window=win)
    assert np.array_equal(got, R.resize_ref(imgs[1], (oh, ow), "bicubic", win))
    if (H, W) == (37, 53):            # the 0 / 255 image, upscaled: the overshoot reaches both ends of the clamp
        full = ops.resize_u8(imgs[1], (oh, ow))
        assert full.min() == 0 and full.max() == 255 and np.array_equal(full, R.resize_ref(imgs[1], (oh, ow)))
    # another mean / std and n_px: the table is the caller's
    got = ops.clip_preprocess(imgs[0], n_px=32, mean=(0.5, 0.5, 0.5), std=(0.5, 0.25, 2.0), device=False)
    assert np.array_equal(got[0], R.clip_preprocess_ref(imgs[0], 32, (0.5, 0.5, 0.5), (0.5, 0.25, 2.0)))


def test_the_workloads_shape_once(ops):
    """720 x 1080 frames to the 224 x 224 crop of 224 x 336: 13 taps per axis, B = 2 distinct frames"""
    H, W = R.WORKLOAD
    imgs = np.stack(R.make_images(2026, (H, W, 3)))
    assert int(ops.resize_coeffs(H, 224)[1][:, 1].max()) == 13 and int(ops.resize_coeffs(W, 336)[1][:, 1].max()) == 13
    want = np.stack([R.clip_preprocess_ref(a) for a in imgs])
    assert np.array_equal(ops.clip_preprocess(imgs, device=False), want)
    u8 = ops.resize_u8(ops.DeviceArray.from_numpy(imgs), (224, 336), window=(0, 56, 224, 224))
    assert np.array_equal(u8, np.stack([R.resize_ref(a, (224, 336), "bicubic", (0, 56, 224, 224)) for a in imgs]))


def write_scene(root, frames):
    from PIL import Image
    (root / "rgb").mkdir(parents=True)
    for i, a in enumerate(frames):
        Image.fromarray(a).save(root / "rgb" / f"{i:06d}.png")
    poses = np.zeros((len(frames), 7))
    poses[:, 0], poses[:, 6] = np.arange(len(frames)) * 0.25, 1.0
    np.savetxt(root / "poses.txt", poses)


def test_area_map_in_batches_end_to_end(ops, tmp_path):
    """Five 48 x 64 frames, batch_size 2 (a ragged last batch).  The stand-in encoder computes its means, its 48-term projection and
    its norm in float64 and rounds once to float32; the GPU's float64 sums differ from NumPy's in their order only, by at most
    3136 * 2^-53 relative per mean and far less than 2^-40 at the end, so the two float32 roundings of a component (|v| < 1, float32
    spacing at most 2^-24 there) either agree or are neighbours: |a - b| <= 2^-24, asserted as <= 2^-23 to leave the float64 slop
    out of the argument.  Measured nowhere: the bound is the format's."""
    from avlmaps_amd.apps.common import HashBatchImageEncoder
    from avlmaps_amd.map.area_map import AreaMap
    from avlmaps_amd.utils.clip_utils import ClipPreprocess, get_img_feats, get_imgs_feats_batch
    rng = np.random.default_rng(48)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in range(5)]
    write_scene(tmp_path, frames)
    enc = HashBatchImageEncoder()
    want = enc(np.stack([R.clip_preprocess_ref(a) for a in frames]))
    am = AreaMap()
    am.create_map(tmp_path, batch_encoder=enc, batch_size=2)
    assert am.clip_sparse_map.shape == (5, 768) and am.clip_sparse_map.dtype == np.float32
    assert np.abs(am.clip_sparse_map - want).max() <= 2.0 ** -23
    assert am.robot_pose_list.shape == (5, 4, 4) and am.robot_pose_list[3, 0, 3] != am.robot_pose_list[0, 0, 3]
    built = am.clip_sparse_map.copy()
    again = AreaMap()
    assert AreaMap.map_exists(tmp_path) and again.load_map(tmp_path)
    assert np.array_equal(again.clip_sparse_map, built) and np.array_equal(again.robot_pose_list, am.robot_pose_list)

    class Tower:                     # the stand-in behind CLIP's encode_image, for the upstream-shaped functions
        def encode_image(self, x):
            import torch
            return torch.from_numpy(enc(x)).to(x.device)
    pre = ClipPreprocess()
    feats = get_imgs_feats_batch(frames + [np.zeros((0, 5, 3), np.uint8)], pre, Tower(), 768, batch_size=4)
    assert feats.shape == (6, 768) and feats.dtype == np.float64
    assert np.abs(feats[:5] - want).max() <= 2.0 ** -22          # one more float32 rounding: the functions normalise again
    black = enc(R.clip_preprocess_ref(np.zeros((1, 1, 3), np.uint8))[None])
    assert np.abs(feats[5] - black[0]).max() <= 2.0 ** -22
    one = get_img_feats(frames[2], pre, Tower())
    assert one.shape == (1, 768) and one.dtype == np.float32 and np.abs(one[0] - want[2]).max() <= 2.0 ** -22
    p = pre(frames[0])
    assert tuple(p.shape) == (3, 224, 224) and np.array_equal(p.cpu().numpy(), R.clip_preprocess_ref(frames[0]))
