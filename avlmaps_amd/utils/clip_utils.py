"""Text-query scoring with the interface of the reference's avlmaps/utils/clip_utils.py.

get_lseg_score keeps the reference's semantics (clip_utils.py:196-242): optional "other" column, 63 prompt
templates averaged WITHOUT re-normalisation, raw dot product -- but the (N x D) . (D x Q) contraction runs in
the HIP similarity kernel instead of NumPy/OpenBLAS.  CLIP itself stays on PyTorch-ROCm.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np


def _build_templates() -> List[str]:
    """The 63 prompt templates of clip_utils.py:10-74 (CLIP's prompt-engineering set as used by VLMaps),
    same order, including the upstream 'picture of of' typo (the text encoder sees exactly these strings)."""
    t = ["There is {} in the scene.", "There is the {} in the scene.", "a photo of {} in the scene.",
         "a photo of the {} in the scene.", "a photo of one {} in the scene."]
    t += [f"I took a picture of of {x}{{}}." for x in ("", "my ", "the ")]
    t += [f"a photo of {x}{{}}." for x in ("", "my ", "the ", "one ", "many ")]
    for adj in ("good", "bad"):
        t += [f"a {adj} photo of {{}}.", f"a {adj} photo of the {{}}."]
    for adj in ("nice", "cool", "weird", "small", "large", "clean", "dirty"):
        t += [f"a photo of a {adj} {{}}.", f"a photo of the {adj} {{}}."]
    for adj in ("bright", "dark"):
        t += [f"a {adj} photo of {{}}.", f"a {adj} photo of the {{}}."]
    t += ["a photo of a hard to see {}.", "a photo of the hard to see {}."]
    for adj in ("low resolution", "cropped", "close-up", "jpeg corrupted", "blurry", "pixelated"):
        t += [f"a {adj} photo of {{}}.", f"a {adj} photo of the {{}}."]
    t += ["a black and white photo of the {}.", "a black and white photo of {}."]
    for noun in ("plastic", "toy", "plushie", "cartoon"):
        t += [f"a {noun} {{}}.", f"the {noun} {{}}."]
    t += ["an embroidered {}.", "the embroidered {}.", "a painting of the {}.", "a painting of a {}."]
    assert len(t) == 63
    return t


multiple_templates = _build_templates()


class ClipPreprocess:
    """CLIP's `preprocess` (clip.load(...)[1], _transform(n_px)) on the GPU: a callable that takes a PIL image, an (H, W, 3) uint8
    array or a (B, H, W, 3) batch of equally sized frames (host or device) and returns the normalised (3, n_px, n_px) float32 torch
    tensor on the GPU, (B, 3, n_px, n_px) for a batch -- ops.clip_preprocess, Pillow's bicubic resize bit for bit.  Passed as
    `preprocess` to get_img_feats / get_imgs_feats_batch it makes them preprocess a whole batch in one call."""

    def __init__(self, n_px: int = 224, mean=None, std=None):
        from ..ops.resize import CLIP_MEAN, CLIP_STD
        self.n_px = int(n_px)
        self.mean, self.std = tuple(mean or CLIP_MEAN), tuple(std or CLIP_STD)

    def batch(self, images):
        """(B, H, W, 3) uint8 frames -> (B, 3, n_px, n_px) float32 torch tensor on the GPU"""
        from .. import ops
        return ops.clip_preprocess(images, n_px=self.n_px, mean=self.mean, std=self.std, as_torch=True)

    def __call__(self, img):
        if not hasattr(img, "shape"):
            img = np.asarray(img.convert("RGB") if hasattr(img, "convert") else img, dtype=np.uint8)
        out = self.batch(img)
        return out if len(img.shape) == 4 else out[0]


def _image_or_black(img):
    """upstream's guard (clip_utils.py:117-118): an image without rows or columns becomes one black pixel"""
    img = np.asarray(img)
    if img.ndim < 2 or img.shape[0] == 0 or img.shape[1] == 0:
        img = np.zeros((1, 1, 3), np.uint8)
    return np.uint8(img)


def _encode_images(img_in, clip_model) -> np.ndarray:
    import torch
    with torch.no_grad():
        f = clip_model.encode_image(img_in.cuda()).float()
    f /= f.norm(dim=-1, keepdim=True)
    return np.float32(f.cpu())


def get_img_feats(img, preprocess, clip_model) -> np.ndarray:
    """(1, D) float32, L2-normalised.  Reference: clip_utils.py:96-103."""
    if isinstance(preprocess, ClipPreprocess):
        return _encode_images(preprocess(np.uint8(img))[None, ...], clip_model)
    from PIL import Image
    return _encode_images(preprocess(Image.fromarray(np.uint8(img)))[None, ...], clip_model)


def get_imgs_feats(raw_imgs, preprocess, clip_model, clip_feat_dim) -> np.ndarray:
    """(len(raw_imgs), clip_feat_dim) float64, one image at a time.  Reference: clip_utils.py:106-110."""
    imgs_feats = np.zeros((len(raw_imgs), clip_feat_dim))
    for img_id, img in enumerate(raw_imgs):
        imgs_feats[img_id, :] = get_img_feats(img, preprocess, clip_model)
    return imgs_feats


def get_imgs_feats_batch(raw_imgs, preprocess, clip_model, clip_feat_dim, batch_size=64) -> np.ndarray:
    """(len(raw_imgs), clip_feat_dim) float64, encoded batch_size images at a time.  Reference: clip_utils.py:113-130.
    With a ClipPreprocess, consecutive images of one size are preprocessed in ONE launch pair (images of another size start a new
    group inside the batch) and the batch is encoded in one call; any other `preprocess` is applied per image on the host, as
    upstream does.  An empty image counts as one black pixel."""
    import torch
    imgs_feats = np.zeros((len(raw_imgs), clip_feat_dim))
    gpu = isinstance(preprocess, ClipPreprocess)
    if not gpu:
        from PIL import Image
    for start in range(0, len(raw_imgs), batch_size):
        imgs = [_image_or_black(img) for img in raw_imgs[start:start + batch_size]]
        if gpu:
            parts, i = [], 0
            while i < len(imgs):
                j = i + 1
                while j < len(imgs) and imgs[j].shape == imgs[i].shape:
                    j += 1
                parts.append(preprocess.batch(np.stack(imgs[i:j])))
                i = j
        else:
            parts = [preprocess(Image.fromarray(img))[None, ...] for img in imgs]
        imgs_feats[start:start + len(imgs), :] = _encode_images(torch.cat(parts, dim=0), clip_model)
    return imgs_feats


def get_text_feats(in_text: Sequence[str], clip_model, clip_feat_dim: int, batch_size: int = 64) -> np.ndarray:
    """CLIP text embeddings, each row L2-normalised, float32 (len(in_text), clip_feat_dim).
    Reference: clip_utils.py:133-149.  `clip_model` is an OpenAI-CLIP style model (encode_text); the tokenizer is
    clip.tokenize, or clip_model.tokenize when the model object carries its own."""
    import torch
    tokenize = getattr(clip_model, "tokenize", None)
    if tokenize is None:
        import clip  # OpenAI CLIP (pip git+https://github.com/openai/CLIP.git), as upstream
        tokenize = clip.tokenize
    device = "cuda" if torch.cuda.is_available() else "cpu"
    tokens = tokenize(list(in_text)).to(device)
    feats = np.zeros((len(in_text), clip_feat_dim), dtype=np.float32)
    i = 0
    while i < len(tokens):
        bs = min(len(in_text) - i, batch_size)
        with torch.no_grad():
            b = clip_model.encode_text(tokens[i:i + bs]).float()
        b /= b.norm(dim=-1, keepdim=True)
        feats[i:i + bs] = b.cpu().numpy().astype(np.float32)
        i += bs
    return feats


def get_text_feats_multiple_templates(in_text, clip_model, clip_feat_dim, batch_size=64) -> np.ndarray:
    """Reference: clip_utils.py:152-160."""
    prompts = [t.format(lm) for lm in in_text for t in multiple_templates]
    f = get_text_feats(prompts, clip_model, clip_feat_dim)
    return np.mean(f.reshape((-1, len(multiple_templates), f.shape[-1])), axis=1)


def landmark_text_feats(clip_model, landmarks: list, clip_feat_dim: int, use_multiple_templates=False, add_other=True):
    """(Q, D) query matrix + the landmark list actually scored (clip_utils.py:213-225)."""
    landmarks_other = landmarks
    if add_other and landmarks_other[-1] != "other":
        landmarks_other = landmarks + ["other"]
    if use_multiple_templates:
        prompts = [t.format(lm) for lm in landmarks_other for t in multiple_templates]
        f = get_text_feats(prompts, clip_model, clip_feat_dim)
        f = np.mean(f.reshape((-1, len(multiple_templates), f.shape[-1])), axis=1)
    else:
        f = get_text_feats(landmarks_other, clip_model, clip_feat_dim)
    return np.ascontiguousarray(f, dtype=np.float32), landmarks_other


def get_lseg_score(clip_model, landmarks: list, lseg_map, clip_feat_dim: int, use_multiple_templates: bool = False,
                   avg_mode: int = 0, add_other=True, precision: str = "auto"):
    """scores (N, Q) float32 = map_feats @ text_feats.T.  Reference: clip_utils.py:196-242.

    lseg_map: (h, w, D) / (N, D) numpy array, or a device-resident (N, D) array (torch CUDA tensor /
    avlmaps_amd.device.DeviceArray) to skip the upload.  avg_mode=1 (average scores instead of features)
    scores every template separately and averages on the host, as upstream."""
    from .. import ops
    landmarks_other = landmarks
    if add_other and landmarks_other[-1] != "other":
        landmarks_other = landmarks + ["other"]
    if isinstance(lseg_map, np.ndarray):
        lseg_map = np.ascontiguousarray(lseg_map.reshape((-1, lseg_map.shape[-1])), dtype=np.float32)
    if use_multiple_templates and avg_mode == 1:
        prompts = [t.format(lm) for lm in landmarks_other for t in multiple_templates]
        f = get_text_feats(prompts, clip_model, clip_feat_dim)
        sc, _, _ = ops.sim_scores(lseg_map, f, want_argmax=False, precision=precision)
        sc = _to_numpy(sc)
        return np.mean(sc.reshape((-1, len(landmarks_other), len(multiple_templates))), axis=2)
    f, _ = landmark_text_feats(clip_model, landmarks, clip_feat_dim, use_multiple_templates, add_other)
    sc, _, _ = ops.sim_scores(lseg_map, f, want_argmax=False, precision=precision)
    return _to_numpy(sc)


def _to_numpy(x):
    if isinstance(x, np.ndarray):
        return x
    if hasattr(x, "numpy") and not hasattr(x, "cpu"):
        return x.numpy()
    return x.cpu().numpy()
