"""AreaMap with the reference's interface (avlmaps/map/area_map.py:19-119): one image embedding per frame (the "sparse" CLIP map)
and the pose it was taken from.  Scoring a text query against the F frame embeddings runs through the similarity kernel
(ops.sim_scores, float32-exact form) on a device copy kept per loaded map.

The image encoder and the text tower are pluggable: upstream both are CLIP ViT-L/14 (768-d); `image_encoder(rgb) -> (768,)`
and any object with encode_text (+ tokenize, as utils/clip_utils.get_text_feats expects) can stand in."""
from __future__ import annotations

from pathlib import Path
from typing import Callable, List, Optional, Union

import numpy as np

from ..utils.mapping_utils import cvt_pose_vec2tf, load_rgb_png, map_file_exists, read_map_datasets, write_map_datasets

AREA_MAP_FILE = Path("area_map") / "clip_sparse_map.h5df"


class AreaMap:
    def __init__(self, data_dir: str = "", clip_model=None, clip_feat_dim: int = 768) -> None:
        self.clip_sparse_map = None
        self.robot_pose_list = None
        self.categories = None
        self.scores_mat = None
        self.clip_feat_dim = clip_feat_dim
        if clip_model is not None:
            self.clip_model = clip_model
        self._dev = None
        if data_dir:
            self._setup_paths(data_dir)

    def _init_clip(self, clip_version: str = "ViT-L/14"):
        """Reference: area_map.py:27-51 (OpenAI CLIP on PyTorch-ROCm)."""
        if hasattr(self, "clip_model"):
            return
        import clip
        import torch
        from .vlmap import CLIP_FEAT_DIM
        self.clip_version = clip_version
        self.clip_feat_dim = CLIP_FEAT_DIM[clip_version]
        self.clip_model, self.preprocess = clip.load(clip_version)
        self.clip_model.to("cuda" if torch.cuda.is_available() else "cpu").eval()

    def _setup_paths(self, data_dir: Union[Path, str]) -> None:
        self.data_dir = Path(data_dir)
        self.rgb_dir = self.data_dir / "rgb"
        self.pose_path = self.data_dir / "poses.txt"
        self.map_save_dir = self.data_dir / "area_map"
        self.rgb_paths = sorted(self.rgb_dir.glob("*.png"))

    @staticmethod
    def map_exists(data_dir) -> bool:
        return map_file_exists(Path(data_dir) / AREA_MAP_FILE)

    def create_map(self, data_dir: Union[Path, str], image_encoder: Optional[Callable[[np.ndarray], np.ndarray]] = None) -> None:
        """One embedding per frame of rgb/*.png and its habitat pose from poses.txt.  Reference: area_map.py:66-98.
        image_encoder(rgb uint8 (H, W, 3)) -> (clip_feat_dim,) L2-normalised; None = CLIP ViT-L/14 (get_img_feats)."""
        self._setup_paths(data_dir)
        if image_encoder is None:
            image_encoder = self._clip_image_encoder()
        base_poses = np.loadtxt(self.pose_path).reshape(-1, 7)
        n = len(self.rgb_paths)
        sparse = np.zeros((n, self.clip_feat_dim), dtype=np.float32)
        poses = []
        for i, (rgb_path, pose) in enumerate(zip(self.rgb_paths, base_poses)):
            sparse[i] = np.asarray(image_encoder(load_rgb_png(rgb_path)), dtype=np.float32).reshape(-1)
            poses.append(cvt_pose_vec2tf(pose))
        self.map_save_dir.mkdir(parents=True, exist_ok=True)
        write_map_datasets(self.data_dir / AREA_MAP_FILE, {"clip_sparse_map": sparse, "robot_pose_list": np.asarray(poses, np.float64)})
        self._set(sparse, np.asarray(poses, np.float64))

    def _clip_image_encoder(self):
        import torch
        from PIL import Image
        self._init_clip()

        def enc(rgb):
            with torch.no_grad():
                f = self.clip_model.encode_image(self.preprocess(Image.fromarray(np.uint8(rgb)))[None].cuda()).float()
            f /= f.norm(dim=-1, keepdim=True)
            return f.cpu().numpy().astype(np.float32)
        return enc

    def load_map(self, data_dir: Union[Path, str]) -> bool:
        """Reads area_map/clip_sparse_map.h5df (datasets clip_sparse_map, robot_pose_list).  Reference: area_map.py:100-103."""
        self._setup_paths(data_dir)
        path = self.data_dir / AREA_MAP_FILE
        if not map_file_exists(path):
            return False
        d = read_map_datasets(path)
        self._set(np.asarray(d["clip_sparse_map"], dtype=np.float32), np.asarray(d["robot_pose_list"], dtype=np.float64))
        return True

    def _set(self, sparse, poses):
        self.clip_sparse_map, self.robot_pose_list = sparse, poses
        self.scores_mat = self.categories = None
        self._dev = None

    def _device_map(self):
        """the (F, D) sparse map in HBM, uploaded once per loaded map"""
        from ..device import DeviceArray
        if self._dev is None or self._dev[0] is not self.clip_sparse_map:
            self._dev = (self.clip_sparse_map, DeviceArray.from_numpy(np.ascontiguousarray(self.clip_sparse_map, dtype=np.float32)))
        return self._dev[1]

    def _text_feats(self, texts: List[str]) -> np.ndarray:
        from ..utils.clip_utils import get_text_feats
        self._init_clip()
        return get_text_feats(texts, self.clip_model, self.clip_feat_dim)

    def _scores(self, q: np.ndarray) -> np.ndarray:
        """clip_sparse_map @ q.T, (F, Q) float32 on the GPU"""
        from .. import ops
        if self.clip_sparse_map is None:
            raise RuntimeError("AreaMap: no map loaded (load_map / create_map)")
        if len(self.clip_sparse_map) == 0:
            return np.zeros((0, len(q)), np.float32)
        sc, _, _ = ops.sim_scores(self._device_map(), np.ascontiguousarray(q, dtype=np.float32), want_scores=True, want_argmax=False,
                                  precision="exact")
        return sc.numpy()

    def init_categories(self, categories: List[str]) -> np.ndarray:
        """scores_mat (F, C) float32.  Reference: area_map.py:105-109."""
        self.categories = categories
        self.scores_mat = self._scores(self._text_feats(list(categories)))
        return self.scores_mat

    def index_map(self, language_desc: str, with_init_cat: bool = True) -> np.ndarray:
        """(F,) float32 frame scores of a text query.  Reference: area_map.py:111-126.
        Departure: the category lookup of with_init_cat is utils/index_utils.find_similar_category_id (exact, then
        case-insensitive / unique-substring match; KeyError otherwise) instead of upstream's LLM matcher."""
        if with_init_cat and self.scores_mat is not None and self.categories is not None:
            from ..utils.index_utils import find_similar_category_id
            return self.scores_mat[:, find_similar_category_id(language_desc, self.categories)].flatten()
        if with_init_cat:
            raise Exception("Categories are not preloaded. Call init_categories(categories: List[str]) to initialize categories.")
        return self._scores(self._text_feats([language_desc])).flatten()
