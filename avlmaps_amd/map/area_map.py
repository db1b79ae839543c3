"""AreaMap with the reference's interface (avlmaps/map/area_map.py:19-119): one image embedding per frame (the "sparse" CLIP map)
and the pose it was taken from.  Scoring a text query against the F frame embeddings runs through the similarity kernel
(ops.sim_scores, float32-exact form) on a device copy kept per loaded map.

The image encoder and the text tower are pluggable: upstream both are CLIP ViT-L/14 (768-d); `image_encoder(rgb) -> (768,)`,
`batch_encoder((B, 3, n_px, n_px) tensor) -> (B, 768)` on frames preprocessed by the GPU (ops.clip_preprocess), and any object
with encode_text (+ tokenize, as utils/clip_utils.get_text_feats expects) can stand in."""
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

    def create_map(self, data_dir: Union[Path, str], image_encoder: Optional[Callable[[np.ndarray], np.ndarray]] = None,
                   batch_encoder: Optional[Callable] = None, batch_size: int = 64) -> None:
        """One embedding per frame of rgb/*.png and its habitat pose from poses.txt.  Reference: area_map.py:66-98.
        image_encoder(rgb uint8 (H, W, 3)) -> (clip_feat_dim,) L2-normalised: the frames are encoded one at a time.
        batch_encoder((B, 3, n_px, n_px) float32 torch tensor on the GPU) -> (B, clip_feat_dim) L2-normalised rows (a tensor or an
        array): the frames are decoded on the host, preprocessed `batch_size` at a time by ops.clip_preprocess (CLIP's preprocess
        in one launch pair, n_px = batch_encoder.n_px or 224) and encoded as batches; all frames must have one size.
        Neither: CLIP ViT-L/14's image tower on such batches, the norm taken on the device."""
        self._setup_paths(data_dir)
        if image_encoder is not None and batch_encoder is not None:
            raise ValueError("AreaMap.create_map: give image_encoder or batch_encoder, not both")
        base_poses = np.loadtxt(self.pose_path).reshape(-1, 7)
        n = len(self.rgb_paths)
        sparse = np.zeros((n, self.clip_feat_dim), dtype=np.float32)
        poses = []
        if image_encoder is not None:
            for i, (rgb_path, pose) in enumerate(zip(self.rgb_paths, base_poses)):
                sparse[i] = np.asarray(image_encoder(load_rgb_png(rgb_path)), dtype=np.float32).reshape(-1)
                poses.append(cvt_pose_vec2tf(pose))
        else:
            m = min(n, len(base_poses))
            self._encode_batches(batch_encoder or self._clip_batch_encoder(), self.rgb_paths[:m], int(batch_size), sparse)
            poses = [cvt_pose_vec2tf(pose) for pose in base_poses[:m]]
        self.map_save_dir.mkdir(parents=True, exist_ok=True)
        write_map_datasets(self.data_dir / AREA_MAP_FILE, {"clip_sparse_map": sparse, "robot_pose_list": np.asarray(poses, np.float64)})
        self._set(sparse, np.asarray(poses, np.float64))

    @staticmethod
    def _encode_batches(batch_encoder, paths, batch_size, sparse) -> None:
        """sparse[i] = the embedding of paths[i].  PNG decoding stays on the host, on at most four threads, one batch ahead of the
        GPU; everything between the decoded bytes and the embedding runs on the device."""
        from concurrent.futures import ThreadPoolExecutor
        from .. import ops
        if batch_size < 1:
            raise ValueError(f"batch_size={batch_size} must be at least 1")
        n_px = int(getattr(batch_encoder, "n_px", 224))
        chunks = [paths[s:s + batch_size] for s in range(0, len(paths), batch_size)]
        with ThreadPoolExecutor(max_workers=4, thread_name_prefix="avl-png") as pool:
            ahead = [pool.submit(load_rgb_png, p) for p in chunks[0]] if chunks else []
            at = 0
            for ci, chunk in enumerate(chunks):
                frames = [f.result() for f in ahead]
                ahead = [pool.submit(load_rgb_png, p) for p in chunks[ci + 1]] if ci + 1 < len(chunks) else []
                if any(f.shape != frames[0].shape for f in frames):
                    raise ValueError(f"AreaMap.create_map: the frames {chunk[0].name} .. {chunk[-1].name} differ in size; the batched "
                                     "path needs one size (image_encoder= takes them one at a time)")
                feats = batch_encoder(ops.clip_preprocess(np.stack(frames), n_px=n_px, as_torch=True))
                feats = feats.detach().float().cpu().numpy() if hasattr(feats, "detach") else np.asarray(feats)
                sparse[at:at + len(chunk)] = feats.astype(np.float32).reshape(len(chunk), -1)
                at += len(chunk)

    def _clip_batch_encoder(self):
        import torch
        self._init_clip()

        def enc(x):
            with torch.no_grad():
                f = self.clip_model.encode_image(x).float()
            return f / f.norm(dim=-1, keepdim=True)
        enc.n_px = int(getattr(getattr(self.clip_model, "visual", None), "input_resolution", 224))
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
