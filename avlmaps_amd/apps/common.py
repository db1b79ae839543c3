"""Config + stand-in models shared by the CLI apps.

The reference drives its apps with hydra (config/map_creation_cfg.yaml, config/map_indexing_cfg.yaml); here a plain YAML
file (or the built-in defaults below, = config/map_config/vlmaps.yaml + config/params/default.yaml) is enough."""
from __future__ import annotations

import hashlib
from pathlib import Path

import numpy as np

DEFAULTS = {
    "params": {"gs": 1000, "cs": 0.05, "camera_height": 1.5},
    "map_config": {
        "map_type": "vlmap",
        "pose_info": {"pose_type": "mobile_base", "camera_height": 1.5, "base2cam_rot": [1, 0, 0, 0, -1, 0, 0, 0, -1],
                      "base_forward_axis": [0, 0, -1], "base_left_axis": [-1, 0, 0], "base_up_axis": [0, 1, 0]},
        "cam_calib_mat": [540, 0, 540, 0, 540, 360, 0, 0, 1], "grid_size": 1000, "cell_size": 0.05,
        "depth_sample_rate": 100, "dilate_iter": 3, "gaussian_sigma": 1.0,
        "potential_obstacle_names": ["chair", "wall", "wall above the door", "table", "window", "floor", "stairs", "other"],
        "obstacle_names": ["wall", "chair", "table", "window", "stairs", "other"],
    },
    # the sound queries' categories (ESC-50 classes by major category; utils/audio_utils.get_level_categories)
    # (the values of upstream's config/sound_data_collect_params/sound_collect_default.yaml that the sound map reads)
    "sound_data_collect_params": {"difficulty": "level_3", "fps": 25, "sample_rate": 44100, "silence_duration_s": 1,
                                  "silence_threshold": 0, "considered_seq_num_per_scene": 20},
    "sound_config": {
        "difficulty": {
            "level_1": ["Interior/domestic sounds"],
            "level_2": ["Interior/domestic sounds", "Human, non-speech sounds"],
            "level_3": ["Interior/domestic sounds", "Human, non-speech sounds", "Animals"],
            "level_4": ["Interior/domestic sounds", "Human, non-speech sounds", "Animals", "Natural soundscapes"],
            "level_5": ["Interior/domestic sounds", "Human, non-speech sounds", "Animals", "Natural soundscapes",
                        "Exterior/urban noises"],
        },
        "major_categories": {
            "Animals": ["dog", "rooster", "pig", "cow", "frog", "cat", "hen", "insects", "sheep", "crow"],
            "Natural soundscapes": ["rain", "sea_waves", "crackling_fire", "crickets", "chirping_birds", "water_drops", "wind",
                                    "pouring_water", "toilet_flush", "thunderstorm"],
            "Human, non-speech sounds": ["crying_baby", "sneezing", "clapping", "breathing", "coughing", "footsteps", "laughing",
                                         "brushing_teeth", "snoring", "drinking_sipping"],
            "Interior/domestic sounds": ["door_wood_knock", "mouse_click", "keyboard_typing", "door_wood_creaks", "can_opening",
                                         "washing_machine", "vacuum_cleaner", "clock_alarm", "clock_tick", "glass_breaking"],
            "Exterior/urban noises": ["helicopter", "chainsaw", "siren", "car_horn", "engine", "train", "church_bells", "airplane",
                                      "fireworks", "hand_saw"],
        },
    },
}


class Cfg(dict):
    """attribute + item access, nested (stand-in for omegaconf.DictConfig)"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def to_cfg(d):
    return Cfg({k: to_cfg(v) for k, v in d.items()}) if isinstance(d, dict) else d


def load_config(path=None, overrides=None):
    import copy
    cfg = copy.deepcopy(DEFAULTS)
    if path:
        import yaml
        user = yaml.safe_load(Path(path).read_text()) or {}
        for k, v in user.items():
            if isinstance(v, dict) and isinstance(cfg.get(k), dict):
                _deep_update(cfg[k], v)
            else:
                cfg[k] = v
    for k, v in (overrides or {}).items():
        node = cfg
        parts = k.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = v
    cfg["map_config"]["grid_size"] = cfg["map_config"].get("grid_size", cfg["params"]["gs"])
    cfg["map_config"]["cell_size"] = cfg["map_config"].get("cell_size", cfg["params"]["cs"])
    return to_cfg(cfg)


def _deep_update(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _deep_update(dst[k], v)
        else:
            dst[k] = v


def read_categories_file(path):
    """class names, one per line (blank lines dropped); the line number is the class id"""
    return [line.strip() for line in Path(path).read_text().splitlines() if line.strip()]


class HashFeatureExtractor:
    """Stand-in for LSeg when no checkpoint is available (demo / smoke runs): a fixed random projection of a small
    colour + position code to D channels, normalised to the LSeg logit scale, computed on the GPU, channels-last."""

    def __init__(self, D=512, scale=8, seed=0):
        import torch
        self.D, self.scale = D, scale
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.proj = torch.randn((5, D), device="cuda", generator=g)

    def __call__(self, rgb):
        import torch
        t = torch.from_numpy(np.array(rgb, copy=True)).cuda().float().div_(255.0)
        H, W, _ = t.shape
        t = t[:: self.scale // 4 or 1, :: self.scale // 4 or 1][: max(1, H // 2), : max(1, W // 2)]
        h, w, _ = t.shape
        yy = torch.linspace(0, 1, h, device="cuda").view(h, 1, 1).expand(h, w, 1)
        xx = torch.linspace(0, 1, w, device="cuda").view(1, w, 1).expand(h, w, 1)
        f = torch.cat([t, yy, xx], dim=2) @ self.proj
        f = f / f.norm(dim=2, keepdim=True) * 14.2857
        return f.half().float().contiguous()


class HashClip:
    """Stand-in for CLIP's text tower (demo / smoke runs): deterministic unit vectors derived from the prompt text."""

    def __init__(self, D=512):
        self.D = D
        self._texts = []

    def tokenize(self, texts):
        import torch
        base = len(self._texts)
        self._texts.extend(texts)
        return torch.arange(base, base + len(texts), dtype=torch.int64)

    def encode_text(self, ids):
        import torch
        rows = []
        for i in ids.cpu().tolist():
            seed = int.from_bytes(hashlib.sha256(self._texts[i].encode()).digest()[:8], "little")
            rows.append(np.random.default_rng(seed).standard_normal(self.D).astype(np.float32))
        return torch.from_numpy(np.stack(rows)).to(ids.device)


def _hash_unit(text: str, D: int) -> np.ndarray:
    seed = int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")
    v = np.random.default_rng(seed).standard_normal(D).astype(np.float32)
    return v / np.linalg.norm(v)


class HashImageEncoder:
    """Stand-in for CLIP ViT-L/14's image tower of the area map (demo / smoke runs): a fixed random projection of the image's
    4 x 4 grid of mean colours to D = 768 channels, L2-normalised, float32."""

    def __init__(self, D=768, seed=0):
        self.D = D
        self.proj = np.random.default_rng(seed).standard_normal((48, D)).astype(np.float32)

    def __call__(self, rgb):
        a = np.asarray(rgb, dtype=np.float32) / 255.0
        H, W = a.shape[:2]
        code = np.array([a[i * H // 4:(i + 1) * H // 4 or None, j * W // 4:(j + 1) * W // 4 or None].reshape(-1, 3).mean(0)
                         for i in range(4) for j in range(4)], dtype=np.float32).reshape(-1) - 0.5
        f = code @ self.proj
        return (f / np.linalg.norm(f)).astype(np.float32)


class HashBatchImageEncoder:
    """Stand-in for CLIP ViT-L/14's image tower on PREPROCESSED batches (AreaMap.create_map(batch_encoder=...), demo / smoke runs):
    the 4 x 4 grid of means of each of the 3 planes of a (B, 3, n_px, n_px) tensor (48 numbers, plane-major), through a fixed seeded
    projection to D = 768 channels, L2-normalised.  Means, projection and norm are float64 on the device the batch lives on (a
    torch tensor stays where it is; an array is taken on the host), so that the float32 rows it returns, a host array (B, D), do not
    depend on the device beyond their last bit."""

    def __init__(self, D=768, seed=0, n_px=224):
        self.D, self.n_px = D, n_px
        self.proj = np.random.default_rng(seed).standard_normal((48, D))

    def __call__(self, batch):
        import torch
        t = batch if isinstance(batch, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(batch.numpy() if hasattr(batch, "ptr") else batch))
        t = t.double()
        B, _, h, w = t.shape
        code = torch.stack([t[:, c, i * h // 4:(i + 1) * h // 4, j * w // 4:(j + 1) * w // 4].mean(dim=(1, 2))
                            for c in range(3) for i in range(4) for j in range(4)], dim=1)
        f = code @ torch.from_numpy(self.proj).to(t.device)
        f = f / f.norm(dim=1, keepdim=True)
        return f.float().cpu().numpy()


class HashAudioText:
    """Stand-in for AudioCLIP's text side (demo / smoke runs): deterministic 1024-d unit vectors per category name and a fixed
    logit scale (log 100 -> the clamp's upper end)."""

    def __init__(self, D=1024):
        self.D = D
        self.logit_scale_at = float(np.log(100.0))

    def encode_text(self, texts):
        return np.stack([_hash_unit(t, self.D) for t in texts]) if len(texts) else np.zeros((0, self.D), np.float32)


class HashAudioEncoder:
    """Stand-in for AudioCLIP's audio head (demo / smoke runs): a D-d unit vector per row of a (B, L) float32 batch, deterministic
    from the row's bytes, so equal five-second contexts get equal features and different ones are nearly orthogonal."""

    def __init__(self, D=1024):
        self.D = D

    def __call__(self, batch):
        b = np.ascontiguousarray(batch, dtype=np.float32)
        b = b.reshape(1, -1) if b.ndim == 1 else b
        rows = []
        for row in b:
            seed = int.from_bytes(hashlib.sha256(row.tobytes()).digest()[:8], "little")
            v = np.random.default_rng(seed).standard_normal(self.D).astype(np.float32)
            rows.append(v / np.linalg.norm(v))
        return np.stack(rows) if rows else np.zeros((0, self.D), np.float32)


class FixedPoseLocalizer:
    """Stand-in for HLoc (demo / smoke runs): every query image is 'localised' at one fixed base pose, given as a habitat
    (px, py, pz, qx, qy, qz, qw) vector (a row of poses.txt).  Returns (camera tf, base tf) like VisualMap.localize_image."""

    def __init__(self, pose_vec, base2cam_tf):
        from ..utils.mapping_utils import cvt_pose_vec2tf
        self.base_tf = cvt_pose_vec2tf(np.asarray(pose_vec, dtype=np.float64))
        self.base2cam_tf = np.asarray(base2cam_tf, dtype=np.float64)

    def __call__(self, img, query_cam_intrinsic_mat=None):
        return self.base_tf @ self.base2cam_tf, self.base_tf
