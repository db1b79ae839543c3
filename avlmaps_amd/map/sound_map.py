"""SoundMap with the reference's interface (avlmaps/map/sound_map.py:19-153).  The models are pluggable.  The audio-text model:
any object with encode_text(texts) -> (C, D) float32 text features and logit_scale_at (the log of the audio-text logit scale, a
float or a 0-d tensor) stands in for AudioCLIP; apps/common.HashAudioText is a model-free one.  The audio encoder (create_sound_map,
get_pos_with_audio): any callable audio_encoder(batch (B, 5 * sample_rate) float32) -> (B, D) float32;
apps/common.HashAudioEncoder is a model-free one.  Building the database (utils/audio_mapping_utils.create_audio_map_batch) decodes,
segments and packs the recordings on the GPU (csrc/avl_audio.hip); the sound track comes from a .wav next to the video or from an
installed ffmpeg.

The sound database (audio_video/audio_data_<difficulty>.pkl) maps a segment id to {"audio_features": (D,), "locations":
[(3,) habitat positions]}."""
from __future__ import annotations

import pickle
from pathlib import Path
from typing import List, Tuple

import numpy as np

from ..utils.audio_utils import get_level_categories


class SoundMap:
    def __init__(self, avlmaps_data_dir: str, sound_config, sound_data_collect_config, is_ambiguous: bool = False, is_real: bool = False,
                 audio_text_model=None, audio_encoder=None):
        self.avlmaps_data_dir = avlmaps_data_dir
        self.difficulty_level = sound_data_collect_config["difficulty"]
        self.sound_config = sound_config
        self.manual_str = "_manual" if is_ambiguous else ""
        self.is_real = is_real
        self.sound_categories = get_level_categories(self.difficulty_level, sound_config)
        self.sound_data_collect_config = sound_data_collect_config
        self.aclp = audio_text_model
        self.audio_encoder = audio_encoder
        self.audio_database = None
        self._dev = None

    def sound_map_path(self, data_dir) -> Path:
        """Reference: sound_map.py:74-78."""
        name = "audio_data.pkl" if self.is_real else f"audio_data{self.manual_str}_{self.difficulty_level}.pkl"
        return Path(data_dir) / "audio_video" / name

    def create_sound_map(self, data_dir: str, audio_encoder=None):
        """Builds audio_video/audio_data_<level>.pkl and the statistics file from the sequences under data_dir/audio_video, with the
        parameters of sound_data_collect_config (sample_rate, silence_duration_s, silence_threshold, fps, difficulty,
        considered_seq_num_per_scene).  Reference: sound_map.py:52-71.  Returns the database's path."""
        from ..utils.audio_mapping_utils import create_audio_map_batch, create_audio_map_statistics
        enc = audio_encoder if audio_encoder is not None else self.audio_encoder
        if enc is None:
            raise RuntimeError("SoundMap.create_sound_map: no audio encoder attached (audio_encoder=)")
        c = self.sound_data_collect_config
        data_dir = Path(data_dir).as_posix()
        path = create_audio_map_batch(data_dir, enc, sample_rate=c["sample_rate"], silence_duration_s=c["silence_duration_s"],
                                      silence_thres=c["silence_threshold"], fps=c["fps"], difficulty_level=c["difficulty"],
                                      manual_mode=False, seq_num=c["considered_seq_num_per_scene"])
        create_audio_map_statistics(data_dir, difficulty_level=c["difficulty"], manual_mode=False,
                                    seq_num=c["considered_seq_num_per_scene"])
        return path

    def load_sound_map(self, data_dir: str):
        """Reference: sound_map.py:73-84."""
        with open(self.sound_map_path(data_dir), "rb") as f:
            self.audio_database = pickle.load(f)
        self._dev = None
        return self.audio_database

    def get_all_audio_features_and_locations(self) -> Tuple[np.ndarray, List[List[np.ndarray]]]:
        """(S, D) stacked features and the per-segment location lists, ids 0 .. S-1 in order.  Reference: sound_map.py:86-97."""
        feats, locs = [], []
        for i in range(len(self.audio_database.keys())):
            feats.append(self.audio_database[i]["audio_features"])
            locs.append(self.audio_database[i]["locations"])
        return np.stack(feats, axis=0), locs

    def logit_scale(self) -> np.float32:
        """clamp(exp(logit_scale_at), 1, 100) in float32 (sound_map.py:142)"""
        s = self.aclp.logit_scale_at
        s = float(s.detach().cpu().item()) if hasattr(s, "detach") else float(s)
        return np.float32(np.clip(np.exp(np.float32(s)), np.float32(1.0), np.float32(100.0)))

    def _device_features(self, scale):
        """(scale * A) in float32 (the first product of `scale * audio_features @ text_features.T`) in HBM, kept per database
        and scale"""
        from ..device import DeviceArray
        db = self.audio_database
        if self._dev is None or self._dev[0] is not db or self._dev[1] != scale:
            a, _ = self.get_all_audio_features_and_locations()
            self._dev = (db, scale, DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32) * scale, dtype=np.float32)))
        return self._dev[2]

    def get_distribution_and_locations(self, name: str) -> Tuple[np.ndarray, List[np.ndarray]]:
        """(S,) float32 min-max normalised probabilities of category `name` over the segments, and the segments' locations.
        Reference: sound_map.py:135-153 (logits on the GPU through the similarity kernel).
        Departures: the category lookup is utils/index_utils.find_similar_category_id (KeyError when nothing matches) instead of
        upstream's LLM matcher; a constant column (max == min, NaN upstream) raises ValueError."""
        from .. import ops
        from ..utils.index_utils import find_similar_category_id
        if self.aclp is None:
            raise RuntimeError("SoundMap: no audio-text model attached (audio_text_model=)")
        cat_id = find_similar_category_id(name, self.sound_categories)
        _, locations = self.get_all_audio_features_and_locations()
        scale = self.logit_scale()
        text = np.ascontiguousarray(self.aclp.encode_text(list(self.sound_categories)), dtype=np.float32)
        sc, _, _ = ops.sim_scores(self._device_features(scale), text, want_scores=True, want_argmax=False, precision="exact")
        p = sc.numpy()[:, cat_id]
        lo, hi = np.min(p), np.max(p)
        if not hi > lo:
            raise ValueError(f"sound {name!r}: every segment has the same probability, the min-max normalisation is undefined")
        return (p - lo) / (hi - lo), locations

    def get_pos(self, name: str) -> List[np.ndarray]:
        """The locations of the segment with the largest logit for category `name` (the first among equals, np.argmax).
        Reference: sound_map.py:102-120; the logits are the similarity kernel's, the argmax over the small (S, C) table is host
        code.  The category lookup departs as in get_distribution_and_locations."""
        from .. import ops
        from ..utils.index_utils import find_similar_category_id
        if self.aclp is None:
            raise RuntimeError("SoundMap: no audio-text model attached (audio_text_model=)")
        cat_id = find_similar_category_id(name, self.sound_categories)
        _, locations = self.get_all_audio_features_and_locations()
        text = np.ascontiguousarray(self.aclp.encode_text(list(self.sound_categories)), dtype=np.float32)
        sc, _, _ = ops.sim_scores(self._device_features(self.logit_scale()), text, want_scores=True, want_argmax=False,
                                  precision="exact")
        return locations[int(np.argmax(sc.numpy(), axis=0)[cat_id])]

    def get_pos_with_audio(self, audio_path: str, sample_rate: int, audio_encoder=None):
        """The locations of the segment whose feature is most similar to the recording at audio_path (its first five seconds,
        scaled by 32768, through the audio encoder).  Reference: sound_map.py:122-133; a missing path returns ([], []) like
        upstream; a clip recorded at another rate is resampled to sample_rate, as upstream's librosa.load does.  Load, pack and
        encode, then ops.retrieve_frame."""
        import os
        from .. import ops
        from ..utils.audio_mapping_utils import TRACK_SCALE
        from ..utils.audio_utils import encode_audio_batch, load_wav
        if not os.path.exists(audio_path):
            return [], []
        enc = audio_encoder if audio_encoder is not None else self.audio_encoder
        if enc is None:
            raise RuntimeError("SoundMap.get_pos_with_audio: no audio encoder attached (audio_encoder=)")
        audio = load_wav(audio_path, sample_rate, device=True, resample=True)
        q = encode_audio_batch([(0, audio.shape[0])], enc, sample_rate, audio=audio, scale=TRACK_SCALE)
        feats, locations = self.get_all_audio_features_and_locations()
        idx, _ = ops.retrieve_frame(np.ascontiguousarray(feats, dtype=np.float32), q[0])
        return locations[idx]
