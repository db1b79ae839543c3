"""Builds the sound database of a scene with the reference's file layout (avlmaps/utils/audio_mapping_utils.py:26-152).

    <data_dir>/audio_video/<seq>/range_and_audio<manual>_meta_<level>.txt     one line per placed sound; a sequence without it is skipped
    <data_dir>/audio_video/<seq>/output_with_audio<manual>_<level>.mp4        the sequence's video with its sound track
    <data_dir>/audio_video/<seq>/output_with_audio<manual>_<level>.wav        the sound track, read when it exists (see find_audio)
    <data_dir>/audio_video/<seq>/poses.txt                                    one habitat pose (x y z qx qy qz qw) per video frame
    <data_dir>/audio_video/audio_data<manual>_<level>.pkl                     the result: {id: {"audio_features", "locations"}}
    <data_dir>/audio_video/audio_map_statistics<manual>_<level>.pkl           the last two fields of every meta line

Per sequence the recording is uploaded once; decoding, resampling to the configured rate (a .wav at any rate and PCM width:
csrc/avl_resample.hip), segmentation and the encoder's zero-padded batch run on the GPU (csrc/avl_audio.hip), and only the (B, 5 * sample_rate) batches come back for the encoder."""
from __future__ import annotations

import os
import pickle
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from .audio_utils import (convert_time_ranges_to_frame_ranges, create_audio_dictionary, encode_audio_batch, load_wav,
                          setup_audio_paths)

TRACK_SCALE = 32768.0       # audio_mapping_utils.py:85: the encoder is fed int16-range amplitudes


def sound_file_names(difficulty_level: str, manual_mode: bool = False):
    """(meta file, video file, database file, statistics file) names of a difficulty level"""
    m = "_manual" if manual_mode else ""
    return (f"range_and_audio{m}_meta_{difficulty_level}.txt", f"output_with_audio{m}_{difficulty_level}.mp4",
            f"audio_data{m}_{difficulty_level}.pkl", f"audio_map_statistics{m}_{difficulty_level}.pkl")


def find_audio(video_path, sample_rate, tmp_dir):
    """The path of a WAV file with the sound track of `video_path`: the .wav with the video's stem when it exists, else extracted
    with ffmpeg into tmp_dir (upstream: audio_utils.py:508-512, always ffmpeg into /tmp after an `rm` through the shell)."""
    video_path = Path(video_path)
    wav = video_path.with_suffix(".wav")
    if wav.exists():
        return wav
    ffmpeg = shutil.which("ffmpeg")
    if ffmpeg is None or not video_path.exists():
        raise FileNotFoundError(f"no sound track: neither {wav} exists nor can ffmpeg extract it from {video_path} "
                                f"({'ffmpeg is not on PATH' if ffmpeg is None else 'the video is missing'})")
    out = Path(tmp_dir) / (video_path.parent.name + "_" + video_path.stem + ".wav")
    r = subprocess.run([ffmpeg, "-y", "-i", str(video_path), "-vn", "-ar", str(int(sample_rate)), "-c:a", "pcm_s16le", str(out)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0 or not out.exists():
        raise RuntimeError(f"ffmpeg could not extract the sound track of {video_path}: {r.stderr[-500:]}")
    return out


def segment_locations(poses, frame_ranges):
    """[[(3,) position of every frame f0 <= f < f1] per segment]: poses[f0:f1, :3], which is cvt_pose_vec2tf(p)[:3, 3]
    (audio_mapping_utils.py:102-108)"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    return [[p[:3].copy() for p in poses[f0:f1]] for f0, f1 in frame_ranges]


def create_audio_map_batch(data_dir: str, audio_encoder, sample_rate: int = 44100, silence_duration_s: float = 1,
                           silence_thres: float = 0, fps: float = 20, difficulty_level: str = "level_1", manual_mode: bool = False,
                           seq_num: int = None, details: dict = None):
    """Reference: audio_mapping_utils.py:26-122.  audio_encoder(batch (B, 5 * sample_rate) float32) -> (B, D) replaces AudioCLIP and
    its transforms.  Returns the path of the database it wrote.  details (a dict, optional) receives per kept sequence its
    segments, time ranges and frame ranges."""
    from .. import ops
    if audio_encoder is None:
        raise ValueError("create_audio_map_batch needs an audio_encoder (AudioCLIP's audio head, or apps/common.HashAudioEncoder)")
    data_dir = str(data_dir)
    meta_name, video_name, db_name, _ = sound_file_names(difficulty_level, manual_mode)
    audio_video_dir, seq_dirs = setup_audio_paths(data_dir)
    seq_dirs = seq_dirs[:seq_num] if seq_num is not None else seq_dirs
    features, locations = [], []
    with tempfile.TemporaryDirectory(prefix="avlmaps_audio_") as tmp:
        for seq_dir in seq_dirs:
            if not os.path.exists(os.path.join(seq_dir, meta_name)):
                continue
            wav = find_audio(os.path.join(seq_dir, video_name), sample_rate, tmp)
            audio = load_wav(wav, sample_rate, device=True, resample=True)
            seg = ops.segment_audio(audio, sample_rate, silence_duration_s, silence_thres)
            if len(seg) == 0:
                continue
            features.extend(encode_audio_batch(seg.segments_host, audio_encoder, sample_rate, audio=seg.audio, scale=TRACK_SCALE))
            frame_ranges = convert_time_ranges_to_frame_ranges(seg.time_ranges, fps)
            locations.extend(segment_locations(np.loadtxt(Path(seq_dir) / "poses.txt"), frame_ranges))
            if details is not None:
                details[os.path.basename(seq_dir)] = dict(segments=seg.segments_host, time_ranges=seg.time_ranges,
                                                          frame_ranges=np.asarray(frame_ranges, np.int64).reshape(-1, 2))
    save_path = os.path.join(audio_video_dir, db_name)
    with open(save_path, "wb") as f:
        pickle.dump(create_audio_dictionary(features, locations), f)
    return save_path


def create_audio_map_statistics(data_dir: str, difficulty_level: str = "level_1", manual_mode: bool = False, seq_num: int = None):
    """Reference: audio_mapping_utils.py:125-152: the last two comma-separated fields of every meta line, pickled."""
    meta_name, _, _, stats_name = sound_file_names(difficulty_level, manual_mode)
    audio_video_dir, seq_dirs = setup_audio_paths(str(data_dir))
    seq_dirs = seq_dirs[:seq_num] if seq_num is not None else seq_dirs
    scene_data = []
    for seq_dir in seq_dirs:
        meta_path = os.path.join(seq_dir, meta_name)
        if not os.path.exists(meta_path):
            continue
        with open(meta_path, "r") as f:
            for line in f:
                scene_data.append(line.strip("\n").split(",")[-2:])
    save_path = os.path.join(audio_video_dir, stats_name)
    with open(save_path, "wb") as f:
        pickle.dump(scene_data, f)
    return save_path
