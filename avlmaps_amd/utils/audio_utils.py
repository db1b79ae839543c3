"""Sound-map audio helpers with the reference's names (avlmaps/utils/audio_utils.py): the sound categories, WAV loading, silence
segmentation, the five-second contexts and the encoder batches.  The per-sample work (PCM decoding, segmentation, packing) runs in
csrc/avl_audio.hip through ops; there is no CPU fallback.

A file at another rate than the one asked for is resampled on the GPU with load_wav(..., resample=True) (ops.resample_audio,
csrc/avl_resample.hip: scipy.signal.resample_poly's default filter, not the soxr_hq of upstream's librosa.load, with which nothing
here was compared); 16-, 24- and 32-bit PCM and 32-bit float files are read.

Not here: AudioCLIP and its spectrogram front end (any callable audio_encoder(batch (B, 5 * sr) float32) -> (B, D) stands in;
apps/common.HashAudioEncoder is a model-free one), noisereduce, 8-bit and float64 WAV files, and the dataset-synthesis functions
(assign_sound_to_video*)."""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import numpy as np

ENCODER_BATCH = 10          # audio_utils.py:620: upstream encodes its tracks in groups of ten
CONTEXT_SECONDS = 5


def get_level_categories(difficulty_level: str, sound_config) -> List[str]:
    """Sorted sound categories of a difficulty level: the union of its major categories' classes, '_' read as ' '.
    Reference: audio_utils.py:230-236."""
    major2categories = sound_config["major_categories"]
    cats = []
    for major in sound_config["difficulty"][difficulty_level]:
        cats.extend([x.replace("_", " ") for x in major2categories[major]])
    return sorted(cats)


def setup_audio_paths(root_dir: str) -> Tuple[str, List[str]]:
    """(audio_video dir, its sorted entries that are not .pkl files).  Reference: audio_utils.py:239-243."""
    audio_video_dir = os.path.join(root_dir, "audio_video")
    return audio_video_dir, sorted(os.path.join(audio_video_dir, x) for x in os.listdir(audio_video_dir) if not x.endswith(".pkl"))


def read_wav(path, raw24=False):
    """(rate, samples): 16-bit PCM as (n,) or (n, channels) int16; 24- and 32-bit PCM as int32, a 24-bit sample left-justified
    (value * 256: scipy.io.wavfile's convention); a float32 WAV as float32 (multi-channel averaged in float32).  With raw24 a
    24-bit file the wave module reads comes back as its packed frames, (n, channels, 3) uint8, for ops.decode_pcm(width=3).
    The standard library's wave module reads plain PCM; scipy.io.wavfile reads what wave does not (IEEE float, and
    WAVE_FORMAT_EXTENSIBLE where wave refuses it).  Other formats (8-bit, float64) raise ValueError."""
    import wave
    try:
        with wave.open(str(path), "rb") as w:
            width = w.getsampwidth()
            if width not in (2, 3, 4) or w.getcomptype() != "NONE":
                raise wave.Error("not 16-, 24- or 32-bit PCM")
            rate, ch = w.getframerate(), w.getnchannels()
            raw = w.readframes(w.getnframes())
        if width == 3:
            b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, ch, 3)
            if raw24:
                return rate, b
            wide = np.zeros(b.shape[:2] + (4,), np.uint8)
            wide[..., 1:] = b
            pcm = wide.view("<i4").astype(np.int32, copy=False).reshape(-1, ch)
        else:
            pcm = np.frombuffer(raw, dtype="<i2" if width == 2 else "<i4").astype(np.int16 if width == 2 else np.int32, copy=False)
            pcm = pcm.reshape(-1, ch)
        return rate, pcm if ch > 1 else pcm[:, 0]
    except wave.Error:
        pass
    from scipy.io import wavfile
    rate, data = wavfile.read(str(path))
    if data.dtype in (np.int16, np.int32):
        return rate, data
    if data.dtype != np.float32:
        raise ValueError(f"{path}: {data.dtype} samples; only 16-, 24- and 32-bit PCM and 32-bit float WAV files are read")
    return rate, data if data.ndim == 1 else data.mean(axis=1, dtype=np.float32)


def load_wav(path, sample_rate, device=False, resample=False):
    """The mono float32 recording of a WAV file (host array, or the DeviceArray with device=True): PCM is decoded on the GPU
    (ops.decode_pcm16 / ops.decode_pcm; a plain 24-bit file is uploaded as its packed 3-byte frames), a float32 file is passed
    through.  Stands in for librosa.load(path, sr=sample_rate): with resample=True a file recorded at another rate is resampled
    on the GPU (ops.resample_audio: SciPy's resample_poly filter, not librosa's soxr_hq); without it such a file raises
    ValueError."""
    from .. import ops
    from ..device import DeviceArray
    rate, data = read_wav(path, raw24=True)
    if int(rate) != int(sample_rate) and not resample:
        raise ValueError(f"{path}: recorded at {rate} Hz, asked for {sample_rate} Hz; resampling is off (pass resample=True)")
    if len(data) == 0:
        raise ValueError(f"{path}: no samples")
    convert = int(rate) != int(sample_rate)
    if data.dtype == np.float32:
        data = np.ascontiguousarray(data, dtype=np.float32)
        audio = DeviceArray.from_numpy(data) if device or convert else data
    elif data.dtype == np.int16:
        audio = ops.decode_pcm16(data, device=device or convert)
    else:
        audio = ops.decode_pcm(data, width=3 if data.dtype == np.uint8 else 4, device=device or convert)
    return ops.resample_audio(audio, int(rate), int(sample_rate), device=device) if convert else audio


def segment_audio_with_silence(audio_path, silence_duration_s: float = 1, silence_thres: float = 0, sample_rate: int = 44100):
    """(time ranges [(start s, end s)], tracks [audio[l:r] float32 host copies]) of a WAV path or a mono float32 array.
    Reference: audio_utils.py:515-546; a missing path returns ([], []) like upstream, a recording without a loud sample too
    (upstream: IndexError).  A path at another rate is resampled like upstream's librosa.load (load_wav(..., resample=True)).  The
    segmentation is ops.segment_audio."""
    from .. import ops
    if isinstance(audio_path, (str, os.PathLike)):
        if not os.path.exists(audio_path):
            return [], []
        audio = load_wav(audio_path, sample_rate, device=True, resample=True)
    else:
        audio = audio_path
    seg = ops.segment_audio(audio, sample_rate, silence_duration_s, silence_thres)
    host = audio if isinstance(audio, np.ndarray) else seg.audio.numpy()
    time_ranges = [(t[0], t[1]) for t in seg.time_ranges]
    return time_ranges, [host[l:r].copy() for l, r in seg.segments_host]


def convert_time_ranges_to_frame_ranges(time_ranges, fps: float) -> List[Tuple[int, int]]:
    """Reference: audio_utils.py:549-550."""
    return [(int(s * fps), int(e * fps)) for (s, e) in time_ranges]


def create_audio_dictionary(audio_features, locations) -> Dict[int, Dict]:
    """{id: {"audio_features": (D,), "locations": [(3,) ...]}}.  Reference: audio_utils.py:558-566 (without the prints)."""
    return {i: {"audio_features": f, "locations": l} for i, (f, l) in enumerate(zip(audio_features, locations))}


def get_five_second_contexts_audio(audio, times, sample_rate: int) -> np.ndarray:
    """(T, 1, 5 * sample_rate) float64 like upstream (audio_utils.py:569-583): five seconds around every time, zero-padded; the
    slices are ops.context_ranges, the gather is ops.pack_tracks with scale 1.  float32 input."""
    from .. import ops
    n = audio.shape[-1]
    ranges = ops.context_ranges(n, times, sample_rate, CONTEXT_SECONDS)
    if not len(ranges):
        return np.array([])
    out = ops.pack_tracks(audio, ranges, CONTEXT_SECONDS * sample_rate, scale=1.0)
    return out.astype(np.float64).reshape(len(ranges), 1, -1)


def encode_audio_batch(tracks_or_ranges, audio_encoder, sample_rate: int, batch: int = ENCODER_BATCH, audio=None, scale=1.0):
    """(S, D) float32 features.  Reference: audio_utils.py:602-648: every track cut or zero-padded to five seconds
    (get_five_second_contexts_audio(track, [2.5], sr)), then encoded in groups of `batch`.  Two forms:
      encode_audio_batch(tracks, enc, sr)                      a list of host float32 tracks, as upstream (already scaled)
      encode_audio_batch(ranges, enc, sr, audio=dev, scale=s)  (S, 2) (start, stop) ranges of one device recording: packed on the
                                                               GPU (ops.pack_tracks) without a host copy of any track
    audio_encoder receives (B, 5 * sample_rate) float32 host batches.  Left to the encoder, being the model's affair: upstream's
    duplicate of a lone sample (a batch of one is encoded twice there) and the centre pad / crop to 220 500 samples its transforms
    apply when sample_rate != 44100."""
    from .. import ops
    L = CONTEXT_SECONDS * int(sample_rate)
    if audio is None:
        tracks = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t in tracks_or_ranges]
        if not tracks:
            return np.zeros((0, 0), np.float32)
        lens = np.array([len(t) for t in tracks], np.int64)
        stops = np.cumsum(lens)
        ranges = np.stack([stops - lens, stops], axis=1)
        if stops[-1] == 0:
            packed = np.zeros((len(tracks), L), np.float32)
        else:
            packed = ops.pack_tracks(np.concatenate(tracks), ranges, L, scale=scale)
    else:
        ranges = np.asarray(tracks_or_ranges, dtype=np.int64).reshape(-1, 2)
        if not len(ranges):
            return np.zeros((0, 0), np.float32)
        packed = ops.pack_tracks(audio, ranges, L, scale=scale)
    feats = [np.asarray(audio_encoder(packed[i:i + batch]), dtype=np.float32) for i in range(0, len(packed), batch)]
    for f, i in zip(feats, range(0, len(packed), batch)):
        if f.ndim != 2 or f.shape[0] != len(packed[i:i + batch]):
            raise ValueError(f"audio_encoder returned shape {f.shape} for a batch of {len(packed[i:i + batch])}")
    return np.concatenate(feats, axis=0)
