"""NumPy restatements of the sound map's audio steps (csrc/avl_audio.hip), used by the sound tests and tools/probe_sound.py.

segment_closed_form is segment_audio_with_silence (upstream audio_utils.py:515-546) without its loop.  Upstream walks the loud
samples keeping `r`, which is always the previous loud sample when the next one is looked at; a segment is closed exactly when a
loud sample lies `gap` or more after its predecessor.  So the starts are the first loud sample and every loud sample whose distance
to the previous loud one is >= gap, and a segment's r is the loud sample before the next start (the last loud sample for the last
segment).  Valid for gap >= 1 (with gap == 0 upstream's loop closes a segment on the very first sample)."""
import numpy as np

TILE = 4096                    # samples per workgroup of the segmentation kernels (256 threads x 16)
SUMMARY_THREADS = 256          # threads of the workgroup that scans the tile summaries


def loud_mask(audio, threshold):
    audio = np.asarray(audio, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return audio > np.float32(threshold)              # NaN compares false


def segment_closed_form(audio, threshold, gap):
    """(S, 2) int64 (l, r)"""
    idx = np.flatnonzero(loud_mask(audio, threshold)).astype(np.int64)
    if not len(idx):
        return np.zeros((0, 2), np.int64)
    first = np.flatnonzero(np.concatenate([[True], np.diff(idx) >= gap]))       # positions in idx of the starts
    last = np.concatenate([first[1:] - 1, [len(idx) - 1]])
    return np.stack([idx[first], idx[last]], axis=1)


def segment_walk(audio, threshold, gap):
    """the same result from one Python iteration per loud sample, the cost structure of upstream's loop (timing comparisons only)"""
    idx = np.where(loud_mask(audio, threshold))[0]
    out, prev = [], -1
    for i in idx:
        if prev < 0:
            start = i
        elif i - prev >= gap:
            out.append((start, prev))
            start = i
        prev = i
    if prev >= 0:
        out.append((start, prev))
    return np.asarray(out, np.int64).reshape(-1, 2)


def pack_ref(audio, ranges, length, scale):
    audio = np.asarray(audio, dtype=np.float32)
    out = np.zeros((len(ranges), length), np.float32)
    for k, (a, b) in enumerate(ranges):
        t = audio[a:b][:length] * np.float32(scale)
        out[k, :len(t)] = t
    return out


def decode_ref(pcm):
    pcm = np.asarray(pcm, dtype=np.int16)
    pcm = pcm.reshape(len(pcm), -1)
    return np.mean(pcm.astype(np.float32) / np.float32(32768), axis=1, dtype=np.float32)


def context_ref(audio, times, sample_rate, seconds=5):
    """get_five_second_contexts_audio restated with plain slicing: (T, 1, seconds * sr) float64"""
    audio = np.asarray(audio)
    out = []
    for t in times:
        if t - seconds / 2 > (audio.shape[-1] - 1) / sample_rate:
            continue
        b = (np.asarray([t - seconds / 2, t + seconds / 2]) * sample_rate).astype(int)
        sub = audio[b[0]:b[1]]
        buf = np.zeros((1, seconds * sample_rate))
        buf[0, :len(sub)] = sub
        out.append(buf)
    return np.array(out)
