#!/usr/bin/env python3
"""Write a small synthetic scene in the reference's dataset layout (dataset/README.md:76-93):
<out>/rgb/%06d.png, <out>/depth/%06d.npy (float32 metres), <out>/poses.txt (x y z qx qy qz qw).
--audio adds <out>/audio_video/000000/ for the sound map: output_with_audio_<level>.wav (PCM16 mono: bursts of noise separated by
silence, one per placed sound), poses.txt (one pose per video frame) and range_and_audio_meta_<level>.txt."""
import argparse
from pathlib import Path

import numpy as np
from PIL import Image


def make(out, frames=8, H=120, W=160, seed=0):
    out = Path(out)
    (out / "rgb").mkdir(parents=True, exist_ok=True)
    (out / "depth").mkdir(exist_ok=True)
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    poses = []
    for i in range(frames):
        d = 2.2 + 1.0 * np.sin(2.0 * xx + 0.2 * i) * np.cos(1.5 * yy) + 0.6 * yy
        np.save(out / "depth" / f"{i:06d}.npy", d.astype(np.float32))
        rgb = np.stack([(127 + 120 * np.sin(3 * xx + i)), (127 + 120 * np.cos(2 * yy)), 255 * (xx > 0)], -1)
        rgb = np.clip(rgb + rng.normal(0, 3, rgb.shape), 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(out / "rgb" / f"{i:06d}.png")
        yaw = 0.08 * i
        poses.append([0.1 * i, 0.0, -0.05 * i, 0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)])
    np.savetxt(out / "poses.txt", np.array(poses))
    return out


def make_audio(out, level="level_3", sample_rate=44100, fps=25, bursts=3, seed=0):
    """one sequence of `bursts` sounds of 1.5 s, 2 s of silence between them (longer than the default silence_duration_s = 1)"""
    import wave
    seq = Path(out) / "audio_video" / "000000"
    seq.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    burst, quiet = int(1.5 * sample_rate), 2 * sample_rate
    pcm = np.zeros(quiet // 2 + bursts * (burst + quiet), np.int16)
    names = ["clock_alarm", "dog", "coughing", "door_wood_knock", "cat"]
    lines = []
    for b in range(bursts):
        s0 = quiet // 2 + b * (burst + quiet)
        pcm[s0:s0 + burst] = rng.integers(-12000, 12000, burst)
        pcm[s0], pcm[s0 + burst - 1] = 9000, 9000                  # a loud first and last sample: the segment is the burst
        lines.append(f"{int(s0 / sample_rate * fps)},{int((s0 + burst) / sample_rate * fps)},{names[b % len(names)]},{b}.wav")
    with wave.open(str(seq / f"output_with_audio_{level}.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(pcm.astype("<i2").tobytes())
    frames = int(np.ceil(len(pcm) / sample_rate * fps)) + 1
    poses = [[0.02 * i, 0.0, -0.01 * i, 0.0, 0.0, 0.0, 1.0] for i in range(frames)]
    np.savetxt(seq / "poses.txt", np.array(poses))
    (seq / f"range_and_audio_meta_{level}.txt").write_text("\n".join(lines) + "\n")
    return seq


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=120)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--audio", action="store_true", help="also write audio_video/000000 for the sound map")
    ap.add_argument("--audio-rate", type=int, default=44100, help="sample rate of the sound track (sound_data_collect_params.sample_rate)")
    a = ap.parse_args()
    print(make(a.out, a.frames, a.height, a.width))
    if a.audio:
        print(make_audio(a.out, sample_rate=a.audio_rate))
