"""What rounding the prepared wav to fp32 does to the f0 track: DEX-TTS/synthesize.py feeds DIO + StoneMask the fp64 wav that trim /
resample / peak normalisation leave, while the device chain (dex_tts_amd.wavprep.preprocess_wav) rounds that wav to fp32 once and
tracks the fp32 samples.  Runs the float64 restatements (tests/wav_prep.py, tests/world_f0.py) on both inputs, CPU only, and prints
one JSON line per signal: voicing flips and the largest relative f0 difference on frames voiced in both.

    python tools/dio_input_precision.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import wav_prep as P  # noqa: E402
from tests import world_f0 as W  # noqa: E402

FS = 22050.0
FP = 256.0 / 22050.0 * 1000.0


def track(x):
    f, t = W.dio(x, FS, frame_period=FP)
    return W.stonemask(x, f, t, FS)


def chain64(x, sr):
    """The reference's wav up to the tracker, fp64 throughout."""
    s, e = P.trim_bounds(x)
    y = x[s:e]
    if sr != P.SR:
        y = P.resample(y, sr, P.SR)
    return P.peak_normalize(y)


def tone(f0, sec=2.0, fs=FS):
    n = np.arange(int(sec * fs))
    x = sum(np.sin(2 * np.pi * f0 * k * n / fs) / k for k in range(1, 8))
    return 0.3 * x / np.abs(x).max()


def main():
    w = np.load(os.path.join(ROOT, "tests", "golden", "sample1_wav.npz"))["wav"].astype(np.float64)
    rng = np.random.default_rng(0)
    pad = lambda x, sr: np.concatenate([1e-4 * rng.standard_normal(sr // 4), x, np.zeros(sr // 8)])   # noqa: E731
    signals = {"sample1@22050": (w, 22050), "tone130@22050": (tone(130.0), 22050), "tone220@22050": (tone(220.0), 22050)}
    for sr in (16000, 24000, 44100, 48000):
        signals[f"sample1@{sr}"] = (pad(P.resample(w, 22050, sr).astype(np.float32).astype(np.float64), sr), sr)
    for name, (x, sr) in signals.items():
        y64 = chain64(x, sr)
        f64 = track(y64)
        f32 = track(y64.astype(np.float32).astype(np.float64))
        v64, v32 = f64 > 0, f32 > 0
        both = v64 & v32
        rel = float(np.abs(f32[both] / f64[both] - 1).max()) if both.any() else 0.0
        print(json.dumps({"signal": name, "frames": int(len(f64)), "voiced": int(v64.sum()), "voicing_flips": int((v64 != v32).sum()),
                          "max_rel_f0": rel}))


if __name__ == "__main__":
    main()
