"""Timing of the wav preparation (csrc/wavprep.hip): trim, resample (48 kHz -> 22050 Hz) and preprocess_wav (trim + resample + peak
normalise + mel + f0 tracker + lf0), with device events after warm-up, median of --iters, at B = 1 and B = 32 on 4 s utterances at
48 kHz built from tests/golden/sample1_wav.npz; next to it reference_features on the same utterances already at 22050 Hz, the
baseline the trim and the resampler add to.  Prints one JSON line.

    python tools/wavprep_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dex_tts_amd import f0 as F0, wavprep as WP  # noqa: E402


def gpu_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def utterances(w, B, L, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([np.roll(np.resize(w, L), int(s)) * float(g) for s, g in zip(rng.integers(0, L, B), rng.uniform(0.5, 1.0, B))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    w22 = np.load(os.path.join(ROOT, "tests", "golden", "sample1_wav.npz"))["wav"]
    # 48 kHz material: sample1 upsampled on the device (the timing does not depend on the content)
    w48 = WP.resample(torch.from_numpy(w22).cuda(), 22050, 48000)[0].cpu().numpy()
    out = {"metric": "wavprep_ms"}
    for B in (1, 32):
        x48 = torch.from_numpy(utterances(w48, B, 4 * 48000).astype(np.float32)).cuda()
        x22 = torch.from_numpy(utterances(w22, B, 4 * 22050).astype(np.float32)).cuda()
        out[f"b{B}_trim_ms"] = gpu_ms(lambda: WP.trim(x48), args.iters)
        out[f"b{B}_resample_ms"] = gpu_ms(lambda: WP.resample(x48, 48000, 22050), args.iters)
        out[f"b{B}_prepare_ms"] = gpu_ms(lambda: WP.prepare(x48, 48000), args.iters)
        out[f"b{B}_preprocess_wav_ms"] = gpu_ms(lambda: WP.preprocess_wav(x48, 48000), args.iters)
        out[f"b{B}_reference_features_22k_ms"] = gpu_ms(lambda: F0.reference_features(x22), args.iters)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
