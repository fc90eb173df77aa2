"""Timing of the f0 tracker (csrc/f0.hip): dio + stonemask alone and reference_features (peak normalise + mel + dio + stonemask +
lf0) with device events after warm-up, at B = 1 on the 4.04 s reference utterance (tests/golden/sample1_wav.npz) and B = 32 on 4 s
utterances; next to it the float64 numpy restatement (tests/world_f0.py) on one CPU core, a rough stand-in for a CPU tracker.
Prints one JSON line.

    python tools/f0bench.py [--iters 20] [--cpu-reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dex_tts_amd import f0 as F0  # noqa: E402
from tests import world_f0 as W  # noqa: E402

FS = 22050.0
FP = 256.0 / 22050.0 * 1000.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    args = ap.parse_args()
    w = np.load(os.path.join(ROOT, "tests", "golden", "sample1_wav.npz"))["wav"]
    x1 = torch.from_numpy(w).cuda()
    rng = np.random.default_rng(0)
    L4 = 88200
    xb = np.stack([np.roll(np.resize(w, L4), int(s)) * float(g) for s, g in zip(rng.integers(0, L4, 32), rng.uniform(0.5, 1.0, 32))])
    x32 = torch.from_numpy(xb.astype(np.float32)).cuda()

    def track(x):
        f, t = F0.dio(x, FS, frame_period=FP)
        return F0.stonemask(x, f, t, FS, frame_period=FP)

    out = {"metric": "f0_tracker_ms"}
    out["b1_dio_stonemask_ms"] = gpu_ms(lambda: track(x1), args.iters)
    out["b1_reference_features_ms"] = gpu_ms(lambda: F0.reference_features(x1), args.iters)
    out["b32_dio_stonemask_ms"] = gpu_ms(lambda: track(x32), args.iters)
    out["b32_reference_features_ms"] = gpu_ms(lambda: F0.reference_features(x32), args.iters)
    torch.set_num_threads(1)
    ts = []
    for _ in range(args.cpu_reps):
        t0 = time.perf_counter()
        f, t = W.dio(w.astype(np.float64), FS, frame_period=FP)
        W.stonemask(w.astype(np.float64), f, t, FS)
        ts.append(time.perf_counter() - t0)
    out["b1_restatement_cpu_1core_ms"] = 1e3 * float(np.median(ts))
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
