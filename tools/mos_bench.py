#!/usr/bin/env python
"""Time the UTMOS naturalness score (dex_tts_amd/mos.py, UTMOS.forward: the group-norm wav2vec 2.0 base trunk, the conditioned
bidirectional LSTM and the projection in fp32, scores left on the device) on an MI355X, next to the same graph written with
``transformers.Wav2Vec2Model`` + ``nn.LSTM`` + linears in fp32 on the same GPU (tests/mos_ref.py hf_modules / hf_forward) - for 1 wav
and for 32 wavs of 4 s (64000 samples, 199 frames each) - and the recurrence alone (UTMOS.bilstm: the conditioning, the input
projections and mos_lstm_kernel) next to ``nn.LSTM`` on the same features.

    python tools/mos_bench.py [--reps 30] [--warmup 3] [--seed 0] [--layers 12] [--json out.json]

Each timing is a host clock around one call that ends in a device synchronise.  The two implementations alternate inside every
repetition, so drift of the shared machine hits both alike; median and the 10th / 90th percentiles of the repetitions are printed.
The config is the default one; weights are synthetic and seeded: the time does not depend on their values.  The scores of the two
are compared before anything is timed."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dex_tts_amd import mos  # noqa: E402
from tests import mos_ref as R  # noqa: E402

SECONDS = 4


def make_wavs(B, seed):
    g = torch.Generator().manual_seed(seed + 1)
    n = SECONDS * mos.SAMPLING_RATE
    t = torch.arange(n) / mos.SAMPLING_RATE
    f0 = 100 + 100 * torch.rand(B, 1, generator=g)
    x = sum(torch.sin(2 * np.pi * (k + 1) * f0 * t) / (k + 1) for k in range(6)) + 0.05 * torch.randn(B, n, generator=g)
    return (0.1 * x / x.abs().amax(dim=1, keepdim=True)).float()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--layers", type=int, default=12, help="encoder layers (12 = the default config)")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mos_bench needs an MI355X: no device, no number")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    dev = torch.device("cuda", 0)
    rcfg = R.variant(R.DEFAULT, num_hidden_layers=a.layers)
    sd = R.make_weights(rcfg, a.seed)
    model = mos.UTMOS(dataclasses.replace(mos.MOSConfig(), num_hidden_layers=a.layers), dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    mods = R.hf_modules(rcfg, sd, torch.float32, dev)
    lstm = mods[3]
    cond = torch.cat([mods[1].weight[R.DOMAIN], mods[2].weight[R.JUDGE]])
    rows = []
    q = lambda v: [float(np.percentile(v, p)) for p in (50, 10, 90)]      # noqa: E731
    for B in [int(v) for v in a.batches.split(",")]:
        wavs = make_wavs(B, a.seed).to(dev)
        lib_fn = lambda: model.forward(wavs)                                # noqa: E731
        ref_fn = lambda: R.hf_forward(mods, wavs)[3]                        # noqa: E731
        ref = ref_fn()
        diff, scale = float((lib_fn() - ref).abs().max()), float(ref.abs().max())
        feats = model.hidden_states(wavs)
        T = feats.shape[1]
        lib_rnn = lambda: model.bilstm(feats)                               # noqa: E731

        def ref_rnn():
            with torch.no_grad():
                return lstm(torch.cat([feats, cond.expand(B, T, -1)], dim=2))[0]
        rdiff = float((lib_rnn() - ref_rnn()).abs().max())
        for _ in range(a.warmup):
            lib_fn(); ref_fn(); lib_rnn(); ref_rnn()
        tl, tr, rl, rr = [], [], [], []
        for _ in range(a.reps):
            tl.append(timed(lib_fn)); tr.append(timed(ref_fn)); rl.append(timed(lib_rnn)); rr.append(timed(ref_rnn))
        row = {"wavs": B, "seconds": SECONDS, "frames": T, "layers": a.layers, "library_ms": q(tl), "torch_ms": q(tr),
               "library_bilstm_ms": q(rl), "torch_lstm_ms": q(rr), "max_abs_score_diff": diff, "max_abs_score": scale,
               "max_abs_bilstm_diff": rdiff, "reps": a.reps, "warmup": a.warmup, "seed": a.seed}
        rows.append(row)
        f = lambda k: f"{row[k][0]:.2f} ms [{row[k][1]:.2f}, {row[k][2]:.2f}]"        # noqa: E731
        print(f"{B:2d} wavs of {SECONDS} s: library {f('library_ms')}  torch {f('torch_ms')}  max|library - torch| {diff:.2e} at |score| {scale:.2f}\n"
              f"   the recurrence alone ({T} steps): library {f('library_bilstm_ms')}  torch nn.LSTM {f('torch_lstm_ms')}  max|diff| {rdiff:.2e}", flush=True)
    print(json.dumps({"mos_bench": rows}))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
