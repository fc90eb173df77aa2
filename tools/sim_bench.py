#!/usr/bin/env python
"""Time the WavLM x-vector embedding of the SIM score (dex_tts_amd/wavlm.py, WavLMXVector.embed_utterances: the group-norm feature
extractor, the 12-layer gated-relative-position encoder and the TDNN / statistics-pooling head in fp32, embeddings left on the
device) on an MI355X, next to the same graph written with torch ops in fp32 on the same GPU (tests/wavlm_ref.py torch_graph) - for
1 wav and for 32 wavs of 4 s (64000 samples, 199 frames each).

    python tools/sim_bench.py [--reps 30] [--warmup 3] [--seed 0] [--layers 12] [--json out.json]

Each timing is a host clock around one call that ends in a device synchronise.  The two implementations alternate inside every
repetition, so drift of the shared machine hits both alike; median and the 10th / 90th percentiles of the repetitions are printed.
The config is the default one (wavlm-base-plus-sv); weights are synthetic and seeded: the time does not depend on their values.  The
embeddings of the two are compared before anything is timed."""
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

from dex_tts_amd import wavlm  # noqa: E402
from tests import wavlm_ref as R  # noqa: E402

SECONDS = 4


def make_weights(cfg, seed, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in R.make_weights(cfg, seed).items()}


def make_wavs(B, seed):
    g = torch.Generator().manual_seed(seed + 1)
    n = SECONDS * wavlm.SAMPLING_RATE
    t = torch.arange(n) / wavlm.SAMPLING_RATE
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
        raise SystemExit("sim_bench needs an MI355X: no device, no number")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    dev = torch.device("cuda", 0)
    rcfg = R.variant(R.DEFAULT, num_hidden_layers=a.layers)
    model = wavlm.WavLMXVector(dataclasses.replace(wavlm.WavLMConfig(), num_hidden_layers=a.layers), dev)
    sd = make_weights(rcfg, a.seed, dev)
    model.load_state_dict(sd)
    rows = []
    for B in [int(v) for v in a.batches.split(",")]:
        wavs = make_wavs(B, a.seed).to(dev)
        lib_fn = lambda: model.embed_utterances(wavs)
        ref_fn = lambda: R.torch_graph(rcfg, sd, wavs)[1]
        ref = ref_fn()
        diff = float((lib_fn() - ref).abs().max())
        scale = float(ref.abs().max())
        for _ in range(a.warmup):
            lib_fn(); ref_fn()
        tl, tr = [], []
        for _ in range(a.reps):
            tl.append(timed(lib_fn)); tr.append(timed(ref_fn))
        q = lambda v: [float(np.percentile(v, p)) for p in (50, 10, 90)]
        row = {"wavs": B, "seconds": SECONDS, "frames": wavlm.num_frames(wavs.shape[1]), "layers": a.layers, "library_ms": q(tl), "torch_ms": q(tr),
               "max_abs_embedding_diff": diff, "max_abs_embedding": scale, "reps": a.reps, "warmup": a.warmup, "seed": a.seed}
        rows.append(row)
        print(f"{B:2d} wavs of {SECONDS} s: library {row['library_ms'][0]:.2f} ms [{row['library_ms'][1]:.2f}, {row['library_ms'][2]:.2f}]  "
              f"torch {row['torch_ms'][0]:.2f} ms [{row['torch_ms'][1]:.2f}, {row['torch_ms'][2]:.2f}]  "
              f"max|library - torch| {diff:.2e} at |embedding| {scale:.2f}", flush=True)
    print(json.dumps({"sim_bench": rows}))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
