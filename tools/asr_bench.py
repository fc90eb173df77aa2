#!/usr/bin/env python
"""Time the ASR transcription of the ASR score (dex_tts_amd/asr.py, Wav2Vec2CTC.transcribe_ids: input normalisation, the
wav2vec 2.0 large network in fp32, greedy CTC, one copy of ids and counts to the host) on an MI355X, next to the same graph
written with torch ops in fp32 on the same GPU (tests/asr_ref.py torch_graph + argmax + a copy of the per-frame ids) - for 1 wav
and for 32 wavs of 4 s (64000 samples, 199 frames each).

    python tools/asr_bench.py [--reps 30] [--warmup 3] [--seed 0] [--layers 24] [--json out.json]

Each timing is a host clock around one call that ends in a device synchronise.  The two implementations alternate inside every
repetition, so drift of the shared machine hits both alike; median and the 10th / 90th percentiles of the repetitions are printed.
The config is the default one (large-lv60-self); weights are synthetic and seeded: the time does not depend on their values.  The
logits of the two are compared before anything is timed."""
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

from dex_tts_amd import asr  # noqa: E402
from tests import asr_ref as R  # noqa: E402

SECONDS = 4


def make_weights(model, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    sd = {}
    for k, shape in model.state_dict_shapes().items():
        if k.endswith("weight_g"):
            v = 0.5 + torch.rand(shape, generator=g, device=dev)
        elif "layer_norm.weight" in k:
            v = 1.0 + 0.2 * torch.randn(shape, generator=g, device=dev)
        elif k.endswith(".bias"):
            v = 0.1 * torch.randn(shape, generator=g, device=dev)
        else:
            v = torch.randn(shape, generator=g, device=dev) / float(np.sqrt(np.prod(shape[1:])))
        sd[k] = v
    return sd


def make_wavs(B, seed):
    g = torch.Generator().manual_seed(seed + 1)
    n = SECONDS * asr.SAMPLING_RATE
    t = torch.arange(n) / asr.SAMPLING_RATE
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
    ap.add_argument("--layers", type=int, default=24, help="encoder layers (24 = the default config)")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("asr_bench needs an MI355X: no device, no number")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    dev = torch.device("cuda", 0)
    cfg = dataclasses.replace(asr.Wav2Vec2Config(), num_hidden_layers=a.layers)
    model = asr.Wav2Vec2CTC(cfg, dev)
    sd = make_weights(model, a.seed, dev)
    model.load_state_dict(sd)
    rcfg = R._cfg(num_hidden_layers=a.layers)
    rows = []
    for B in [int(v) for v in a.batches.split(",")]:
        wavs = make_wavs(B, a.seed).to(dev)
        lib_fn = lambda: model.transcribe_ids(wavs)
        ref_fn = lambda: torch.argmax(R.torch_graph(rcfg, sd, wavs), dim=-1).to(torch.int32).cpu()
        ref_logits = R.torch_graph(rcfg, sd, wavs)
        diff = float((model.forward(wavs) - ref_logits).abs().max())
        scale = float(ref_logits.abs().max())
        for _ in range(a.warmup):
            lib_fn(); ref_fn()
        tl, tr = [], []
        for _ in range(a.reps):
            tl.append(timed(lib_fn)); tr.append(timed(ref_fn))
        q = lambda v: [float(np.percentile(v, p)) for p in (50, 10, 90)]
        row = {"wavs": B, "seconds": SECONDS, "frames": asr.num_frames(wavs.shape[1]), "layers": a.layers, "library_ms": q(tl), "torch_ms": q(tr),
               "max_abs_logit_diff": diff, "max_abs_logit": scale, "reps": a.reps, "warmup": a.warmup, "seed": a.seed}
        rows.append(row)
        print(f"{B:2d} wavs of {SECONDS} s: library {row['library_ms'][0]:.2f} ms [{row['library_ms'][1]:.2f}, {row['library_ms'][2]:.2f}]  "
              f"torch {row['torch_ms'][0]:.2f} ms [{row['torch_ms'][1]:.2f}, {row['torch_ms'][2]:.2f}]  "
              f"max|library - torch| {diff:.2e} at |logit| {scale:.2f}", flush=True)
    print(json.dumps({"asr_bench": rows}))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
