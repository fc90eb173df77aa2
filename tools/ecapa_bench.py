#!/usr/bin/env python
"""Time the WavLM-large + ECAPA-TDNN embedding of the SIM-o score (dex_tts_amd/ecapa.py, WavLMEcapa.embed_utterances: the layer-norm
feature extractor, the 24-layer stable-layer-norm encoder with the gated relative-position bias, and the ECAPA-TDNN head in fp32,
embeddings left on the device) on an MI355X, next to the same graph in torch ops in fp32 on the same GPU - ``transformers.WavLMModel``
(output_hidden_states=True) for the trunk where transformers is installed (else tests/ecapa_ref.py torch_trunk), and the torch
transcription of the head (tests/ecapa_ref.py torch_head) - for 1 wav and for 32 wavs of 4 s (64000 samples, 199 frames each).

    python tools/ecapa_bench.py [--reps 20] [--warmup 3] [--seed 0] [--layers 24] [--json out.json]

Three timings per batch size:
  whole     ``embed_utterances`` against trunk + head in torch;
  head      the library's head as ``forward`` minus ``hidden_states`` (the two calls differ by the head alone, and a call's launches
            run one after another on one stream) against ``torch_head`` on hidden states computed beforehand;
  res2      the Res2 chain of one SE-Res2 block in its one launch (``WavLMEcapa.res2``, block 1, dilation 3) against its seven-launch
            composition in torch (tests/ecapa_ref.py torch_res2: seven dilated convolutions, each with its ReLU and BatchNorm).

Each timing is a host clock around one call that ends in a device synchronise.  The two implementations alternate inside every
repetition, so drift of the shared machine hits both alike; median and the 10th / 90th percentiles of the repetitions are printed.
The config is the default one; weights are synthetic and seeded: the time does not depend on their values.  The embeddings of the
two are compared before anything is timed."""
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

from dex_tts_amd import ecapa  # noqa: E402
from tests import ecapa_ref as R  # noqa: E402

SECONDS = 4


def make_wavs(B, seed):
    g = torch.Generator().manual_seed(seed + 1)
    n = SECONDS * ecapa.SAMPLING_RATE
    t = torch.arange(n) / ecapa.SAMPLING_RATE
    f0 = 100 + 100 * torch.rand(B, 1, generator=g)
    x = sum(torch.sin(2 * np.pi * (k + 1) * f0 * t) / (k + 1) for k in range(6)) + 0.05 * torch.randn(B, n, generator=g)
    return (0.1 * x / x.abs().amax(dim=1, keepdim=True)).float()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def q(v):
    return [float(np.percentile(v, p)) for p in (50, 10, 90)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--layers", type=int, default=24, help="encoder layers (24 = the default config)")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ecapa_bench needs an MI355X: no device, no number")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    dev = torch.device("cuda", 0)
    rcfg = R.variant(R.DEFAULT, num_hidden_layers=a.layers)
    model = ecapa.WavLMEcapa(dataclasses.replace(ecapa.EcapaConfig(), num_hidden_layers=a.layers), dev)
    sd_host = R.make_weights(rcfg, a.seed)
    sd = {k: torch.from_numpy(v).to(dev) for k, v in sd_host.items()}
    model.load_state_dict(sd)
    try:
        hf = R.hf_wavlm_model(rcfg, sd_host, torch.float32).to(dev)
        trunk_name = "transformers.WavLMModel"

        def trunk(x):
            with torch.no_grad():
                x = torch.nn.functional.layer_norm(x, (x.shape[1],), eps=R.NORM_EPS)
                return list(hf(x, output_hidden_states=True).hidden_states)
    except ImportError:
        trunk_name = "torch_trunk"

        def trunk(x):
            with torch.no_grad():
                return R.torch_trunk(rcfg, sd, x)

    def head(hidden):
        with torch.no_grad():
            return R.torch_head(rcfg, sd, hidden)[1]

    rows = []
    for B in [int(v) for v in a.batches.split(",")]:
        wavs = make_wavs(B, a.seed).to(dev)
        T = ecapa.num_frames(wavs.shape[1])
        hidden = trunk(wavs)
        xr = torch.randn(B, T, rcfg.channels, device=dev)
        pr = "layer3.Res2Conv1dReluBn."
        fns = {"whole": (lambda: model.embed_utterances(wavs), lambda: head(trunk(wavs))),
               "hidden": (lambda: model.hidden_states(wavs), lambda: None),
               "head": (lambda: None, lambda: head(hidden)),
               "res2": (lambda: model.res2(1, xr), lambda: R.torch_res2(xr.transpose(1, 2), sd, pr, rcfg.dilations[1], rcfg.res2_scale))}
        ref = fns["whole"][1]()
        diff = float((fns["whole"][0]() - ref).abs().max())
        scale = float(ref.abs().max())
        with torch.no_grad():
            r2diff = float((fns["res2"][0]() - fns["res2"][1]().transpose(1, 2)).abs().max())
        t = {k: ([], []) for k in fns}
        with torch.no_grad():
            for rep in range(a.warmup + a.reps):
                for k, (lib_fn, ref_fn) in fns.items():
                    tl, tr = timed(lib_fn), timed(ref_fn)
                    if rep >= a.warmup:
                        t[k][0].append(tl); t[k][1].append(tr)
        lib_head = q(np.asarray(t["whole"][0]) - np.asarray(t["hidden"][0]))
        row = {"wavs": B, "seconds": SECONDS, "frames": T, "layers": a.layers, "torch_trunk": trunk_name,
               "library_ms": q(t["whole"][0]), "torch_ms": q(t["whole"][1]),
               "library_hidden_ms": q(t["hidden"][0]), "library_head_ms": lib_head, "torch_head_ms": q(t["head"][1]),
               "library_res2_ms": q(t["res2"][0]), "torch_res2_ms": q(t["res2"][1]),
               "max_abs_embedding_diff": diff, "max_abs_embedding": scale, "max_abs_res2_diff": r2diff,
               "reps": a.reps, "warmup": a.warmup, "seed": a.seed}
        rows.append(row)
        f = lambda v: f"{v[0]:.2f} ms [{v[1]:.2f}, {v[2]:.2f}]"
        print(f"{B:2d} wavs of {SECONDS} s ({T} frames), trunk in torch: {trunk_name}\n"
              f"   whole  library {f(row['library_ms'])}  torch {f(row['torch_ms'])}  max|library - torch| {diff:.2e} at |embedding| {scale:.2f}\n"
              f"   head   library {f(lib_head)} (forward - hidden_states)  torch {f(row['torch_head_ms'])}\n"
              f"   res2   library {f(row['library_res2_ms'])} (one launch)  torch {f(row['torch_res2_ms'])} (seven convolutions)  "
              f"max|library - torch| {r2diff:.2e}", flush=True)
    print(json.dumps({"ecapa_bench": rows}))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
