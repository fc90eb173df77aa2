#!/usr/bin/env python
"""Time CTC forced alignment and text likelihood (dex_tts_amd/ctc_align.py, csrc/ctc_align.hip) on an MI355X.

    python tools/ctc_align_bench.py [--reps 20] [--warmup 3] [--seed 0] [--layers 24] [--skip-network] [--json out.json]

Per shape (B, T, L) at V = 32 — (1, 199, 60), (32, 199, 60), (1, 4096, 1023), and (1, 4096, 60) for the register form's time per frame:

  kernels      dex_ctc_nll, dex_ctc_align without and with the likelihood, on logits that are already on the device;
               ``F.ctc_loss`` on fp64 log-probs on the same GPU (and with the ``log_softmax`` that makes them) is the comparison for the
               likelihood.  No torch op exists for the Viterbi pass: the numpy restatement (tests/ctc_ref.py) is timed on the HOST, once
               per row, and labelled so.
  network      ``Wav2Vec2CTC.align`` (dex_asr_align + one copy to the host) against ``Wav2Vec2CTC.transcribe_ids`` (dex_asr_transcribe +
               one copy) at the default config with seeded synthetic weights, and their difference: what an alignment adds to a
               transcription.

Every timing is a pair of device events around one call, the median (and 10th / 90th percentile) of ``--reps`` calls after ``--warmup``.
The likelihood is compared with ``F.ctc_loss`` before anything is timed."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dex_tts_amd import _lib, asr, ctc_align as CA  # noqa: E402
from dex_tts_amd._native import i32_ptr, stream  # noqa: E402
from tests import ctc_ref as R  # noqa: E402

SHAPES = [(1, 199, 60), (32, 199, 60), (1, 4096, 1023), (1, 4096, 60)]
V = 32


def events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return [float(np.percentile(ts, p)) for p in (50, 10, 90)]


def kernels(B, T, L, a, dev):
    rows = [R.make_case(a.seed + 100 * b, T, L, V) for b in range(B)]
    x = torch.from_numpy(np.stack([r[0] for r in rows])).to(dev)
    fr, tg, tl = CA.check_targets(B, T, V, None, [r[1].tolist() for r in rows], feasible=True)
    lib = _lib.load()
    ws = CA.ctc_workspace(dev, B, T, V, L)
    out = CA.AlignBuffers(B, T, L, dev)
    p = out.pointers()
    st = stream(dev)
    head = (x.data_ptr(), i32_ptr(fr), B, T, V, i32_ptr(tg), i32_ptr(tl), L, 0)
    tail = (ws.data_ptr(), ws.numel(), st)
    nll_fn = lambda: lib.dex_ctc_nll(*head, p[4], *tail)
    align_fn = lambda: lib.dex_ctc_align(*head, *p[:4], None, *tail)
    both_fn = lambda: lib.dex_ctc_align(*head, *p, *tail)
    x64 = x.double()
    lp = torch.log_softmax(x64, dim=-1).transpose(0, 1).contiguous()
    tgt, il, tll = torch.from_numpy(tg.astype(np.int64)).to(dev), torch.full((B,), T, dtype=torch.long), torch.from_numpy(tl.astype(np.int64))
    loss_fn = lambda: F.ctc_loss(lp, tgt, il, tll, blank=0, reduction="none", zero_infinity=False)
    full_fn = lambda: F.ctc_loss(torch.log_softmax(x.double(), dim=-1).transpose(0, 1), tgt, il, tll, blank=0, reduction="none", zero_infinity=False)
    assert both_fn() == 0
    got, ref = out.views()["nll"].cpu().numpy(), loss_fn().cpu().numpy()
    diff = float(np.abs(got - ref).max())
    t0 = time.perf_counter()
    R.ctc_align(*rows[0])
    host_ms = (time.perf_counter() - t0) * 1e3
    row = {"B": B, "T": T, "L": L, "V": V, "ctc_nll_ms": events(nll_fn, a.reps, a.warmup), "ctc_align_ms": events(align_fn, a.reps, a.warmup),
           "ctc_align_with_nll_ms": events(both_fn, a.reps, a.warmup), "torch_ctc_loss_ms": events(loss_fn, a.reps, a.warmup),
           "torch_log_softmax_ctc_loss_ms": events(full_fn, a.reps, a.warmup), "numpy_viterbi_HOST_ms_per_row": host_ms,
           "max_abs_nll_diff_to_torch": diff, "nll_max": float(np.abs(ref).max())}
    row["ns_per_frame_align"] = row["ctc_align_ms"][0] * 1e6 / T
    row["ns_per_frame_nll"] = row["ctc_nll_ms"][0] * 1e6 / T
    print(f"(B, T, L) = ({B}, {T}, {L}): ctc_nll {row['ctc_nll_ms'][0]:.3f} ms, ctc_align {row['ctc_align_ms'][0]:.3f} ms, with nll "
          f"{row['ctc_align_with_nll_ms'][0]:.3f} ms; F.ctc_loss {row['torch_ctc_loss_ms'][0]:.3f} ms (with log_softmax "
          f"{row['torch_log_softmax_ctc_loss_ms'][0]:.3f} ms); numpy Viterbi on the HOST {host_ms:.1f} ms per row; "
          f"max |nll - torch| {diff:.2e} at {row['nll_max']:.1f}", flush=True)
    return row


def network(B, T, L, model, a, dev):
    n = 320 * T + 80                                                   # the samples of exactly T frames
    assert asr.num_frames(n) == T
    wavs = (0.1 * torch.randn(B, n, generator=torch.Generator().manual_seed(a.seed + 2))).to(dev)
    g = np.random.default_rng(a.seed)
    letters = [s for s in asr.VOCAB[5:] if s != "'"]
    texts = ["".join(g.choice(letters, L)) for _ in range(B)]
    al_fn = lambda: model.align(wavs, texts)
    tr_fn = lambda: model.transcribe_ids(wavs)
    ta, tt = events(al_fn, a.reps, a.warmup), events(tr_fn, a.reps, a.warmup)
    row = {"B": B, "T": T, "L": L, "layers": a.layers, "align_ms": ta, "transcribe_ms": tt, "alignment_adds_ms": ta[0] - tt[0]}
    print(f"(B, T, L) = ({B}, {T}, {L}): Wav2Vec2CTC.align {ta[0]:.2f} ms [{ta[1]:.2f}, {ta[2]:.2f}], transcribe_ids {tt[0]:.2f} ms "
          f"[{tt[1]:.2f}, {tt[2]:.2f}]: the alignment adds {ta[0] - tt[0]:.2f} ms", flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--layers", type=int, default=24, help="encoder layers (24 = the default config)")
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_bench needs an MI355X: no device, no number")
    dev = torch.device("cuda", 0)
    result = {"kernels": [kernels(B, T, L, a, dev) for B, T, L in SHAPES], "network": []}
    if not a.skip_network:
        import asr_bench
        model = asr.Wav2Vec2CTC(dataclasses.replace(asr.Wav2Vec2Config(), num_hidden_layers=a.layers), dev)
        model.load_state_dict(asr_bench.make_weights(model, a.seed, dev))
        result["network"] = [network(B, T, L, model, a, dev) for B, T, L in SHAPES[:3]]
    print(json.dumps({"ctc_align_bench": result}))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
