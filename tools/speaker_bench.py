#!/usr/bin/env python
"""Time the d-vector embedding of the speaker-similarity score (dex_tts_amd/speaker.py, VoiceEncoder.embed_utterances) on an MI355X,
next to the same embedding written with torch ops on the same GPU - torch.stft, a matmul mel, torch.nn.LSTM, which is what resemblyzer
runs - for 1 pair and for 32 pairs of 4 s wavs (2 and 64 utterances of 64000 samples; compute_partial_slices
gives each 4 partials, so 8 and 256 rows through the network).

    python tools/speaker_bench.py [--reps 30] [--warmup 5] [--seed 0] [--json out.json]

Each timing is a host clock around one call that ends in a device synchronise.  The two implementations alternate inside every
repetition, so drift of the shared machine hits both alike; median and the 10th / 90th percentiles of the repetitions are printed.
Weights are synthetic (torch's default init, seeded): the time does not depend on their values.  The outputs of the two are compared
before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dex_tts_amd import speaker  # noqa: E402

SECONDS = 4


def make_weights(seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / 16
    return {name: (torch.rand(*shape, generator=g) * 2 - 1) * k for name, shape in speaker.state_dict_shapes().items()}


def make_wavs(B, seed):
    g = torch.Generator().manual_seed(seed + 1)
    n = SECONDS * speaker.SAMPLING_RATE
    t = torch.arange(n) / speaker.SAMPLING_RATE
    f0 = 100 + 100 * torch.rand(B, 1, generator=g)
    x = sum(torch.sin(2 * np.pi * (k + 1) * f0 * t) / (k + 1) for k in range(6)) + 0.05 * torch.randn(B, n, generator=g)
    return (0.1 * x / x.abs().amax(dim=1, keepdim=True)).float()


class TorchEncoder(torch.nn.Module):
    """resemblyzer's embed_utterance for a batch of equal-length wavs, in torch ops on the device."""

    def __init__(self, sd, device):
        super().__init__()
        self.lstm = torch.nn.LSTM(speaker.N_MELS, speaker.HIDDEN, speaker.LAYERS, batch_first=True)
        self.linear = torch.nn.Linear(speaker.HIDDEN, speaker.EMBED)
        self.load_state_dict(sd)
        self.to(device)
        self.lstm.flatten_parameters()
        self.window = torch.hann_window(speaker.N_FFT, periodic=True, device=device)
        self.basis = None

    def set_basis(self, basis):
        self.basis = basis

    @torch.no_grad()
    def forward(self, wavs):
        B, n = wavs.shape
        _, mel_slices = speaker.compute_partial_slices(n)
        need = mel_slices[-1].stop * speaker.HOP
        if need > n:
            wavs = torch.nn.functional.pad(wavs, (0, need - n))
        spec = torch.stft(wavs, speaker.N_FFT, speaker.HOP, speaker.N_FFT, self.window, center=True, pad_mode="constant", return_complex=True)
        mel = (spec.abs() ** 2).transpose(1, 2) @ self.basis                                    # [B, F, 40]
        parts = torch.stack([mel[:, s] for s in mel_slices], dim=1).reshape(-1, speaker.PARTIALS_N_FRAMES, speaker.N_MELS)
        _, (h, _) = self.lstm(parts)
        raw = torch.relu(self.linear(h[-1]))
        e = (raw / torch.norm(raw, dim=1, keepdim=True)).reshape(B, len(mel_slices), -1).mean(dim=1)
        return e / torch.norm(e, dim=1, keepdim=True)


def slaney_mel_basis(device):
    """librosa.filters.mel(sr=16000, n_fft=400, n_mels=40) (Slaney scale and normalisation), transposed, for the torch formulation."""
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    hz_to_mel = lambda f: min_log_mel + np.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp
    mel_to_hz = lambda m: min_log_hz * np.exp(logstep * (m - min_log_mel)) if m >= min_log_mel else f_sp * m
    lo, hi = hz_to_mel(0.0), hz_to_mel(speaker.SAMPLING_RATE / 2)
    pts = np.array([mel_to_hz(lo + (hi - lo) * i / (speaker.N_MELS + 1)) for i in range(speaker.N_MELS + 2)])
    freqs = np.arange(speaker.N_FFT // 2 + 1) * speaker.SAMPLING_RATE / speaker.N_FFT
    w = np.zeros((speaker.N_MELS, len(freqs)))
    for m in range(speaker.N_MELS):
        lower, upper = (freqs - pts[m]) / (pts[m + 1] - pts[m]), (pts[m + 2] - freqs) / (pts[m + 2] - pts[m + 1])
        w[m] = np.maximum(0, np.minimum(lower, upper)) * 2.0 / (pts[m + 2] - pts[m])
    return torch.from_numpy(w.T.astype(np.float32)).to(device)                                 # [201, 40]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("speaker_bench needs an MI355X: no device, no number")
    dev = torch.device("cuda", 0)
    sd = make_weights(a.seed)
    enc = speaker.VoiceEncoder(dev).load_state_dict(sd)
    ref = TorchEncoder(sd, dev)
    ref.set_basis(slaney_mel_basis(dev))
    rows = []
    for pairs in (1, 32):
        B = 2 * pairs
        wavs = make_wavs(B, a.seed).to(dev)
        P = B * len(speaker.compute_partial_slices(wavs.shape[1])[1])
        lib_fn = lambda: enc.embed_utterances(wavs)
        ref_fn = lambda: ref(wavs)
        diff = float((lib_fn() - ref_fn()).abs().max())
        for _ in range(a.warmup):
            lib_fn(); ref_fn()
        tl, tr = [], []
        for _ in range(a.reps):
            tl.append(timed(lib_fn)); tr.append(timed(ref_fn))
        q = lambda v: [float(np.percentile(v, p)) for p in (50, 10, 90)]
        row = {"pairs": pairs, "utterances": B, "partials": P, "library_ms": q(tl), "torch_ms": q(tr), "max_abs_diff": diff,
               "reps": a.reps, "warmup": a.warmup, "seed": a.seed}
        rows.append(row)
        print(f"{pairs:2d} pairs ({B} utterances, {P} partials): library {row['library_ms'][0]:.3f} ms [{row['library_ms'][1]:.3f}, "
              f"{row['library_ms'][2]:.3f}]  torch {row['torch_ms'][0]:.3f} ms [{row['torch_ms'][1]:.3f}, {row['torch_ms'][2]:.3f}]  "
              f"max|library - torch| {diff:.2e}", flush=True)
    print(json.dumps({"speaker_bench": rows}))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
