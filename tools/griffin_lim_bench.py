"""Time Griffin-Lim mel inversion on one MI355X: dex_tts_amd.griffin_lim.mel_to_wav (1024-point real FFTs in LDS, two launches per
iteration) against a self-contained torch restatement of the reference's formulation (audio/stft.py: conv1d with the 1026 x 1024
windowed Fourier basis, conv_transpose1d with pinv(4 basis).T, window_sumsquare division), written here, on the same GPU.  The two
convolutions run as the GEMMs they are (unfold / fold + matmul): the same dense arithmetic, without MIOpen's first-use kernel search.
Both get the same explicit initial angles (the host draw is left out of both timings).

    python tools/griffin_lim_bench.py [--T 512] [--iters 60] [--reps 10] [--out profiles/griffin_lim_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dex_tts_amd import griffin_lim as G  # noqa: E402

N, HOP = 1024, 256


def slaney_mel_basis(sr=22050, n_mels=80, fmin=0.0, fmax=8000.0):
    """librosa.filters.mel(sr, 1024, n_mels, fmin, fmax): Slaney mel scale, slaney area normalisation, float32 [n_mels, 513]."""
    def hz2mel(f):
        f = np.asarray(f, np.float64)
        return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-12) / 1000.0) / (np.log(6.4) / 27.0), f * 3 / 200.0)

    def mel2hz(m):
        return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 15.0)), 200.0 / 3 * m)

    freqs = np.linspace(0, sr / 2.0, 513)
    mf = mel2hz(np.linspace(hz2mel(fmin), hz2mel(fmax), n_mels + 2))
    lower = (freqs[None] - mf[:-2, None]) / np.diff(mf)[:-1, None]
    upper = (mf[2:, None] - freqs[None]) / np.diff(mf)[1:, None]
    return (np.maximum(0, np.minimum(lower, upper)) * (2.0 / (mf[2:] - mf[:-2]))[:, None]).astype(np.float32)


class TorchGriffinLim:
    """The reference's dense formulation on the GPU, fp32."""

    def __init__(self, dev):
        fb = np.fft.fft(np.eye(N))
        fb = np.vstack([np.real(fb[:513]), np.imag(fb[:513])])
        win = 0.5 + 0.5 * np.cos(np.linspace(-np.pi, np.pi, N + 1)[:N])
        self.fwd = (torch.FloatTensor(fb[:, None, :]) * torch.from_numpy(win).float()).to(dev)
        self.inv = (torch.FloatTensor(np.linalg.pinv(4 * fb).T[:, None, :]) * torch.from_numpy(win).float()).to(dev)
        self.wsq = win ** 2
        self.dev = dev
        self.mel_basis = torch.from_numpy(slaney_mel_basis()).to(dev)

    def envelope(self, frames):
        n = N + HOP * (frames - 1)
        x = np.zeros(n, np.float32)
        for i in range(frames):
            x[i * HOP:min(n, i * HOP + N)] += self.wsq[:max(0, min(N, n - i * HOP))]
        return torch.from_numpy(x).to(self.dev)

    # conv1d(y, basis, stride 256) and conv_transpose1d(X, inv_basis, stride 256) as the GEMMs they are (frames x basis, then
    # unfold / fold for the framing and the overlap-add): the same dense arithmetic through hipBLAS
    def transform(self, y):
        y = F.pad(y[:, None, None, :], (512, 512, 0, 0), mode="reflect")[:, 0, 0]
        X = (y.unfold(-1, N, HOP) @ self.fwd[:, 0, :].T).transpose(1, 2)              # [B, 1026, F]
        return torch.atan2(X[:, 513:], X[:, :513])

    def inverse(self, S, phase, wss, nz):
        X = torch.cat([S * torch.cos(phase), S * torch.sin(phase)], dim=1)            # [B, 1026, F]
        frames = (X.transpose(1, 2) @ self.inv[:, 0, :]).transpose(1, 2)               # [B, 1024, F]
        n = N + HOP * (S.shape[-1] - 1)
        x = F.fold(frames, (1, n), (1, N), stride=(1, HOP))[:, 0]                      # [B, 1, n]
        x[:, :, nz] /= wss[nz]
        x *= 4.0
        return x[:, 0, 512:-512]

    def __call__(self, mel, angles, n_iters):
        S = (torch.exp(mel).transpose(1, 2) @ self.mel_basis).transpose(1, 2)[:, :, :-1] * 1000
        wss = self.envelope(S.shape[-1])
        nz = torch.nonzero(wss > np.finfo(np.float32).tiny)[:, 0]
        x = self.inverse(S, angles, wss, nz)
        for _ in range(n_iters):
            x = self.inverse(S, self.transform(x), wss, nz)
        return x


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="time only the HIP path (for a rocprofv3 kernel trace of it)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mel1 = np.load(os.path.join(ROOT, "tests", "golden", "audio_mel.npz"))["sample1_1s_mel"]
    mel1 = np.tile(mel1, (1, a.T // mel1.shape[1] + 1))[:, : a.T]
    base = TorchGriffinLim(dev)
    res = {"T": a.T, "iters": a.iters, "device": torch.cuda.get_device_name(0), "rows": []}
    for B in [int(v) for v in a.batches.split(",")]:
        mel = torch.from_numpy(np.repeat(mel1[None], B, 0)).to(dev)
        ang = torch.from_numpy(np.angle(np.exp(2j * np.pi * np.random.RandomState(0).rand(B, 513, a.T - 1))).astype(np.float32)).to(dev)
        hip = timed(lambda: G.mel_to_wav(mel, n_iters=a.iters, angles=ang), a.reps)
        print(json.dumps({"B": B, "hip_ms": hip}), flush=True)
        if a.hip_only:
            continue
        ref = timed(lambda: base(mel, ang, a.iters), max(2, a.reps // 2))
        x, y = G.mel_to_wav(mel, n_iters=a.iters, angles=ang), base(mel, ang, a.iters)
        row = {"B": B, "hip_ms": hip, "torch_ms": ref, "speedup": ref / hip, "max_abs_diff": float((x - y).abs().max())}
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
