"""Vocoder throughput: HiFi-GAN V1, BigVGAN-base and BigVGAN 22 kHz / 80 bands (112 M) at B = 1 and B = 8, T = 512 mel frames, in the
fp32 / bf16 / fp16 operand modes.  Per case: mel-frames/s, ms per call, the algorithmic GFLOP and the fraction of the MFMA peak of the
mode, with bench.py:vocoder_block's formula (every Conv1d / ConvTranspose1d as 2 * L_out * Cin * Cout * taps-per-output) and its timing
helper.  One JSON line per case on stdout; --out also writes them all to a file.

    python tools/vocoder_bench.py [--models hifigan_v1,bigvgan_base,bigvgan_22khz] [--batches 1,8] [--precisions fp32,bf16,fp16]
                                  [--T 512] [--steps 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import DTYPE_KEY, PEAK_TFLOPS, timed_calls  # noqa: E402
from dex_tts_amd import synth, vocoder as V  # noqa: E402

MODELS = {"hifigan_v1": V.HIFIGAN_V1, "bigvgan_base": V.BIGVGAN_BASE, "bigvgan_22khz": V.BIGVGAN_22KHZ}


def algorithmic_flops(h, T):
    """bench.py:vocoder_block's count for one utterance; also the per-stage split (ConvTranspose1d into the stage + its ResBlocks)."""
    fl, L, c = 2.0 * T * 80 * h["upsample_initial_channel"] * 7, T, h["upsample_initial_channel"]
    stages = []
    for u, k in zip(h["upsample_rates"], h["upsample_kernel_sizes"]):
        s = 2.0 * L * c * (c // 2) * k
        L, c = L * u, c // 2
        s += sum(2.0 * L * c * c * kk * 6 for kk in h["resblock_kernel_sizes"])
        stages.append(s)
        fl += s
    fl += 2.0 * L * c * 7
    return fl, stages


def run(name, B, T, prec, steps, warmup, device):
    h = MODELS[name]
    gen = V.Generator(V.AttrDict(h))
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_vocoder_weights(V.param_shapes(h)).items()})
    gen = gen.to(device).eval()
    gen.precision = prec
    mel = torch.from_numpy(synth.make_inputs(B, T, None, seed=1234)[0]).to(device)
    stream = torch.cuda.Stream(device)
    with torch.cuda.stream(stream):
        dt, ev, wav = timed_calls(lambda: gen(mel), steps, warmup, device)
    assert torch.isfinite(wav).all()
    fl, stages = algorithmic_flops(h, T)
    sec = dt / steps
    peak = PEAK_TFLOPS[DTYPE_KEY[prec]]
    out = {"model": name, "B": B, "T": T, "precision": prec, "mel_frames_per_s": round(B * T / sec, 1), "ms_per_call": round(sec * 1e3, 3),
           "hip_event_median_ms": round(statistics.median(ev), 3), "algorithmic_GFLOP": round(B * fl / 1e9, 1),
           "TFLOP_per_s": round(B * fl / sec / 1e12, 1), f"frac_of_{DTYPE_KEY[prec]}_mfma_peak": round(B * fl / sec / 1e12 / peak, 3),
           "stage_GFLOP": [round(B * s / 1e9, 1) for s in stages]}
    del gen
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--precisions", default="fp32,bf16,fp16")
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    rows = []
    for name in a.models.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            for prec in a.precisions.split(","):
                r = run(name, B, a.T, prec, a.steps, a.warmup, device)
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
