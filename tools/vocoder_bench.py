"""Vocoder throughput: HiFi-GAN V1, BigVGAN-base and BigVGAN 22 kHz / 80 bands (112 M) at B = 1 and B = 8, T = 512 mel frames, in the
fp32 / bf16 / fp16 operand modes.  Per case: mel-frames/s, ms per call, the algorithmic GFLOP and the fraction of the MFMA peak of the
mode, with bench.py:vocoder_block's formula (every Conv1d / ConvTranspose1d as 2 * L_out * Cin * Cout * taps-per-output) and its timing
helper.  One JSON line per case on stdout; --out also writes them all to a file.

    python tools/vocoder_bench.py [--models hifigan_v1,bigvgan_base,bigvgan_22khz] [--batches 1,8] [--precisions fp32,bf16,fp16]
                                  [--T 512] [--steps 10] [--warmup 3] [--lengths LO:HI] [--chunk N] [--out FILE]

--lengths LO:HI: a ragged batch, utterance i holding int(T * (LO + (HI - LO) * ((7 i) % 11) / 10)) frames (0.6:1.0 is bench.py's ragged
batch).  Each case is then timed twice on the same mel - the padded call ``gen(mel)`` and the ragged call ``gen(mel, lengths)``
(dex_vocode_ragged, lengths on the device) - with ``valid_frames_per_s`` next to ``mel_frames_per_s`` (which counts the padding).

--chunk N: next to the whole call, the windowed one (``Generator.stream``, dex_vocode_window, N mel frames per window) on the same mel:
``first_chunk_ms`` - host time from the call to the first window's event, the time to first audio - against ``whole_call_ms`` (the
whole call's first audio is its last sample), ``chunked_total_ms`` for all windows, and both workspaces.  Medians over --steps runs,
each synchronised on both sides.
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def ragged_lengths(B, T, lo, hi):
    return [max(1, min(T, int(T * (lo + (hi - lo) * ((7 * i) % 11) / 10.0)))) for i in range(B)]


def host_ms(device, work):
    """Host milliseconds of ``work()`` from an idle device; ``work`` returns once what it measures is complete on the device."""
    torch.cuda.synchronize(device)
    t = time.perf_counter()
    work()
    return (time.perf_counter() - t) * 1e3


def chunked(gen, mel, ln, N, steps, warmup, device):
    """The windowed call next to the whole one, each from an idle device: median host ms of the whole call, to the first window's
    event, and for all windows (a run of its own: waiting for the first event stalls the host's launches); the number of windows."""
    def whole():
        gen(mel) if ln is None else gen(mel, ln)
        torch.cuda.synchronize(device)

    def first():
        it = gen.stream(mel, ln, chunk_frames=N)
        next(it)[2].synchronize()
        it.close()

    n = [0]

    def total():
        n[0] = sum(1 for _ in gen.stream(mel, ln, chunk_frames=N))
        torch.cuda.synchronize(device)
    ms = {f.__name__: statistics.median([host_ms(device, f) for _ in range(warmup + steps)][warmup:]) for f in (whole, first, total)}
    torch.cuda.synchronize(device)
    return ms["whole"], ms["first"], ms["total"], n[0]


def run(name, B, T, prec, steps, warmup, device, lengths=None, chunk=None):
    """One case; ``lengths`` (B frame counts): the ragged call, else the padded one."""
    h = MODELS[name]
    gen = V.Generator(V.AttrDict(h))
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_vocoder_weights(V.param_shapes(h)).items()})
    gen = gen.to(device).eval()
    gen.precision = prec
    mel = torch.from_numpy(synth.make_inputs(B, T, None, seed=1234)[0]).to(device)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=device)     # on the device once: no copy per call
    stream = torch.cuda.Stream(device)
    with torch.cuda.stream(stream):
        dt, ev, wav = timed_calls((lambda: gen(mel)) if ln is None else (lambda: gen(mel, ln)), steps, warmup, device)
    assert torch.isfinite(wav).all()
    fl, stages = algorithmic_flops(h, T)
    sec = dt / steps
    peak = PEAK_TFLOPS[DTYPE_KEY[prec]]
    out = {"model": name, "B": B, "T": T, "precision": prec, "mel_frames_per_s": round(B * T / sec, 1), "ms_per_call": round(sec * 1e3, 3),
           "hip_event_median_ms": round(statistics.median(ev), 3), "algorithmic_GFLOP": round(B * fl / 1e9, 1),
           "TFLOP_per_s": round(B * fl / sec / 1e12, 1), f"frac_of_{DTYPE_KEY[prec]}_mfma_peak": round(B * fl / sec / 1e12 / peak, 3),
           "stage_GFLOP": [round(B * s / 1e9, 1) for s in stages]}
    if lengths is not None:
        out.update(call="ragged", lengths=list(lengths), valid_frames_per_s=round(sum(lengths) / sec, 1))
    if chunk:
        with torch.cuda.stream(stream):
            whole_ms, first_ms, total_ms, windows = chunked(gen, mel, ln, chunk, steps, warmup, device)
        H = gen.halo_frames
        N = min(chunk, T)
        out.update(chunk_frames=N, halo_frames=H, windows=windows, whole_call_ms=round(whole_ms, 3), first_chunk_ms=round(first_ms, 3),
                   chunked_total_ms=round(total_ms, 3), chunked_over_whole=round(total_ms / whole_ms, 3), halo_model=round((N + 2 * H) / N, 3),
                   whole_workspace_MB=round((gen._lib.dex_voc_workspace_bytes if ln is None else gen._lib.dex_voc_ragged_workspace_bytes)(gen._ctx, B, T) / 2**20, 1),
                   window_workspace_MB=round(gen._lib.dex_voc_window_workspace_bytes(gen._ctx, B, N) / 2**20, 1))
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
    ap.add_argument("--lengths", default=None, metavar="LO:HI", help="ragged batch: lengths between LO * T and HI * T frames (bench.py's "
                                                                     "ragged batch is 0.6:1.0); times the padded and the ragged call")
    ap.add_argument("--chunk", type=int, default=None, metavar="N", help="also time the windowed call with N mel frames per window: time to "
                                                                         "the first window's event, the total of all windows, both workspaces")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    frac = None
    if a.lengths:
        frac = tuple(float(v) for v in a.lengths.split(":"))
        if len(frac) != 2 or not 0.0 <= frac[0] <= frac[1] <= 1.0:
            ap.error("--lengths wants LO:HI with 0 <= LO <= HI <= 1")
    if a.chunk is not None and a.chunk < 1:
        ap.error("--chunk wants a positive number of mel frames")
    device = torch.device("cuda", 0)
    rows = []
    for name in a.models.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            for prec in a.precisions.split(","):
                r = run(name, B, a.T, prec, a.steps, a.warmup, device, chunk=a.chunk)
                if frac:
                    ln = ragged_lengths(B, a.T, *frac)
                    r.update(call="padded", lengths=ln, valid_frames_per_s=round(sum(ln) * r["mel_frames_per_s"] / (B * a.T), 1))
                print(json.dumps(r), flush=True)
                rows.append(r)
                if frac:
                    r = run(name, B, a.T, prec, a.steps, a.warmup, device, ln, chunk=a.chunk)
                    print(json.dumps(r), flush=True)
                    rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
