"""Time DeXTTS.loss_value (the validation compute_loss) at DEX-VCTK geometry with synthetic weights: B = 32, out_size 172
(fix_len_compatibility(2 * 22050 // 256), train.fix_len 2), ragged 250-450-frame rows.  Prints one JSON line: the end-to-end
median and the split by stage (each stage timed alone between device synchronisations).

    python tools/loss_bench.py [--B 32] [--iters 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dex_tts_amd import align, synth, tts  # noqa: E402
from tests.test_tts_module import full_state_dict, model_cfg  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), out


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    m = tts.DeXTTS(model_cfg("dex_vctk"))
    m.load_state_dict(full_state_dict(m, "dex_vctk"))
    m = m.to(dev).eval()
    B, out_size = a.B, 172
    rng = np.random.default_rng(0)
    yl = rng.integers(250, 451, B)
    xl = np.maximum(yl // 6, 10)
    Ty = int(yl.max())
    tok, xl = synth.make_text_inputs(B, int(xl.max()), xl)
    y = np.zeros((B, 80, Ty), np.float32)
    for b in range(B):
        y[b, :, :yl[b]] = rng.standard_normal((80, yl[b])).astype(np.float32) - 5.0
    mel, lf0, sl = synth.make_style_inputs(B, 200, rng.integers(120, 201, B))
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    x, x_l, yy, y_l = T(tok), T(xl), T(y), T(yl)
    ref, rl, lf, ll = T(mel), T(sl), T(lf0), T(sl)
    off = align.segment_offsets(yl, out_size)
    e2e, _ = timed(lambda: m.loss_value(x, x_l, yy, y_l, ref, rl, ref, rl, lf, ll, out_size=out_size, offsets=off), a.iters)
    t_style, (sk, sd, se, vq) = timed(lambda: m.style(ref, rl, ref, rl, lf, ll, return_vq_loss=True), a.iters)
    t_text, (mu, logw, _) = timed(lambda: m.encoder(x, x_l, se), a.iters)
    t_mas, dur = timed(lambda: align.mas_durations(mu, x_l, yy, y_l), a.iters)

    def seg():
        yc, mc, mk, cl = align.segment(mu, dur, yy, y_l, out_size, off)
        return (yc, mc, mk) + align.dur_prior_losses(logw, dur, x_l, yc, mc, cl)
    t_seg, (yc, mc, mk, _, _) = timed(seg, a.iters)
    m.decoder._bind_owner()
    t_diff, _ = timed(lambda: m.decoder.loss_fn(m.decoder.precond_model, yc, mk, mc, sk, rl, sd, rl), a.iters)
    print(json.dumps({"metric": "loss_value_ms", "config": "dex_vctk", "B": B, "out_size": out_size, "y_lengths": [250, 450],
                      "loss_value_ms": round(e2e, 3),
                      "split_ms": {"style": round(t_style, 3), "text": round(t_text, 3), "mas": round(t_mas, 3),
                                   "segment_dur_prior": round(t_seg, 3), "diffusion_loop": round(t_diff, 3)},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
