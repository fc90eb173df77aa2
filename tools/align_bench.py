"""Timing of the monotonic alignment search (csrc/mas.hip) with device events: medians of --iters runs after warm-up of

    mas_vctk      the search alone (durations), B = 32, Tx = 256, Ty = 1024 (bit matrices in LDS)
    mas_libritts  the search alone (durations), B = 36, Tx = 600, Ty = 3000 (bit matrices in global memory)
    path_vctk     the drop-in maximum_path at the VCTK size ([b, t_x, t_y] value and mask, dense path out)
    forced_vctk   log-prior from mu_x / y (n_feats 80) + search at the VCTK size
    log_prior_vctk the log-prior alone

Inputs are seeded mel-like log-priors.  Prints one JSON line.

    python tools/align_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dex_tts_amd import align  # noqa: E402


def gpu_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4)


def inputs(B, Tx, Ty, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mu = torch.randn(B, 80, Tx, generator=g) * 1.5 - 4.0
    idx = (torch.arange(Ty)[None, :] * Tx // Ty).expand(B, Ty)
    y = torch.gather(mu, 2, idx[:, None, :].expand(B, 80, Ty).contiguous()) + 0.8 * torch.randn(B, 80, Ty, generator=g)
    return mu.to(dev), y.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {}
    for name, (B, Tx, Ty) in (("vctk", (32, 256, 1024)), ("libritts", (36, 600, 3000))):
        mu, y = inputs(B, Tx, Ty, dev, 7)
        lp = align._log_prior_yx(mu, y).transpose(1, 2)
        tx, ty = np.full(B, Tx, np.int32), np.full(B, Ty, np.int32)
        out[f"mas_{name}_ms"] = gpu_ms(lambda: align._search(lp, None, tx, ty, False), a.iters)
        if name == "vctk":
            v = lp.contiguous()
            m = torch.ones_like(v)
            out["path_vctk_ms"] = gpu_ms(lambda: align.maximum_path(v, m), a.iters)
            out["forced_vctk_ms"] = gpu_ms(lambda: align.mas_durations(mu, tx, y, ty), a.iters)
            out["log_prior_vctk_ms"] = gpu_ms(lambda: align._log_prior_yx(mu, y), a.iters)
    print(json.dumps({"align_bench": out, "iters": a.iters}))


if __name__ == "__main__":
    main()
