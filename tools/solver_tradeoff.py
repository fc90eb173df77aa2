"""Accuracy against cost of the three solvers on the device: for n in {8, 12, 16, 24, 50} steps of the EDM discretisation, each solver's
network evaluations, time per sampler call (whole-call graph replay, device events) and masked mean / max |error| against the Heun
solution at n = 96 computed by the same engine.  GeDEX-LJ with the portable synthetic weights; needs the GPU.

    python tools/solver_tradeoff.py [--B 2] [--T 256] [--precision fp32] [--iters 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dex_tts_amd import _lib, config as C, synth  # noqa: E402
from dex_tts_amd.edm import ablation_tables  # noqa: E402
from dex_tts_amd.engine import ScoreNetEngine  # noqa: E402

SOLVERS = ("euler", "heun", "dpmpp_2m")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--precision", default="fp32", choices=sorted(_lib.PRECISION))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--n-ref", type=int, default=96)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("solver_tradeoff needs the GPU: nothing here is measured without one")

    cfg = C.gedex_lj()
    eng = ScoreNetEngine(cfg, torch.device("cuda", 0))
    eng.load_weights({k: torch.from_numpy(v) for k, v in synth.make_weights(C.param_shapes(cfg)).items()})
    eng.set_precision(a.precision)
    lengths = [a.T - (b * 3 * a.T // 8) % a.T for b in range(a.B)]            # ragged: T, 5T/8, ...
    mu, mask, z, _ = synth.make_inputs(a.B, a.T, lengths, seed=1234)
    tmu, tmask, tz = (torch.from_numpy(v).cuda() for v in (mu, mask, z))

    def call(solver, n, graph):
        tab = ablation_tables(n, solver, "edm", "linear", "none")
        return eng.sample(tz, tmask, tmu, n, solver=solver, tables=tab, use_graph=graph)

    ref = call("heun", a.n_ref, False).cpu().numpy().astype(np.float64)
    w = mask.astype(np.float64)
    print(f"GeDEX-LJ B={a.B} T={a.T} lengths={lengths} {a.precision}; error against Heun n={a.n_ref} on the same engine; "
          f"time = mean of {a.iters} graph replays")
    print("| n | solver | evaluations | ms / call | ms / evaluation | masked mean abs err | max abs err |")
    print("|---|---|---|---|---|---|---|")
    for n in (8, 12, 16, 24, 50):
        for solver in SOLVERS:
            out = call(solver, n, True)
            call(solver, n, True)                                             # (capture, then one replay, before the timed ones)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(a.iters):
                call(solver, n, True)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.iters
            e = np.abs(out.cpu().numpy().astype(np.float64) - ref) * w
            evals = int(eng.lib.dex_num_evals(n, _lib.SOLVER[solver]))
            print(f"| {n} | {solver} | {evals} | {ms:.3f} | {ms / evals:.4f} | {e.sum() / (w.sum() * 80):.4f} | {e.max():.4f} |", flush=True)


if __name__ == "__main__":
    main()
