"""ORACLE TOOLING — goldens of the general ablation_sampler (tests/golden/ablation.npz) from the REAL reference's own
``ablation_sampler`` (GeDEX-TTS/model/edm.py:109-216, DEX :104-211), imported through oracle/ref_import.py.

Run only where the reference exists:   python tools/make_golden_ablation.py
Writes numeric arrays only:
  (a) ``<preset>_<disc>_<sched>_<scaling>_<solver>_n<n>[_churn]``: the reference sampler's output on the fixture inputs of
      oracle/make_golden.py (gedex_lj: B = 2, T = 64, lengths 64 / 44; dex_vctk: B = 1, T = 64, 57), and ``..._params``.  Every run
      gets its randn_like draws from the portable generator, synth.normalish("ablation_<key>", (n, B, 80, T), 4321): a schedule
      whose t(sigma(t)) round trip moves t adds noise even at S_churn = 0, so the draws are part of the input.  ``_coef`` /
      ``_step``: the run's tables (dex_tts_amd.edm.ablation_tables on this host): the schedule's last bits depend on the host
      CPU's fp32 transcendentals, and whether a step's noise term is 0 with them.
  (b) ``rec_[ovr<j>_]<disc>_<sched>_<scaling>_<solver>_n<n>``: a recording stand-in net (returns x * 0.5) on random latents
      [1, 2, 4]; ``_sigma`` (float64: the exact value of every sigma the net was called with), ``_x`` (every input it received),
      ``_out`` (the sampler's result), ``_params`` for the range overrides.  Draws: synth.normalish("ablation_rec_n<n>", ...).
``_params`` = [sigma_min, sigma_max, rho, epsilon_s, C_1, C_2, M, alpha, S_churn, S_min, S_max, S_noise], NaN = None (the default).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dex_tts_amd import config as C, synth  # noqa: E402
from dex_tts_amd.edm import ablation_tables  # noqa: E402
from oracle import ref_import  # noqa: E402
from oracle.make_golden import OUT, manifest  # noqa: E402

PARAMS = ("sigma_min", "sigma_max", "rho", "epsilon_s", "C_1", "C_2", "M", "alpha", "S_churn", "S_min", "S_max", "S_noise")
DEFAULTS = dict(sigma_min=None, sigma_max=None, rho=7, epsilon_s=1e-3, C_1=0.001, C_2=0.008, M=1000, alpha=1, S_churn=0, S_min=0,
                S_max=float("inf"), S_noise=1)

# (a): preset, solver, n, discretization, schedule, scaling, overrides
MODEL_RUNS = [
    ("gedex_lj", "euler", 6, "vp", "vp", "vp", {}),                 # the paper's VP configuration
    ("gedex_lj", "euler", 6, "ve", "ve", "none", {}),               # the VE configuration
    ("gedex_lj", "heun", 4, "iddpm", "linear", "none", {}),
    ("gedex_lj", "heun", 4, "edm", "linear", "none", {"alpha": 0.7}),
    ("gedex_lj", "heun", 4, "edm", "vp", "vp", {}),
    ("gedex_lj", "euler", 6, "vp", "vp", "vp", {"S_churn": 10.0}),
    ("dex_vctk", "euler", 4, "ve", "ve", "none", {}),
]
# (b) range overrides on top of the full grid: solver, n, discretization, schedule, scaling, overrides
REC_OVERRIDES = [
    ("heun", 5, "edm", "linear", "none", {"sigma_min": 0.01, "sigma_max": 50.0, "rho": 5}),
    ("euler", 5, "vp", "vp", "vp", {"sigma_min": 0.01, "sigma_max": 50.0, "epsilon_s": 1e-2}),
    ("euler", 5, "iddpm", "linear", "none", {"M": 300, "C_1": 0.002, "C_2": 0.01}),
    ("heun", 5, "ve", "ve", "none", {"sigma_min": 0.05, "sigma_max": 20.0, "alpha": 0.6}),
    ("heun", 5, "edm", "vp", "vp", {"S_churn": 15.0, "S_min": 0.05, "S_max": 30.0, "S_noise": 1.003}),
    ("euler", 18, "iddpm", "ve", "vp", {"M": 300, "sigma_max": 40.0}),
]


def params_array(kw):
    p = dict(DEFAULTS, **kw)
    return np.asarray([np.nan if p[k] is None else float(p[k]) for k in PARAMS], dtype=np.float64)


def model_key(preset, solver, n, disc, sched, scal, kw):
    return f"{preset}_{disc}_{sched}_{scal}_{solver}_n{n}" + ("_churn" if kw.get("S_churn") else "")


def draws(tag, shape):
    it = iter(torch.from_numpy(synth.normalish(tag, shape, 4321)))
    return lambda x: next(it)


@torch.no_grad()
def golden_models(out):
    fixtures = {"gedex_lj": (C.gedex_lj(), 2, 64, [64, 44], None), "dex_vctk": (C.dex_vctk(), 1, 64, [57], (40, 40, [33]))}
    nets = {}
    for preset, solver, n, disc, sched, scal, kw in MODEL_RUNS:
        cfg, B, T, lengths, dex_dims = fixtures[preset]
        if preset not in nets:
            nets[preset] = manifest(preset + "_ablation", cfg)       # (not a preset name: writes no manifest)
        m = nets[preset]
        edm = sys.modules[type(m.precond_model).__module__]
        mu, mask, z, _ = synth.make_inputs(B, T, lengths, seed=1234)
        tmu, tmask, tz = map(torch.from_numpy, (mu, mask, z))
        extra = {}
        if dex_dims is not None:
            Tr, Ts, sl = dex_dims
            ref, ref_len, sty, sty_len = synth.make_dex_style(B, Tr, Ts, cfg.mid_dim, sty_lengths=sl)
            extra = dict(ref=[torch.from_numpy(r) for r in ref], ref_lengths=torch.from_numpy(ref_len), sty=torch.from_numpy(sty),
                         sty_lengths=torch.from_numpy(sty_len))
        key = model_key(preset, solver, n, disc, sched, scal, kw)
        y = edm.ablation_sampler(net=m.precond_model, latents=tz, mask=tmask, mu=tmu, spk=None, num_steps=n, solver=solver,
                                 discretization=disc, schedule=sched, scaling=scal, randn_like=draws(f"ablation_{key}", (n, B, 80, T)),
                                 **extra, **kw)
        out[key] = y.numpy()
        out[key + "_params"] = params_array(kw)
        # the schedule's last bits depend on the host CPU's fp32 transcendentals (the reference's too): the tables of THIS run,
        # which tests/test_ablation_tables_cpu.py pins to the reference, go with it, so that the device can be held to the output
        tab = ablation_tables(n, solver, disc, sched, scal, **kw)
        out[key + "_coef"], out[key + "_step"] = tab.coef.numpy(), tab.step.numpy()
        print(key, float(np.abs(out[key]).max()))


class Rec:
    """Stand-in net: records the sigma and the input of every evaluation and returns x * 0.5."""
    sigma_min, sigma_max = 0, float("inf")

    def __init__(self):
        self.sig, self.x = [], []

    def round_sigma(self, s):
        return torch.as_tensor(s)

    def __call__(self, x, sigma, mask, mu, spk=None):
        sg = torch.as_tensor(sigma)
        assert sg.dtype == torch.float32 and sg.dim() == 0, (sg.dtype, sg.shape)
        self.sig.append(float(sg))
        self.x.append(x.clone())
        return x * 0.5


def record(edm, out, key, solver, n, disc, sched, scal, kw):
    latents = torch.from_numpy(synth.normalish("ablation_rec_latents", (1, 2, 4), 11))
    r = Rec()
    y = edm.ablation_sampler(net=r, latents=latents, num_steps=n, solver=solver, discretization=disc, schedule=sched, scaling=scal,
                             randn_like=draws(f"ablation_rec_n{n}", (n, 1, 2, 4)), **kw)
    out[key + "_sigma"] = np.asarray(r.sig, dtype=np.float64)
    out[key + "_x"] = torch.stack(r.x).numpy()
    out[key + "_out"] = y.numpy()


@torch.no_grad()
def golden_recorded(out):
    ref_import.import_reference("GeDEX-TTS")
    edm = sys.modules["model.edm"]
    for disc in ("vp", "ve", "iddpm", "edm"):
        for sched in ("vp", "ve", "linear"):
            for scal in ("vp", "none"):
                for solver in ("euler", "heun"):
                    for n in (2, 5, 18, 50):
                        record(edm, out, f"rec_{disc}_{sched}_{scal}_{solver}_n{n}", solver, n, disc, sched, scal, {})
    for j, (solver, n, disc, sched, scal, kw) in enumerate(REC_OVERRIDES):
        key = f"rec_ovr{j}_{disc}_{sched}_{scal}_{solver}_n{n}"
        record(edm, out, key, solver, n, disc, sched, scal, kw)
        out[key + "_params"] = params_array(kw)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {}
    golden_models(out)
    golden_recorded(out)
    path = os.path.join(OUT, "ablation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
