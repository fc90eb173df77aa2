"""GPU: the general ablation_sampler (dex_tts_amd.edm.ablation_sampler, DexSampleArgs.tables) against the real reference's own
sampler (tests/golden/ablation.npz, tools/make_golden_ablation.py) and against the CPU oracle restatement of it
(tests/test_ablation_tables_cpu.py::oracle_replay); reduced-precision modes, graph replay, repeatability, the module surface,
ragged DEX batches and the EDM path through the tables."""
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests.test_ablation_tables_cpu import gold, model_cases, oracle_replay, overrides, parse, stored_tables
from tests.tolerances import LOWP

pytestmark = pytest.mark.gpu

VP = "gedex_lj_vp_vp_vp_euler_n6"
_MOD = {}


def module(preset):
    """A Diffusion of the preset on cuda:0 with the portable synthetic weights (the engines of tests/gpu_util.py hold the same)."""
    from dex_tts_amd.diffusion import from_config
    if preset not in _MOD:
        cfg, _, w = U.engine_for(preset)
        m = from_config(cfg)
        sd = {}
        for k, v in w.items():
            sd[f"denoise_fn.{k}"] = torch.from_numpy(v)
            sd[f"precond_model.model.{k}"] = torch.from_numpy(v)
        m.load_state_dict(sd, strict=True)
        _MOD[preset] = m.cuda().eval()
    return _MOD[preset]


def case(key):
    """(module, preset inputs on the device, sampler keyword arguments incl. the golden's randn_like draws) of a golden key."""
    from dex_tts_amd import synth
    g = gold()
    preset = "dex_vctk" if key.startswith("dex_vctk") else "gedex_lj"
    m = module(preset)
    B, T, lengths = (1, 64, [57]) if preset == "dex_vctk" else (2, 64, [64, 44])
    mu, mask, z, _ = synth.make_inputs(B, T, lengths, seed=1234)
    d, sc, sl, solver, n = parse(key)
    kw = dict(num_steps=n, solver=solver, discretization=d, schedule=sc, scaling=sl, **overrides(g[key + "_params"]))
    if preset == "dex_vctk":
        ref, ref_len, sty, sty_len = synth.make_dex_style(B, 40, 40, m.cfg.mid_dim, sty_lengths=[33])
        kw.update(ref=[torch.from_numpy(r).cuda() for r in ref], ref_lengths=torch.from_numpy(ref_len).cuda(),
                  sty=torch.from_numpy(sty).cuda(), sty_lengths=torch.from_numpy(sty_len).cuda())
    noise = torch.from_numpy(synth.normalish(f"ablation_{key}", (n, B, 80, T), 4321)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (z, mask, mu)]
    return m, dev, kw, noise


def run(key, precision="fp32", use_graph=False):
    from dex_tts_amd.edm import ablation_sampler
    m, (z, mask, mu), kw, noise = case(key)
    it = iter(noise)
    m.precision, m.use_graph = precision, use_graph
    try:
        return ablation_sampler(m.precond_model, z, mask, mu, randn_like=lambda x: next(it), **kw).cpu().numpy()
    finally:
        m.precision, m.use_graph = "fp32", False


def tag():
    return os.environ.get("PYTEST_CURRENT_TEST", "").split("::")[-1].split(" ")[0]


_ORC = {}


def oracle(key):
    if key not in _ORC:
        _ORC[key] = oracle_replay(key, gold())
    return _ORC[key]


@pytest.mark.parametrize("key", model_cases(gold()))
def test_reference_configs_fp32(key):
    """Every reference configuration of the golden: the paper's VP and VE samplers, iDDPM, alpha = 0.7, a mixed edm / vp / vp Heun,
    VP with churn, and DEX-VCTK.  The schedule's last bits follow the host CPU's fp32 transcendentals (the reference's as much as
    ours; with VP they decide whether a step's noise term is 0), so the device is held to the reference's output with the tables
    of the golden's own run, and ablation_sampler with this host's tables to the oracle restatement with the same tables."""
    g = gold()
    heun = parse(key)[3] == "heun"
    m, (z, mask, mu), kw, noise = case(key)
    st = stored_tables(key, g)
    dex = {k: kw[k] for k in ("ref", "sty", "sty_lengths") if k in kw}
    got = m.engine(z.device).sample(z, mask, mu, st.n_steps, solver=st.solver, noise=noise if st.noise else None, tables=st,
                                    **dex).cpu().numpy()
    U.fp32_sampler_ok(f"ablation_gold_{tag()}", got, g[key], heun=heun)
    U.fp32_sampler_ok(f"ablation_gold_oracle_{tag()}", got, oracle_replay(key, g, st), heun=heun)
    U.fp32_sampler_ok(f"ablation_oracle_{tag()}", run(key), oracle(key), heun=heun)


@pytest.mark.parametrize("prec", ["bf16", "fp16x2"])
def test_vp_reduced_precision(prec):
    got = run(VP, precision=prec)
    e = np.abs(got - oracle(VP))
    U.record(f"ablation_{VP}:{prec}:sampler", max=e.max(), mean=e.mean())
    mx, mn = LOWP[prec]["sampler"]
    assert np.isfinite(got).all() and e.max() <= mx and e.mean() <= mn, (prec, float(e.max()), float(e.mean()))


@pytest.mark.parametrize("key", [VP, "gedex_lj_edm_vp_vp_heun_n4", "gedex_lj_vp_vp_vp_euler_n6_churn"])
def test_graph_and_repeat_bitwise(key):
    eager = run(key)
    assert np.array_equal(eager, run(key))                       # a repeat call
    assert np.array_equal(eager, run(key, use_graph=True))       # the captured call ...
    assert np.array_equal(eager, run(key, use_graph=True))       # ... and its replay


def test_module_forward_equals_ablation_sampler():
    """Diffusion.forward(infer=True) with the new attributes runs the same sampler, with the same generator draws."""
    from dex_tts_amd.edm import ablation_sampler
    m = module("gedex_lj")
    _, (_, mask, mu), _, _ = case(VP)
    m.solver, m.discretization, m.schedule, m.scaling = "euler", "vp", "vp", "vp"
    try:
        torch.manual_seed(3)
        out = m(mu, mask, mu, n_timesteps=6, infer=True, temperature=1.5).cpu().numpy()
        torch.manual_seed(3)
        z = torch.randn(mu.shape, device="cuda") / 1.5 + mu
        ref = ablation_sampler(m.precond_model, z, mask, mu, num_steps=6, solver="euler", discretization="vp", schedule="vp",
                               scaling="vp").cpu().numpy()
    finally:
        m.solver, m.discretization, m.schedule, m.scaling = "euler", "edm", "linear", "none"
    assert np.isfinite(out).all() and np.array_equal(out, ref)


def test_dex_ragged_batch_equals_stacked_rows():
    """DEX at B = 3 with ragged lengths against its three B = 1 runs (the reference cannot batch DEX): a scaled VP Heun sampler."""
    from dex_tts_amd import synth
    from dex_tts_amd.edm import ablation_tables
    cfg, eng, _ = U.engine_for("dex_vctk")
    c = synth.make_case(cfg, B=3, T=64, lengths=[64, 51, 37], Tr=40, Ts=40, sty_lengths=[40, 33, 21])
    tab = ablation_tables(4, "heun", "vp", "vp", "vp")
    noise = torch.from_numpy(synth.normalish("ablation_dex_b3", (4, 3, 80, 64), 5)) if tab.noise else None
    mu, mask, z = (torch.from_numpy(c[k]) for k in ("mu", "mask", "z"))
    kw = U.engine_kwargs(c)
    got = eng.sample(z, mask, mu, 4, solver="heun", noise=noise, tables=tab, **kw).cpu().numpy()
    rows = []
    for b in range(3):
        s = slice(b, b + 1)
        kb = dict(ref=[r[s] for r in kw["ref"]], sty=kw["sty"][s], sty_lengths=kw["sty_lengths"][s])
        rows.append(eng.sample(z[s], mask[s], mu[s], 4, solver="heun", noise=None if noise is None else noise[:, s], tables=tab,
                               **kb).cpu().numpy())
    U.fp32_sampler_ok(f"ablation_{tag()}", got, np.concatenate(rows, 0), heun=True)


@pytest.mark.parametrize("solver,n", [("euler", 6), ("heun", 4)])
def test_edm_defaults_through_tables(solver, n):
    """The EDM sampler handed over as tables (the general update, final_kernel<FinalGP>) against the tables = NULL path."""
    from dex_tts_amd.edm import ablation_tables
    cfg, eng, _ = U.engine_for("gedex_lj")
    c = U.make_case(cfg, B=2, T=64, lengths=[64, 44])
    mu, mask, z = (torch.from_numpy(c[k]) for k in ("mu", "mask", "z"))
    ref = eng.sample(z, mask, mu, n, solver=solver).cpu().numpy()
    got = eng.sample(z, mask, mu, n, solver=solver, tables=ablation_tables(n, solver, "edm", "linear", "none")).cpu().numpy()
    U.fp32_sampler_ok(f"ablation_{tag()}", got, ref, heun=(solver == "heun"))
    U.record(f"ablation_{tag()}:bitwise", equal=float(np.array_equal(got, ref)))
