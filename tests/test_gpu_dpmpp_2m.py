"""GPU: the DPM-Solver++(2M) sampler (solver='dpmpp_2m': DEX_SOLVER_DPMPP_2M, final_kernel<FinalMP>) against the fp32 table replay of
its restatement (tests/dpmpp_2m.py) around the CPU oracle network; graph replay and repeatability, the history buffer it shares with
Heun, ragged DEX batches, the reduced-precision modes, the module surface and the C ABI's refusals.  T = 64 throughout."""
import numpy as np
import pytest
import torch

from tests import dpmpp_2m as R
from tests import gpu_util as U
from tests.test_gpu_ablation_sampler import module, tag
from tests.tolerances import LOWP

pytestmark = pytest.mark.gpu

SHAPES = {"gedex_lj": dict(B=2, T=64, lengths=[64, 44]),
          "dex_vctk": dict(B=1, T=64, lengths=[57], Tr=40, Ts=40, sty_lengths=[33])}
_CASE, _ORC = {}, {}


def case(preset):
    """(cfg, engine, the preset's inputs as numpy, (z, mask, mu) as host tensors) - the engine is the session's cached one."""
    if preset not in _CASE:
        cfg, eng, _ = U.engine_for(preset)
        c = U.make_case(cfg, **SHAPES[preset])
        _CASE[preset] = (cfg, eng, c, tuple(torch.from_numpy(c[k]) for k in ("z", "mask", "mu")))
    return _CASE[preset]


def tables(n, disc="edm"):
    from dex_tts_amd.edm import ablation_tables
    return ablation_tables(n, "dpmpp_2m", disc, "linear", "none")


def oracle(preset, n, disc="edm"):
    """The fp32 table replay around the CPU oracle's EDMPrecond, once per (preset, n, discretisation)."""
    key = (preset, n, disc)
    if key not in _ORC:
        from oracle import dex_oracle as O
        cfg, _, c, (z, mask, mu) = case(preset)
        W = O.as_torch(U.engine_for(preset)[2], torch.float32)
        kw = U.oracle_kwargs(c)
        _ORC[key] = R.dpmpp_2m_replay(tables(n, disc), z, lambda x, s: O.edm_precond(W, cfg, x, s, mask, mu, **kw)).numpy()
    return _ORC[key]


def sampler(preset, n, disc="edm", precision="fp32", use_graph=False):
    """ablation_sampler(precond_model, z, mask, mu, num_steps=n, solver='dpmpp_2m', ...) on the preset's module."""
    from dex_tts_amd.edm import ablation_sampler
    m = module(preset)
    _, _, c, hz = case(preset)
    z, mask, mu = (t.cuda() for t in hz)
    kw = {}
    if "ref" in c:
        kw = dict(ref=[torch.from_numpy(r).cuda() for r in c["ref"]], ref_lengths=torch.from_numpy(c["ref_lengths"]).cuda(),
                  sty=torch.from_numpy(c["sty"]).cuda(), sty_lengths=torch.from_numpy(np.asarray(c["sty_lengths"])).cuda())
    m.precision, m.use_graph = precision, use_graph
    try:
        return ablation_sampler(m.precond_model, z, mask, mu, num_steps=n, solver="dpmpp_2m", discretization=disc, **kw).cpu().numpy()
    finally:
        m.precision, m.use_graph = "fp32", False


def engine_run(preset, n, **kw):
    _, eng, c, (z, mask, mu) = case(preset)
    return eng.sample(z, mask, mu, n, solver="dpmpp_2m", tables=tables(n), **U.engine_kwargs(c), **kw).cpu().numpy()


@pytest.mark.parametrize("preset,n,disc", [("gedex_lj", 2, "edm"), ("gedex_lj", 3, "edm"), ("gedex_lj", 6, "edm"), ("gedex_lj", 6, "vp"),
                                           ("dex_vctk", 4, "edm")])
def test_fp32_parity(preset, n, disc):
    """n = 2 never reads the history, n = 3 reads it once, n = 6 reuses the buffer over several steps.  The update's coefficients
    are O(1), so the Euler bounds of an fp32 sampler call apply."""
    got, ref = sampler(preset, n, disc), oracle(preset, n, disc)
    e = np.abs(got - ref)
    print(f"{preset} n={n} {disc}: max {e.max():.3e} mean {e.mean():.3e}")
    U.fp32_sampler_ok(f"dpmpp_2m_{tag()}", got, ref)


def test_positional_order_equals_keywords():
    """The reference's positional argument order of the GeDEX tree (spk, class_labels, randn_like, num_steps, sigma_min, sigma_max, rho,
    solver, ...) reaches the same sampler as the keywords."""
    from dex_tts_amd.edm import ablation_sampler
    m = module("gedex_lj")
    z, mask, mu = (t.cuda() for t in case("gedex_lj")[3])
    pos = ablation_sampler(m.precond_model, z, mask, mu, None, None, torch.randn_like, 3, None, None, 7, "dpmpp_2m").cpu().numpy()
    assert np.array_equal(pos, sampler("gedex_lj", 3))


def test_graph_and_repeat_bitwise():
    eager = sampler("gedex_lj", 6)
    assert np.isfinite(eager).all()
    assert np.array_equal(eager, sampler("gedex_lj", 6))                        # a repeat call
    assert np.array_equal(eager, sampler("gedex_lj", 6, use_graph=True))        # the captured call ...
    assert np.array_equal(eager, sampler("gedex_lj", 6, use_graph=True))        # ... and its replay


def test_history_does_not_leak():
    """D_prev lives in the slope buffer Heun writes: a Heun call in between, or a workspace full of NaN, changes nothing - the first
    evaluation of a call does not read the buffer."""
    _, eng, c, (z, mask, mu) = case("gedex_lj")
    first = engine_run("gedex_lj", 6)
    eng.sample(z, mask, mu, 4, solver="heun")
    assert np.isfinite(first).all() and np.array_equal(first, engine_run("gedex_lj", 6))
    clean = engine_run("gedex_lj", 3)
    ws = getattr(eng, "_ws", None)
    assert ws is not None
    ws.fill_(0xFF)                                          # every fp32 word of the workspace: NaN
    dirty = engine_run("gedex_lj", 3)
    assert np.isfinite(dirty).all() and np.array_equal(clean, dirty)


def test_dex_ragged_batch_equals_stacked_rows():
    from dex_tts_amd import synth
    cfg, eng, _ = U.engine_for("dex_vctk")
    c = synth.make_case(cfg, B=3, T=64, lengths=[64, 51, 37], Tr=40, Ts=40, sty_lengths=[40, 33, 21])
    mu, mask, z = (torch.from_numpy(c[k]) for k in ("mu", "mask", "z"))
    kw = U.engine_kwargs(c)
    tab = tables(4)
    got = eng.sample(z, mask, mu, 4, solver="dpmpp_2m", tables=tab, **kw).cpu().numpy()
    rows = []
    for b in range(3):
        s = slice(b, b + 1)
        kb = dict(ref=[r[s] for r in kw["ref"]], sty=kw["sty"][s], sty_lengths=kw["sty_lengths"][s])
        rows.append(eng.sample(z[s], mask[s], mu[s], 4, solver="dpmpp_2m", tables=tab, **kb).cpu().numpy())
    U.fp32_sampler_ok(f"dpmpp_2m_{tag()}", got, np.concatenate(rows, 0))


@pytest.mark.parametrize("prec", ["bf16", "fp16x2"])
def test_reduced_precision(prec):
    got = sampler("gedex_lj", 6, precision=prec)
    e = np.abs(got - oracle("gedex_lj", 6))
    print(f"{prec} n=6: max {e.max():.3e} mean {e.mean():.3e}")
    U.record(f"dpmpp_2m_gedex_lj_n6:{prec}:sampler", max=e.max(), mean=e.mean())
    mx, mn = LOWP[prec]["sampler"]
    assert np.isfinite(got).all() and e.max() <= mx and e.mean() <= mn, (prec, float(e.max()), float(e.mean()))


def test_module_forward_equals_ablation_sampler():
    """Diffusion.solver = 'dpmpp_2m': forward(infer=True) runs the same sampler on the same z, and leaves the generator where the
    Euler path leaves it."""
    from dex_tts_amd.edm import ablation_sampler
    m = module("gedex_lj")
    _, mask, mu = (t.cuda() for t in case("gedex_lj")[3])
    torch.manual_seed(3)
    m(mu, mask, mu, n_timesteps=6, infer=True, temperature=1.5)
    after_euler = torch.randn(4, device="cuda").cpu()
    m.solver = "dpmpp_2m"
    try:
        torch.manual_seed(3)
        out = m(mu, mask, mu, n_timesteps=6, infer=True, temperature=1.5).cpu().numpy()
        after = torch.randn(4, device="cuda").cpu()
        torch.manual_seed(3)
        z = torch.randn(mu.shape, device="cuda") / 1.5 + mu
        ref = ablation_sampler(m.precond_model, z, mask, mu, num_steps=6, solver="dpmpp_2m").cpu().numpy()
    finally:
        m.solver = "euler"
    assert np.isfinite(out).all() and np.array_equal(out, ref)
    assert torch.equal(after, after_euler)


def test_cabi_refusals_leave_the_context_usable():
    """dex_sample refuses the solver without tables, and with tables flagged DEX_TABLES_SCALED / DEX_TABLES_CHURN, with the argument
    error before anything is enqueued; the next valid call runs."""
    from dex_tts_amd.edm import TABLES_CHURN, TABLES_SCALED, AblationTables
    _, eng, c, (z, mask, mu) = case("gedex_lj")
    good = engine_run("gedex_lj", 3)
    with pytest.raises(RuntimeError, match=r"libdexamd error -1: .*tables only"):
        eng.sample(z, mask, mu, 3, solver="dpmpp_2m")
    t = tables(3)
    for flag in (TABLES_SCALED, TABLES_CHURN):
        bad = AblationTables("dpmpp_2m", 3, t.sigma, t.coef, t.step, flag, False)
        with pytest.raises(RuntimeError, match=r"libdexamd error -1: .*DEX_TABLES_SCALED"):
            eng.sample(z, mask, mu, 3, solver="dpmpp_2m", tables=bad)
    assert np.array_equal(good, engine_run("gedex_lj", 3))
