"""CPU: the general ablation_sampler's host tables (dex_tts_amd.edm.ablation_tables) against goldens from the REAL reference's own
ablation_sampler (tools/make_golden_ablation.py -> tests/golden/ablation.npz).

(b) A recording stand-in net pins every table entry: the sigma and the input of every evaluation are reproduced at tolerance 0, and
so is the sampler's result, by a CPU replay of exactly the update the device runs from the tables (final_kernel<FinalGP>, the
x_hat and init kernels: one fp32 rounding per product and sum).  (a) The same replay around the CPU oracle's EDMPrecond reproduces
the reference's sampler outputs on the model fixtures within the oracle's sampler bound."""
import os

import numpy as np
import pytest
import torch

from dex_tts_amd import config as C, synth
from dex_tts_amd.edm import TABLES_CHURN, TABLES_SCALED, ablation_sampler, ablation_tables
from dex_tts_amd.engine import edm_sigmas, heun_eval_sigmas

PARAMS = ("sigma_min", "sigma_max", "rho", "epsilon_s", "C_1", "C_2", "M", "alpha", "S_churn", "S_min", "S_max", "S_noise")
INT_PARAMS = ("rho", "M")


def gold():
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "ablation.npz")))


def overrides(params):
    """The keyword arguments a ``_params`` row of the golden stands for (NaN = None, the default)."""
    if params is None:
        return {}
    kw = {}
    defaults = dict(sigma_min=None, sigma_max=None, rho=7, epsilon_s=1e-3, C_1=0.001, C_2=0.008, M=1000, alpha=1, S_churn=0, S_min=0,
                    S_max=float("inf"), S_noise=1)
    for k, v in zip(PARAMS, params):
        v = None if np.isnan(v) else (int(v) if k in INT_PARAMS else float(v))
        if v != defaults[k]:
            kw[k] = v
    return kw


def parse(key):
    """(discretization, schedule, scaling, solver, n) of a golden key ``..._<disc>_<sched>_<scaling>_<solver>_n<n>[_churn]``."""
    parts = key.replace("_churn", "").split("_")
    return parts[-5], parts[-4], parts[-3], parts[-2], int(parts[-1][1:])


def replay(tab, latents, net, noise):
    """The device's update (include/dex_amd.h, DexSamplerTables) on the CPU, operation for operation.  net(x_in, sigma) -> D."""
    coef, step = tab.coef, tab.step
    n, heun = tab.n_steps, tab.solver == "heun"
    scaled, churn = bool(tab.flags & TABLES_SCALED), bool(tab.flags & TABLES_CHURN)
    inputs = []

    def evaluate(x, e):
        xin = x / coef[e, 1] if scaled else x
        inputs.append(xin)
        D = net(xin, coef[e, 0])
        return coef[e, 2] * x - coef[e, 3] * D

    x = latents * step[0, 2]
    e = 0
    for i in range(n):
        if churn:
            x = step[i, 0] * x + step[i, 1] * (noise[i] if noise is not None else torch.zeros_like(x))
        d = evaluate(x, e)
        if heun and i < n - 1:
            xp = x + coef[e, 5] * d
            dp = evaluate(xp, e + 1)
            x = x + coef[e, 4] * (coef[e, 6] * d + coef[e, 7] * dp)
            e += 2
        else:
            x = x + coef[e, 4] * d
            e += 1
    return x, inputs


def rec_keys(g):
    return sorted(k[:-len("_out")] for k in g if k.startswith("rec_") and k.endswith("_out"))


def test_golden_covers_the_grid():
    g = gold()
    keys = rec_keys(g)
    assert len(keys) == 4 * 3 * 2 * 2 * 4 + 6
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "ablation.npz")) < 1 << 20


@pytest.mark.parametrize("disc", ["vp", "ve", "iddpm", "edm", "ovr"])
def test_tables_reproduce_recorded_sigmas_inputs_and_outputs(disc):
    """Every combination of discretization x schedule x scaling x solver at n in {2, 5, 18, 50} (and the range overrides): the
    evaluation sigmas, every input the network received and the sampler's result equal the reference's, bit for bit."""
    g = gold()
    latents = torch.from_numpy(synth.normalish("ablation_rec_latents", (1, 2, 4), 11))
    keys = [k for k in rec_keys(g) if k.startswith(f"rec_{disc}")]
    assert keys
    for key in keys:
        d, sc, sl, solver, n = parse(key)
        tab = ablation_tables(n, solver, d, sc, sl, **overrides(g.get(key + "_params")))
        noise = torch.from_numpy(synth.normalish(f"ablation_rec_n{n}", (n, 1, 2, 4), 4321))
        out, inputs = replay(tab, latents, lambda x, s: x * 0.5, noise if tab.noise else None)
        np.testing.assert_array_equal(tab.coef[:, 0].double().numpy(), g[key + "_sigma"], err_msg=key)
        np.testing.assert_array_equal(tab.sigma[:-1].numpy(), tab.coef[:, 0].numpy())
        assert tab.n_rows == (n if solver == "euler" else 2 * n - 1) and float(tab.sigma[-1]) == 0.0
        np.testing.assert_array_equal(torch.stack(inputs).numpy(), g[key + "_x"], err_msg=key)
        np.testing.assert_array_equal(out.numpy(), g[key + "_out"], err_msg=key)


def test_noise_flag_is_exact():
    """The draws are skipped only where the reference's noise term is exactly 0: replaying a table whose ``noise`` is False with
    random draws changes nothing."""
    latents = torch.from_numpy(synth.normalish("ablation_rec_latents", (1, 2, 4), 11))
    seen = set()
    for d in ("vp", "ve", "iddpm", "edm"):
        for sc in ("vp", "ve", "linear"):
            for sl in ("vp", "none"):
                tab = ablation_tables(18, "heun", d, sc, sl)
                seen.add(tab.noise)
                if not tab.noise:
                    noise = torch.from_numpy(synth.normalish("any", (18, 1, 2, 4), 1))
                    a, _ = replay(tab, latents, lambda x, s: x * 0.5, None)
                    b, _ = replay(tab, latents, lambda x, s: x * 0.5, noise)
                    assert torch.equal(a, b), (d, sc, sl)
    assert not ablation_tables(18, "heun", "edm", "linear", "none").noise
    assert ablation_tables(6, "euler", "edm", "linear", "none", S_churn=10.0).noise


@pytest.mark.parametrize("n", [2, 4, 18, 50])
def test_edm_defaults_equal_the_edm_path(n):
    """edm / linear / none at alpha = 1: the tables hold the EDM path's schedule (edm_sigmas / heun_eval_sigmas), A = Bc = 1 / sigma,
    h = t_next - t_hat, unit scale and the 1/2, 1/2 Heun weights."""
    te = ablation_tables(n, "euler", "edm", "linear", "none")
    ts = edm_sigmas(n)
    assert torch.equal(te.sigma, ts)
    assert torch.equal(te.coef[:, 2], 1 / ts[:n]) and torch.equal(te.coef[:, 3], 1 / ts[:n])
    assert torch.equal(te.coef[:, 4], ts[1:] - ts[:n]) and torch.equal(te.coef[:, 1], torch.ones(n))
    assert torch.equal(te.step[:, 0], torch.ones(n)) and torch.equal(te.step[:, 1], torch.zeros(n)) and float(te.step[0, 2]) == float(ts[0])
    assert te.flags == 0 and not te.noise
    th = ablation_tables(n, "heun", "edm", "linear", "none")
    assert torch.equal(th.sigma, heun_eval_sigmas(n))
    assert torch.equal(th.coef[:, 6], torch.full((2 * n - 1,), 0.5)) and torch.equal(th.coef[:, 7], torch.full((2 * n - 1,), 0.5))
    assert torch.equal(th.coef[:, 5], th.coef[:, 4])


def test_flags_and_cache():
    assert ablation_tables(6, "euler", "vp", "vp", "vp").flags & TABLES_SCALED
    assert not ablation_tables(6, "euler", "ve", "ve", "none").flags & TABLES_SCALED
    assert ablation_tables(6, "euler", "vp", "vp", "vp") is ablation_tables(6, "euler", "vp", "vp", "vp")
    with pytest.raises(ValueError):
        ablation_tables(1, "euler", "edm", "linear", "none")
    with pytest.raises(ValueError):
        ablation_tables(4, "midpoint", "edm", "linear", "none")
    with pytest.raises(ValueError):
        ablation_tables(4, "euler", "cosine", "linear", "none")


def test_sampler_refuses_other_nets():
    class Net:
        sigma_min, sigma_max = 0, float("inf")

        def round_sigma(self, s):
            return torch.as_tensor(s)

        def __call__(self, x, sigma, mask, mu, spk=None):
            return x
    z = torch.zeros(1, 80, 8)
    with pytest.raises(TypeError):
        ablation_sampler(Net(), z, torch.ones(1, 1, 8), z, num_steps=4)


def model_cases(g):
    return sorted(k for k in g if k.startswith(("gedex_lj_", "dex_vctk_")) and not k.endswith(("_params", "_coef", "_step")))


def stored_tables(key, g):
    """The tables the golden's own run used (written with it: their last bits follow the host CPU's fp32 transcendentals)."""
    from dex_tts_amd.edm import AblationTables
    d, sc, sl, solver, n = parse(key)
    return AblationTables.from_arrays(solver, n, g[key + "_coef"], g[key + "_step"], sl == "vp")


def test_stored_tables_are_the_hosts():
    """On a CPU that rounds like the goldens' (the condition of every bit-exact golden here, tests/conftest.py) the tables stored
    with the model goldens are ablation_tables' own."""
    g = gold()
    for key in model_cases(g):
        d, sc, sl, solver, n = parse(key)
        tab, st = ablation_tables(n, solver, d, sc, sl, **overrides(g[key + "_params"])), stored_tables(key, g)
        assert torch.equal(tab.coef, st.coef) and torch.equal(tab.step, st.step) and tab.flags == st.flags, key


def oracle_replay(key, g, tab=None):
    """The reference's sampler on a model fixture, restated: the table replay around the CPU oracle's EDMPrecond (with this host's
    tables unless ``tab`` is given)."""
    from oracle import dex_oracle as O
    preset = "dex_vctk" if key.startswith("dex_vctk") else "gedex_lj"
    cfg = C.PRESETS[preset]()
    B, T, lengths = (1, 64, [57]) if preset == "dex_vctk" else (2, 64, [64, 44])
    mu, mask, z, _ = synth.make_inputs(B, T, lengths, seed=1234)
    kw = {}
    if preset == "dex_vctk":
        ref, _, sty, sty_len = synth.make_dex_style(B, 40, 40, cfg.mid_dim, sty_lengths=[33])
        kw = dict(ref=[torch.from_numpy(r) for r in ref], sty=torch.from_numpy(sty), sty_lengths=torch.from_numpy(sty_len))
    d, sc, sl, solver, n = parse(key)
    tab = tab or ablation_tables(n, solver, d, sc, sl, **overrides(g[key + "_params"]))
    W = O.as_torch(synth.make_weights(C.param_shapes(cfg)), torch.float32)
    tmu, tmask = torch.from_numpy(mu), torch.from_numpy(mask)
    noise = torch.from_numpy(synth.normalish(f"ablation_{key}", (n, B, 80, T), 4321))
    out, _ = replay(tab, torch.from_numpy(z), lambda x, s: O.edm_precond(W, cfg, x, s, tmask, tmu, **kw), noise if tab.noise else None)
    return out.numpy()


@pytest.mark.usefixtures("golden_threads")
def test_oracle_restatement_reproduces_reference_samplers():
    g = gold()
    keys = model_cases(g)
    assert len(keys) == 7
    for key in keys:
        err = np.abs(oracle_replay(key, g) - g[key])
        assert err.max() <= 1e-3 and err.mean() <= 1e-4, (key, float(err.max()), float(err.mean()))
