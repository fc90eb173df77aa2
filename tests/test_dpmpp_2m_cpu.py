"""CPU: the DPM-Solver++(2M) tables (dex_tts_amd.edm.ablation_tables(..., 'dpmpp_2m', ...)) against the float64 formulas, the solver's
restatement (tests/dpmpp_2m.py) on denoisers with closed-form solutions, and its discretisation error on the model against Euler's
at the same number of network evaluations.  The reference tree has no such solver: tests/dpmpp_2m.py is the yardstick."""
import os

import numpy as np
import pytest
import torch

from dex_tts_amd.edm import ablation_tables
from dex_tts_amd.tolerances import FP32_SAMPLER_MAX, FP32_SAMPLER_MEAN
from tests import dpmpp_2m as R

DISCS = ("vp", "ve", "iddpm", "edm")


@pytest.mark.parametrize("disc", DISCS)
def test_tables_equal_the_float64_formulas(disc):
    for n in (2, 3, 5, 18, 50):
        tab, eul = ablation_tables(n, "dpmpp_2m", disc, "linear", "none"), ablation_tables(n, "euler", disc, "linear", "none")
        assert torch.equal(tab.sigma, eul.sigma) and torch.equal(tab.coef[:, 0], eul.coef[:, 0]), (disc, n)
        assert torch.equal(tab.step[:, 2], eul.step[:, 2]) and float(tab.step[0, 2]) == float(tab.sigma[0]), (disc, n)
        assert torch.equal(tab.step[:, 0], torch.ones(n)) and torch.equal(tab.step[:, 1], torch.zeros(n))
        want = R.coefficients(tab.sigma.numpy()).astype(np.float32)
        np.testing.assert_array_equal(tab.coef[:, 2:5].numpy(), want, err_msg=f"{disc} n={n}")
        assert torch.equal(tab.coef[:, 1], torch.ones(n)) and not tab.coef[:, 5:].any()
        assert float(tab.coef[0, 4]) == 0.0 and tab.coef[-1, 2:5].tolist() == [0.0, 1.0, 0.0]
        assert tab.n_rows == n and tab.n_steps == n and tab.flags == 0 and not tab.noise and tab.solver == "dpmpp_2m"
    # n = 2: one first-order step, then the jump to D - the history coefficient is never used
    assert not ablation_tables(2, "dpmpp_2m", disc, "linear", "none").coef[:, 4].any()


def test_range_overrides_and_alpha():
    """The range overrides pick the noise levels as they do for Euler; alpha changes nothing."""
    tab = ablation_tables(6, "dpmpp_2m", "edm", "linear", "none", sigma_min=0.01, sigma_max=40, rho=5)
    assert torch.equal(tab.sigma, ablation_tables(6, "euler", "edm", "linear", "none", sigma_min=0.01, sigma_max=40, rho=5).sigma)
    assert torch.equal(tab.coef, ablation_tables(6, "dpmpp_2m", "edm", "linear", "none", sigma_min=0.01, sigma_max=40, rho=5, alpha=0.7).coef)


def test_refusals():
    for schedule, scaling in (("vp", "none"), ("ve", "none"), ("linear", "vp")):
        with pytest.raises(ValueError):
            ablation_tables(6, "dpmpp_2m", "edm", schedule, scaling)
    with pytest.raises(ValueError):
        ablation_tables(6, "dpmpp_2m", "edm", "linear", "none", S_churn=10.0)
    with pytest.raises(ValueError):
        ablation_tables(1, "dpmpp_2m", "edm", "linear", "none")
    with pytest.raises(ValueError):                     # an unknown solver: as before
        ablation_tables(4, "midpoint", "edm", "linear", "none")


def test_exact_on_a_constant_denoiser():
    """D(x, sigma) = x_0: every step of the exponential integrator is exact, whatever the history."""
    g = torch.Generator().manual_seed(5)
    x0, z = torch.randn(2, 3, 4, generator=g, dtype=torch.float64), torch.randn(2, 3, 4, generator=g, dtype=torch.float64)
    for n in (2, 3, 7):
        sig = ablation_tables(n, "euler", "edm", "linear", "none").sigma.numpy()
        states = []
        out = R.dpmpp_2m(lambda x, s: x0, z, sig, states)
        assert float((out - x0).abs().max()) <= 1e-12
        for i, x in enumerate(states[:-1]):             # on the way: x(sigma) = x_0 + (sigma / sigma_0) (x(sigma_0) - x_0)
            want = x0 + (float(sig[i]) / float(sig[0])) * (states[0] - x0)
            assert float((x - want).abs().max()) <= 1e-12 * float(sig[0]), (n, i)


def test_second_order_on_a_linear_denoiser():
    """D(x, sigma) = kappa x: dx/dsigma = (1 - kappa) x / sigma, x(sigma) = x(sigma_0) (sigma / sigma_0)^(1 - kappa).  Compared at
    sigma_{n-1}, before the jump to D: halving the steps' size divides the error by about 4."""
    kappa = 0.5
    z = torch.full((1,), 1.0, dtype=torch.float64)
    err = {}
    for n in (64, 128):
        sig = ablation_tables(n, "euler", "edm", "linear", "none").sigma.numpy().astype(np.float64)
        states = []
        R.dpmpp_2m(lambda x, s: kappa * x, z, sig, states)
        exact = states[0] * (sig[n - 1] / sig[0]) ** (1 - kappa)
        err[n] = float((states[n - 1] - exact).abs().max() / exact.abs().max())
    ratio = err[64] / err[128]
    print(f"relative error at sigma_(n-1): n=64 {err[64]:.3e}, n=128 {err[128]:.3e}, ratio {ratio:.2f}")
    assert 3 <= ratio <= 5, (err, ratio)


_MODEL = {}


def model():
    """The model case (tests/dpmpp_2m.py CASE) with the float64 solutions every test below shares, computed once."""
    if not _MODEL:
        net32, z, mask = R.model_case()
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", R.GOLDEN))
        _MODEL.update(net32=net32, z=z, mask=mask, ref=g["heun96"].astype(np.float64), f64={})
    return _MODEL


def solution_f64(n):
    m = model()
    if n not in m["f64"]:
        sig = ablation_tables(n, "euler", "edm", "linear", "none").sigma.numpy()
        m["f64"][n] = R.dpmpp_2m(R.f64_around(m["net32"]), m["z"], sig).numpy()
    return m["f64"][n]


@pytest.mark.usefixtures("golden_threads")
def test_half_of_eulers_error_at_the_same_evaluations():
    """gedex_lj, B = 2, T = 32, lengths [32, 20], seed 1234, EDM discretisation, oracle network: the masked mean |error| against the
    float64 Heun solution at n = 96 (tests/golden/dpmpp_2m_ref.npz, written by tools/make_golden_dpmpp_2m.py: 191 oracle
    evaluations the suite does not repeat).  Measured: 2M 0.157, Euler 0.519 at n = 16 (ratio 0.30)."""
    m = model()
    sig = ablation_tables(16, "euler", "edm", "linear", "none").sigma.numpy()
    e_2m = R.masked_mean_max(solution_f64(16) - m["ref"], m["mask"])
    e_eu = R.masked_mean_max(R.euler(R.f64_around(m["net32"]), m["z"], sig).numpy() - m["ref"], m["mask"])
    print(f"n=16 against Heun n=96: 2M mean {e_2m[0]:.4f} max {e_2m[1]:.4f}; Euler mean {e_eu[0]:.4f} max {e_eu[1]:.4f}; ratio {e_2m[0] / e_eu[0]:.3f}")
    assert e_2m[0] <= 0.5 * e_eu[0], (e_2m, e_eu)


@pytest.mark.usefixtures("golden_threads")
@pytest.mark.parametrize("n", [6, 16])
def test_fp32_table_replay_agrees_with_float64(n):
    """What the device computes from the fp32 tables (one rounding per operation) against the float64 restatement, both around the
    float32 oracle network, inside the bound the project holds an fp32 sampler call to."""
    m = model()
    got = R.dpmpp_2m_replay(ablation_tables(n, "dpmpp_2m", "edm", "linear", "none"), m["z"], m["net32"]).numpy()
    e = np.abs(got - solution_f64(n))
    print(f"n={n}: fp32 table replay against float64: max {e.max():.3e} mean {e.mean():.3e}")
    assert np.isfinite(got).all() and e.max() <= FP32_SAMPLER_MAX and e.mean() <= FP32_SAMPLER_MEAN, (n, float(e.max()), float(e.mean()))
