"""Restatement of DPM-Solver++(2M) (Lu et al. 2022, arXiv:2211.01095: the multistep second-order solver with the data-prediction model)
in the (x, sigma) frame, the yardstick of ``solver='dpmpp_2m'`` (dex_tts_amd.edm.ablation_tables, DEX_SOLVER_DPMPP_2M).  The reference
tree has no such solver, so there is no reference implementation to pin to: the formulas below are the yardstick, and the tests hold
them to what a solver of this kind must do (exact on a constant denoiser, second order on a linear one, Heun's accuracy on the model).

    x_0 = z sigma_0;   h_i = ln(sigma_i / sigma_{i+1}),  r_i = h_{i-1} / h_i,  e_i = -expm1(-h_i)
    i = 0          : x_1     = (sigma_1 / sigma_0) x_0 + e_0 D_0
    0 < i < n - 1  : x_{i+1} = (sigma_{i+1} / sigma_i) x_i + e_i (1 + 1 / (2 r_i)) D_i - e_i / (2 r_i) D_{i-1}
    i = n - 1      : x_n     = D_{n-1}                                            (sigma_n = 0)

``net(x, sigma) -> D`` everywhere; the float64 functions hand it float64 tensors (a float32 network is wrapped by ``f64_around``)."""
import numpy as np
import torch


def coefficients(sigmas):
    """Rows (a, b, c) of x_{i+1} = a x_i + b D_i + c D_{i-1} in float64, from the noise levels sigma_0 .. sigma_{n-1} (and sigma_n = 0)."""
    sg = np.asarray(sigmas, dtype=np.float64)
    assert sg[-1] == 0.0 and len(sg) >= 3
    n = len(sg) - 1
    rows = []
    for i in range(n - 1):
        h = np.log(sg[i] / sg[i + 1])
        e = -np.expm1(-h)
        if i == 0:
            rows.append((sg[1] / sg[0], e, 0.0))
        else:
            r = np.log(sg[i - 1] / sg[i]) / h
            rows.append((sg[i + 1] / sg[i], e * (1 + 1 / (2 * r)), -e / (2 * r)))
    rows.append((0.0, 1.0, 0.0))
    return np.asarray(rows, dtype=np.float64)


def dpmpp_2m(net, z, sigmas, states=None):
    """The solver in float64.  ``sigmas``: [n + 1] noise levels ending in 0; ``states`` (a list) receives x_0 .. x_n."""
    sg = torch.as_tensor(np.asarray(sigmas, dtype=np.float64))
    n = len(sg) - 1
    x = z.double() * sg[0]
    D_prev = None
    if states is not None:
        states.append(x)
    for i in range(n):
        D = net(x, sg[i]).double()
        if i == n - 1:
            x = D
        else:
            h = torch.log(sg[i] / sg[i + 1])
            e = -torch.expm1(-h)
            x_new = (sg[i + 1] / sg[i]) * x
            if i == 0:
                x_new = x_new + e * D
            else:
                r = torch.log(sg[i - 1] / sg[i]) / h
                x_new = x_new + e * (1 + 1 / (2 * r)) * D - e / (2 * r) * D_prev
            x = x_new
        D_prev = D
        if states is not None:
            states.append(x)
    return x


def dpmpp_2m_replay(tab, z, net):
    """The device's update from the fp32 tables (include/dex_amd.h: row e = [sigma, 1, a, b, c, 0, 0, 0]) on the CPU, operation for
    operation: x_0 = z c0, then x = (a x + b D) + c D_prev with one fp32 rounding per product and sum (final_kernel<FinalMP>).  The
    first evaluation has no history: its c is 0 and the kernel adds 0 * 0."""
    coef, step = tab.coef, tab.step
    assert tab.solver == "dpmpp_2m" and tab.flags == 0 and coef.dtype == torch.float32
    x = z.float() * step[0, 2]
    D_prev = torch.zeros_like(x)
    for e in range(tab.n_rows):
        D = net(x, coef[e, 0])
        x = (coef[e, 2] * x + coef[e, 3] * D) + coef[e, 4] * D_prev
        D_prev = D
    return x


def euler(net, z, sigmas):
    """ablation_sampler(solver='euler', linear, none) in float64 on the same noise levels (n evaluations)."""
    sg = torch.as_tensor(np.asarray(sigmas, dtype=np.float64))
    x = z.double() * sg[0]
    for i in range(len(sg) - 1):
        d = (x - net(x, sg[i]).double()) / sg[i]
        x = x + (sg[i + 1] - sg[i]) * d
    return x


def heun(net, z, sigmas):
    """ablation_sampler(solver='heun', alpha = 1, linear, none) in float64 on the same noise levels (2n - 1 evaluations)."""
    sg = torch.as_tensor(np.asarray(sigmas, dtype=np.float64))
    n = len(sg) - 1
    x = z.double() * sg[0]
    for i in range(n):
        h = sg[i + 1] - sg[i]
        d = (x - net(x, sg[i]).double()) / sg[i]
        xp = x + h * d
        if i < n - 1:
            dp = (xp - net(xp, sg[i + 1]).double()) / sg[i + 1]
            x = x + h * (0.5 * d + 0.5 * dp)
        else:
            x = xp
    return x


def f64_around(net32):
    """A float32 network ``net32(x, sigma)`` as seen from a float64 solver: inputs rounded to float32, output widened."""
    return lambda x, s: net32(x.float(), torch.as_tensor(s).float()).double()


def masked_mean_max(err, mask):
    """(mean, max) of |err| [B,80,T] over the frames ``mask`` [B,1,T] keeps."""
    e = np.abs(np.asarray(err, dtype=np.float64)) * np.asarray(mask, dtype=np.float64)
    return float(e.sum() / (np.asarray(mask, dtype=np.float64).sum() * err.shape[1])), float(e.max())


# ---- the model case of tests/test_dpmpp_2m_cpu.py: gedex_lj, portable synthetic weights, B = 2, T = 32, lengths [32, 20], seed 1234
CASE = dict(preset="gedex_lj", B=2, T=32, lengths=[32, 20], seed=1234)
GOLDEN = "dpmpp_2m_ref.npz"          # tests/golden/: the float64 Heun solution at n = 96 of that case (tools/make_golden_dpmpp_2m.py)


def model_case():
    """(net32, z, mask) of CASE around the CPU oracle's EDMPrecond (float32)."""
    from dex_tts_amd import config as C, synth
    from oracle import dex_oracle as O
    cfg = C.PRESETS[CASE["preset"]]()
    mu, mask, z, _ = synth.make_inputs(CASE["B"], CASE["T"], CASE["lengths"], seed=CASE["seed"])
    W = O.as_torch(synth.make_weights(C.param_shapes(cfg)), torch.float32)
    tmu, tmask = torch.from_numpy(mu), torch.from_numpy(mask)
    return (lambda x, s: O.edm_precond(W, cfg, x, s, tmask, tmu)), torch.from_numpy(z), mask
