"""Host-side mirror of the reference's ``EDMLoss`` (GeDEX-TTS/model/edm.py:22-68, DEX-TTS/model/edm.py:22-68) — the
``infer=False`` branch of ``Diffusion.forward`` (diffusion.py:222-224 / :252-254), SURVEY §8 row f4.

Same constructor, same ``forward`` argument order, same two generator draws in the same order (``randn([B,1,1])`` for the
noise level, then ``randn_like(x0)``), same weighting branches (``loss_type`` 'base', 'base_min_k', 'base_log_k', 'min_snr_k',
'max_snr_k', 'snr', 'inv_snr').  The denoiser evaluation ``D(x0 + n; sigma)`` — all of the arithmetic that matters — runs in
libdexamd.so.  Every utterance has its own sigma.  ``batched=False`` (the default, whose results keep their bits) reads the B
levels back to the host and calls ``dex_denoise_once`` once per utterance at B = 1; ``batched=True`` evaluates the whole batch in
ONE ``dex_denoise_batch`` call - the library builds a conditioning row per utterance from the device vector of levels, as the
reference's ``EDMPrecond.forward`` does with ``sigma.reshape(-1, 1, 1)`` - with sigma, the weight and the masked mean staying on
the device.  The per-utterance scalars (sigma, weight) and the final masked mean are a handful of stock torch ops on [B,1,1] /
[B,80,T] tensors, as VERDICT round 2 item 7 allows.

This is the loss VALUE (validation / monitoring, parity with the reference on fixed draws — tests/golden/edm_loss.npz).  The HIP
path has no backward pass: training stays with the reference module, and a tensor that requires grad is refused loudly rather
than silently detached.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn as nn


def loss_weight(sigma: torch.Tensor, loss_type: str, sigma_data: float = 0.5) -> torch.Tensor:
    """lambda(sigma) of edm.py:37-63 (per utterance, [B,1,1])."""
    snr = 1 / sigma ** 2
    base = (sigma ** 2 + sigma_data ** 2) / (sigma * sigma_data) ** 2
    if loss_type == "base":
        return base
    for prefix, fn in (("base_min_", lambda k: torch.clamp(base, max=k)),
                       ("base_log_", lambda k: torch.where(base >= k, torch.log(base) + (k - math.log(k)), base)),
                       ("min_snr_", lambda k: torch.clamp(snr, max=k)),
                       ("max_snr_", lambda k: torch.clamp(snr, min=k))):
        if loss_type.startswith(prefix):
            return fn(float(loss_type.split(prefix)[-1]))
    if loss_type == "snr":
        return snr
    if loss_type == "inv_snr":
        return 1.0 / snr
    raise ValueError(f"unknown loss_type {loss_type!r} (edm.py:37-63 knows base, base_min_k, base_log_k, min_snr_k, max_snr_k, snr, inv_snr)")


class EDMLoss(nn.Module):
    def __init__(self, P_mean=-1.2, P_std=1.2, sigma_data=0.5, n_feats=80, loss_type="base"):
        super().__init__()
        self.P_mean, self.P_std, self.sigma_data, self.n_feats, self.loss_type = P_mean, P_std, sigma_data, n_feats, loss_type

    @torch.no_grad()
    def forward(self, precond_model, x0, mask, mu, *dex_args, spk=None, mask_ratio=0, rnd_normal=None, eps=None, batched=False):
        """GeDEX: ``forward(precond_model, x0, mask, mu, spk=None, mask_ratio=0)``; DEX: ``forward(precond_model, x0, mask, mu,
        ref, ref_lengths, sty, sty_lengths, spk=None, mask_ratio=0)``.  ``precond_model`` is the owning ``Diffusion``'s
        ``precond_model`` (it carries the engine hook); ``rnd_normal`` / ``eps`` inject the two draws (tests), otherwise they
        come from the device generator exactly as in the reference.  ``batched``: one ``denoise_batch`` call with the B noise levels
        on the device instead of a host read and B calls at B = 1 (same draws, same weighting; the network's arithmetic is that of
        a batch-B evaluation, so the value agrees with the looped one to the kernels' single-call bound, not bit for bit)."""
        if mask_ratio:
            raise NotImplementedError("mask_ratio > 0 (DiT token masking, dit.py:145-163) is unreachable with the shipped configs and not built")
        if any(t is not None and torch.is_tensor(t) and t.requires_grad for t in (x0, mu)):
            raise RuntimeError("EDMLoss here is forward-only (the HIP score network has no backward); train with the reference module")
        denoise = getattr(precond_model, "_denoise_once", None)
        if denoise is None:
            raise TypeError("precond_model must be dex_tts_amd.diffusion.Diffusion.precond_model")
        ref = ref_lengths = sty = sty_lengths = None
        if dex_args:
            if len(dex_args) != 4:
                raise TypeError("DEX: forward(precond_model, x0, mask, mu, ref, ref_lengths, sty, sty_lengths, ...)")
            ref, ref_lengths, sty, sty_lengths = dex_args
        B = x0.shape[0]
        if rnd_normal is None:
            rnd_normal = torch.randn([B, 1, 1], device=x0.device)                 # edm.py:33
        sigma = (rnd_normal.to(x0.device) * self.P_std + self.P_mean).exp()
        weight = loss_weight(sigma, self.loss_type, self.sigma_data)
        if eps is None:
            eps = torch.randn_like(x0)                                            # edm.py:65
        n = (eps.to(x0.device) + mu) * sigma
        xn = x0 + n
        if batched:
            denoise_b = getattr(precond_model, "_denoise_batch", None)
            if denoise_b is None:
                raise TypeError("precond_model must be dex_tts_amd.diffusion.Diffusion.precond_model")
            kw = {}
            if ref is not None:
                kw = dict(ref=ref, sty=sty, sty_lengths=sty_lengths)
            if spk is not None:
                kw["spk"] = spk
            D_yn = denoise_b(xn, sigma, mask, mu, **kw)
            return torch.sum(weight * ((D_yn - x0) ** 2)) / torch.sum(mask * self.n_feats)      # edm.py:66
        sig_host = sigma.reshape(B).tolist()                                       # one host read: each utterance has its own sigma
        rows = []
        for b in range(B):
            kw = {}
            if ref is not None:
                kw = dict(ref=[r[b:b + 1] for r in ref], sty=sty[b:b + 1], sty_lengths=sty_lengths[b:b + 1])
            if spk is not None:
                kw["spk"] = spk[b:b + 1]
            rows.append(denoise(xn[b:b + 1], sig_host[b], mask[b:b + 1], mu[b:b + 1], **kw))
        D_yn = torch.cat(rows, 0)
        return torch.sum(weight * ((D_yn - x0) ** 2)) / torch.sum(mask * self.n_feats)          # edm.py:66


# ---- the general ablation_sampler (GeDEX-TTS/model/edm.py:109-216, DEX :104-211) ----------------------------------------------------
# Every time-step discretisation, noise schedule, scaling schedule, solver, alpha and range its signature selects.  The host turns the
# arguments into fp32 tables once (ablation_tables: cached per argument tuple); the device runs the sampler from them (dex_sample with
# DexSampleArgs.tables, include/dex_amd.h).  The scalar arithmetic below repeats the reference's: torch CPU fp32 operations on 0-dim
# tensors, one rounding per operation, with Python / numpy float64 scalars exactly where the reference has them.
#
# solver 'dpmpp_2m' is NOT in the reference: DPM-Solver++(2M) (Lu et al. 2022, arXiv:2211.01095, algorithm 2 with the data
# prediction model), a two-step multistep exponential integrator in the (x, sigma) frame that reuses the previous step's denoised
# output - second order at ONE network evaluation per step.  It runs on the noise levels of any discretisation; its rows are
# computed in float64 from the fp32 levels and rounded once (_dpmpp_2m_rows).

TABLES_SCALED, TABLES_CHURN = 1, 2        # DEX_TABLES_* of include/dex_amd.h


def _vp_sigma(beta_d, beta_min):
    """The VP schedule's noise level: sigma(t) = (e^(beta_d t^2 / 2 + beta_min t) - 1)^(1/2)."""
    def sigma(t):
        expo = 0.5 * beta_d * (t ** 2) + beta_min * t
        return (math.e ** expo - 1) ** 0.5
    return sigma


def _vp_sigma_inv(beta_d, beta_min):
    """Its inverse: t(sigma) = ((beta_min^2 + 2 beta_d ln(sigma^2 + 1))^(1/2) - beta_min) / beta_d."""
    def inv(sig):
        root = (beta_min ** 2 + 2 * beta_d * (sig ** 2 + 1).log()).sqrt()
        return (root - beta_min) / beta_d
    return inv


@functools.lru_cache(maxsize=8, typed=True)
def _iddpm_levels(M, C_1, C_2):
    """iDDPM's M + 1 noise levels (cosine alpha-bar): u_M = 0 and, for j = M .. 1 in that order, in fp32,
    u_{j-1} = ((u_j^2 + 1) / max(abar(j - 1) / abar(j), C_1) - 1)^(1/2)."""
    def abar(j):                                   # j: a 0-dim int64 tensor; the arithmetic is fp32
        return (0.5 * np.pi * j / M / (C_2 + 1)).sin() ** 2
    u = torch.zeros(M + 1)
    for j in torch.arange(M, 0, -1):
        ratio = (abar(j - 1) / abar(j)).clip(min=C_1)
        u[j - 1] = ((u[j] ** 2 + 1) / ratio - 1).sqrt()
    return u


class AblationTables:
    """The fp32 tables of one ablation_sampler configuration, laid out as DexSamplerTables: ``sigma`` [E + 1] (the noise level of
    every network evaluation, then 0; E = n_steps for Euler and DPM-Solver++(2M), 2 n_steps - 1 for Heun), ``coef`` [E, 8] (sigma,
    s, A, Bc, h, alpha h, w0, w1; for 'dpmpp_2m': sigma, 1, a, b, c, 0, 0, 0), ``step`` [n_steps, 4] (r, k, c0 on row 0, 0).  ``flags``: DEX_TABLES_*; ``noise``: some step's k is not 0, so the
    per-step randn_like draws change the result."""

    def __init__(self, solver, n_steps, sigma, coef, step, flags, noise):
        self.solver, self.n_steps = solver, n_steps
        self.sigma, self.coef, self.step = sigma, coef, step
        self.flags, self.noise = flags, noise
        self._dev = {}

    @classmethod
    def from_arrays(cls, solver, n_steps, coef, step, scaled):
        """Tables from their coef [E, 8] and step [n_steps, 4] arrays; the flags and the noise flag follow from the values."""
        coef, step = torch.as_tensor(coef, dtype=torch.float32), torch.as_tensor(step, dtype=torch.float32)
        sig = torch.cat([coef[:, 0], torch.zeros(1)])
        noise = bool((step[:, 1] != 0).any())
        churn = noise or bool((step[:, 0] != 1).any())
        flags = (TABLES_SCALED if scaled else 0) | (TABLES_CHURN if churn else 0)
        return cls(solver, n_steps, sig, coef, step, flags, noise)

    @property
    def n_rows(self) -> int:
        return int(self.coef.shape[0])

    def to(self, device):
        """(sigma, coef, step) on ``device``, copied once per device."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device) for t in (self.sigma, self.coef, self.step))
        return self._dev[key]


def _dpmpp_2m_rows(sigma):
    """The (a, b, c) of x_{i+1} = a x_i + b D_i + c D_{i-1} for the fp32 noise levels sigma_0 > ... > sigma_{n-1} (> 0; sigma_n = 0),
    in float64:  h_i = ln(sigma_i / sigma_{i+1}), r_i = h_{i-1} / h_i, e_i = -expm1(-h_i);  a = sigma_{i+1} / sigma_i,
    b = e_i (1 + 1 / (2 r_i)), c = -e_i / (2 r_i);  first row: first order (b = e_0, c = 0);  last row (sigma -> 0): (0, 1, 0)."""
    sg = np.asarray(sigma, dtype=np.float64)
    n = len(sg)
    if not (np.all(sg > 0) and np.all(np.diff(sg) < 0)):
        raise ValueError("dpmpp_2m needs strictly decreasing positive noise levels (this discretisation repeats one at this num_steps)")
    rows, h_prev = [], None
    for i in range(n - 1):
        h = np.log(sg[i] / sg[i + 1])
        e = -np.expm1(-h)
        if i == 0:
            b, c = e, 0.0
        else:
            r = h_prev / h
            b, c = e * (1 + 1 / (2 * r)), -e / (2 * r)
        rows.append((sg[i + 1] / sg[i], b, c))
        h_prev = h
    rows.append((0.0, 1.0, 0.0))
    return rows


@functools.lru_cache(maxsize=64, typed=True)
def ablation_tables(num_steps, solver, discretization, schedule, scaling, sigma_min=None, sigma_max=None, rho=7, epsilon_s=1e-3,
                    C_1=0.001, C_2=0.008, M=1000, alpha=1, S_churn=0, S_min=0, S_max=float("inf"), S_noise=1) -> AblationTables:
    """Everything the device needs for ``ablation_sampler(..., num_steps, solver, discretization, schedule, scaling, ...)``
    (edm.py:109-216), computed on the CPU in fp32 in the reference's operation order; cached per argument tuple.

    Row e of ``coef`` belongs to network evaluation e at time t (t_hat_i for step i's Euler / predictor evaluation, t'_i = t_hat_i +
    alpha h_i for its corrector): sigma(t), s(t), A = sigma'(t)/sigma(t) + s'(t)/s(t), Bc = sigma'(t) s(t)/sigma(t), h_i = t_{i+1} -
    t_hat_i, alpha h_i, w0 = 1 - 1/(2 alpha), w1 = 1/(2 alpha).  Row i of ``step``: r = s(t_hat)/s(t_cur) and k = (max(sigma(t_hat)^2
    - sigma(t_cur)^2, 0))^(1/2) s(t_hat) S_noise of x_hat = r x_cur + k randn_like(x_cur) (edm.py:196), and on row 0 c0 = sigma(t_0)
    s(t_0) of x_0 = latents c0.  The network's range is the library EDMPrecond's, sigma_min = 0 and sigma_max = inf (edm.py:77-78).

    ``solver='dpmpp_2m'`` (not in the reference): any discretisation and range - only the noise levels matter - with schedule
    'linear', scaling 'none' and S_churn = 0 (the exponential integrator does not depend on the schedule, and fresh noise would
    invalidate its history); ``alpha`` is ignored.  Row i of ``coef`` is [sigma_i, 1, a, b, c, 0, 0, 0] (_dpmpp_2m_rows)."""
    if solver not in ("euler", "heun", "dpmpp_2m"):
        raise ValueError(f"solver must be 'euler', 'heun' or 'dpmpp_2m', got {solver!r}")
    if discretization not in ("vp", "ve", "iddpm", "edm"):
        raise ValueError(f"discretization must be 'vp', 've', 'iddpm' or 'edm', got {discretization!r}")
    if schedule not in ("vp", "ve", "linear"):
        raise ValueError(f"schedule must be 'vp', 've' or 'linear', got {schedule!r}")
    if scaling not in ("vp", "none"):
        raise ValueError(f"scaling must be 'vp' or 'none', got {scaling!r}")
    n = int(num_steps)
    if n < 2:
        raise ValueError("num_steps must be >= 2 (the reference divides by num_steps - 1)")
    if solver == "dpmpp_2m":
        if schedule != "linear" or scaling != "none":
            raise ValueError("dpmpp_2m runs in the (x, sigma) frame: schedule must be 'linear' and scaling 'none' (the exponential "
                             f"integrator is the same under every schedule), got {schedule!r} / {scaling!r}")
        if S_churn != 0:
            raise ValueError("dpmpp_2m is a multistep solver: S_churn must be 0 (fresh noise invalidates the previous step's output)")

    # the range: the discretisation's defaults, clamped to what the network supports (edm.py:124-134)
    if sigma_min is None:
        sigma_min = {"vp": _vp_sigma(19.9, 0.1)(epsilon_s), "ve": 0.02, "iddpm": 0.002, "edm": 0.002}[discretization]
    if sigma_max is None:
        sigma_max = {"vp": _vp_sigma(19.9, 0.1)(1), "ve": 100, "iddpm": 81, "edm": 80}[discretization]
    sigma_min, sigma_max = max(sigma_min, 0), min(sigma_max, float("inf"))
    # the VP betas that put sigma(epsilon_s) = sigma_min and sigma(1) = sigma_max: numpy float64 (edm.py:137-138)
    log_min, log_max = np.log(sigma_min ** 2 + 1), np.log(sigma_max ** 2 + 1)
    beta_d = 2 * (log_min / epsilon_s - log_max) / (epsilon_s - 1)
    beta_min = log_max - 0.5 * beta_d

    # noise levels of the steps (edm.py:141-157)
    idx = torch.arange(n)
    if discretization == "vp":
        sigma_steps = _vp_sigma(beta_d, beta_min)(1 + idx / (n - 1) * (epsilon_s - 1))
    elif discretization == "ve":
        t_ve = (sigma_max ** 2) * ((sigma_min ** 2 / sigma_max ** 2) ** (idx / (n - 1)))
        sigma_steps = t_ve.sqrt()
    elif discretization == "iddpm":
        u = _iddpm_levels(M, C_1, C_2)
        u = u[torch.logical_and(u >= sigma_min, u <= sigma_max)]
        pick = ((len(u) - 1) / (n - 1) * idx).round().to(torch.int64)          # round half to even
        sigma_steps = u[pick]
    else:
        top, bottom = sigma_max ** (1 / rho), sigma_min ** (1 / rho)
        sigma_steps = (top + idx / (n - 1) * (bottom - top)) ** rho

    # sigma(t), sigma'(t), t(sigma) of the schedule and s(t), s'(t) of the scaling (edm.py:159-181).  Where the reference has the
    # Python ints 1 / 0 (linear sigma', the 'none' scaling) they stay ints: they leave the fp32 operations they meet unrounded.
    if schedule == "vp":
        sigma, sigma_inv = _vp_sigma(beta_d, beta_min), _vp_sigma_inv(beta_d, beta_min)

        def sigma_d(t):
            return 0.5 * (beta_min + beta_d * t) * (sigma(t) + 1 / sigma(t))
    elif schedule == "ve":
        def sigma(t):
            return t.sqrt()

        def sigma_d(t):
            return 0.5 / t.sqrt()

        def sigma_inv(sig):
            return sig ** 2
    else:
        def sigma(t):
            return t

        def sigma_d(t):
            return 1

        def sigma_inv(sig):
            return sig
    if scaling == "vp":
        def s(t):
            return 1 / (1 + sigma(t) ** 2).sqrt()

        def s_d(t):
            return -sigma(t) * sigma_d(t) * (s(t) ** 3)
    else:
        def s(t):
            return 1

        def s_d(t):
            return 0

    # time steps t_i = t(sigma_i) (the library's EDMPrecond.round_sigma is the identity), t_N = 0 (edm.py:184-185)
    t_steps = torch.cat([sigma_inv(sigma_steps), torch.zeros(1)])
    if solver == "dpmpp_2m":
        sg = t_steps[:n].to(torch.float32)                                    # (linear schedule: t IS sigma)
        coef = torch.zeros(n, 8, dtype=torch.float32)
        coef[:, 0], coef[:, 1] = sg, 1
        coef[:, 2:5] = torch.tensor(_dpmpp_2m_rows(sg.numpy()), dtype=torch.float64).to(torch.float32)
        step = torch.zeros(n, 4, dtype=torch.float32)
        step[:, 0], step[0, 2] = 1, sg[0]
        return AblationTables.from_arrays(solver, n, coef, step, False)
    heun = solver == "heun"
    w0, w1 = (1 - 1 / (2 * alpha), 1 / (2 * alpha)) if heun else (0.5, 0.5)

    def row(t, h):
        sg, st, dsg = sigma(t), s(t), sigma_d(t)
        return [sg, st, dsg / sg + s_d(t) / st, dsg * st / sg, h, alpha * h, w0, w1]

    rows, steps = [], []
    for i in range(n):                                                        # edm.py:190-214
        t_cur, t_next = t_steps[i], t_steps[i + 1]
        sg_cur = sigma(t_cur)
        gamma = min(S_churn / n, np.sqrt(2) - 1) if S_min <= sg_cur <= S_max else 0
        t_hat = sigma_inv(sg_cur + gamma * sg_cur)
        k = (sigma(t_hat) ** 2 - sg_cur ** 2).clip(min=0).sqrt() * s(t_hat) * S_noise
        c0 = sigma(t_steps[0]) * s(t_steps[0]) if i == 0 else 0
        steps.append([s(t_hat) / s(t_cur), k, c0, 0])
        h = t_next - t_hat
        rows.append(row(t_hat, h))
        if heun and i < n - 1:
            rows.append(row(t_hat + alpha * h, h))

    def f32(table):
        return torch.stack([torch.stack([torch.as_tensor(v, dtype=torch.float32).reshape(()) for v in r]) for r in table])

    return AblationTables.from_arrays(solver, n, f32(rows), f32(steps), scaling == "vp")


_SAMPLER_ARGS = ("spk", "class_labels", "randn_like", "num_steps", "sigma_min", "sigma_max", "rho", "solver", "discretization", "schedule",
                 "scaling", "epsilon_s", "C_1", "C_2", "M", "alpha", "S_churn", "S_min", "S_max", "S_noise")
_DEX_ARGS = ("ref", "ref_lengths", "sty", "sty_lengths")
_SAMPLER_DEFAULTS = dict(spk=None, class_labels=None, randn_like=torch.randn_like, num_steps=18, sigma_min=None, sigma_max=None, rho=7,
                         solver="heun", discretization="edm", schedule="linear", scaling="none", epsilon_s=1e-3, C_1=0.001, C_2=0.008,
                         M=1000, alpha=1, S_churn=0, S_min=0, S_max=float("inf"), S_noise=1, ref=None, ref_lengths=None, sty=None,
                         sty_lengths=None)
_TABLE_ARGS = ("sigma_min", "sigma_max", "rho", "epsilon_s", "C_1", "C_2", "M", "alpha", "S_churn", "S_min", "S_max", "S_noise")


def _owner_of(net):
    from .diffusion import _Precond
    if not isinstance(net, _Precond):
        raise TypeError("net must be the precond_model of a dex_tts_amd.diffusion.Diffusion (the score network runs in libdexamd.so)")
    owner = net._owner() if net._owner is not None else None
    if owner is None:
        raise RuntimeError("precond_model has no live owner (it belongs to a dex_tts_amd.diffusion.Diffusion)")
    return owner


@torch.no_grad()
def ablation_sampler(net, latents, mask=None, mu=None, *args, **kwargs):
    """The reference's ``ablation_sampler`` (GeDEX-TTS/model/edm.py:109-216, DEX-TTS :104-211) on the device, with its full signature
    in the argument order of the net's tree:
        GeDEX: ablation_sampler(net, latents, mask, mu, spk, class_labels, randn_like, num_steps, sigma_min, sigma_max, rho, solver,
                                discretization, schedule, scaling, epsilon_s, C_1, C_2, M, alpha, S_churn, S_min, S_max, S_noise)
        DEX:   ablation_sampler(net, latents, mask, mu, ref, ref_lengths, sty, sty_lengths, spk, class_labels, ...)
    and the reference's defaults (solver 'heun', 18 steps, edm / linear / none).  ``net`` must be a library ``Diffusion``'s
    ``precond_model``; ``class_labels`` is accepted and unused, as in the reference.  ``randn_like(latents)`` is called once per step,
    in the reference's order, when the noise term of some step is not zero (S_churn > 0, or a schedule whose t(sigma(t)) round trip
    moves t); the draws are handed to the device."""
    owner = _owner_of(net)
    names = (_DEX_ARGS if owner.cfg.variant == "dex" else ()) + _SAMPLER_ARGS
    if len(args) > len(names):
        raise TypeError(f"ablation_sampler() takes at most {4 + len(names)} positional arguments")
    a = dict(_SAMPLER_DEFAULTS)
    a.update(zip(names, args))
    for k, v in kwargs.items():
        if k not in names:
            raise TypeError(f"ablation_sampler() got an unexpected keyword argument {k!r}")
        if k in names[:len(args)]:
            raise TypeError(f"ablation_sampler() got multiple values for argument {k!r}")
        a[k] = v
    if mask is None or mu is None:
        raise ValueError("mask and mu are required: the score network is conditioned on them")
    tab = ablation_tables(a["num_steps"], a["solver"], a["discretization"], a["schedule"], a["scaling"], **{k: a[k] for k in _TABLE_ARGS})
    return owner._sample_tables(latents, mask, mu, tab, a["randn_like"], spk=a["spk"], ref=a["ref"], sty=a["sty"],
                                sty_lengths=a["sty_lengths"])
