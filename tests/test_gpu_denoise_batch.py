"""GPU: dex_denoise_batch - EDMPrecond.forward with a noise level per utterance in ONE network evaluation - against the CPU oracle
called with the same [B] sigma, in all four arithmetic modes, and the Python layers built on it (precond_model.forward,
EDMLoss / Diffusion.forward / loss_value with batched=True).

Bounds are the single-call bounds of dex_tts_amd/tolerances.py (row b of the batched call is one EDMPrecond evaluation at sigma_b).

Every comparison records its measured error where the other parity tests do (tests/gpu_util.py record, tags "dbatch_*"); the worst
values over the fifteen cases, measured on one MI355X, are in DESIGN.md section 4.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from dex_tts_amd import _lib
from dex_tts_amd.tolerances import FP32_CALL_REL, LOWP
from oracle import dex_oracle as O
from tests import gpu_util as U

pytestmark = pytest.mark.gpu

LEVELS = [80.0, 1.0, 0.002, 0.7, 20.0, 0.05, 4.0, 0.2]          # the sampler's range; 80 / 1 / 0.002 are the goldens' levels


def sigmas(B):
    if B == 2:
        return torch.tensor([80.0, 0.002])
    return torch.tensor([LEVELS[b % len(LEVELS)] for b in range(B)])


def ragged(B, T):
    return [T if b == 0 else max(4, (T * (3 + (7 * b) % 11)) // 14) for b in range(B)]


def case_kw(name, B, T):
    kw = dict(B=B, T=T, lengths=ragged(B, T))
    if name.startswith("dex"):
        Ts = 40 if T < 512 else 96
        kw.update(Tr=37 if T < 512 else 96, Ts=Ts, sty_lengths=[Ts if b == 0 else max(3, (Ts * (2 + (5 * b) % 9)) // 11) for b in range(B)])
    return kw


SHAPES = [(2, 36), (3, 100), (8, 64), (32, 64), (3, 512)]
CASES = [(name, B, T if not (name.startswith("dex") and T == 36) else 52) for name in ("gedex_lj", "gedex_vctk", "dex_vctk") for B, T in SHAPES]
_REF = {}


def inputs(name, B, T):
    cfg, eng, w = U.engine_for(name)
    case = U.make_case(cfg, **case_kw(name, B, T))
    mu, mask, eps = (torch.from_numpy(case[k]) for k in ("mu", "mask", "eps"))
    sig = sigmas(B)
    x = mu + sig.reshape(-1, 1, 1) * eps
    return cfg, eng, w, case, x, sig, mask, mu


def oracle(name, B, T):
    if (name, B, T) not in _REF:
        cfg, eng, w, case, x, sig, mask, mu = inputs(name, B, T)
        with torch.no_grad():
            _REF[(name, B, T)] = O.edm_precond(O.as_torch(w, torch.float32), cfg, x, sig, mask, mu, **U.oracle_kwargs(case)).numpy()
    return _REF[(name, B, T)]


def within(tag, prec, got, ref):
    """The mode's single-call bound; records the measurement first (tests/gpu_util.py record: the parity tests' measurement log)."""
    e = np.abs(got - ref)
    U.record(f"{tag}:{prec}:call", max=e.max(), mean=e.mean(), ref_absmax=np.abs(ref).max())
    print(f"{tag}:{prec}: max {e.max():.3e} mean {e.mean():.3e} |ref|max {np.abs(ref).max():.3f}")
    assert np.isfinite(got).all(), tag
    if prec == "fp32":
        assert e.max() <= FP32_CALL_REL * max(1.0, np.abs(ref).max()), (tag, float(e.max()), float(np.abs(ref).max()))
    else:
        mx, mn = LOWP[prec]["call"]
        assert e.max() <= mx and e.mean() <= mn, (tag, prec, float(e.max()), float(e.mean()))


@pytest.mark.parametrize("name,B,T", CASES)
def test_oracle_per_utterance_levels(name, B, T):
    cfg, eng, w, case, x, sig, mask, mu = inputs(name, B, T)
    ref = oracle(name, B, T)
    try:
        for prec in ("fp32", "bf16", "fp16", "fp16x2"):
            eng.set_precision(prec)
            got = eng.denoise_batch(x, sig, mask, mu, **U.engine_kwargs(case)).cpu().numpy()
            within(f"dbatch_{name}_B{B}_T{T}", prec, got, ref)
    finally:
        eng.set_precision("fp32")


@pytest.mark.parametrize("name", ["gedex_lj", "gedex_vctk", "dex_vctk"])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16", "fp16x2"])
def test_really_per_utterance(name, prec):
    """(a) swapping two levels moves the output far beyond the bound; all levels equal = dex_denoise_once at that level, within the
    bound (bitwise is reported, not required: see DESIGN.md - the same launches run with row_bstride = 1 over B identical rows);
    (b) permuting utterances with their levels, masks and style inputs permutes the output rows bitwise; (c) two runs, same bits."""
    B, T = 3, 100
    cfg, eng, w, case, x, sig, mask, mu = inputs(name, B, T)
    kw = U.engine_kwargs(case)
    eng.set_precision(prec)
    try:
        got = eng.denoise_batch(x, sig, mask, mu, **kw).cpu().numpy()
        again = eng.denoise_batch(x, sig.reshape(B, 1, 1), mask, mu, **kw).cpu().numpy()
        assert np.array_equal(got, again)                                                     # (c), and the [B,1,1] shape
        swapped = sig.clone(); swapped[1], swapped[2] = sig[2], sig[1]      # 1 <-> 0.002 (inputs noised at 80 and read at 0.002 leave fp16's range)
        moved = np.abs(eng.denoise_batch(x, swapped, mask, mu, **kw).cpu().numpy() - got)
        bound = FP32_CALL_REL * max(1.0, np.abs(got).max()) if prec == "fp32" else LOWP[prec]["call"][0]
        assert moved[1].max() > 10 * bound and moved[2].max() > 10 * bound, (float(moved[1].max()), float(moved[2].max()), bound)
        assert np.array_equal(moved[0], np.zeros_like(moved[0]))                              # the utterance whose level stayed keeps its bits
        for s in (80.0, 0.002):                                                               # (a) equal levels = the one-level call
            xs = mu + s * torch.from_numpy(case["eps"])
            one = eng.denoise_once(xs, s, mask, mu, **kw).cpu().numpy()
            same = eng.denoise_batch(xs, torch.full((B,), s), mask, mu, **kw).cpu().numpy()
            print(f"dbatch_equal_{name}_{prec}_sigma{s}: bitwise {np.array_equal(one, same)}")
            within(f"dbatch_equal_{name}_sigma{s}", prec, same, one)
        perm = torch.tensor([2, 0, 1])                                                         # (b)
        kp = {k: ([r[perm] for r in v] if isinstance(v, list) else v[perm]) for k, v in kw.items()}
        gp = eng.denoise_batch(x[perm], sig[perm], mask[perm], mu[perm], **kp).cpu().numpy()
        assert np.array_equal(gp, got[perm.numpy()])
    finally:
        eng.set_precision("fp32")


def _loss_model(name, B, T, lengths, dex_dims):
    from dex_tts_amd import config as Cf, synth
    from dex_tts_amd.diffusion import from_config
    from oracle.make_golden_loss import case_inputs
    cfg, mu, mask, x0, kw = case_inputs(name, B, T, lengths, dex_dims)
    m = from_config(cfg)
    w = synth.make_weights(Cf.param_shapes(cfg), seed=0)
    sd = {}
    for k, v in w.items():
        sd[f"denoise_fn.{k}"] = torch.from_numpy(v); sd[f"precond_model.model.{k}"] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return cfg, m.cuda().eval(), mu, mask, x0, kw


def _loss_cases():
    from oracle.make_golden_loss import CASES as LC
    return LC


@pytest.mark.parametrize("name,B,T,lengths,dex_dims,seed", _loss_cases())
def test_batched_loss_matches_the_references_golden(name, B, T, lengths, dex_dims, seed):
    """Diffusion.forward(infer=False, batched=True) on the fixed draws of tests/golden/edm_loss.npz: the reference's own batched
    EDMLoss values, within the relative bound tests/test_edm_loss.py holds the looped path to (2e-5)."""
    from oracle.make_golden_loss import LOSS_TYPES
    G = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "edm_loss.npz")))
    cfg, m, mu, mask, x0, kw = _loss_model(name, B, T, lengths, dex_dims)
    c = lambda a: torch.from_numpy(np.asarray(a)).cuda()
    rnd, eps = c(G[f"{name}_rnd_normal"]), c(G[f"{name}_eps"])
    dex = ([c(r) for r in kw["ref"]], c(kw["ref_lengths"]), c(kw["sty"]), c(kw["sty_lengths"])) if cfg.variant == "dex" else ()
    spk = c(kw["spk"]) if "spk" in kw else None
    for lt in LOSS_TYPES:
        m.loss_fn.loss_type = lt
        got = float(m(c(x0), c(mask), c(mu), *dex, spk=spk, infer=False, batched=True, rnd_normal=rnd, eps=eps))
        want = float(G[f"{name}_{lt}"])
        print(f"dbatch_loss_{name}_{lt}: got {got!r} want {want!r} rel {abs(got - want) / max(1.0, abs(want)):.2e}")
        assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (lt, got, want)
    # the reference's call surface: precond_model(x, sigma[B,1,1], mask, mu, ...) = denoise_batch; a float still takes the one-level call
    sigma = (rnd * 1.2 - 1.2).exp()
    xn = c(x0) + (eps + c(mu)) * sigma
    ekw = {} if not dex else dict(ref=dex[0], sty=dex[2], sty_lengths=dex[3])
    if spk is not None:
        ekw["spk"] = spk
    a = m.precond_model(xn, sigma, c(mask), c(mu), *dex, spk=spk)
    b = m.engine(xn.device).denoise_batch(xn, sigma, c(mask), c(mu), **ekw)
    assert torch.equal(a, b)
    one = m.precond_model(xn, 0.7, c(mask), c(mu), *dex, spk=spk)
    assert torch.equal(one, m.engine(xn.device).denoise_once(xn, 0.7, c(mask), c(mu), **ekw))
    with pytest.raises(NotImplementedError):
        m.precond_model(xn, sigma, c(mask), c(mu), *dex, spk=spk, mask_ratio=0.5)
    with pytest.raises(RuntimeError):
        m.precond_model(xn.clone().requires_grad_(True), sigma, c(mask), c(mu), *dex, spk=spk)


@pytest.mark.parametrize("case", ["gedex_lj", "gedex_vctk", "dex_vctk"])
def test_loss_value_batched_equals_looped(case):
    from tests.test_gpu_loss_value import args, model
    a, kw = args(case)
    loop = model(case).loss_value(*a, **kw)
    bat = model(case).loss_value(*a, batched=True, **kw)
    names = ["dur", "prior", "diff", "vq"][:len(loop)]
    for n, u, v in zip(names, loop, bat):
        if n == "diff":
            rel = abs(float(u) - float(v)) / max(1.0, abs(float(u)))
            print(f"dbatch_loss_value_{case}: looped {float(u)!r} batched {float(v)!r} rel {rel:.2e}")
            assert rel <= 2e-5, (float(u), float(v))
        else:
            assert torch.equal(u, v), n


def test_refusals_workspace_and_taps():
    """DEX_ERR_ARG with a message and nothing enqueued for a null sigma_dev / x_dev, B < 1, a bad T and use_graph = 1; a workspace of
    dex_workspace_bytes(..., n_evals = B) is accepted and one byte less refused; taps copy out after a batched call."""
    name, B, T = "gedex_lj", 3, 100
    cfg, eng, w, case, x, sig, mask, mu = inputs(name, B, T)
    dev = eng.device
    with torch.cuda.device(dev):
        mu_d, mask_d, x_d, sig_d = (t.to(dev).contiguous() for t in (mu, mask.reshape(B, T), x, sig))
        sentinel = torch.full_like(mu_d, 12345.0)
        out = sentinel.clone()
        need = int(eng.lib.dex_workspace_bytes(eng.h, B, T, 0, 0, B))
        ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = (ws.data_ptr() + 255) // 256 * 256

        def call(**over):
            d = _lib.DexDenoiseBatchArgs()
            d.s.B, d.s.T, d.s.n_steps = B, T, 1
            d.s.mu_dev, d.s.mask_dev, d.s.out_dev = mu_d.data_ptr(), mask_d.data_ptr(), out.data_ptr()
            d.s.workspace_dev, d.s.workspace_bytes = base, need
            d.x_dev, d.sigma_dev = x_d.data_ptr(), sig_d.data_ptr()
            for k, v in over.items():
                if k in ("x_dev", "sigma_dev"):
                    setattr(d, k, v)
                else:
                    setattr(d.s, k, v)
            rc = eng.lib.dex_denoise_batch(eng.h, C.byref(d), None)
            torch.cuda.synchronize(dev)
            return rc, (eng.lib.dex_last_error(eng.h) or b"").decode()

        for over in (dict(sigma_dev=None), dict(x_dev=None), dict(B=0), dict(T=T + 1), dict(use_graph=1)):
            rc, msg = call(**over)
            assert rc == -1, (over, rc, msg)                            # DEX_ERR_ARG
            assert msg, over
            assert torch.equal(out, sentinel), over                     # nothing ran
        rc, msg = call(workspace_bytes=need - 1)
        assert rc == -4 and "workspace" in msg and torch.equal(out, sentinel)
        rc, msg = call()
        assert rc == 0, msg
        want = eng.denoise_batch(x, sig, mask, mu)
        assert torch.equal(out, want)
        taps = eng.taps()
        assert "dit_out" in taps and "down0" in taps and taps["mlp"].shape[0] == B and all(torch.isfinite(v).all() for v in taps.values())
        # the per-utterance rows of the time MLP: row b is what a one-level call at sigma_b builds
        eng.denoise_once(x, float(sig[1]), mask, mu)
        assert torch.equal(eng.taps()["mlp"][0], taps["mlp"][1])
