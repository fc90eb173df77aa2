"""GPU: loss_value — the reference's validation compute_loss — against tests/golden/compute_loss.npz, and its new kernels
(dex_loss_segment, dex_style_encode_loss) against torch restatements and against themselves."""
import json
import os

import numpy as np
import pytest
import torch

from dex_tts_amd import align, tts
from tests.test_tts_module import full_state_dict, model_cfg

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "compute_loss.npz"))
CASES = ["gedex_lj", "gedex_vctk", "dex_vctk"]
LOSS_REL = 2e-6          # measured on one MI355X: <= 3.7e-7 relative on every case and loss
DEV = "cuda"


def g(case, k):
    return G[f"{case}__{k}"]


def t(case, k, dtype=None):
    v = torch.from_numpy(np.ascontiguousarray(g(case, k))).to(DEV)
    return v if dtype is None else v.to(dtype)


_MODELS = {}


def model(case):
    if case not in _MODELS:
        m = (tts.DeXTTS if case.startswith("dex") else tts.GeDEXTTS)(model_cfg(case))
        sd = full_state_dict(m, case)
        sd["encoder.encoder.retnet_rel_pos.angle"] = torch.from_numpy(g(case, "angle"))
        sd["encoder.encoder.retnet_rel_pos.decay"] = torch.from_numpy(g(case, "decay"))
        m.load_state_dict(sd)
        _MODELS[case] = m.cuda().eval()
    return _MODELS[case]


def args(case):
    a = [t(case, "tokens"), t(case, "x_lengths"), t(case, "y"), t(case, "y_lengths")]
    kw = dict(out_size=int(g(case, "out_size")) or None, offsets=g(case, "offsets"), rnd_normal=t(case, "rnd_normal"), eps=t(case, "eps"))
    if case.startswith("dex"):
        a += [t(case, k) for k in ("ref", "ref_lengths", "sty", "sty_lengths", "lf0", "lf0_lengths")]
    elif f"{case}__spk" in G:
        kw["spk"] = t(case, "spk")
    return a, kw


def by_hand(case):
    """loss_value's chain, stage by public stage."""
    m = model(case)
    a, kw = args(case)
    x, xl, y, yl = a[:4]
    spk = dex = None
    vq = ()
    if case.startswith("dex"):
        ref, rl, sty, sl, lf0, ll = a[4:]
        skips, sty_dec, sty_enc, vq_loss = m.style(ref, rl, sty, sl, lf0, ll, return_vq_loss=True)
        mu_x, logw, _ = m.encoder(x, xl, sty_enc)
        dex, vq = (skips, rl, sty_dec, sl), (vq_loss,)
    else:
        spk = m.spk_emb(kw["spk"]) if "spk" in kw else None
        mu_x, logw, _ = m.encoder(x, xl, spk=spk)
    dur = align.mas_durations(mu_x, xl, y, yl)
    y_cut, mu_y, mask, cl = align.segment(mu_x, dur, y, yl, kw["out_size"], kw["offsets"])
    if kw["out_size"] is None:
        y_cut = y
    dl, pl = align.dur_prior_losses(logw, dur, xl, y_cut, mu_y, cl)
    diff = m.decoder.loss_fn(m.decoder.precond_model, y_cut, mask, mu_y, *(dex or ()), spk=spk, rnd_normal=kw["rnd_normal"], eps=kw["eps"])
    return (dl, pl, diff) + vq, dur, y_cut, mu_y


@pytest.mark.parametrize("case", CASES)
def test_loss_value_matches_reference(case):
    a, kw = args(case)
    got = model(case).loss_value(*a, **kw)
    names = ["dur_loss", "prior_loss", "diff_loss", "vq_loss"][:len(got)]
    errs = {}
    for n, v in zip(names, got):
        assert v.dim() == 0 and v.is_cuda
        ref = float(g(case, n))
        errs[n] = abs(float(v) - ref) / abs(ref)
    print(f"loss_value {case}: rel err " + json.dumps({k: f"{v:.2e}" for k, v in errs.items()}))
    hand, dur, y_cut, mu_y = by_hand(case)
    assert np.array_equal(dur.cpu().numpy(), g(case, "dur"))
    assert np.array_equal(y_cut.cpu().numpy(), g(case, "y_cut"))
    assert all(e <= LOSS_REL for e in errs.values()), errs
    for u, v in zip(got, hand):
        assert torch.equal(u, v)


def _gather(mu, dur, y, yl, S, off):
    """torch restatement of the cut: the frame -> token map from cumulative durations, then plain indexing."""
    B, F, Tx = mu.shape
    yc, mc, mk = (torch.zeros(B, F, S, device=DEV), torch.zeros(B, F, S, device=DEV), torch.zeros(B, 1, S, device=DEV))
    end = torch.cumsum(dur.long(), 1)
    for b in range(B):
        c = min(S, int(yl[b]))
        f = torch.arange(off[b], off[b] + c, device=DEV)
        tok = torch.searchsorted(end[b], f, right=True)
        ok = tok < Tx
        yc[b, :, :c] = y[b, :, off[b]:off[b] + c]
        mc[b, :, :c] = torch.where(ok[None], mu[b][:, tok.clamp(max=Tx - 1)], torch.zeros((), device=DEV))
        mk[b, 0, :c] = 1
    return yc, mc, mk


def _ragged(B, F, Tx, Ty, tx, ty, seed):
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn(B, F, Tx, generator=gen).to(DEV)
    y = torch.randn(B, F, Ty, generator=gen).to(DEV)
    dur = torch.zeros(B, Tx, dtype=torch.int32)
    for b in range(B):
        cuts = torch.sort(torch.randperm(ty[b] - 1, generator=gen)[:tx[b] - 1] + 1).values
        edges = torch.cat([torch.tensor([0]), cuts, torch.tensor([ty[b]])])
        dur[b, :tx[b]] = (edges[1:] - edges[:-1]).int()
    return mu, dur.to(DEV), y


@pytest.mark.parametrize("B,F,Tx,Ty,tx,ty,S", [
    (4, 80, 37, 200, [37, 20, 5, 30], [200, 150, 40, 64], 64),       # cut: rows longer and shorter than out_size
    (3, 80, 25, 90, [25, 10, 3], [90, 50, 12], None),                 # out_size None: S = Ty
    (2, 80, 2048, 8192, [2048, 1500], [8192, 6000], 172),             # the MAS caps
])
def test_segment_matches_torch_gather(B, F, Tx, Ty, tx, ty, S):
    mu, dur, y = _ragged(B, F, Tx, Ty, tx, ty, 7 + B)
    yl = torch.tensor(ty)
    off = align.segment_offsets(yl, S) if S is not None and S < Ty else np.zeros(B, np.int64)
    got = align.segment(mu, dur, y, yl, S, off)
    want = _gather(mu, dur, y, yl, S if S is not None and S < Ty else Ty, off.tolist())
    for u, v in zip(got[:3], want):
        assert torch.equal(u, v)
    assert got[3].tolist() == [min(S or Ty, v) for v in ty]
    for b in range(B):                                                # a row alone: the same bits as in its batch
        one = align.segment(mu[b:b + 1], dur[b:b + 1], y[b:b + 1], yl[b:b + 1], S, off[b:b + 1])
        for u, v in zip(one[:3], got[:3]):
            assert torch.equal(u[0], v[b])


def test_segment_refuses_bad_offsets():
    mu, dur, y = _ragged(1, 80, 5, 40, [5], [40], 1)
    with pytest.raises(ValueError):
        align.segment(mu, dur, y, [40], 16, [25])                     # 25 + 16 > 40


def test_style_encode_loss_leaves_outputs_bitwise():
    m = model("dex_vctk").style
    a = [t("dex_vctk", k) for k in ("ref", "ref_lengths", "sty", "sty_lengths", "lf0", "lf0_lengths")]
    base = m(*a, return_indices=True)
    with_loss = m(*a, return_indices=True, return_vq_loss=True)
    for u, v in zip(base[0], with_loss[0]):
        assert torch.equal(u, v)
    for u, v in zip(base[1:], with_loss[1:4]):
        assert torch.equal(u, v)
    assert np.array_equal(with_loss[3].cpu().numpy(), g("dex_vctk", "vq_idx"))
    again = m(*a, return_vq_loss=True)[-1]
    assert torch.equal(with_loss[4], again)                            # no atomics: the same bits on every run
