"""Golden values of the reference's own validation ``compute_loss`` (tests/golden/compute_loss.npz): GeDEX-TTS/model/tts.py:58-122 and
DEX-TTS/model/tts.py:76-153, run on the CPU in eval mode under no_grad with the portable synthetic weights and the import recipe of
oracle/make_golden_tts.py.  ``model.monotonic_align`` is the real Cython core, built in a temporary directory as
tools/make_golden_align.build_core does.

Per case the tool seeds ``random`` and torch, runs compute_loss once, and records what the reference drew and computed on the way:
the cut offsets (``random.choice``) and the ``random.random()`` that follows, the two EDM draws (re-derived by re-seeding and checked
against what EDMLoss received), the durations ``attn.sum(-1)``, the decoder's ``y`` (y_cut) and ``mu_y``, the VQ codes and the losses.
The target ``y`` is a noisy walk through the reference's own ``mu_x`` (captured by a first call): the first of a fixed sequence of
walks whose search decisions all clear the margin below.  The library's ``mu_x`` differs from the reference's by ~2e-5, so a case
whose smallest MAS decision margin (tests/mas_restatement.py) in the recorded run is below 1e-2 is refused rather than written.

    python tools/make_golden_compute_loss.py          # writes tests/golden/compute_loss.npz
"""
from __future__ import annotations

import contextlib
import io
import os
import random
import sys
import tempfile

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dex_tts_amd import config as C, synth  # noqa: E402
from oracle import make_golden_tts as GT  # noqa: E402
from tests import mas_restatement as R  # noqa: E402
import make_golden_align  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "compute_loss.npz")
MIN_MARGIN = 1e-2
# DEX-VCTK: with the synthetic weights the style-conditioned mu_x columns lie close together and no target reaches 1e-2 (the best of
# 200 walks is ~1e-4 relative, ~0.7 absolute at |Q| ~ 7e3, against a log-prior error of ~1e-3 per cell); the floor is lowered for it
MIN_MARGIN_DEX = 1e-4
# name -> (tree, YAML, n_spks, token lengths, y lengths, Ty, out_size, seed)
CASES = {
    "gedex_lj": ("GeDEX-TTS", "config/LJSpeech/base.yaml", 1, [23, 15, 9], [100, 70, 40], 100, 64, 101),
    "gedex_vctk": ("GeDEX-TTS", "config/VCTK/base.yaml", 108, [19, 11], [80, 57], 80, None, 102),
    "dex_vctk": ("DEX-TTS", "config/VCTK/base.yaml", 0, [17, 12], [88, 60], 88, 48, 103),
}
DEX_STYLE = dict(ref=(48, [48, 35], 99), sty=(40, [40, 29], 199), lf0_lengths=[40, 33])


def build_model(sub, yml, n_spks, core):
    m = yaml.safe_load(open(f"/root/reference/{sub}/{yml}"))["model"]
    cfg = GT.to_attr(dict(m, n_vocab=GT.N_VOCAB, n_spks=n_spks))
    tts = GT.import_tts(sub)

    def maximum_path(value, mask):       # the reference wrapper's semantics around the real core: value * mask, lengths from the mask
        v = (value * mask).numpy().astype(np.float32)
        mk = mask.numpy()
        path = np.zeros(v.shape, np.int32)
        core.maximum_path_c(path, np.ascontiguousarray(v), mk.sum(1)[:, 0].astype(np.int32), mk.sum(2)[:, 0].astype(np.int32))
        return torch.from_numpy(path).to(dtype=value.dtype)

    sys.modules["model.monotonic_align"].maximum_path = maximum_path
    with contextlib.redirect_stdout(io.StringIO()):
        model = (tts.DeXTTS if sub == "DEX-TTS" else tts.GeDEXTTS)(cfg).eval()
    c = model.encoder.encoder.config
    for k, v in dict(use_cache=True, output_retentions=False, output_hidden_states=False).items():
        if not hasattr(c, k):
            setattr(c, k, v)
    sd = model.state_dict()        # the weights of oracle/make_golden_tts.py, sub-module by sub-module
    new = {}
    tw = synth.make_text_weights({k[len("encoder."):]: list(v.shape) for k, v in sd.items() if k.startswith("encoder.")})
    for k in ("encoder.retnet_rel_pos.angle", "encoder.retnet_rel_pos.decay"):
        tw[k] = sd["encoder." + k].numpy().copy()
    new.update({"encoder." + k: v for k, v in tw.items()})
    scfg = C.dex_vctk() if sub == "DEX-TTS" else (C.gedex_vctk() if n_spks > 1 else C.gedex_lj())
    for k, v in synth.make_weights(C.param_shapes(scfg)).items():
        new["decoder.denoise_fn." + k] = v
        new["decoder.precond_model.model." + k] = v
    if n_spks > 1:
        new["spk_emb.weight"] = synth.normalish("spk_emb", tuple(sd["spk_emb.weight"].shape), 2)
    if sub == "DEX-TTS":
        new.update(synth.make_style_weights({k: list(v.shape) for k, v in sd.items()
                                             if k.split(".")[0] in ("tv_encoder", "lf0_encoder", "tiv_encoder", "conv_sty")}))
    assert set(sd) == set(new), sorted(set(sd) ^ set(new))[:6]
    model.load_state_dict({k: torch.as_tensor(v) for k, v in new.items()}, strict=True)
    return model, tts


def y_from_mu(mu, x_len, y_len, Ty, seed):
    """A mel-like target: each row walks through its tokens' mu columns with random durations, plus noise; 0 past y_len."""
    rng = np.random.default_rng(seed)
    B, F, _ = mu.shape
    y = np.zeros((B, F, Ty), np.float32)
    for b in range(B):
        d = rng.multinomial(y_len[b] - x_len[b], np.ones(x_len[b]) / x_len[b]) + 1
        idx = np.repeat(np.arange(x_len[b]), d)
        y[b, :, :y_len[b]] = mu[b][:, idx] + rng.standard_normal((F, y_len[b])).astype(np.float32) * 0.3
    return y


@torch.no_grad()
def run(name, core):
    sub, yml, n_spks, xl, yl, Ty, out_size, seed = CASES[name]
    model, tts = build_model(sub, yml, n_spks, core)
    B = len(xl)
    tok, x_len = synth.make_text_inputs(B, max(xl), xl, GT.N_VOCAB)
    x, x_lengths = torch.from_numpy(tok), torch.from_numpy(x_len)
    y_lengths = torch.tensor(yl, dtype=torch.int64)
    out = {"tokens": tok, "x_lengths": x_len, "y_lengths": np.asarray(yl, np.int64), "out_size": np.int64(out_size or 0), "seed": np.int64(seed)}
    extra, kw = (), {}
    if sub == "DEX-TTS":
        Tr, rl, rs = DEX_STYLE["ref"]
        Ts, sl, ss = DEX_STYLE["sty"]
        ref, _, ref_len = synth.make_style_inputs(B, Tr, rl, rs)
        sty, lf0, sty_len = synth.make_style_inputs(B, Ts, sl, ss)
        lf0_len = np.asarray(DEX_STYLE["lf0_lengths"], np.int64)
        out.update(ref=ref, ref_lengths=ref_len, sty=sty, sty_lengths=sty_len, lf0=lf0, lf0_lengths=lf0_len)
        extra = tuple(torch.from_numpy(a) for a in (ref, ref_len, sty, sty_len, lf0, lf0_len))
    elif n_spks > 1:
        spk = np.array([3, 77][:B], np.int64)
        out["spk"] = spk
        kw["spk"] = torch.from_numpy(spk)

    cap = {}
    hooks = [model.encoder.register_forward_hook(lambda m, a, o: cap.update(mu_x=o[0].clone(), logw=o[1].clone())),
             model.decoder.register_forward_pre_hook(lambda m, a: cap.__setitem__("dec", tuple(t.clone() for t in a[:3])))]
    # pass 1: the reference's mu_x (it does not depend on y), then the target built from it
    random.seed(seed)
    torch.manual_seed(seed)
    model.compute_loss(x, x_lengths, torch.zeros(B, 80, Ty), y_lengths, *extra, out_size=out_size, **kw)
    mu = cap["mu_x"].numpy()
    floor = MIN_MARGIN_DEX if sub == "DEX-TTS" else MIN_MARGIN
    best = (-1.0, seed)
    for y_seed in range(seed, seed + 200):       # the first target whose every search decision clears the floor, else the best one
        lp = make_golden_align.log_prior_ref(mu, y_from_mu(mu, x_len, yl, Ty, y_seed))
        best = max(best, (min(R.min_margin(lp[b], int(x_len[b]), int(yl[b])) for b in range(B)), y_seed))
        if best[0] >= floor:
            break
    y_seed = best[1]
    y = y_from_mu(mu, x_len, yl, Ty, y_seed)
    out.update(y=y, y_seed=np.int64(y_seed))
    if sub == "DEX-TTS":         # the VQ's input z_beforeVQ and mask (ref_encoder.py:201-204)
        hooks.append(model.tv_encoder.vq.register_forward_pre_hook(lambda m, a: cap.update(vq_x=a[0].clone(), vq_mask=a[1].clone())))
    # pass 2, recorded: the draws (random.choice for the offsets, randn / randn_like in EDMLoss), the search, the VQ codes
    rec = {"choice": [], "randn": []}
    real_choice, real_randn, real_randn_like, real_emb = random.choice, torch.randn, torch.randn_like, torch.nn.functional.embedding

    def choice(seq):
        v = real_choice(seq)
        rec["choice"].append((len(seq), v))
        return v

    def randn(*a, **k):
        t = real_randn(*a, **k); rec["randn"].append(t.clone()); return t

    def randn_like(*a, **k):
        t = real_randn_like(*a, **k); rec["randn"].append(t.clone()); return t

    def embedding(inp, weight, *a, **k):
        if sub == "DEX-TTS" and weight is model.tv_encoder.vq.embedding:
            rec["vq_idx"] = inp.clone()
        return real_emb(inp, weight, *a, **k)

    real_mp = sys.modules["model.monotonic_align"].maximum_path

    def mp(value, mask):
        rec["log_prior"], rec["mask"] = value.clone(), mask.clone()
        p = real_mp(value, mask)
        rec["attn"] = p.clone()
        return p

    sys.modules["model.monotonic_align"].maximum_path = mp
    random.choice, torch.randn, torch.randn_like, torch.nn.functional.embedding = choice, randn, randn_like, embedding
    try:
        random.seed(seed)
        torch.manual_seed(seed)
        losses = model.compute_loss(x, x_lengths, torch.from_numpy(y), y_lengths, *extra, out_size=out_size, **kw)
        after = random.random()
    finally:
        random.choice, torch.randn, torch.randn_like, torch.nn.functional.embedding = real_choice, real_randn, real_randn_like, real_emb
        sys.modules["model.monotonic_align"].maximum_path = real_mp
    for h in hooks:
        h.remove()
    # the EDM draws, re-derived by re-seeding: nothing before EDMLoss draws from torch's generator
    y_cut, y_mask, mu_y = cap["dec"]
    torch.manual_seed(seed)
    rnd = torch.randn([B, 1, 1])
    eps = torch.randn_like(y_cut)
    assert len(rec["randn"]) == 2 and torch.equal(rec["randn"][0], rnd) and torch.equal(rec["randn"][1], eps)
    # the offsets: one draw per row with max_offset > 0, in row order
    offsets = np.zeros(B, np.int64)
    rows = [b for b in range(B) if out_size is not None and out_size < Ty and yl[b] > out_size]
    assert len(rec["choice"]) == len(rows)
    for b, (n, v) in zip(rows, rec["choice"]):
        assert n == yl[b] - out_size
        offsets[b] = v
    # the margin of every row's search
    lp, mk = rec["log_prior"].numpy(), rec["mask"].numpy()
    margins = [R.min_margin((lp[b] * mk[b]).astype(np.float32), int(x_len[b]), int(yl[b])) for b in range(B)]
    dur = rec["attn"].sum(-1).numpy().astype(np.int32)
    assert (dur == R.durations((lp * mk).astype(np.float32), x_len, yl)).all()
    print(f"{name}: losses {[float(l) for l in losses]} offsets {offsets.tolist()} margins {[f'{m:.3g}' for m in margins]}")
    if min(margins) < floor:
        raise SystemExit(f"{name}: smallest MAS decision margin {min(margins):.3g} < {floor}: refusing to write the case")
    out.update(offsets=offsets, random_after=np.float64(after), rnd_normal=rnd.numpy(), eps=eps.numpy(), dur=dur, y_cut=y_cut.numpy(),
               y_mask=y_mask.numpy(), mu_y=mu_y.numpy(), mu_x=cap["mu_x"].numpy(), logw=cap["logw"].numpy(), min_margin=np.float64(min(margins)),
               angle=model.encoder.encoder.retnet_rel_pos.angle.numpy(), decay=model.encoder.encoder.retnet_rel_pos.decay.numpy())
    if sub == "DEX-TTS":
        out["vq_idx"] = rec["vq_idx"].numpy().astype(np.int32).reshape(B, -1)
        out.update(vq_x=cap["vq_x"].numpy(), vq_mask=cap["vq_mask"].numpy())
    names = ["dur_loss", "prior_loss", "diff_loss", "vq_loss"]
    for n, l in zip(names, losses):
        out[n] = np.float32(l.item())
    return {f"{name}__{k}": v for k, v in out.items()}


def main():
    torch.set_num_threads(8)
    blob = {}
    with tempfile.TemporaryDirectory() as tmp:
        core = make_golden_align.build_core(tmp)
        for name in CASES:
            blob.update(run(name, core))
    np.savez_compressed(OUT, **blob)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB)")


if __name__ == "__main__":
    main()
