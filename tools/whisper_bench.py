#!/usr/bin/env python
"""Time the Whisper ASR score (dex_tts_amd/whisper.py: log-mel front end, encoder, cross-attention K / V, prompt, cached greedy
steps, fp32) on an MI355X, next to the same graph written with torch ops in fp32 with a key/value cache on the same GPU in the same
process - at whisper-base.en and whisper-large-v3 geometry, random weights, 4 s wavs, B in {1, 8, 32}, 48 new tokens with eos
suppressed so that every run does the same work.

    python tools/whisper_bench.py [--models base.en,large-v3] [--batches 1,8,32] [--reps 5] [--warmup 1] [--tokens 48] [--json out.json]

Each timing is a host clock around one call that ends in a device synchronise (the encoder and the cross K / V of the library are
split by events inside its call); the two implementations alternate inside every repetition; medians are printed.  ``prompt`` and
``per token`` are derived: a 1-token and an n-token decode differ by n - 1 steps.  For the step the bytes of the decoder's weights
(read once per token for the whole batch) and of the cross-attention K / V (read once per token per row) are divided by its time.
The second table times one linear of the step alone, the skinny-M streaming kernel against launch_igemm, at M = 1, 8 and 32 rows.

    python tools/whisper_bench.py --long 46 [--batches 1,8] [--reps 5] [--tokens 48]

The long form at whisper-large-v3 geometry, random weights: (a) the per-token time of ``generate`` under the timestamp rule against
plain ``generate`` on the same features with the same forced step count (eos suppressed), the two alternating inside every
repetition, with the run-to-run spread (max - min over the repetitions) of each; (b) one ``generate_segments`` call on wavs of that
many seconds (``--tokens`` new tokens per window at most): its time and window count against the sum of its window calls (gather,
encoder, decode) run one by one, and the long front end alone.

    python tools/whisper_bench.py --beams 5 [--batches 1,6] [--reps 5] [--tokens 48]

Beam search at whisper-large-v3 geometry, random weights, eos suppressed: the per-token time of ``generate_beam`` at U utterances of
K beams against the greedy ``generate`` on U x K independent rows (the same row count, each row with its own cross-attention K / V)
and against the torch graph with a key/value cache where a beam step is ``log_softmax`` + ``topk`` + ``index_select`` of the cache;
the three alternate inside every repetition; medians and the run-to-run spread (max - min) of each.

    python tools/whisper_bench.py --policy [--batches 1,8] [--reps 5] [--tokens 48]

Fallback decoding at whisper-large-v3 geometry, random weights, eos suppressed: per token the plain greedy tail, the policy tail at
T = 0 and at T = 0.4 of the same build, alternating inside every repetition, with their spreads; and one retried window (no encoder)
against a fresh one."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dex_tts_amd import _lib, whisper  # noqa: E402
from tests import whisper_ref as R  # noqa: E402

MODELS = {"base.en": R._cfg(vocab_size=51864, num_mel_bins=80, d_model=512, encoder_layers=6, encoder_attention_heads=8, encoder_ffn_dim=2048,
                            decoder_layers=6, decoder_attention_heads=8, decoder_ffn_dim=2048),
          "large-v3": R.DEFAULT}
PROMPT = (1, 2, 3, 4)
SECONDS = 4
ENC, DEC = R.ENC, R.DEC


def make_weights(cfg, seed, dev):
    """tests/whisper_ref.make_weights' recipe, drawn on the device (the large model has 1.5 G parameters)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    sd = {}
    for k, shape in R.state_dict_shapes(cfg).items():
        if k.endswith(".bias"):
            v = torch.zeros(shape, device=dev)
        elif "layer_norm" in k:
            v = torch.ones(shape, device=dev)
        else:
            a = 1.0 if k == DEC + "embed_positions.weight" else (6.0 if ("q_proj" in k or "k_proj" in k) else 3.0) / float(np.prod(shape[1:])) ** 0.5
            v = (torch.rand(shape, device=dev, generator=g) * 2 - 1) * a
        sd[k] = v
    return sd


def make_wavs(B, seed):
    g = torch.Generator().manual_seed(seed + 1)
    n = SECONDS * 16000
    t = torch.arange(n) / 16000
    f0 = 100 + 100 * torch.rand(B, 1, generator=g)
    x = sum(torch.sin(2 * np.pi * (k + 1) * f0 * t) / (k + 1) for k in range(6)) + 0.05 * torch.randn(B, n, generator=g)
    return (0.1 * x / x.abs().amax(dim=1, keepdim=True)).float()


class TorchWhisper:
    """The same graph in torch ops, fp32, with a key/value cache; nothing travels to the host inside a decode."""

    def __init__(self, cfg, w):
        self.cfg, self.w = cfg, w
        self.win = torch.hann_window(400, periodic=True, device="cuda")
        self.mel = torch.from_numpy(R.mel_filters(cfg.num_mel_bins)).float().cuda()

    def log_mel(self, wavs):
        x = F.pad(wavs, (0, R.n_samples(self.cfg) - wavs.shape[1]))
        p = torch.stft(x, 400, 160, window=self.win, center=True, pad_mode="reflect", return_complex=True)[..., :-1].abs() ** 2
        ls = torch.clamp(self.mel.T @ p, min=1e-10).log10()
        ls = torch.maximum(ls, ls.amax(dim=(1, 2), keepdim=True) - 8.0)
        return (ls + 4.0) / 4.0

    def _proj(self, p, n, x):
        return F.linear(x, self.w[p + n + ".weight"], self.w.get(p + n + ".bias"))

    def _ln(self, x, p):
        return F.layer_norm(x, (self.cfg.d_model,), self.w[p + ".weight"], self.w[p + ".bias"], 1e-5)

    def _heads(self, x, nh):
        return x.reshape(x.shape[0], x.shape[1], nh, -1).transpose(1, 2)

    def encode(self, feat):
        cfg, w = self.cfg, self.w
        x = F.gelu(F.conv1d(feat, w[ENC + "conv1.weight"], w[ENC + "conv1.bias"], padding=1))
        h = F.gelu(F.conv1d(x, w[ENC + "conv2.weight"], w[ENC + "conv2.bias"], stride=2, padding=1)).transpose(1, 2) + w[ENC + "embed_positions.weight"]
        nh = cfg.encoder_attention_heads
        for l in range(cfg.encoder_layers):
            p = f"{ENC}layers.{l}."
            y = self._ln(h, p + "self_attn_layer_norm")
            q, k, v = (self._heads(self._proj(p + "self_attn.", n, y), nh) for n in ("q_proj", "k_proj", "v_proj"))
            a = torch.softmax((q * 0.125) @ k.transpose(2, 3), dim=-1) @ v
            h = h + self._proj(p + "self_attn.", "out_proj", a.transpose(1, 2).reshape(h.shape))
            h = h + self._proj(p, "fc2", F.gelu(self._proj(p, "fc1", self._ln(h, p + "final_layer_norm"))))
        return self._ln(h, ENC + "layer_norm")

    def cross_kv(self, enc):
        nh = self.cfg.decoder_attention_heads
        self.cross = [(self._heads(self._proj(f"{DEC}layers.{l}.encoder_attn.", "k_proj", enc), nh),
                       self._heads(self._proj(f"{DEC}layers.{l}.encoder_attn.", "v_proj", enc), nh)) for l in range(self.cfg.decoder_layers)]
        B = enc.shape[0]
        self.k = torch.zeros(self.cfg.decoder_layers, B, nh, self.cfg.max_target_positions, 64, device="cuda")
        self.v = torch.zeros_like(self.k)

    def step(self, tok, p):
        cfg, w, nh = self.cfg, self.w, self.cfg.decoder_attention_heads
        h = (w[DEC + "embed_tokens.weight"][tok] + w[DEC + "embed_positions.weight"][p])[:, None]
        for l in range(cfg.decoder_layers):
            pl = f"{DEC}layers.{l}."
            y = self._ln(h, pl + "self_attn_layer_norm")
            self.k[l, :, :, p] = self._heads(self._proj(pl + "self_attn.", "k_proj", y), nh)[:, :, 0]
            self.v[l, :, :, p] = self._heads(self._proj(pl + "self_attn.", "v_proj", y), nh)[:, :, 0]
            q = self._heads(self._proj(pl + "self_attn.", "q_proj", y), nh) * 0.125
            a = torch.softmax(q @ self.k[l, :, :, : p + 1].transpose(2, 3), dim=-1) @ self.v[l, :, :, : p + 1]
            h = h + self._proj(pl + "self_attn.", "out_proj", a.transpose(1, 2).reshape(h.shape))
            y = self._ln(h, pl + "encoder_attn_layer_norm")
            q = self._heads(self._proj(pl + "encoder_attn.", "q_proj", y), nh) * 0.125
            ck, cv = self.cross[l]
            a = torch.softmax(q @ ck.transpose(2, 3), dim=-1) @ cv
            h = h + self._proj(pl + "encoder_attn.", "out_proj", a.transpose(1, 2).reshape(h.shape))
            h = h + self._proj(pl, "fc2", F.gelu(self._proj(pl, "fc1", self._ln(h, pl + "final_layer_norm"))))
        return F.linear(self._ln(h, DEC + "layer_norm"), w[DEC + "embed_tokens.weight"])[:, 0]

    def decode(self, B, n_new, mask):
        """Prompt, then n_new greedy tokens under ``mask`` (-inf where suppressed) -> ids [B, n_new] on the device."""
        for p, t in enumerate(PROMPT[:-1]):
            self.step(torch.full((B,), t, device="cuda"), p)
        tok, out = torch.full((B,), PROMPT[-1], device="cuda"), []
        for i in range(n_new):
            tok = torch.argmax(self.step(tok, len(PROMPT) - 1 + i) + mask, dim=-1)
            out.append(tok)
        return torch.stack(out, dim=1)


    def decode_beam(self, U, K, n_new, mask):
        """Beam search as torch users write it: U x K rows, the caches reordered by ``index_select`` every step -> ids [U, n_new]."""
        B = U * K
        for p, t in enumerate(PROMPT[:-1]):
            self.step(torch.full((B,), t, device="cuda"), p)
        tok = torch.full((B,), PROMPT[-1], device="cuda")
        score = torch.tensor([0.0] + [-1e9] * (K - 1), device="cuda").repeat(U)
        seqs, base = torch.zeros(B, 0, dtype=torch.long, device="cuda"), (torch.arange(U, device="cuda") * K)[:, None]
        for i in range(n_new):
            lp = torch.log_softmax(self.step(tok, len(PROMPT) - 1 + i), dim=-1) + mask + score[:, None]
            top, flat = lp.reshape(U, -1).topk(2 * K, dim=1)
            score, parent, tok = top[:, :K].reshape(B), (base + flat[:, :K] // lp.shape[1]).reshape(B), (flat[:, :K] % lp.shape[1]).reshape(B)
            self.k, self.v = self.k.index_select(1, parent), self.v.index_select(1, parent)
            seqs = torch.cat([seqs[parent], tok[:, None]], dim=1)
        return seqs.reshape(U, K, -1)[:, 0]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def med(xs):
    return float(np.median(xs))


def bench_model(name, cfg, batches, reps, warmup, n_tok, seed):
    with torch.no_grad():
        w = make_weights(cfg, seed, "cuda")
        lib = whisper.Whisper(R.library_config(cfg), "cuda").load_state_dict(w)
        ref = TorchWhisper(cfg, w)
        eos = cfg.vocab_size - 1
        spec = whisper.GenerationSpec(PROMPT, (eos,), (eos,), eos)
        mask = torch.zeros(cfg.vocab_size, device="cuda")
        mask[eos] = float("-inf")
        d, Fd, Ld = cfg.d_model, cfg.decoder_ffn_dim, cfg.decoder_layers
        w_bytes = 4 * (Ld * (6 * d * d + 2 * d * Fd) + cfg.vocab_size * d)
        rows = []
        for B in batches:
            wavs = make_wavs(B, seed).cuda()
            kv_bytes = 4 * Ld * B * cfg.max_source_positions * 2 * d
            t = {k: [] for k in ("mel", "enc", "ckv", "one", "all", "r_mel", "r_enc", "r_ckv", "r_one", "r_all")}
            ms = (C.c_float * 2)()
            for rep in range(warmup + reps):
                a, feat = timed(lambda: lib.log_mel(wavs))
                lib._encode(feat, None, ms)
                one, _ = timed(lambda: lib.generate(feat, spec, 1))
                all_, (ids, _) = timed(lambda: lib.generate(feat, spec, n_tok))
                b, rfeat = timed(lambda: ref.log_mel(wavs))
                c, enc = timed(lambda: ref.encode(feat))
                e, _ = timed(lambda: ref.cross_kv(enc))
                r_one, _ = timed(lambda: ref.decode(B, 1, mask))
                r_all, rids = timed(lambda: ref.decode(B, n_tok, mask))
                if rep >= warmup:
                    for k, v in zip(t, (a, ms[0], ms[1], one, all_, b, c, e, r_one + c + e, r_all + c + e)):
                        t[k].append(v)
            m = {k: med(v) for k, v in t.items()}
            tok, r_tok = (m["all"] - m["one"]) / (n_tok - 1), (m["r_all"] - m["r_one"]) / (n_tok - 1)
            row = dict(model=name, B=B, tokens=n_tok, mel_ms=m["mel"], encoder_ms=m["enc"], cross_kv_ms=m["ckv"],
                       prompt_ms=m["one"] - m["enc"] - m["ckv"] - tok, per_token_ms=tok, call_ms=m["mel"] + m["all"],
                       step_weight_GBps=w_bytes / tok / 1e6, step_weight_and_kv_GBps=(w_bytes + kv_bytes) / tok / 1e6,
                       weight_GB=w_bytes / 1e9, cross_kv_GB=kv_bytes / 1e9,
                       torch_mel_ms=m["r_mel"], torch_encoder_ms=m["r_enc"], torch_cross_kv_ms=m["r_ckv"],
                       torch_prompt_ms=m["r_one"] - m["r_enc"] - m["r_ckv"] - r_tok, torch_per_token_ms=r_tok, torch_call_ms=m["r_mel"] + m["r_all"],
                       mel_max_diff=float((feat - rfeat).abs().max()), ids_equal=float((ids.long() == rids).float().mean()))
            rows.append(row)
            print(json.dumps(row), flush=True)
        return rows


def bench_linear(cfg, reps):
    """One linear of the step alone at M = 1, 8, 32: ms and GB/s of the weight's bytes, skinny kernel | launch_igemm."""
    lib, st = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d, Fd = cfg.d_model, cfg.decoder_ffn_dim
    rows = []
    for K, N in ((d, 3 * d), (d, d), (d, Fd), (Fd, d)):
        ws = [torch.randn(K, N, device="cuda") for _ in range(8)]              # rotated: 8 x the matrix does not sit in the caches
        for M in (1, 8, 32):
            x, y, scratch = torch.randn(M, K, device="cuda"), torch.empty(M, N, device="cuda"), torch.empty((K // 64) * M * N, device="cuda")
            out = {}
            for form in (0, 1):
                def run(n):
                    for i in range(n):
                        lib.dex_whisper_step_linear(x.data_ptr(), ws[i % 8].data_ptr(), y.data_ptr(), scratch.data_ptr(), scratch.numel(), M, K, N, form, st)
                run(8)
                ts = [timed(lambda: run(64))[0] / 64 for _ in range(reps)]
                out[form] = med(ts)
            row = dict(K=K, N=N, M=M, skinny_us=out[0] * 1e3, igemm_us=out[1] * 1e3, skinny_GBps=4 * K * N / out[0] / 1e6, igemm_GBps=4 * K * N / out[1] / 1e6)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


LONG_NOTS, LONG_EOS = 50364, 50257          # whisper-large-v3: <|notimestamps|>, <|endoftext|>; 1501 timestamps behind the former


def bench_long(cfg, seconds, batches, reps, warmup, n_tok, seed):
    with torch.no_grad():
        lib = whisper.Whisper(R.library_config(cfg), "cuda").load_state_dict(make_weights(cfg, seed, "cuda"))
        plain = whisper.GenerationSpec(PROMPT, (LONG_EOS,), (LONG_EOS,), LONG_EOS)
        rule = whisper.GenerationSpec(PROMPT, (LONG_EOS,), (LONG_EOS,), LONG_EOS, LONG_NOTS, 50)
        rows = []
        for B in batches:
            g = torch.Generator().manual_seed(seed + 1)
            n = int(seconds * 16000)
            wavs = (0.1 * torch.randn(B, n, generator=g).cumsum(1).sin() + 0.01 * torch.randn(B, n, generator=g)).float().cuda()
            feat = lib.log_mel(wavs[:, : R.n_samples(cfg)])
            t = {k: [] for k in ("plain", "rule", "mel", "call", "windows")}
            for r in range(warmup + reps):
                one, _ = timed(lambda: lib.generate(feat, plain, 1))
                all_, _ = timed(lambda: lib.generate(feat, plain, n_tok))
                r_one, _ = timed(lambda: lib.generate(feat, rule, 1, timestamps=True))
                r_all, (ids, _) = timed(lambda: lib.generate(feat, rule, n_tok, timestamps=True))
                assert ids.shape[1] == n_tok
                mel, _ = timed(lambda: lib.log_mel_long(wavs))
                trace = []
                call, _ = timed(lambda: lib.generate_segments(wavs, rule, max_new_tokens=n_tok, _trace=trace))
                feats, _ = lib.log_mel_long(wavs)
                parts = 0.0
                for grp in trace:
                    ms, _ = timed(lambda: lib.generate(lib._gather(feats, [b for b, _, _, _ in grp], [s for _, s, _, _ in grp], [nn for _, _, nn, _ in grp]),
                                                       rule, n_tok, timestamps=True))
                    parts += ms
                if r >= warmup:
                    for k, v in zip(t, ((all_ - one) / (n_tok - 1), (r_all - r_one) / (n_tok - 1), mel, call, parts)):
                        t[k].append(v)
            row = dict(model="large-v3", B=B, seconds=seconds, tokens=n_tok, reps=reps,
                       plain_per_token_ms=med(t["plain"]), plain_spread_ms=max(t["plain"]) - min(t["plain"]),
                       rule_per_token_ms=med(t["rule"]), rule_spread_ms=max(t["rule"]) - min(t["rule"]),
                       long_mel_ms=med(t["mel"]), long_call_ms=med(t["call"]), window_calls=len(trace), windows=sum(len(grp) for grp in trace),
                       sum_of_windows_ms=med(t["windows"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        return rows


def bench_beams(cfg, K, batches, reps, warmup, n_tok, seed):
    with torch.no_grad():
        w = make_weights(cfg, seed, "cuda")
        lib = whisper.Whisper(R.library_config(cfg), "cuda").load_state_dict(w)
        ref = TorchWhisper(cfg, w)
        eos = cfg.vocab_size - 1
        spec = whisper.GenerationSpec(PROMPT, (eos,), (eos,), eos)
        mask = torch.zeros(cfg.vocab_size, device="cuda")
        mask[eos] = float("-inf")
        rows = []
        for U in batches:
            feat = lib.log_mel(make_wavs(U, seed).cuda())
            rep_feat = feat.repeat_interleave(K, dim=0)
            enc = ref.encode(feat).repeat_interleave(K, dim=0)
            t = {k: [] for k in ("beam", "greedy", "torch")}
            for r in range(warmup + reps):
                b1, _ = timed(lambda: lib.generate_beam(feat, spec, K, max_new_tokens=1))
                bn, (ids, _, _) = timed(lambda: lib.generate_beam(feat, spec, K, max_new_tokens=n_tok))
                g1, _ = timed(lambda: lib.generate(rep_feat, spec, 1))
                gn, _ = timed(lambda: lib.generate(rep_feat, spec, n_tok))
                ref.cross_kv(enc)
                t1, _ = timed(lambda: ref.decode_beam(U, K, 1, mask))
                ref.cross_kv(enc)
                tn, rids = timed(lambda: ref.decode_beam(U, K, n_tok, mask))
                assert ids.shape[1] == n_tok
                if r >= warmup:
                    for k, v in zip(t, (bn - b1, gn - g1, tn - t1)):
                        t[k].append(v / (n_tok - 1))
            row = dict(model="large-v3", U=U, K=K, rows=U * K, tokens=n_tok, reps=reps, ids_equal_torch=float((ids.long() == rids).float().mean()))
            for k, v in t.items():
                row[f"{k}_per_token_ms"], row[f"{k}_spread_ms"] = med(v), max(v) - min(v)
            rows.append(row)
            print(json.dumps(row), flush=True)
        return rows


def bench_policy(cfg, batches, reps, warmup, n_tok, seed):
    """Per token: the plain greedy tail, the policy tail at T = 0 (one attempt) and at T = 0.4 (the second of two attempts: a log-prob
    threshold of 0 refuses every first one), alternating inside every repetition, with the run-to-run spread of each; and one retried
    window (the second attempt: no encoder) against a fresh window (encoder + one attempt)."""
    with torch.no_grad():
        lib = whisper.Whisper(R.library_config(cfg), "cuda").load_state_dict(make_weights(cfg, seed, "cuda"))
        eos = cfg.vocab_size - 1
        spec = whisper.GenerationSpec(PROMPT, (eos,), (eos,), eos)
        one = whisper.DecodingPolicy(temperatures=(0.0,))
        two = whisper.DecodingPolicy(temperatures=(0.0, 0.4), logprob_threshold=0.0)
        rows = []
        for B in batches:
            feat = lib.log_mel(make_wavs(B, seed).cuda())
            t = {k: [] for k in ("plain", "policy_t0", "policy_t04", "fresh_window", "retried_window")}
            for r in range(warmup + reps):
                p1, _ = timed(lambda: lib.generate(feat, spec, 1))
                pn, _ = timed(lambda: lib.generate(feat, spec, n_tok))
                a1, _ = timed(lambda: lib.generate(feat, spec, 1, policy=one))
                an, (ids, _, _) = timed(lambda: lib.generate(feat, spec, n_tok, policy=one))
                b1, _ = timed(lambda: lib.generate(feat, spec, 1, policy=two))
                bn, (_, _, info) = timed(lambda: lib.generate(feat, spec, n_tok, policy=two))
                assert ids.shape[1] == n_tok and (info["attempts"] == 2).all()
                if r >= warmup:
                    t0 = (an - a1) / (n_tok - 1)
                    for k, v in zip(t, ((pn - p1) / (n_tok - 1), t0, (bn - b1) / (n_tok - 1) - t0, an, bn - an)):
                        t[k].append(v)
            row = dict(model="large-v3", B=B, tokens=n_tok, reps=reps)
            for k, v in t.items():
                row[f"{k}_ms" if "window" in k else f"{k}_per_token_ms"], row[f"{k}_spread_ms"] = med(v), max(v) - min(v)
            rows.append(row)
            print(json.dumps(row), flush=True)
        return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="base.en,large-v3")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tokens", type=int, default=48)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--long", type=float, default=None, metavar="SECONDS", help="the long-form case alone (large-v3 geometry, B = 1 and 8 by default)")
    ap.add_argument("--beams", type=int, default=None, metavar="K", help="the beam-search case alone (large-v3 geometry, U = 1 and 6 by default)")
    ap.add_argument("--policy", action="store_true", help="the fallback-decoding case alone (large-v3 geometry, B = 1 and 8 by default)")
    a = ap.parse_args(argv)
    if a.policy:
        out = {"policy": bench_policy(MODELS["large-v3"], [int(b) for b in (a.batches if a.batches != "1,8,32" else "1,8").split(",")], a.reps, a.warmup,
                                      a.tokens, a.seed)}
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.beams is not None:
        out = {"beams": bench_beams(MODELS["large-v3"], a.beams, [int(b) for b in (a.batches if a.batches != "1,8,32" else "1,6").split(",")], a.reps,
                                    a.warmup, a.tokens, a.seed)}
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.long is not None:
        out = {"long": bench_long(MODELS["large-v3"], a.long, [int(b) for b in (a.batches if a.batches != "1,8,32" else "1,8").split(",")], a.reps,
                                  a.warmup, a.tokens, a.seed)}
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    out = {"network": [], "linear": []}
    for name in a.models.split(","):
        out["linear"] += [dict(r, model=name) for r in bench_linear(MODELS[name], a.reps)]
        out["network"] += bench_model(name, MODELS[name], [int(b) for b in a.batches.split(",")], a.reps, a.warmup, a.tokens, a.seed)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
