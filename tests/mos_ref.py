"""Restatement of the UTMOS path of dex_tts_amd/mos.py (csrc/mos.hip): the UTMOS22 strong learner in eval mode for one utterance at its
own length - HF's ``Wav2Vec2Model`` (group-norm feature extractor, post-layer-norm encoder, no mask) -> ``last_hidden_state``, every
frame concatenated with ``Embedding[domain]`` and ``Embedding[judge]``, ``nn.LSTM(bidirectional=True)``, Linear - ReLU - Linear,
``mean * 2 + 3`` - in float64 numpy (``forward``, ``bilstm``), and the same graph in torch ops (``torch_graph``), which in fp32 on the
CPU is the GPU tests' yardstick (``torch_forward_fp32``).  The tolerance rule is tests/asr_ref.py's: the device may lie ``NET_FACTOR``
= 8 times as far from the float64 restatement as the fp32 CPU evaluation does, floored at ``NET_FLOOR`` of the largest magnitude.

``hf_modules`` / ``hf_forward`` build the network from ``transformers.Wav2Vec2Model`` and ``torch.nn`` modules: in double precision
tests/test_mos_cpu.py holds ``forward`` to them, in fp32 on the GPU tools/mos_bench.py times them.  Nothing here has seen the real
UTMOS checkpoint: the network is the one a reading of the public model describes."""
import math
import types

import numpy as np

from tests.asr_ref import NET_FACTOR, NET_FLOOR, _conv1d, _gelu, _ln, fold_weight_norm, normalize_input, synth_wav  # noqa: F401
from tests.wavlm_ref import GN_EPS, dc_wav, tolerance  # noqa: F401


def _cfg(**kw):
    base = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_bias=False,
                feat_extract_norm="group", hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                do_stable_layer_norm=False, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
                hidden_act="gelu", feat_extract_activation="gelu", num_domains=3, domain_dim=128, num_judges=3000, judge_dim=128,
                lstm_hidden=512, proj_hidden=2048)
    base.update(kw)
    return types.SimpleNamespace(**base)


def variant(cfg, **kw):
    return _cfg(**{**vars(cfg), **kw})


DEFAULT = _cfg()
TINY = _cfg(conv_dim=(32,) * 7, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256,
            num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, domain_dim=32, judge_dim=32, lstm_hidden=64, proj_hidden=128)
TINY_H512 = variant(TINY, lstm_hidden=512, proj_hidden=2048)      # the production recurrence on a small trunk
WIDE = _cfg(num_hidden_layers=1)

FE, ENC, FP = "wav2vec2.feature_extractor.conv_layers.", "wav2vec2.encoder.", "wav2vec2.feature_projection."
RNN, DIRS = "decoder_rnn.", ("", "_reverse")
DOMAIN, JUDGE = 0, 288


def library_config(cfg):
    from dex_tts_amd import mos
    return mos.MOSConfig(**vars(cfg))


def num_frames(cfg, n):
    for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def state_dict_shapes(cfg):
    out = {}
    for l, (c, k) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel)):
        out[f"{FE}{l}.conv.weight"] = (c, cfg.conv_dim[l - 1] if l else 1, k)
        if cfg.conv_bias:
            out[f"{FE}{l}.conv.bias"] = (c,)
        if l == 0:
            out[f"{FE}0.layer_norm.weight"], out[f"{FE}0.layer_norm.bias"] = (c,), (c,)
    C, H, I = cfg.conv_dim[-1], cfg.hidden_size, cfg.intermediate_size
    out[FP + "layer_norm.weight"], out[FP + "layer_norm.bias"] = (C,), (C,)
    out[FP + "projection.weight"], out[FP + "projection.bias"] = (H, C), (H,)
    out[ENC + "pos_conv_embed.conv.bias"] = (H,)
    out[ENC + "pos_conv_embed.conv.weight_g"] = (1, 1, cfg.num_conv_pos_embeddings)
    out[ENC + "pos_conv_embed.conv.weight_v"] = (H, H // cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings)
    out[ENC + "layer_norm.weight"], out[ENC + "layer_norm.bias"] = (H,), (H,)
    for l in range(cfg.num_hidden_layers):
        p = f"{ENC}layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[f"{p}attention.{n}.weight"], out[f"{p}attention.{n}.bias"] = (H, H), (H,)
        out[p + "layer_norm.weight"], out[p + "layer_norm.bias"] = (H,), (H,)
        out[p + "feed_forward.intermediate_dense.weight"], out[p + "feed_forward.intermediate_dense.bias"] = (I, H), (I,)
        out[p + "feed_forward.output_dense.weight"], out[p + "feed_forward.output_dense.bias"] = (H, I), (H,)
        out[p + "final_layer_norm.weight"], out[p + "final_layer_norm.bias"] = (H,), (H,)
    L, P, IN = cfg.lstm_hidden, cfg.proj_hidden, H + cfg.domain_dim + cfg.judge_dim
    out["domain_embedding.weight"] = (cfg.num_domains, cfg.domain_dim)
    out["judge_embedding.weight"] = (cfg.num_judges, cfg.judge_dim)
    for d in DIRS:
        out[f"{RNN}weight_ih_l0{d}"], out[f"{RNN}weight_hh_l0{d}"] = (4 * L, IN), (4 * L, L)
        out[f"{RNN}bias_ih_l0{d}"], out[f"{RNN}bias_hh_l0{d}"] = (4 * L,), (4 * L,)
    out["projection.0.weight"], out["projection.0.bias"] = (P, 2 * L), (P,)
    out["projection.3.weight"], out["projection.3.bias"] = (1, P), (1,)
    return out


LSTM_GAIN = 2.0


def make_weights(cfg, seed=0):
    """Seeded float32 weights, as tests/asr_ref.py makes them (matrices N(0, 1 / fan_in), LayerNorm gains 1 + 0.2 N, biases 0.1 N, a
    weight-norm g that is NOT the norm of v), with what this network needs on top: unit-scale embeddings, and LSTM matrices LSTM_GAIN
    = 2 times N(0, 1 / fan_in), so the pre-activations of the gates have a deviation near 2 and the sigmoids and tanhs leave their
    linear range (tests/test_mos_cpu.py asserts the share that does)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in state_dict_shapes(cfg).items():
        if k.endswith("weight_g"):
            v = 0.5 + rng.random(shape)
        elif "layer_norm.weight" in k:
            v = 1.0 + 0.2 * rng.standard_normal(shape)
        elif k.endswith(".bias") or ".bias_" in k:
            v = 0.1 * rng.standard_normal(shape)
        elif k.endswith("embedding.weight"):
            v = rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) * ((LSTM_GAIN if k.startswith(RNN) else 1.0) / math.sqrt(int(np.prod(shape[1:]))))
        sd[k] = v.astype(np.float32)
    return sd


# ---------------------------------------------------------------------------------------------------- float64 numpy
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def trunk(cfg, w, wav, do_normalize=False):
    """``Wav2Vec2Model(...).last_hidden_state`` of one utterance without a mask: raw samples [n] -> float64 [T, H] (``w``: the state
    dict as float64 arrays)."""
    eps = cfg.layer_norm_eps
    x = (normalize_input(wav) if do_normalize else np.asarray(wav, np.float64))[:, None]
    for l, s in enumerate(cfg.conv_stride):
        x = _conv1d(x, w[f"{FE}{l}.conv.weight"], w.get(f"{FE}{l}.conv.bias"), s)
        if l == 0:                                          # GroupNorm(C, C): per channel over the frames, biased variance
            m = x.mean(axis=0, keepdims=True)
            v = ((x - m) ** 2).mean(axis=0, keepdims=True)
            x = (x - m) / np.sqrt(v + GN_EPS) * w[f"{FE}0.layer_norm.weight"] + w[f"{FE}0.layer_norm.bias"]
        x = _gelu(x)
    x = _ln(x, w[FP + "layer_norm.weight"], w[FP + "layer_norm.bias"], eps)
    h = x @ w[FP + "projection.weight"].T + w[FP + "projection.bias"]
    K = cfg.num_conv_pos_embeddings
    pw = fold_weight_norm(w[ENC + "pos_conv_embed.conv.weight_g"], w[ENC + "pos_conv_embed.conv.weight_v"])
    pos = _conv1d(h, pw, w[ENC + "pos_conv_embed.conv.bias"], 1, K // 2, cfg.num_conv_pos_embedding_groups)
    if K % 2 == 0:
        pos = pos[:-1]
    h = _ln(h + _gelu(pos), w[ENC + "layer_norm.weight"], w[ENC + "layer_norm.bias"], eps)
    T, H = h.shape
    nh = cfg.num_attention_heads
    hd = H // nh
    for l in range(cfg.num_hidden_layers):
        p = f"{ENC}layers.{l}."
        q = (h @ w[p + "attention.q_proj.weight"].T + w[p + "attention.q_proj.bias"]) * hd ** -0.5
        k = h @ w[p + "attention.k_proj.weight"].T + w[p + "attention.k_proj.bias"]
        v = h @ w[p + "attention.v_proj.weight"].T + w[p + "attention.v_proj.bias"]
        q, k, v = (a.reshape(T, nh, hd).transpose(1, 0, 2) for a in (q, k, v))
        s = q @ k.transpose(0, 2, 1)
        s = np.exp(s - s.max(axis=-1, keepdims=True))
        a = ((s / s.sum(axis=-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(T, H)
        h = _ln(h + a @ w[p + "attention.out_proj.weight"].T + w[p + "attention.out_proj.bias"], w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], eps)
        y = _gelu(h @ w[p + "feed_forward.intermediate_dense.weight"].T + w[p + "feed_forward.intermediate_dense.bias"])
        h = _ln(h + y @ w[p + "feed_forward.output_dense.weight"].T + w[p + "feed_forward.output_dense.bias"], w[p + "final_layer_norm.weight"],
                w[p + "final_layer_norm.bias"], eps)
    return h


def gate_preactivations(cfg, w, feats, domain=DOMAIN, judge=JUDGE, reverse=False):
    """[T, 4 H] pre-activations (i | f | g | o) the recurrence of one direction sees, for make_weights' check."""
    return _lstm(cfg, w, feats, domain, judge, reverse)[1]


def _lstm(cfg, w, feats, domain, judge, reverse):
    T, L = feats.shape[0], cfg.lstm_hidden
    d = DIRS[int(reverse)]
    x = np.concatenate([feats, np.tile(w["domain_embedding.weight"][domain], (T, 1)), np.tile(w["judge_embedding.weight"][judge], (T, 1))], axis=1)
    gi = x @ w[f"{RNN}weight_ih_l0{d}"].T + w[f"{RNN}bias_ih_l0{d}"] + w[f"{RNN}bias_hh_l0{d}"]
    whh = w[f"{RNN}weight_hh_l0{d}"]
    h, c = np.zeros(L), np.zeros(L)
    out, pre = np.zeros((T, L)), np.zeros((T, 4 * L))
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = gi[t] + whh @ h
        pre[t] = g
        i, f, gg, o = _sigmoid(g[:L]), _sigmoid(g[L:2 * L]), np.tanh(g[2 * L:3 * L]), _sigmoid(g[3 * L:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        out[t] = h
    return out, pre


def bilstm(cfg, sd, feats, domain=DOMAIN, judge=JUDGE):
    """``nn.LSTM(hidden + domain_dim + judge_dim, H, bidirectional=True)`` of one row: features [T, hidden] concatenated with the two
    embeddings -> float64 [T, 2 H] (forward | reverse; the reverse direction starts at frame T - 1)."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items() if not k.startswith("wav2vec2.")}
    feats = np.asarray(feats, np.float64)
    return np.concatenate([_lstm(cfg, w, feats, domain, judge, False)[0], _lstm(cfg, w, feats, domain, judge, True)[0]], axis=1)


def head(cfg, sd, lstm_out):
    """The projection and the utterance score: [T, 2 H] -> (frame scores [T], score)."""
    w = {k: np.asarray(sd[k], np.float64) for k in ("projection.0.weight", "projection.0.bias", "projection.3.weight", "projection.3.bias")}
    y = np.maximum(lstm_out @ w["projection.0.weight"].T + w["projection.0.bias"], 0.0)
    frames = (y @ w["projection.3.weight"].T + w["projection.3.bias"])[:, 0]
    return frames, float(frames.mean() * 2.0 + 3.0)


def forward(cfg, sd, wav, domain=DOMAIN, judge=JUDGE, do_normalize=False):
    """One utterance: raw samples [n] -> float64 (hidden [T, hidden], lstm_out [T, 2 H], frame scores [T], score)."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    hidden = trunk(cfg, w, wav, do_normalize)
    lo = bilstm(cfg, sd, hidden, domain, judge)
    frames, score = head(cfg, sd, lo)
    return hidden, lo, frames, score


# ---------------------------------------------------------------------------------------------------- torch ops (the yardstick)
def torch_lstm(cfg, w):
    """``nn.LSTM`` with the state dict's ``decoder_rnn.*`` tensors, in their dtype and on their device."""
    import torch
    ref = w[RNN + "weight_ih_l0"]
    lstm = torch.nn.LSTM(cfg.hidden_size + cfg.domain_dim + cfg.judge_dim, cfg.lstm_hidden, num_layers=1, batch_first=True, bidirectional=True)
    lstm = lstm.to(device=ref.device, dtype=ref.dtype).eval()
    lstm.load_state_dict({k[len(RNN):]: v for k, v in w.items() if k.startswith(RNN)})
    return lstm


def torch_graph(cfg, w, x, domain=DOMAIN, judge=JUDGE, do_normalize=False, lstm=None):
    """The same graph with torch's operators on whatever device and dtype the tensors have: ``w`` the state dict as tensors, ``x``
    [B, n] raw samples of equal length, ``domain`` / ``judge`` an int each -> (hidden [B, T, H], lstm_out [B, T, 2 L], frame scores
    [B, T], score [B]).  The group norm is per sample and the rows are all n samples long: row b is the row alone."""
    import torch
    import torch.nn.functional as F
    eps = cfg.layer_norm_eps
    with torch.no_grad():
        if do_normalize:
            x = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + 1e-7)
        x = x[:, None]
        for l, s in enumerate(cfg.conv_stride):
            x = F.conv1d(x, w[f"{FE}{l}.conv.weight"], w.get(f"{FE}{l}.conv.bias"), stride=s)
            if l == 0:
                x = F.group_norm(x, x.shape[1], w[f"{FE}0.layer_norm.weight"], w[f"{FE}0.layer_norm.bias"], GN_EPS)
            x = F.gelu(x)
        x = x.transpose(1, 2)
        x = F.layer_norm(x, (x.shape[2],), w[FP + "layer_norm.weight"], w[FP + "layer_norm.bias"], eps)
        h = F.linear(x, w[FP + "projection.weight"], w[FP + "projection.bias"])
        K = cfg.num_conv_pos_embeddings
        g, v = w[ENC + "pos_conv_embed.conv.weight_g"], w[ENC + "pos_conv_embed.conv.weight_v"]
        pw = g * v / torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True))
        pos = F.conv1d(h.transpose(1, 2), pw, w[ENC + "pos_conv_embed.conv.bias"], padding=K // 2,
                       groups=cfg.num_conv_pos_embedding_groups).transpose(1, 2)
        if K % 2 == 0:
            pos = pos[:, :-1]
        B, T, H = h.shape
        h = F.layer_norm(h + F.gelu(pos), (H,), w[ENC + "layer_norm.weight"], w[ENC + "layer_norm.bias"], eps)
        nh = cfg.num_attention_heads
        hd = H // nh
        for l in range(cfg.num_hidden_layers):
            p = f"{ENC}layers.{l}."
            q = F.linear(h, w[p + "attention.q_proj.weight"], w[p + "attention.q_proj.bias"]) * hd ** -0.5
            k = F.linear(h, w[p + "attention.k_proj.weight"], w[p + "attention.k_proj.bias"])
            v = F.linear(h, w[p + "attention.v_proj.weight"], w[p + "attention.v_proj.bias"])
            q, k, v = (a.reshape(B, T, nh, hd).transpose(1, 2) for a in (q, k, v))
            a = (torch.softmax(q @ k.transpose(2, 3), dim=-1) @ v).transpose(1, 2).reshape(B, T, H)
            h = F.layer_norm(h + F.linear(a, w[p + "attention.out_proj.weight"], w[p + "attention.out_proj.bias"]), (H,), w[p + "layer_norm.weight"],
                             w[p + "layer_norm.bias"], eps)
            y = F.gelu(F.linear(h, w[p + "feed_forward.intermediate_dense.weight"], w[p + "feed_forward.intermediate_dense.bias"]))
            h = F.layer_norm(h + F.linear(y, w[p + "feed_forward.output_dense.weight"], w[p + "feed_forward.output_dense.bias"]), (H,),
                             w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], eps)
        cond = torch.cat([w["domain_embedding.weight"][domain], w["judge_embedding.weight"][judge]]).expand(B, T, -1)
        lo, _ = (lstm or torch_lstm(cfg, w))(torch.cat([h, cond], dim=2))
        y = F.relu(F.linear(lo, w["projection.0.weight"], w["projection.0.bias"]))
        frames = F.linear(y, w["projection.3.weight"], w["projection.3.bias"])[..., 0]
        return h, lo, frames, frames.mean(dim=1) * 2.0 + 3.0


def torch_forward_fp32(cfg, sd, wav, domain=DOMAIN, judge=JUDGE, do_normalize=False):
    """``torch_graph`` in fp32 on the CPU for one utterance: raw samples [n] -> float32 (hidden, lstm_out, frame scores, score)."""
    import torch
    w = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()}
    hid, lo, fr, sc = torch_graph(cfg, w, torch.from_numpy(np.asarray(wav, np.float32))[None], domain, judge, do_normalize)
    return hid[0].numpy(), lo[0].numpy(), fr[0].numpy(), float(sc[0])


def torch_bilstm_fp32(cfg, sd, feats, domain=DOMAIN, judge=JUDGE):
    """``nn.LSTM`` in fp32 on the CPU on one row's features [T, hidden] -> float32 [T, 2 L]: the yardstick of the recurrence alone."""
    import torch
    w = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items() if not k.startswith("wav2vec2.")}
    f = torch.from_numpy(np.asarray(feats, np.float32))
    with torch.no_grad():
        cond = torch.cat([w["domain_embedding.weight"][domain], w["judge_embedding.weight"][judge]]).expand(f.shape[0], -1)
        return torch_lstm(cfg, w)(torch.cat([f, cond], dim=1)[None])[0][0].numpy()


# ---------------------------------------------------------------------------------------------------- transformers + torch.nn modules
def hf_modules(cfg, sd, dtype=None, device="cpu"):
    """(``transformers.Wav2Vec2Model``, domain ``nn.Embedding``, judge ``nn.Embedding``, ``nn.LSTM``, the projection ``nn.Sequential``)
    of ``cfg`` in eval mode with the weights ``sd``, in ``dtype`` (default double) on ``device``."""
    import torch
    import transformers
    dtype = dtype or torch.float64
    hc = transformers.Wav2Vec2Config(
        hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
        intermediate_size=cfg.intermediate_size, hidden_act="gelu", layer_norm_eps=cfg.layer_norm_eps, feat_extract_norm="group",
        feat_extract_activation="gelu", conv_dim=list(cfg.conv_dim), conv_stride=list(cfg.conv_stride), conv_kernel=list(cfg.conv_kernel),
        conv_bias=cfg.conv_bias, num_conv_pos_embeddings=cfg.num_conv_pos_embeddings,
        num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups, do_stable_layer_norm=False, apply_spec_augment=False)
    ssl = transformers.Wav2Vec2Model(hc).to(dtype).eval()
    own = ssl.state_dict()
    new = {}
    for k, v in sd.items():
        if not k.startswith("wav2vec2."):
            continue
        k = k[len("wav2vec2."):]
        for a, b in (("weight_g", "parametrizations.weight.original0"), ("weight_v", "parametrizations.weight.original1")):
            if k.endswith(a) and k not in own:
                k = k[: -len(a)] + b
        new[k] = torch.as_tensor(np.asarray(v)).to(dtype)
    missing, unexpected = ssl.load_state_dict(new, strict=False)
    assert not unexpected and all(m == "masked_spec_embed" for m in missing), (missing, unexpected)
    t = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if not k.startswith("wav2vec2.")}
    dom = torch.nn.Embedding(cfg.num_domains, cfg.domain_dim)
    jud = torch.nn.Embedding(cfg.num_judges, cfg.judge_dim)
    dom.load_state_dict({"weight": t["domain_embedding.weight"]})
    jud.load_state_dict({"weight": t["judge_embedding.weight"]})
    lstm = torch_lstm(cfg, t)
    proj = torch.nn.Sequential(torch.nn.Linear(2 * cfg.lstm_hidden, cfg.proj_hidden), torch.nn.ReLU(), torch.nn.Dropout(0.3),
                               torch.nn.Linear(cfg.proj_hidden, 1))
    proj.load_state_dict({k[len("projection."):]: v for k, v in t.items() if k.startswith("projection.")})
    return tuple(m.to(device=device, dtype=dtype).eval() for m in (ssl, dom, jud, lstm, proj))


def hf_forward(mods, x, domain=DOMAIN, judge=JUDGE):
    """``x`` [B, n] raw samples of equal length through the modules of ``hf_modules`` -> (hidden, lstm_out, frame scores, score)."""
    import torch
    ssl, dom, jud, lstm, proj = mods
    with torch.no_grad():
        h = ssl(x).last_hidden_state
        B, T, _ = h.shape
        ids = lambda v: torch.full((B,), int(v), dtype=torch.long, device=h.device)       # noqa: E731
        cond = torch.cat([dom(ids(domain)), jud(ids(judge))], dim=1)[:, None].expand(B, T, -1)
        lo, _ = lstm(torch.cat([h, cond], dim=2))
        frames = proj(lo)[..., 0]
        return h, lo, frames, frames.mean(dim=1) * 2.0 + 3.0


# ---------------------------------------------------------------------------------------------------- the upstream checkpoint's names
_TO_FAIRSEQ = (("attention.", "self_attn."), ("feed_forward.intermediate_dense.", "fc1."), ("feed_forward.output_dense.", "fc2."))


def to_utmos_checkpoint(sd):
    """The inverse of ``mos.from_utmos_checkpoint``: ``load_state_dict``'s keys -> the upstream Lightning checkpoint's, as a
    reading of the public model names them."""
    out = {}
    for k, v in sd.items():
        if k.startswith("wav2vec2."):
            k = k[len("wav2vec2."):]
            p = k.split(".")
            if k.startswith("feature_extractor.conv_layers."):
                k = ".".join(p[:3] + [{"conv": "0", "layer_norm": "2"}[p[3]], p[4]])
            elif k.startswith("feature_projection.projection."):
                k = "post_extract_proj." + p[-1]
            elif k.startswith("feature_projection.layer_norm."):
                k = "layer_norm." + p[-1]
            elif k.startswith("encoder.pos_conv_embed.conv."):
                k = "encoder.pos_conv.0." + p[-1]
            elif k.startswith("encoder.layers."):
                rest = ".".join(p[3:])
                if rest.startswith("layer_norm."):
                    rest = "self_attn_" + rest
                for new, old in _TO_FAIRSEQ:
                    if rest.startswith(new):
                        rest = old + rest[len(new):]
                k = ".".join(p[:3]) + "." + rest
            out["feature_extractors.0.ssl_model." + k] = v
        elif k == "domain_embedding.weight":
            out["feature_extractors.1.embedding.weight"] = v
        elif k == "judge_embedding.weight":
            out["output_layers.0.judge_embedding.weight"] = v
        elif k.startswith(RNN):
            out["output_layers.0." + k] = v
        elif k.startswith("projection."):
            out["output_layers.1.net." + k[len("projection."):]] = v
        else:
            out[k] = v
    return out
