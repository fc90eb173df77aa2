"""Restatement of the WavLM-large + ECAPA-TDNN path of dex_tts_amd/ecapa.py (csrc/ecapa.hip), one utterance at its own length, eval
mode: HF's ``WavLMModel`` of the large family (layer-norm feature extractor, stable layer norm; all L + 1 hidden states) feeding the
``ECAPA_TDNN`` head of the UniSpeech speaker-verification recipe - in float64 numpy (``forward``, with ``trunk_hidden_states``,
``head`` and ``res2`` as its parts), and the same graph in torch ops (``torch_graph`` = ``torch_trunk`` + ``torch_head``), which in
fp32 on the CPU is the GPU tests' yardstick (``torch_forward_fp32``, ``torch_res2_fp32``) and on the GPU is what tools/ecapa_bench.py
times.  The tolerance rule is tests/asr_ref.py's: the device may lie ``NET_FACTOR`` = 8 times as far from the float64 restatement as
the fp32 CPU evaluation does, floored at 1e-6 of the largest magnitude.

tests/test_ecapa_cpu.py holds the trunk to ``transformers.WavLMModel`` and the head to a ``torch.nn`` transcription, both in double
precision.  Nothing here has seen the real checkpoint: the definition was written down from a reading of the public code."""
import math
import types

import numpy as np

from tests.asr_ref import NET_FACTOR, NET_FLOOR, _conv1d, _gelu, _ln, fold_weight_norm, synth_wav  # noqa: F401
from tests.wavlm_ref import _sigmoid, cosine, dc_wav, relative_position_buckets, tolerance  # noqa: F401

BN_EPS = IN_EPS = NORM_EPS = 1e-5
BN = ("weight", "bias", "running_mean", "running_var")
NSTAGE = 7


def _cfg(**kw):
    base = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_bias=True,
                feat_extract_norm="layer", hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                do_stable_layer_norm=True, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
                num_buckets=320, max_bucket_distance=800, hidden_act="gelu", feat_extract_activation="gelu",
                channels=512, emb_dim=256, res2_scale=8, se_bottleneck_dim=128, attention_channels=128, global_context_att=False,
                dilations=(2, 3, 4))
    base.update(kw)
    return types.SimpleNamespace(**base)


def variant(cfg, **kw):
    return _cfg(**{**vars(cfg), **kw})


DEFAULT = _cfg()
# tests/wavlm_ref.py's TINY trunk in the large family (layer norm, stable layer norm, conv bias); slices of 32 channels
TINY = _cfg(conv_dim=(32,) * 7, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256,
            num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, num_buckets=32, max_bucket_distance=40,
            channels=256, emb_dim=32, se_bottleneck_dim=32, attention_channels=64)
WIDE = _cfg(num_hidden_layers=1)                      # the default widths: slices of 64 channels
TINY_GC = variant(TINY, global_context_att=True)

FE, ENC, FP = "wavlm.feature_extractor.conv_layers.", "wavlm.encoder.", "wavlm.feature_projection."


def library_config(cfg):
    from dex_tts_amd import ecapa
    return ecapa.EcapaConfig(**vars(cfg))


def num_frames(cfg, n):
    for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def min_samples(cfg):
    n = 2
    for k, s in zip(reversed(cfg.conv_kernel), reversed(cfg.conv_stride)):
        n = (n - 1) * s + k
    return n


def _bn_shapes(out, p, n):
    for k in BN:
        out[p + k] = (n,)


def state_dict_shapes(cfg):
    """The library's inventory, in its registration order."""
    out = {}
    for l, (c, k) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel)):
        out[f"{FE}{l}.conv.weight"] = (c, cfg.conv_dim[l - 1] if l else 1, k)
        if cfg.conv_bias:
            out[f"{FE}{l}.conv.bias"] = (c,)
        out[f"{FE}{l}.layer_norm.weight"], out[f"{FE}{l}.layer_norm.bias"] = (c,), (c,)
    Cf, H, I, nh = cfg.conv_dim[-1], cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
    out[FP + "layer_norm.weight"], out[FP + "layer_norm.bias"] = (Cf,), (Cf,)
    out[FP + "projection.weight"], out[FP + "projection.bias"] = (H, Cf), (H,)
    out[ENC + "pos_conv_embed.conv.bias"] = (H,)
    out[ENC + "pos_conv_embed.conv.weight_g"] = (1, 1, cfg.num_conv_pos_embeddings)
    out[ENC + "pos_conv_embed.conv.weight_v"] = (H, H // cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings)
    out[ENC + "layer_norm.weight"], out[ENC + "layer_norm.bias"] = (H,), (H,)
    for l in range(cfg.num_hidden_layers):
        p = f"{ENC}layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[f"{p}attention.{n}.weight"], out[f"{p}attention.{n}.bias"] = (H, H), (H,)
        out[p + "attention.gru_rel_pos_const"] = (1, nh, 1, 1)
        out[p + "attention.gru_rel_pos_linear.weight"], out[p + "attention.gru_rel_pos_linear.bias"] = (8, H // nh), (8,)
        if l == 0:
            out[p + "attention.rel_attn_embed.weight"] = (cfg.num_buckets, nh)
        out[p + "layer_norm.weight"], out[p + "layer_norm.bias"] = (H,), (H,)
        out[p + "feed_forward.intermediate_dense.weight"], out[p + "feed_forward.intermediate_dense.bias"] = (I, H), (I,)
        out[p + "feed_forward.output_dense.weight"], out[p + "feed_forward.output_dense.bias"] = (H, I), (H,)
        out[p + "final_layer_norm.weight"], out[p + "final_layer_norm.bias"] = (H,), (H,)
    C, A, S = cfg.channels, cfg.attention_channels, cfg.se_bottleneck_dim
    w, C3 = C // cfg.res2_scale, 3 * C
    out["feature_weight"] = (cfg.num_hidden_layers + 1,)
    out["layer1.conv.weight"], out["layer1.conv.bias"] = (C, H, 5), (C,)
    _bn_shapes(out, "layer1.bn.", C)
    for n in range(len(cfg.dilations)):
        p = f"layer{n + 2}."
        out[p + "Conv1dReluBn1.conv.weight"], out[p + "Conv1dReluBn1.conv.bias"] = (C, C, 1), (C,)
        _bn_shapes(out, p + "Conv1dReluBn1.bn.", C)
        for i in range(NSTAGE):
            out[f"{p}Res2Conv1dReluBn.convs.{i}.weight"], out[f"{p}Res2Conv1dReluBn.convs.{i}.bias"] = (w, w, 3), (w,)
        for i in range(NSTAGE):
            _bn_shapes(out, f"{p}Res2Conv1dReluBn.bns.{i}.", w)
        out[p + "Conv1dReluBn2.conv.weight"], out[p + "Conv1dReluBn2.conv.bias"] = (C, C, 1), (C,)
        _bn_shapes(out, p + "Conv1dReluBn2.bn.", C)
        out[p + "SE_Connect.linear1.weight"], out[p + "SE_Connect.linear1.bias"] = (S, C), (S,)
        out[p + "SE_Connect.linear2.weight"], out[p + "SE_Connect.linear2.bias"] = (C, S), (C,)
    out["conv.weight"], out["conv.bias"] = (C3, C3, 1), (C3,)
    out["pooling.linear1.weight"], out["pooling.linear1.bias"] = (A, 3 * C3 if cfg.global_context_att else C3, 1), (A,)
    out["pooling.linear2.weight"], out["pooling.linear2.bias"] = (C3, A, 1), (C3,)
    _bn_shapes(out, "bn.", 2 * C3)
    out["linear.weight"], out["linear.bias"] = (cfg.emb_dim, 2 * C3), (cfg.emb_dim,)
    return out


CAT_BIAS = 1.5


def make_weights(cfg, seed=0):
    """Seeded float32 weights under the library's keys, the trunk's as tests/wavlm_ref.py makes them (a gate that does something,
    ``feature_weight`` N(0, 1), far from uniform), and for the head: matrices N(0, 1 / fan_in); batch norms with non-trivial running
    statistics (gain 1 + 0.2 N, bias 0.1 N, running_mean 0.2 N, running_var in [0.5, 1.5]); the bias of the 1 x 1 convolution before
    the pooling NEGATIVE (-1.5 +- 0.1): its ReLU is then on for part of the frames only, and some channels are off on every frame
    (pooled deviation exactly sqrt(1e-9)); the pooling's second Linear 4 x larger, so that its softmax over time is far from uniform."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in state_dict_shapes(cfg).items():
        if k.endswith("weight_g"):
            v = 0.5 + rng.random(shape)
        elif k.endswith("gru_rel_pos_const"):
            v = np.where(rng.random(shape) < 0.5, 0.3, 1.2) + 0.5 * rng.random(shape)
        elif k.endswith("rel_attn_embed.weight") or k == "feature_weight":
            v = rng.standard_normal(shape)
        elif k.endswith("gru_rel_pos_linear.weight"):
            v = 0.25 * rng.standard_normal(shape)
        elif k.endswith("running_mean"):
            v = 0.2 * rng.standard_normal(shape)
        elif k.endswith("running_var"):
            v = 0.5 + rng.random(shape)
        elif "layer_norm.weight" in k or k.endswith("bn.weight") or ".bns." in k and k.endswith(".weight"):
            v = 1.0 + 0.2 * rng.standard_normal(shape)
        elif k.endswith(".bias"):
            v = 0.1 * rng.standard_normal(shape) - (CAT_BIAS if k == "conv.bias" else 0.0)
        else:
            v = rng.standard_normal(shape) * ((4.0 if k == "pooling.linear2.weight" else 1.0) / math.sqrt(int(np.prod(shape[1:]))))
        sd[k] = v.astype(np.float32)
    return sd


# ---------------------------------------------------------------------------------------------------- float64 numpy
def normalize_wav(x):
    """s3prl's ``F.layer_norm(wav, wav.shape)``: biased variance, eps 1e-5."""
    x = np.asarray(x, np.float64)
    return (x - x.mean()) / np.sqrt(x.var() + NORM_EPS)


def trunk_hidden_states(cfg, w, wav):
    """``w``: the state dict as float64 arrays; raw (already normalised, where that is wanted) samples [n] -> the L + 1 hidden states
    [T, H] of ``WavLMModel(output_hidden_states=True)``: the inputs of layers 0 .. L - 1 and ``encoder.layer_norm`` of the last output."""
    eps = cfg.layer_norm_eps
    x = np.asarray(wav, np.float64)[:, None]
    for l, s in enumerate(cfg.conv_stride):
        x = _conv1d(x, w[f"{FE}{l}.conv.weight"], w.get(f"{FE}{l}.conv.bias"), s)
        x = _gelu(_ln(x, w[f"{FE}{l}.layer_norm.weight"], w[f"{FE}{l}.layer_norm.bias"], eps))
    x = _ln(x, w[FP + "layer_norm.weight"], w[FP + "layer_norm.bias"], eps)
    h = x @ w[FP + "projection.weight"].T + w[FP + "projection.bias"]
    K = cfg.num_conv_pos_embeddings
    pw = fold_weight_norm(w[ENC + "pos_conv_embed.conv.weight_g"], w[ENC + "pos_conv_embed.conv.weight_v"])
    pos = _conv1d(h, pw, w[ENC + "pos_conv_embed.conv.bias"], 1, K // 2, cfg.num_conv_pos_embedding_groups)
    if K % 2 == 0:
        pos = pos[:-1]
    h = h + _gelu(pos)                                       # no LayerNorm here in the stable-layer-norm encoder
    T, H = h.shape
    nh = cfg.num_attention_heads
    hd = H // nh
    rel = w[f"{ENC}layers.0.attention.rel_attn_embed.weight"][relative_position_buckets(cfg, T)]          # [2T - 1, nh]
    bias = rel[np.arange(T)[None, :] - np.arange(T)[:, None] + T - 1].transpose(2, 0, 1)               # [nh, query, key]
    hidden = []
    for l in range(cfg.num_hidden_layers):
        hidden.append(h)
        p = f"{ENC}layers.{l}."
        y = _ln(h, w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], eps)
        yh = y.reshape(T, nh, hd).transpose(1, 0, 2)         # the gate reads what the attention reads: LayerNorm(h)
        pr = (yh @ w[p + "attention.gru_rel_pos_linear.weight"].T + w[p + "attention.gru_rel_pos_linear.bias"]).reshape(nh, T, 2, 4).sum(-1)
        ga, gb = _sigmoid(pr[..., 0]), _sigmoid(pr[..., 1])
        gate = ga * (gb * w[p + "attention.gru_rel_pos_const"].reshape(nh, 1) - 1.0) + 2.0              # [nh, T]
        q = (y @ w[p + "attention.q_proj.weight"].T + w[p + "attention.q_proj.bias"]) * hd ** -0.5
        k = y @ w[p + "attention.k_proj.weight"].T + w[p + "attention.k_proj.bias"]
        v = y @ w[p + "attention.v_proj.weight"].T + w[p + "attention.v_proj.bias"]
        q, k, v = (a.reshape(T, nh, hd).transpose(1, 0, 2) for a in (q, k, v))
        s = q @ k.transpose(0, 2, 1) + gate[:, :, None] * bias
        s = np.exp(s - s.max(axis=-1, keepdims=True))
        a = ((s / s.sum(axis=-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(T, H)
        h = h + a @ w[p + "attention.out_proj.weight"].T + w[p + "attention.out_proj.bias"]
        y = _ln(h, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], eps)
        y = _gelu(y @ w[p + "feed_forward.intermediate_dense.weight"].T + w[p + "feed_forward.intermediate_dense.bias"])
        h = h + y @ w[p + "feed_forward.output_dense.weight"].T + w[p + "feed_forward.output_dense.bias"]
    hidden.append(_ln(h, w[ENC + "layer_norm.weight"], w[ENC + "layer_norm.bias"], eps))
    return hidden


def _bn(x, w, p):
    return (x - w[p + "running_mean"]) / np.sqrt(w[p + "running_var"] + BN_EPS) * w[p + "weight"] + w[p + "bias"]


def _conv_relu_bn(x, w, p, pad=0, dil=1):
    """``Conv1dReluBn``: bn(relu(conv(x))), x [T, Cin]."""
    W = w[p + "conv.weight"]
    k = W.shape[2]
    T = x.shape[0]
    xp = np.concatenate([np.zeros((pad, x.shape[1])), x, np.zeros((pad, x.shape[1]))]) if pad else x
    y = w[p + "conv.bias"] + sum(xp[j * dil: j * dil + T] @ W[:, :, j].T for j in range(k))
    return _bn(np.maximum(y, 0.0), w, p + "bn.")


def _res2(x, w, p, dil, scale=8):
    """``Res2Conv1dReluBn``: x [T, C] -> [T, C]."""
    T, C = x.shape
    ws = C // scale
    out, sp = [], None
    for i in range(scale - 1):
        sl = x[:, i * ws:(i + 1) * ws]
        sp = sl if i == 0 else sp + sl
        W = w[f"{p}convs.{i}.weight"]
        xp = np.concatenate([np.zeros((dil, ws)), sp, np.zeros((dil, ws))])
        y = w[f"{p}convs.{i}.bias"] + sum(xp[j * dil: j * dil + T] @ W[:, :, j].T for j in range(3))
        sp = _bn(np.maximum(y, 0.0), w, f"{p}bns.{i}.")
        out.append(sp)
    out.append(x[:, (scale - 1) * ws:])
    return np.concatenate(out, axis=1)


def res2(cfg, sd, block, x):
    """The Res2 chain of block ``block`` alone: x [T, channels] -> float64 [T, channels]."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items() if f"layer{block + 2}.Res2" in k}
    return _res2(np.asarray(x, np.float64), w, f"layer{block + 2}.Res2Conv1dReluBn.", cfg.dilations[block], cfg.res2_scale)


def instance_normed_mix(cfg, w, hidden):
    lw = np.exp(w["feature_weight"] - w["feature_weight"].max())
    lw = lw / lw.sum()
    x = sum(a * b for a, b in zip(lw, hidden)) + 1e-6
    m = x.mean(axis=0, keepdims=True)
    return (x - m) / np.sqrt(((x - m) ** 2).mean(axis=0, keepdims=True) + IN_EPS)


def pooled(cfg, w, x):
    """The head from the instance-normed mix x [T, H] up to the attentive statistics: float64 [2 x 3C] (means, then deviations)."""
    out1 = _conv_relu_bn(x, w, "layer1.", pad=2)
    outs, cur = [], out1
    for n, d in enumerate(cfg.dilations):
        p = f"layer{n + 2}."
        y = _conv_relu_bn(cur, w, p + "Conv1dReluBn1.")
        y = _res2(y, w, p + "Res2Conv1dReluBn.", d, cfg.res2_scale)
        y = _conv_relu_bn(y, w, p + "Conv1dReluBn2.")
        s = y.mean(axis=0)
        s = np.maximum(w[p + "SE_Connect.linear1.weight"] @ s + w[p + "SE_Connect.linear1.bias"], 0.0)
        s = _sigmoid(w[p + "SE_Connect.linear2.weight"] @ s + w[p + "SE_Connect.linear2.bias"])
        cur = y * s + cur
        outs.append(cur)
    xc = np.maximum(np.concatenate(outs, axis=1) @ w["conv.weight"][:, :, 0].T + w["conv.bias"], 0.0)      # [T, 3C]
    x_in = xc
    if cfg.global_context_att:
        T = xc.shape[0]
        cm = np.broadcast_to(xc.mean(axis=0), xc.shape)
        cs = np.broadcast_to(np.sqrt(xc.var(axis=0, ddof=1) + 1e-10), xc.shape)
        x_in = np.concatenate([xc, cm, cs], axis=1)
    a = np.tanh(x_in @ w["pooling.linear1.weight"][:, :, 0].T + w["pooling.linear1.bias"])
    a = a @ w["pooling.linear2.weight"][:, :, 0].T + w["pooling.linear2.bias"]
    a = np.exp(a - a.max(axis=0, keepdims=True))
    a = a / a.sum(axis=0, keepdims=True)
    mean = (a * xc).sum(axis=0)
    var = (a * xc ** 2).sum(axis=0) - mean ** 2
    return np.concatenate([mean, np.sqrt(np.maximum(var, 1e-9))])


def head(cfg, w, x):
    """Instance-normed mix x [T, H] -> float64 embedding [emb_dim]."""
    return _bn(pooled(cfg, w, x), w, "bn.") @ w["linear.weight"].T + w["linear.bias"]


def forward(cfg, sd, wav, do_normalize=True):
    """One utterance: raw samples [n] -> (float64 instance-normed layer mix [T, H], float64 embedding [emb_dim])."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    hidden = trunk_hidden_states(cfg, w, normalize_wav(wav) if do_normalize else wav)
    x = instance_normed_mix(cfg, w, hidden)
    return x, head(cfg, w, x)


# ---------------------------------------------------------------------------------------------------- torch ops (the yardstick, the bench)
def torch_trunk(cfg, w, x, do_normalize=True):
    """The trunk with torch's operators on whatever device and dtype the tensors have: x [B, n] raw samples of equal length -> the
    list of L + 1 hidden states [B, T, H]."""
    import torch
    import torch.nn.functional as F
    eps = cfg.layer_norm_eps
    if do_normalize:
        x = F.layer_norm(x, (x.shape[1],), eps=NORM_EPS)
    x = x[:, None]
    for l, s in enumerate(cfg.conv_stride):
        x = F.conv1d(x, w[f"{FE}{l}.conv.weight"], w.get(f"{FE}{l}.conv.bias"), stride=s)
        Cc = x.shape[1]
        x = F.gelu(F.layer_norm(x.transpose(1, 2), (Cc,), w[f"{FE}{l}.layer_norm.weight"], w[f"{FE}{l}.layer_norm.bias"], eps)).transpose(1, 2)
    x = x.transpose(1, 2)
    x = F.layer_norm(x, (x.shape[2],), w[FP + "layer_norm.weight"], w[FP + "layer_norm.bias"], eps)
    h = F.linear(x, w[FP + "projection.weight"], w[FP + "projection.bias"])
    K = cfg.num_conv_pos_embeddings
    g, v = w[ENC + "pos_conv_embed.conv.weight_g"], w[ENC + "pos_conv_embed.conv.weight_v"]
    pw = g * v / torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True))
    pos = F.conv1d(h.transpose(1, 2), pw, w[ENC + "pos_conv_embed.conv.bias"], padding=K // 2, groups=cfg.num_conv_pos_embedding_groups).transpose(1, 2)
    if K % 2 == 0:
        pos = pos[:, :-1]
    h = h + F.gelu(pos)
    B, T, H = h.shape
    nh = cfg.num_attention_heads
    hd = H // nh
    idx = torch.from_numpy(relative_position_buckets(cfg, T)).to(h.device)
    rel = w[f"{ENC}layers.0.attention.rel_attn_embed.weight"][idx]
    ar = torch.arange(T, device=h.device)
    bias = rel[ar[None, :] - ar[:, None] + T - 1].permute(2, 0, 1)
    hidden = []
    for l in range(cfg.num_hidden_layers):
        hidden.append(h)
        p = f"{ENC}layers.{l}."
        y = F.layer_norm(h, (H,), w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], eps)
        yh = y.reshape(B, T, nh, hd).transpose(1, 2)
        pr = F.linear(yh, w[p + "attention.gru_rel_pos_linear.weight"], w[p + "attention.gru_rel_pos_linear.bias"]).reshape(B, nh, T, 2, 4).sum(-1)
        ga, gb = torch.sigmoid(pr[..., 0]), torch.sigmoid(pr[..., 1])
        gate = ga * (gb * w[p + "attention.gru_rel_pos_const"].reshape(1, nh, 1) - 1.0) + 2.0
        q = F.linear(y, w[p + "attention.q_proj.weight"], w[p + "attention.q_proj.bias"]) * hd ** -0.5
        k = F.linear(y, w[p + "attention.k_proj.weight"], w[p + "attention.k_proj.bias"])
        v = F.linear(y, w[p + "attention.v_proj.weight"], w[p + "attention.v_proj.bias"])
        q, k, v = (a.reshape(B, T, nh, hd).transpose(1, 2) for a in (q, k, v))
        a = torch.softmax(q @ k.transpose(2, 3) + gate[..., None] * bias, dim=-1) @ v
        h = h + F.linear(a.transpose(1, 2).reshape(B, T, H), w[p + "attention.out_proj.weight"], w[p + "attention.out_proj.bias"])
        y = F.layer_norm(h, (H,), w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], eps)
        y = F.gelu(F.linear(y, w[p + "feed_forward.intermediate_dense.weight"], w[p + "feed_forward.intermediate_dense.bias"]))
        h = h + F.linear(y, w[p + "feed_forward.output_dense.weight"], w[p + "feed_forward.output_dense.bias"])
    hidden.append(F.layer_norm(h, (H,), w[ENC + "layer_norm.weight"], w[ENC + "layer_norm.bias"], eps))
    return hidden


def hf_wavlm_model(cfg, sd, dtype):
    """``transformers.WavLMModel`` of ``cfg`` in eval mode with the trunk's weights of ``sd`` (numpy arrays or tensors under the
    library's keys) in ``dtype``, on the CPU."""
    import torch
    import transformers
    hc = transformers.WavLMConfig(
        hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
        intermediate_size=cfg.intermediate_size, hidden_act="gelu", layer_norm_eps=cfg.layer_norm_eps, feat_extract_norm="layer",
        feat_extract_activation="gelu", conv_dim=list(cfg.conv_dim), conv_stride=list(cfg.conv_stride), conv_kernel=list(cfg.conv_kernel),
        conv_bias=cfg.conv_bias, num_conv_pos_embeddings=cfg.num_conv_pos_embeddings,
        num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups, num_buckets=cfg.num_buckets,
        max_bucket_distance=cfg.max_bucket_distance, do_stable_layer_norm=True, apply_spec_augment=False)
    model = transformers.WavLMModel(hc).to(dtype).eval()
    own = model.state_dict()
    new = {}
    for k, v in sd.items():
        if not k.startswith("wavlm."):
            continue
        k = k[len("wavlm."):]
        for a, b in (("weight_g", "parametrizations.weight.original0"), ("weight_v", "parametrizations.weight.original1")):
            if k.endswith(a) and k not in own:
                k = k[: -len(a)] + b
        new[k] = torch.as_tensor(v).detach().cpu().to(dtype)
    missing, unexpected = model.load_state_dict(new, strict=False)
    assert not unexpected, unexpected
    assert all(m == "masked_spec_embed" for m in missing), missing
    return model


def _t_bn(x, w, p):
    import torch.nn.functional as F
    return F.batch_norm(x, w[p + "running_mean"], w[p + "running_var"], w[p + "weight"], w[p + "bias"], False, 0.0, BN_EPS)


def _t_crb(x, w, p, pad=0):
    import torch.nn.functional as F
    return _t_bn(F.relu(F.conv1d(x, w[p + "conv.weight"], w[p + "conv.bias"], padding=pad)), w, p + "bn.")


def torch_res2(x, w, p, dil, scale=8):
    """``Res2Conv1dReluBn`` on x [B, C, T] as seven separate convolutions (what tools/ecapa_bench.py times the one launch against)."""
    import torch
    import torch.nn.functional as F
    out, sp = [], None
    spx = torch.split(x, x.shape[1] // scale, 1)
    for i in range(scale - 1):
        sp = spx[i] if i == 0 else sp + spx[i]
        sp = _t_bn(F.relu(F.conv1d(sp, w[f"{p}convs.{i}.weight"], w[f"{p}convs.{i}.bias"], padding=dil, dilation=dil)), w, f"{p}bns.{i}.")
        out.append(sp)
    out.append(spx[scale - 1])
    return torch.cat(out, dim=1)


def torch_head(cfg, w, hidden):
    """The list of hidden states [B, T, H] -> (instance-normed mix [B, T, H], embeddings [B, emb_dim]): a transcription of
    ``ECAPA_TDNN.forward`` after the upstream, in torch ops."""
    import torch
    import torch.nn.functional as F
    lw = torch.softmax(w["feature_weight"], dim=-1)
    x = sum(lw[i] * h for i, h in enumerate(hidden)).transpose(1, 2) + 1e-6            # [B, H, T]
    x = F.instance_norm(x, eps=IN_EPS)
    out1 = _t_crb(x, w, "layer1.", pad=2)
    outs, cur = [], out1
    for n, d in enumerate(cfg.dilations):
        p = f"layer{n + 2}."
        y = _t_crb(cur, w, p + "Conv1dReluBn1.")
        y = torch_res2(y, w, p + "Res2Conv1dReluBn.", d, cfg.res2_scale)
        y = _t_crb(y, w, p + "Conv1dReluBn2.")
        s = F.relu(F.linear(y.mean(dim=2), w[p + "SE_Connect.linear1.weight"], w[p + "SE_Connect.linear1.bias"]))
        s = torch.sigmoid(F.linear(s, w[p + "SE_Connect.linear2.weight"], w[p + "SE_Connect.linear2.bias"]))
        cur = y * s[:, :, None] + cur
        outs.append(cur)
    xc = F.relu(F.conv1d(torch.cat(outs, dim=1), w["conv.weight"], w["conv.bias"]))
    x_in = xc
    if cfg.global_context_att:
        cm = torch.mean(xc, dim=-1, keepdim=True).expand_as(xc)
        cs = torch.sqrt(torch.var(xc, dim=-1, keepdim=True) + 1e-10).expand_as(xc)
        x_in = torch.cat((xc, cm, cs), dim=1)
    a = torch.tanh(F.conv1d(x_in, w["pooling.linear1.weight"], w["pooling.linear1.bias"]))
    a = torch.softmax(F.conv1d(a, w["pooling.linear2.weight"], w["pooling.linear2.bias"]), dim=2)
    mean = torch.sum(a * xc, dim=2)
    std = torch.sqrt((torch.sum(a * xc ** 2, dim=2) - mean ** 2).clamp(min=1e-9))
    emb = F.linear(_t_bn(torch.cat([mean, std], dim=1), w, "bn."), w["linear.weight"], w["linear.bias"])
    return x.transpose(1, 2), emb


def torch_graph(cfg, w, x, do_normalize=True):
    import torch
    with torch.no_grad():
        return torch_head(cfg, w, torch_trunk(cfg, w, x, do_normalize))


def torch_forward_fp32(cfg, sd, wav, do_normalize=True):
    """``torch_graph`` in fp32 on the CPU for one utterance: raw samples [n] -> float32 (instance-normed mix [T, H], embedding) as numpy."""
    import torch
    w = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()}
    hid, emb = torch_graph(cfg, w, torch.from_numpy(np.asarray(wav, np.float32))[None], do_normalize)
    return hid[0].numpy(), emb[0].numpy()


def torch_res2_fp32(cfg, sd, block, x):
    """``torch_res2`` in fp32 on the CPU: x [T, channels] -> float32 [T, channels] as numpy."""
    import torch
    w = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items() if f"layer{block + 2}.Res2" in k}
    with torch.no_grad():
        y = torch_res2(torch.from_numpy(np.asarray(x, np.float32)).T[None], w, f"layer{block + 2}.Res2Conv1dReluBn.", cfg.dilations[block], cfg.res2_scale)
    return y[0].T.numpy()
