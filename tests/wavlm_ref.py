"""Restatement of the WavLM x-vector path of dex_tts_amd/wavlm.py (csrc/wavlm.hip): HF's ``WavLMForXVector`` forward in eval mode with
``attention_mask=None`` for the group-norm / post-layer-norm family, one utterance at its own length - in float64 numpy
(``forward``), and the same graph in torch ops (``torch_graph``), which in fp32 on the CPU is the GPU tests' yardstick
(``torch_forward_fp32``) and on the GPU is what tools/sim_bench.py times.  The tolerance rule is tests/asr_ref.py's: the device may lie
``NET_FACTOR`` = 8 times as far from the float64 restatement as the fp32 CPU evaluation does, floored at 1e-6 of the largest magnitude.

tests/test_wavlm_cpu.py holds ``forward`` to ``transformers``' own model in double precision."""
import math
import types

import numpy as np

from tests.asr_ref import NET_FACTOR, NET_FLOOR, _conv1d, _gelu, _ln, fold_weight_norm, normalize_input, synth_wav  # noqa: F401

GN_EPS = 1e-5                      # nn.GroupNorm's default, which WavLMGroupNormConvLayer does not override


def _cfg(**kw):
    base = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_bias=False,
                feat_extract_norm="group", hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                do_stable_layer_norm=False, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
                num_buckets=320, max_bucket_distance=800, use_weighted_layer_sum=True, tdnn_dim=(512, 512, 512, 512, 1500),
                tdnn_kernel=(5, 3, 3, 1, 1), tdnn_dilation=(1, 2, 3, 1, 1), xvector_output_dim=512, hidden_act="gelu",
                feat_extract_activation="gelu")
    base.update(kw)
    return types.SimpleNamespace(**base)


def variant(cfg, **kw):
    return _cfg(**{**vars(cfg), **kw})


DEFAULT = _cfg()
TINY = _cfg(conv_dim=(32,) * 7, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256,
            num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, num_buckets=32, max_bucket_distance=40,
            tdnn_dim=(64, 64, 64, 64, 96), xvector_output_dim=32)
WIDE = _cfg(num_hidden_layers=1)

FE, ENC, FP = "wavlm.feature_extractor.conv_layers.", "wavlm.encoder.", "wavlm.feature_projection."


def library_config(cfg):
    from dex_tts_amd import wavlm
    return wavlm.WavLMConfig(**vars(cfg))


def num_frames(cfg, n):
    for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def tdnn_frames(cfg, T):
    return T - sum((k - 1) * d for k, d in zip(cfg.tdnn_kernel, cfg.tdnn_dilation))


def state_dict_shapes(cfg):
    out = {}
    for l, (c, k) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel)):
        out[f"{FE}{l}.conv.weight"] = (c, cfg.conv_dim[l - 1] if l else 1, k)
        if cfg.conv_bias:
            out[f"{FE}{l}.conv.bias"] = (c,)
        if l == 0:
            out[f"{FE}0.layer_norm.weight"], out[f"{FE}0.layer_norm.bias"] = (c,), (c,)
    C, H, I, nh = cfg.conv_dim[-1], cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
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
        out[p + "attention.gru_rel_pos_const"] = (1, nh, 1, 1)
        out[p + "attention.gru_rel_pos_linear.weight"], out[p + "attention.gru_rel_pos_linear.bias"] = (8, H // nh), (8,)
        if l == 0:
            out[p + "attention.rel_attn_embed.weight"] = (cfg.num_buckets, nh)
        out[p + "layer_norm.weight"], out[p + "layer_norm.bias"] = (H,), (H,)
        out[p + "feed_forward.intermediate_dense.weight"], out[p + "feed_forward.intermediate_dense.bias"] = (I, H), (I,)
        out[p + "feed_forward.output_dense.weight"], out[p + "feed_forward.output_dense.bias"] = (H, I), (H,)
        out[p + "final_layer_norm.weight"], out[p + "final_layer_norm.bias"] = (H,), (H,)
    if cfg.use_weighted_layer_sum:
        out["layer_weights"] = (cfg.num_hidden_layers + 1,)
    out["projector.weight"], out["projector.bias"] = (cfg.tdnn_dim[0], H), (cfg.tdnn_dim[0],)
    for i, (d, k) in enumerate(zip(cfg.tdnn_dim, cfg.tdnn_kernel)):
        din = cfg.tdnn_dim[i - 1] if i else cfg.tdnn_dim[0]
        out[f"tdnn.{i}.kernel.weight"], out[f"tdnn.{i}.kernel.bias"] = (d, din * k), (d,)
    out["feature_extractor.weight"], out["feature_extractor.bias"] = (cfg.xvector_output_dim, 2 * cfg.tdnn_dim[-1]), (cfg.xvector_output_dim,)
    return out


HEAD_GAIN, HEAD_BIAS = 2.0, 1.5


def make_weights(cfg, seed=0):
    """Seeded float32 weights under HF's keys, as tests/asr_ref.py makes them (matrices N(0, 1 / fan_in), LayerNorm gains 1 + 0.2 N,
    biases 0.1 N, a weight-norm g that is NOT the norm of v), with what this network needs on top:

      * a gate that does something: ``gru_rel_pos_const`` in [0.3, 0.8] or [1.2, 1.7], different per head and never 1;
        ``rel_attn_embed`` N(0, 1) (unit scale against scores of order 1); ``gru_rel_pos_linear`` N(0, 1 / 16) so the sigmoids leave
        their midpoint; ``layer_weights`` N(0, 1), far from uniform.
      * embeddings that depend on the input: after a post-norm encoder every frame has unit scale whatever the wav was, and a mean
        over frames of a default-initialised head is nearly a constant.  The head's matrices (projector, TDNN) are HEAD_GAIN times
        N(0, 1 / fan_in) and the TDNN biases are NEGATIVE (-1.5 +- 0.1): a ReLU channel is then on for part of the frames only, and which
        part depends on the input, so both the means and the deviations move with it.  Some channels are off on every frame
        (deviation exactly 0).  tests/test_wavlm_cpu.py asserts the sensitivity (two wavs' embeddings differ by >= 10 % of their norm)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in state_dict_shapes(cfg).items():
        head = k.startswith(("projector.", "tdnn."))
        if k.endswith("weight_g"):
            v = 0.5 + rng.random(shape)
        elif k.endswith("gru_rel_pos_const"):
            v = np.where(rng.random(shape) < 0.5, 0.3, 1.2) + 0.5 * rng.random(shape)
        elif k.endswith("rel_attn_embed.weight") or k == "layer_weights":
            v = rng.standard_normal(shape)
        elif k.endswith("gru_rel_pos_linear.weight"):
            v = 0.25 * rng.standard_normal(shape)
        elif "layer_norm.weight" in k:
            v = 1.0 + 0.2 * rng.standard_normal(shape)
        elif k.endswith(".bias"):
            v = 0.1 * rng.standard_normal(shape) - (HEAD_BIAS if k.startswith("tdnn.") else 0.0)
        else:
            v = rng.standard_normal(shape) * ((HEAD_GAIN if head else 1.0) / math.sqrt(int(np.prod(shape[1:]))))
        sd[k] = v.astype(np.float32)
    return sd


def dc_wav(n, seed, dc=0.3, amp=0.01):
    """A small signal on a large constant: what a one-pass variance loses."""
    return (dc + synth_wav(n, seed, amp)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- float64 numpy
def relative_position_buckets(cfg, n):
    """``_relative_positions_bucket`` of the distances key - query = -(n - 1) .. n - 1 in float64 -> int64 [2 n - 1]."""
    d = np.arange(-(n - 1), n)
    nb = cfg.num_buckets // 2
    exact = nb // 2
    a = np.abs(d)
    big = exact + (np.log(np.maximum(a, 1) / exact) / math.log(cfg.max_bucket_distance / exact) * (nb - exact)).astype(np.int64)
    return (d > 0) * nb + np.where(a < exact, a, np.minimum(big, nb - 1))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward(cfg, sd, wav, do_normalize=False):
    """One utterance: raw samples [n] -> (float64 layer-mixed hidden states [T, H], float64 embeddings [xvector_output_dim])."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}
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
    rel = w[f"{ENC}layers.0.attention.rel_attn_embed.weight"][relative_position_buckets(cfg, T)]          # [2T - 1, nh]
    bias = rel[np.arange(T)[None, :] - np.arange(T)[:, None] + T - 1].transpose(2, 0, 1)               # [nh, query, key]
    hidden = [h]
    for l in range(cfg.num_hidden_layers):
        p = f"{ENC}layers.{l}."
        xh = h.reshape(T, nh, hd).transpose(1, 0, 2)
        pr = (xh @ w[p + "attention.gru_rel_pos_linear.weight"].T + w[p + "attention.gru_rel_pos_linear.bias"]).reshape(nh, T, 2, 4).sum(-1)
        ga, gb = _sigmoid(pr[..., 0]), _sigmoid(pr[..., 1])
        gate = ga * (gb * w[p + "attention.gru_rel_pos_const"].reshape(nh, 1) - 1.0) + 2.0              # [nh, T]
        q = (h @ w[p + "attention.q_proj.weight"].T + w[p + "attention.q_proj.bias"]) * hd ** -0.5
        k = h @ w[p + "attention.k_proj.weight"].T + w[p + "attention.k_proj.bias"]
        v = h @ w[p + "attention.v_proj.weight"].T + w[p + "attention.v_proj.bias"]
        q, k, v = (a.reshape(T, nh, hd).transpose(1, 0, 2) for a in (q, k, v))
        s = q @ k.transpose(0, 2, 1) + gate[:, :, None] * bias
        s = np.exp(s - s.max(axis=-1, keepdims=True))
        a = ((s / s.sum(axis=-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(T, H)
        h = _ln(h + a @ w[p + "attention.out_proj.weight"].T + w[p + "attention.out_proj.bias"], w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], eps)
        y = _gelu(h @ w[p + "feed_forward.intermediate_dense.weight"].T + w[p + "feed_forward.intermediate_dense.bias"])
        h = _ln(h + y @ w[p + "feed_forward.output_dense.weight"].T + w[p + "feed_forward.output_dense.bias"], w[p + "final_layer_norm.weight"],
                w[p + "final_layer_norm.bias"], eps)
        hidden.append(h)
    if cfg.use_weighted_layer_sum:
        lw = np.exp(w["layer_weights"] - w["layer_weights"].max())
        lw = lw / lw.sum()
        mixed = sum(a * b for a, b in zip(lw, hidden))
    else:
        mixed = hidden[-1]
    return mixed, pooled_statistics(cfg, w, mixed) @ w["feature_extractor.weight"].T + w["feature_extractor.bias"]


def pooled_statistics(cfg, w, mixed):
    """The head up to statistics pooling: hidden states [T, H] -> float64 [2 C]: the TDNN channels' means, then their unbiased
    deviations (``w``: the state dict as float64 arrays)."""
    x = mixed @ w["projector.weight"].T + w["projector.bias"]
    for i, (k, d) in enumerate(zip(cfg.tdnn_kernel, cfg.tdnn_dilation)):
        W = w[f"tdnn.{i}.kernel.weight"].reshape(cfg.tdnn_dim[i], k, -1)                                # [out, tap, in]
        To = x.shape[0] - (k - 1) * d
        y = w[f"tdnn.{i}.kernel.bias"] + sum(x[j * d: j * d + To] @ W[:, j].T for j in range(k))
        x = np.maximum(y, 0.0)
    return np.concatenate([x.mean(axis=0), x.std(axis=0, ddof=1)])


def cosine(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(a @ b / math.sqrt((a @ a) * (b @ b)))


# ---------------------------------------------------------------------------------------------------- torch ops (the yardstick, the bench)
def torch_graph(cfg, w, x, do_normalize=False):
    """The same graph with torch's operators on whatever device and dtype the tensors have: ``w`` the state dict as tensors, ``x``
    [B, n] raw samples of equal length -> (hidden [B, T, H], embeddings [B, xvector_output_dim]).  The group norm is per sample, and
    the rows are all n samples long: row b is the row alone."""
    import torch
    import torch.nn.functional as F
    eps = cfg.layer_norm_eps
    with torch.no_grad():
        if do_normalize:
            x = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + 1e-7)
        x = x[:, None]                                                                        # [B, 1, n]
        for l, s in enumerate(cfg.conv_stride):
            x = F.conv1d(x, w[f"{FE}{l}.conv.weight"], w.get(f"{FE}{l}.conv.bias"), stride=s)
            if l == 0:
                x = F.group_norm(x, x.shape[1], w[f"{FE}0.layer_norm.weight"], w[f"{FE}0.layer_norm.bias"], GN_EPS)
            x = F.gelu(x)
        x = x.transpose(1, 2)                                                                 # [B, T, C]
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
        idx = torch.from_numpy(relative_position_buckets(cfg, T)).to(h.device)
        rel = w[f"{ENC}layers.0.attention.rel_attn_embed.weight"][idx]                        # [2T - 1, nh]
        ar = torch.arange(T, device=h.device)
        bias = rel[ar[None, :] - ar[:, None] + T - 1].permute(2, 0, 1)                        # [nh, query, key]
        lw = torch.softmax(w["layer_weights"], dim=-1) if cfg.use_weighted_layer_sum else None
        mixed = lw[0] * h if lw is not None else None
        for l in range(cfg.num_hidden_layers):
            p = f"{ENC}layers.{l}."
            xh = h.reshape(B, T, nh, hd).transpose(1, 2)
            pr = F.linear(xh, w[p + "attention.gru_rel_pos_linear.weight"], w[p + "attention.gru_rel_pos_linear.bias"]).reshape(B, nh, T, 2, 4).sum(-1)
            ga, gb = torch.sigmoid(pr[..., 0]), torch.sigmoid(pr[..., 1])
            gate = ga * (gb * w[p + "attention.gru_rel_pos_const"].reshape(1, nh, 1) - 1.0) + 2.0
            q = F.linear(h, w[p + "attention.q_proj.weight"], w[p + "attention.q_proj.bias"]) * hd ** -0.5
            k = F.linear(h, w[p + "attention.k_proj.weight"], w[p + "attention.k_proj.bias"])
            v = F.linear(h, w[p + "attention.v_proj.weight"], w[p + "attention.v_proj.bias"])
            q, k, v = (a.reshape(B, T, nh, hd).transpose(1, 2) for a in (q, k, v))
            a = torch.softmax(q @ k.transpose(2, 3) + gate[..., None] * bias, dim=-1) @ v
            a = a.transpose(1, 2).reshape(B, T, H)
            h = F.layer_norm(h + F.linear(a, w[p + "attention.out_proj.weight"], w[p + "attention.out_proj.bias"]), (H,), w[p + "layer_norm.weight"],
                             w[p + "layer_norm.bias"], eps)
            y = F.gelu(F.linear(h, w[p + "feed_forward.intermediate_dense.weight"], w[p + "feed_forward.intermediate_dense.bias"]))
            h = F.layer_norm(h + F.linear(y, w[p + "feed_forward.output_dense.weight"], w[p + "feed_forward.output_dense.bias"]), (H,),
                             w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], eps)
            if lw is not None:
                mixed = mixed + lw[l + 1] * h
        if lw is None:
            mixed = h
        x = F.linear(mixed, w["projector.weight"], w["projector.bias"]).transpose(1, 2)       # [B, C, T]
        for i, (k, d) in enumerate(zip(cfg.tdnn_kernel, cfg.tdnn_dilation)):
            W = w[f"tdnn.{i}.kernel.weight"].reshape(cfg.tdnn_dim[i], k, -1).transpose(1, 2)
            x = F.relu(F.conv1d(x, W, w[f"tdnn.{i}.kernel.bias"], dilation=d))
        stats = torch.cat([x.mean(dim=2), x.std(dim=2)], dim=1)
        return mixed, F.linear(stats, w["feature_extractor.weight"], w["feature_extractor.bias"])


def torch_forward_fp32(cfg, sd, wav, do_normalize=False):
    """``torch_graph`` in fp32 on the CPU for one utterance: raw samples [n] -> float32 (hidden [T, H], embeddings) as numpy."""
    import torch
    w = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()}
    hid, emb = torch_graph(cfg, w, torch.from_numpy(np.asarray(wav, np.float32))[None], do_normalize)
    return hid[0].numpy(), emb[0].numpy()


def tolerance(yard, ref):
    """(bound, yardstick distance): NET_FACTOR x the fp32 CPU evaluation's distance from the float64 restatement, floored at
    NET_FLOOR of the largest magnitude."""
    d = float(np.abs(np.asarray(yard, np.float64) - ref).max())
    return max(NET_FACTOR * d, NET_FLOOR * float(np.abs(ref).max())), d
