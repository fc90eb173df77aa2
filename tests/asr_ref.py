"""Restatement of the ASR path of dex_tts_amd/asr.py (csrc/asr.hip): HF's ``Wav2Vec2ForCTC`` forward in eval mode for the
layer-norm / stable-layer-norm family, input normalisation, greedy CTC and decoding - in float64 numpy (``forward``), and the same
graph in torch fp32 on the CPU (``torch_forward_fp32``), which the GPU tests use as their yardstick: the device may lie
``NET_FACTOR`` times as far from the float64 restatement as that fp32 evaluation does, floored at ``NET_FLOOR`` of the largest
|logit| (the two values of tests/speaker_ref.py, for the reason given there: two correct fp32 evaluations of one graph differ by
a small multiple of either's distance from the exact result, and a yardstick that lands near 0 must not demand the impossible).

tests/test_asr_cpu.py holds ``forward`` to ``transformers``' own model in double precision (1e-10) where that is installed, and to a
recorded fixture of it where it is not.  A batch row is computed on its own length: with an attention mask HF's padded batch gives
the same valid frames (the feature extractor's valid frames lie inside the utterance, masked rows enter the positional convolution
as the zeros its padding would be, masked keys get no weight)."""
import math
import types

import numpy as np
from scipy.special import erf

NET_FACTOR = 8.0
NET_FLOOR = 1e-6

VOCAB = ("<pad>", "<s>", "</s>", "<unk>", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M", "W", "C", "F", "G", "Y", "P",
         "B", "V", "K", "'", "X", "J", "Q", "Z")


def _cfg(**kw):
    base = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_bias=True,
                feat_extract_norm="layer", hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                do_stable_layer_norm=True, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
                vocab_size=32, hidden_act="gelu", feat_extract_activation="gelu")
    base.update(kw)
    return types.SimpleNamespace(**base)


DEFAULT = _cfg()
TINY = _cfg(conv_dim=(32,) * 7, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
            num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
WIDE = _cfg(num_hidden_layers=1)

FE, ENC, FP = "wav2vec2.feature_extractor.conv_layers.", "wav2vec2.encoder.", "wav2vec2.feature_projection."


def library_config(cfg):
    from dex_tts_amd import asr
    return asr.Wav2Vec2Config(**vars(cfg))


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
        out[f"{FE}{l}.layer_norm.weight"] = (c,)
        out[f"{FE}{l}.layer_norm.bias"] = (c,)
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
    out["lm_head.weight"], out["lm_head.bias"] = (cfg.vocab_size, H), (cfg.vocab_size,)
    return out


def make_weights(cfg, seed=0, lm_scale=6.0):
    """Seeded float32 weights under HF's keys: matrices N(0, 1 / fan_in), LayerNorm gains 1 + 0.2 N, biases 0.1 N, a weight-norm g
    that is NOT the norm of v, and an ``lm_head`` ``lm_scale`` times larger, so that the frames' top-2 margins stand clear of fp32
    noise (tests/test_gpu_asr.py records the share that does not)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in state_dict_shapes(cfg).items():
        if k.endswith("weight_g"):
            v = 0.5 + rng.random(shape)
        elif "layer_norm.weight" in k:
            v = 1.0 + 0.2 * rng.standard_normal(shape)
        elif k.endswith(".bias"):
            v = 0.1 * rng.standard_normal(shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            v = rng.standard_normal(shape) * ((lm_scale if k.startswith("lm_head") else 1.0) / math.sqrt(fan_in))
        sd[k] = v.astype(np.float32)
    return sd


def synth_wav(n, seed, amp=0.1):
    """A few drifting partials and noise, float32 in [-1, 1]: not speech, but no constant either."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = np.zeros(n)
    for _ in range(4):
        f0, dr, ph = rng.uniform(90, 2400), rng.uniform(-300, 300), rng.uniform(0, 2 * np.pi)
        x += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (f0 * t + 0.5 * dr * t * t) + ph)
    x += 0.3 * rng.standard_normal(n)
    return (amp * x / np.abs(x).max()).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- float64 numpy
def normalize_input(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    return (x - x.mean()) / np.sqrt(x.var() + dtype(1e-7))


def _gelu(x):
    return 0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))


def _ln(x, g, b, eps):
    m = x.mean(axis=-1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


def _conv1d(x, w, b, stride=1, pad=0, groups=1):
    """x [T, Cin], w [Cout, Cin / groups, k] -> [T', Cout]."""
    T, Cin = x.shape
    Cout, cg, k = w.shape
    if pad:
        x = np.concatenate([np.zeros((pad, Cin), x.dtype), x, np.zeros((pad, Cin), x.dtype)])
    To = (x.shape[0] - k) // stride + 1
    idx = np.arange(To)[:, None] * stride + np.arange(k)[None, :]
    win = x[idx]                                            # [To, k, Cin]
    og = Cout // groups
    out = np.empty((To, Cout), x.dtype)
    for g in range(groups):
        out[:, g * og:(g + 1) * og] = np.einsum("tkc,ock->to", win[:, :, g * cg:(g + 1) * cg], w[g * og:(g + 1) * og], optimize=True)
    return out if b is None else out + b


def fold_weight_norm(g, v):
    """weight_norm(dim = 2): g [1, 1, k] * v / ||v[:, :, k]||."""
    return g * v / np.sqrt((v ** 2).sum(axis=(0, 1), keepdims=True))


def forward(cfg, sd, wav):
    """One utterance: raw samples [n] -> float64 logits [T, V]."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    eps = cfg.layer_norm_eps
    x = normalize_input(wav)[:, None]
    for l, (k, s) in enumerate(zip(cfg.conv_kernel, cfg.conv_stride)):
        x = _conv1d(x, w[f"{FE}{l}.conv.weight"], w.get(f"{FE}{l}.conv.bias"), s)
        x = _gelu(_ln(x, w[f"{FE}{l}.layer_norm.weight"], w[f"{FE}{l}.layer_norm.bias"], eps))
    x = _ln(x, w[FP + "layer_norm.weight"], w[FP + "layer_norm.bias"], eps)
    h = x @ w[FP + "projection.weight"].T + w[FP + "projection.bias"]
    K = cfg.num_conv_pos_embeddings
    pw = fold_weight_norm(w[ENC + "pos_conv_embed.conv.weight_g"], w[ENC + "pos_conv_embed.conv.weight_v"])
    pos = _conv1d(h, pw, w[ENC + "pos_conv_embed.conv.bias"], 1, K // 2, cfg.num_conv_pos_embedding_groups)
    if K % 2 == 0:
        pos = pos[:-1]
    h = h + _gelu(pos)
    T, H = h.shape
    nh = cfg.num_attention_heads
    hd = H // nh
    for l in range(cfg.num_hidden_layers):
        p = f"{ENC}layers.{l}."
        y = _ln(h, w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], eps)
        q = (y @ w[p + "attention.q_proj.weight"].T + w[p + "attention.q_proj.bias"]) * hd ** -0.5
        k = y @ w[p + "attention.k_proj.weight"].T + w[p + "attention.k_proj.bias"]
        v = y @ w[p + "attention.v_proj.weight"].T + w[p + "attention.v_proj.bias"]
        q, k, v = (a.reshape(T, nh, hd).transpose(1, 0, 2) for a in (q, k, v))
        s = q @ k.transpose(0, 2, 1)
        s = np.exp(s - s.max(axis=-1, keepdims=True))
        a = (s / s.sum(axis=-1, keepdims=True)) @ v
        a = a.transpose(1, 0, 2).reshape(T, H)
        h = h + a @ w[p + "attention.out_proj.weight"].T + w[p + "attention.out_proj.bias"]
        y = _ln(h, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], eps)
        y = _gelu(y @ w[p + "feed_forward.intermediate_dense.weight"].T + w[p + "feed_forward.intermediate_dense.bias"])
        h = h + y @ w[p + "feed_forward.output_dense.weight"].T + w[p + "feed_forward.output_dense.bias"]
    h = _ln(h, w[ENC + "layer_norm.weight"], w[ENC + "layer_norm.bias"], eps)
    return h @ w["lm_head.weight"].T + w["lm_head.bias"]


def ctc_greedy(logits):
    """[T, V] -> ids: the first index of each frame's maximum, repeats collapsed, blank (0) dropped."""
    arg = np.argmax(np.asarray(logits), axis=-1)
    out, prev = [], -1
    for a in arg.tolist():
        if a != prev and a != 0:
            out.append(a)
        prev = a
    return out


def collapse(arg):
    """ctc_greedy from the per-frame ids."""
    out, prev = [], -1
    for a in list(arg):
        if a != prev and a != 0:
            out.append(int(a))
        prev = a
    return out


def decode(ids, vocab=VOCAB):
    return "".join(" " if vocab[i] == "|" else vocab[i] for i in ids).strip()


def top2_margin(logits):
    s = np.sort(np.asarray(logits, np.float64), axis=-1)
    return s[:, -1] - s[:, -2]


# ---------------------------------------------------------------------------------------------------- host strings
def levenshtein(a, b):
    d = np.zeros((len(a) + 1, len(b) + 1), np.int64)
    d[:, 0], d[0, :] = np.arange(len(a) + 1), np.arange(len(b) + 1)
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i, j] = min(d[i - 1, j] + 1, d[i, j - 1] + 1, d[i - 1, j - 1] + (a[i - 1] != b[j - 1]))
    return int(d[-1, -1])


def asr_score(texts, preds, normalize):
    """metric.py:46-67 from the transcripts: (cer_mean, cer_stderr, wer_mean, wer_stderr)."""
    c, w = [], []
    for t, p in zip(texts, preds):
        t, p = normalize(t), normalize(p)
        c.append(levenshtein(t, p) / len(t))
        w.append(levenshtein(t.split(), p.split()) / len(t.split()))
    n = len(c)
    return sum(c) / n, np.std(c) / np.sqrt(n), sum(w) / n, np.std(w) / np.sqrt(n)


# ---------------------------------------------------------------------------------------------------- torch fp32 (the yardstick)
def torch_graph(cfg, w, x):
    """The same graph with torch's operators on whatever device and dtype the tensors have: ``w`` the state dict as tensors, ``x``
    [B, n] raw samples of equal length -> logits [B, T, V].  (tools/asr_bench.py times it on the GPU.)"""
    import torch
    import torch.nn.functional as F
    eps = cfg.layer_norm_eps
    with torch.no_grad():
        x = ((x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + 1e-7))[:, None]      # [B, 1, n]
        for l, s in enumerate(cfg.conv_stride):
            x = F.conv1d(x, w[f"{FE}{l}.conv.weight"], w.get(f"{FE}{l}.conv.bias"), stride=s)
            C = x.shape[1]
            x = F.gelu(F.layer_norm(x.transpose(1, 2), (C,), w[f"{FE}{l}.layer_norm.weight"], w[f"{FE}{l}.layer_norm.bias"], eps)).transpose(1, 2)
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
        h = h + F.gelu(pos)
        B, T, H = h.shape
        nh = cfg.num_attention_heads
        hd = H // nh
        for l in range(cfg.num_hidden_layers):
            p = f"{ENC}layers.{l}."
            y = F.layer_norm(h, (H,), w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], eps)
            q = F.linear(y, w[p + "attention.q_proj.weight"], w[p + "attention.q_proj.bias"]) * hd ** -0.5
            k = F.linear(y, w[p + "attention.k_proj.weight"], w[p + "attention.k_proj.bias"])
            v = F.linear(y, w[p + "attention.v_proj.weight"], w[p + "attention.v_proj.bias"])
            q, k, v = (a.reshape(B, T, nh, hd).transpose(1, 2) for a in (q, k, v))
            a = torch.softmax(q @ k.transpose(2, 3), dim=-1) @ v
            a = a.transpose(1, 2).reshape(B, T, H)
            h = h + F.linear(a, w[p + "attention.out_proj.weight"], w[p + "attention.out_proj.bias"])
            y = F.layer_norm(h, (H,), w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], eps)
            y = F.gelu(F.linear(y, w[p + "feed_forward.intermediate_dense.weight"], w[p + "feed_forward.intermediate_dense.bias"]))
            h = h + F.linear(y, w[p + "feed_forward.output_dense.weight"], w[p + "feed_forward.output_dense.bias"])
        h = F.layer_norm(h, (H,), w[ENC + "layer_norm.weight"], w[ENC + "layer_norm.bias"], eps)
        return F.linear(h, w["lm_head.weight"], w["lm_head.bias"])


def torch_forward_fp32(cfg, sd, wav):
    """``torch_graph`` in fp32 on the CPU for one utterance: raw samples [n] -> float32 logits [T, V] (numpy)."""
    import torch
    w = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()}
    return torch_graph(cfg, w, torch.from_numpy(np.asarray(wav, np.float32))[None])[0].numpy()


def tolerance(yard, ref):
    """(bound, yardstick distance): NET_FACTOR x the fp32 CPU evaluation's distance from the float64 restatement, floored at
    NET_FLOOR of the largest |logit|."""
    d = float(np.abs(np.asarray(yard, np.float64) - ref).max())
    return max(NET_FACTOR * d, NET_FLOOR * float(np.abs(ref).max())), d
