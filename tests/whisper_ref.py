"""Restatement of dex_tts_amd/whisper.py (csrc/whisper.hip): HF's ``WhisperForConditionalGeneration`` in eval mode - the log-mel
front end of ``WhisperFeatureExtractor``, the encoder, the decoder as a cached step, teacher-forced ``forward`` and the library's
greedy decoding - in float64 numpy, and the same graph in torch fp32 on the CPU (``torch_forward_fp32``), which the GPU tests use as
their yardstick: the device may lie ``NET_FACTOR`` times as far from the float64 restatement as that fp32 evaluation does, floored at
``NET_FLOOR`` of the largest magnitude (the rule and the two values of tests/asr_ref.py, for the reason given there).

tests/test_whisper_cpu.py holds the restatement to ``transformers``' own model and feature extractor in double precision.

``make_weights`` is not a default initialisation: default-scale random weights decode to one repeated token whatever the input is.
Matrices are uniform +-3 / sqrt(fan_in), ``q_proj`` / ``k_proj`` +-6 / sqrt(fan_in), biases 0, LayerNorm gains 1, the decoder's
positions uniform +-1, and ``make_features`` has standard deviation 2: that decodes to varied, input-dependent ids."""
import math
import types

import numpy as np
from scipy.special import erf

NET_FACTOR = 8.0
NET_FLOOR = 1e-6
N_FFT, HOP = 400, 160


def _cfg(**kw):
    base = dict(vocab_size=51866, num_mel_bins=128, d_model=1280, encoder_layers=32, encoder_attention_heads=20, encoder_ffn_dim=5120,
                decoder_layers=32, decoder_attention_heads=20, decoder_ffn_dim=5120, max_source_positions=1500, max_target_positions=448,
                scale_embedding=False, activation_function="gelu")
    base.update(kw)
    return types.SimpleNamespace(**base)


DEFAULT = _cfg()
# 1 s chunk: 50 encoder frames, below one 64-key tile
TINY = _cfg(vocab_size=96, num_mel_bins=80, d_model=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=256, decoder_layers=2,
            decoder_attention_heads=2, decoder_ffn_dim=256, max_source_positions=50, max_target_positions=32)
# 3 s chunk: 150 encoder frames, not a multiple of 64; a vocabulary that is no multiple of anything
WIDE = _cfg(vocab_size=1031, num_mel_bins=128, d_model=384, encoder_layers=1, encoder_attention_heads=6, encoder_ffn_dim=1536, decoder_layers=2,
            decoder_attention_heads=6, decoder_ffn_dim=1536, max_source_positions=150, max_target_positions=40)

ENC, DEC = "model.encoder.", "model.decoder."


def library_config(cfg):
    from dex_tts_amd import whisper
    return whisper.WhisperConfig(**vars(cfg))


def n_samples(cfg):
    return 2 * cfg.max_source_positions * HOP


def state_dict_shapes(cfg):
    """HF's ``WhisperForConditionalGeneration.state_dict()`` without ``proj_out.weight``, in its order."""
    d, out = cfg.d_model, {}

    def attn(p):
        out[p + "k_proj.weight"] = (d, d)
        for n in ("v_proj", "q_proj", "out_proj"):
            out[p + n + ".weight"], out[p + n + ".bias"] = (d, d), (d,)

    def ln(p):
        out[p + ".weight"], out[p + ".bias"] = (d,), (d,)

    def ffn(p, f):
        out[p + "fc1.weight"], out[p + "fc1.bias"], out[p + "fc2.weight"], out[p + "fc2.bias"] = (f, d), (f,), (d, f), (d,)

    out[ENC + "conv1.weight"], out[ENC + "conv1.bias"] = (d, cfg.num_mel_bins, 3), (d,)
    out[ENC + "conv2.weight"], out[ENC + "conv2.bias"] = (d, d, 3), (d,)
    out[ENC + "embed_positions.weight"] = (cfg.max_source_positions, d)
    for l in range(cfg.encoder_layers):
        p = f"{ENC}layers.{l}."
        attn(p + "self_attn."); ln(p + "self_attn_layer_norm"); ffn(p, cfg.encoder_ffn_dim); ln(p + "final_layer_norm")
    ln(ENC + "layer_norm")
    out[DEC + "embed_tokens.weight"] = (cfg.vocab_size, d)
    out[DEC + "embed_positions.weight"] = (cfg.max_target_positions, d)
    for l in range(cfg.decoder_layers):
        p = f"{DEC}layers.{l}."
        attn(p + "self_attn."); ln(p + "self_attn_layer_norm"); attn(p + "encoder_attn."); ln(p + "encoder_attn_layer_norm")
        ffn(p, cfg.decoder_ffn_dim); ln(p + "final_layer_norm")
    ln(DEC + "layer_norm")
    return out


def make_weights(cfg, seed=0):
    """Seeded float32 weights under HF's keys (the module docstring's recipe)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in state_dict_shapes(cfg).items():
        if k.endswith(".bias"):
            v = np.zeros(shape)
        elif "layer_norm" in k:
            v = np.ones(shape)
        elif k == DEC + "embed_positions.weight":
            v = rng.uniform(-1.0, 1.0, shape)
        else:
            a = (6.0 if ("q_proj" in k or "k_proj" in k) else 3.0) / math.sqrt(int(np.prod(shape[1:])))
            v = rng.uniform(-a, a, shape)
        sd[k] = v.astype(np.float32)
    return sd


def make_features(cfg, seed):
    """float32 [num_mel_bins, 2 x max_source_positions] of standard deviation 2."""
    return (2.0 * np.random.default_rng(1000 + seed).standard_normal((cfg.num_mel_bins, 2 * cfg.max_source_positions))).astype(np.float32)


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
def mel_filters(n_mels):
    """transformers.audio_utils.mel_filter_bank(201, n_mels, 0, 8000, 16000, norm='slaney', mel_scale='slaney') -> [201, n_mels]."""
    def hz2mel(f):
        f = np.asarray(f, np.float64)
        return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)

    def mel2hz(m):
        return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), 200.0 * m / 3.0)

    fft = np.linspace(0.0, 8000.0, N_FFT // 2 + 1)
    ff = mel2hz(np.linspace(hz2mel(0.0), hz2mel(8000.0), n_mels + 2))
    fd = np.diff(ff)
    slopes = ff[None, :] - fft[:, None]
    fb = np.maximum(0.0, np.minimum(-slopes[:, :-2] / fd[:-1], slopes[:, 2:] / fd[1:]))
    return fb * (2.0 / (ff[2:] - ff[:-2]))[None, :]


def log_mel(cfg, wav, dtype=np.float64):
    """One row of 16 kHz samples (at most one chunk) -> [num_mel_bins, 2 x max_source_positions], every step in ``dtype``."""
    N = n_samples(cfg)
    x = np.zeros(N, dtype)
    x[: len(wav)] = np.asarray(wav, dtype)
    x = np.pad(x, N_FFT // 2, mode="reflect")
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)
    T = N // HOP
    frames = x[np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]] * win               # the last (T + 1 th) frame is dropped
    k = np.arange(N_FFT // 2 + 1)
    ang = 2.0 * np.pi * ((k[:, None] * np.arange(N_FFT)[None, :]) % N_FFT) / N_FFT
    re, im = frames @ np.cos(ang).T.astype(dtype), frames @ np.sin(ang).T.astype(dtype)
    mel = (re * re + im * im) @ mel_filters(cfg.num_mel_bins).astype(dtype)                # [T, n_mels]
    ls = np.log10(np.maximum(mel, dtype(1e-10)))
    ls = np.maximum(ls, ls.max() - dtype(8.0))
    return ((ls + dtype(4.0)) / dtype(4.0)).T


def _gelu(x):
    return 0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))


def _ln(x, g, b, eps=1e-5):
    m = x.mean(axis=-1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


def _conv1d(x, w, b, stride):
    """x [T, Cin], w [Cout, Cin, 3], padding 1 -> [T', Cout]."""
    T, Cin = x.shape
    x = np.concatenate([np.zeros((1, Cin)), x, np.zeros((1, Cin))])
    To = (T + 2 - 3) // stride + 1
    win = x[np.arange(To)[:, None] * stride + np.arange(3)[None, :]]
    return np.einsum("tkc,ock->to", win, w, optimize=True) + b


def _f64(sd):
    return {k: np.asarray(v, np.float64) for k, v in sd.items()}


def _attend(q, k, v, nh):
    """q [Tq, d] (scaled), k, v [Tk, d] -> [Tq, d]; no mask."""
    Tq, d = q.shape
    q, k, v = (a.reshape(a.shape[0], nh, d // nh).transpose(1, 0, 2) for a in (q, k, v))
    s = q @ k.transpose(0, 2, 1)
    s = np.exp(s - s.max(axis=-1, keepdims=True))
    return ((s / s.sum(axis=-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(Tq, d)


def _proj(w, p, n, x):
    y = x @ w[p + n + ".weight"].T
    return y + w[p + n + ".bias"] if p + n + ".bias" in w else y


def encode(cfg, sd, feat, w=None):
    """features [num_mel_bins, 2 x max_source_positions] -> the encoder's last hidden state [max_source_positions, d_model]."""
    w = w or _f64(sd)
    x = np.asarray(feat, np.float64).T
    x = _gelu(_conv1d(x, w[ENC + "conv1.weight"], w[ENC + "conv1.bias"], 1))
    h = _gelu(_conv1d(x, w[ENC + "conv2.weight"], w[ENC + "conv2.bias"], 2)) + w[ENC + "embed_positions.weight"]
    nh, scale = cfg.encoder_attention_heads, (cfg.d_model // cfg.encoder_attention_heads) ** -0.5
    for l in range(cfg.encoder_layers):
        p = f"{ENC}layers.{l}."
        y = _ln(h, w[p + "self_attn_layer_norm.weight"], w[p + "self_attn_layer_norm.bias"])
        a = _attend(_proj(w, p + "self_attn.", "q_proj", y) * scale, _proj(w, p + "self_attn.", "k_proj", y), _proj(w, p + "self_attn.", "v_proj", y), nh)
        h = h + _proj(w, p + "self_attn.", "out_proj", a)
        y = _ln(h, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"])
        h = h + _proj(w, p, "fc2", _gelu(_proj(w, p, "fc1", y)))
    return _ln(h, w[ENC + "layer_norm.weight"], w[ENC + "layer_norm.bias"])


class Decoder:
    """The cached step of one utterance: the cross-attention K / V once, the self-attention cache position by position."""

    def __init__(self, cfg, sd, enc, w=None):
        self.cfg, self.w = cfg, w or _f64(sd)
        self.cross = [(_proj(self.w, f"{DEC}layers.{l}.encoder_attn.", "k_proj", enc), _proj(self.w, f"{DEC}layers.{l}.encoder_attn.", "v_proj", enc))
                      for l in range(cfg.decoder_layers)]
        self.k = [np.zeros((0, cfg.d_model)) for _ in range(cfg.decoder_layers)]
        self.v = [np.zeros((0, cfg.d_model)) for _ in range(cfg.decoder_layers)]

    def step_logits(self, tok, p):
        """The logits [V] after feeding id ``tok`` at position ``p`` (= the cache's length)."""
        cfg, w = self.cfg, self.w
        assert p == len(self.k[0]) and p < cfg.max_target_positions
        nh, scale = cfg.decoder_attention_heads, (cfg.d_model // cfg.decoder_attention_heads) ** -0.5
        h = (w[DEC + "embed_tokens.weight"][tok] + w[DEC + "embed_positions.weight"][p])[None]
        for l in range(cfg.decoder_layers):
            pl = f"{DEC}layers.{l}."
            y = _ln(h, w[pl + "self_attn_layer_norm.weight"], w[pl + "self_attn_layer_norm.bias"])
            self.k[l] = np.concatenate([self.k[l], _proj(w, pl + "self_attn.", "k_proj", y)])
            self.v[l] = np.concatenate([self.v[l], _proj(w, pl + "self_attn.", "v_proj", y)])
            h = h + _proj(w, pl + "self_attn.", "out_proj", _attend(_proj(w, pl + "self_attn.", "q_proj", y) * scale, self.k[l], self.v[l], nh))
            y = _ln(h, w[pl + "encoder_attn_layer_norm.weight"], w[pl + "encoder_attn_layer_norm.bias"])
            ck, cv = self.cross[l]
            h = h + _proj(w, pl + "encoder_attn.", "out_proj", _attend(_proj(w, pl + "encoder_attn.", "q_proj", y) * scale, ck, cv, nh))
            y = _ln(h, w[pl + "final_layer_norm.weight"], w[pl + "final_layer_norm.bias"])
            h = h + _proj(w, pl, "fc2", _gelu(_proj(w, pl, "fc1", y)))
        h = _ln(h, w[DEC + "layer_norm.weight"], w[DEC + "layer_norm.bias"])
        return (h @ w[DEC + "embed_tokens.weight"].T)[0]


def step_logits(dec, tok, p):
    return dec.step_logits(tok, p)


def forward(cfg, sd, feat, ids):
    """Teacher-forced: features of one utterance, decoder ids [L] -> (encoder output [S, d], logits [L, V]), float64."""
    w = _f64(sd)
    enc = encode(cfg, sd, feat, w)
    dec = Decoder(cfg, sd, enc, w)
    return enc, np.stack([dec.step_logits(int(t), p) for p, t in enumerate(ids)])


def spec(prompt, suppress=(), begin_suppress=(), eos=0):
    return types.SimpleNamespace(prompt_ids=tuple(prompt), suppress_tokens=tuple(suppress), begin_suppress_tokens=tuple(begin_suppress),
                                 eos_token_id=int(eos))


def masked(logits, sp, i):
    """The logits of new-token step i under the spec's masks (-inf)."""
    x = np.array(logits, np.float64)
    x[list(sp.suppress_tokens)] = -np.inf
    if i == 0:
        x[list(sp.begin_suppress_tokens)] = -np.inf
    return x


def greedy(cfg, sd, feat, sp, max_new=None, step_fn=None):
    """The library's greedy decoding of one utterance -> (ids of every step until the row's eos, the loop's cap or ``max_new``, eos
    included; the masked float64 logits of those steps).  ``step_fn(tok, p) -> logits`` replaces the float64 decoder."""
    if step_fn is None:
        w = _f64(sd)
        dec = Decoder(cfg, sd, encode(cfg, sd, feat, w), w)
        step_fn = dec.step_logits
    room = cfg.max_target_positions - len(sp.prompt_ids)
    n_new = room if max_new is None else min(max_new, room)
    for p, t in enumerate(sp.prompt_ids[:-1]):
        step_fn(int(t), p)
    tok, ids, rows = int(sp.prompt_ids[-1]), [], []
    for i in range(n_new):
        x = masked(step_fn(tok, len(sp.prompt_ids) - 1 + i), sp, i)
        tok = int(np.argmax(x))
        ids.append(tok)
        rows.append(x)
        if tok == sp.eos_token_id:
            break
    return ids, np.stack(rows) if rows else np.zeros((0, cfg.vocab_size))


def top2_margin(logits):
    s = np.sort(np.asarray(logits, np.float64), axis=-1)
    return s[..., -1] - s[..., -2]


# ---------------------------------------------------------------------------------------------------- torch fp32 (the yardstick)
def torch_graph(cfg, w, feat, ids):
    """The same graph with torch's operators on whatever device and dtype the tensors have: ``w`` the state dict as tensors, ``feat``
    [B, n_mels, frames], ``ids`` [B, L] -> (encoder output [B, S, d], logits [B, L, V]); the decoder over all positions at once
    under a causal mask."""
    import torch
    import torch.nn.functional as F
    d = cfg.d_model

    def proj(p, n, x):
        return F.linear(x, w[p + n + ".weight"], w.get(p + n + ".bias"))

    def attend(q, k, v, nh, mask=None):
        B, Tq, _ = q.shape
        q, k, v = (a.reshape(B, a.shape[1], nh, d // nh).transpose(1, 2) for a in (q, k, v))
        s = q @ k.transpose(2, 3)
        if mask is not None:
            s = s + mask
        return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, Tq, d)

    def ln(x, p):
        return F.layer_norm(x, (d,), w[p + ".weight"], w[p + ".bias"], 1e-5)

    with torch.no_grad():
        x = F.gelu(F.conv1d(feat, w[ENC + "conv1.weight"], w[ENC + "conv1.bias"], padding=1))
        x = F.gelu(F.conv1d(x, w[ENC + "conv2.weight"], w[ENC + "conv2.bias"], stride=2, padding=1))
        h = x.transpose(1, 2) + w[ENC + "embed_positions.weight"]
        nh, scale = cfg.encoder_attention_heads, (d // cfg.encoder_attention_heads) ** -0.5
        for l in range(cfg.encoder_layers):
            p = f"{ENC}layers.{l}."
            y = ln(h, p + "self_attn_layer_norm")
            h = h + proj(p + "self_attn.", "out_proj", attend(proj(p + "self_attn.", "q_proj", y) * scale, proj(p + "self_attn.", "k_proj", y),
                                                              proj(p + "self_attn.", "v_proj", y), nh))
            h = h + proj(p, "fc2", F.gelu(proj(p, "fc1", ln(h, p + "final_layer_norm"))))
        enc = ln(h, ENC + "layer_norm")
        L = ids.shape[1]
        h = w[DEC + "embed_tokens.weight"][ids] + w[DEC + "embed_positions.weight"][:L]
        causal = torch.full((L, L), float("-inf"), dtype=h.dtype, device=h.device).triu(1)
        nh, scale = cfg.decoder_attention_heads, (d // cfg.decoder_attention_heads) ** -0.5
        for l in range(cfg.decoder_layers):
            p = f"{DEC}layers.{l}."
            y = ln(h, p + "self_attn_layer_norm")
            h = h + proj(p + "self_attn.", "out_proj", attend(proj(p + "self_attn.", "q_proj", y) * scale, proj(p + "self_attn.", "k_proj", y),
                                                              proj(p + "self_attn.", "v_proj", y), nh, causal))
            y = ln(h, p + "encoder_attn_layer_norm")
            h = h + proj(p + "encoder_attn.", "out_proj", attend(proj(p + "encoder_attn.", "q_proj", y) * scale, proj(p + "encoder_attn.", "k_proj", enc),
                                                                 proj(p + "encoder_attn.", "v_proj", enc), nh))
            h = h + proj(p, "fc2", F.gelu(proj(p, "fc1", ln(h, p + "final_layer_norm"))))
        return enc, F.linear(ln(h, DEC + "layer_norm"), w[DEC + "embed_tokens.weight"])


def torch_forward_fp32(cfg, sd, feat, ids):
    """``torch_graph`` in fp32 on the CPU for one utterance -> (encoder output [S, d], logits [L, V]), float32 numpy."""
    import torch
    w = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()}
    enc, lg = torch_graph(cfg, w, torch.from_numpy(np.asarray(feat, np.float32))[None], torch.from_numpy(np.asarray(ids, np.int64))[None])
    return enc[0].numpy(), lg[0].numpy()


def tolerance(yard, ref):
    """(bound, yardstick distance): NET_FACTOR x the fp32 CPU evaluation's distance from the float64 restatement, floored at
    NET_FLOOR of the largest magnitude."""
    d = float(np.abs(np.asarray(yard, np.float64) - ref).max())
    return max(NET_FACTOR * d, NET_FLOOR * float(np.abs(ref).max())), d
