"""The UTMOS naturalness score (MOS prediction) on the device: the third score zero-shot TTS work reports, next to WER and SIM.  A wav
at 16 kHz goes through the UTMOS22 "strong learner" in eval mode as its public demo scores a wav: the wav2vec 2.0 *base* trunk
(``last_hidden_state``), every frame concatenated with a domain and a listener embedding, a bidirectional LSTM, Linear - ReLU - Linear
per frame, and ``mean over the frames * 2 + 3``.

    MOSConfig(...)                                        HF ``Wav2Vec2Config`` names for the trunk, and the head's widths
    UTMOS(config=None, device='cuda', do_normalize=False):  load_state_dict, hidden_states -> [B, T, hidden], bilstm (the recurrence
                                                          alone) -> [B, T, 2 lstm_hidden], frame_scores -> [B, T], forward -> MOS [B],
                                                          score_utterances(wavs, ...)
    num_frames(n_samples, config=None), min_samples(config=None), state_dict_shapes(config=None), check_lengths(lengths, n)
    from_utmos_checkpoint(sd)                             the upstream Lightning checkpoint's keys -> ``load_state_dict``'s
    mos_score(wavs, ..., model=) -> (mean, stderr)

The network runs in libdexamd.so (``csrc/mos.hip``, C ABI ``dex_mos_*``), fp32 throughout.  Nothing downloads: weights come from a
dict or a local file the caller names, and the library ships no checkpoint.  Only this family is built (group-norm feature extractor,
post-layer-norm encoder, head_dim 64, erf GELU, one bidirectional LSTM layer of at most 512 units); any other config raises
``NotImplementedError`` naming the field.

What a caller comparing numbers must know:
  * the network and the checkpoint's key names were written down from a reading of the public model; this library has NOT been
    checked against the real UTMOS weights.  What it is held to is its own float64 restatement (tests/mos_ref.py), itself held to
    ``transformers.Wav2Vec2Model`` + ``torch.nn`` modules in double precision.
  * batching: row b of any batch is the network applied to row b ALONE at its own length - the group norm, the attention keys, the
    reverse direction of the LSTM (``pack_padded_sequence``: it starts at the row's own last frame) and the mean end there.
  * where a wav is not at 16 kHz it is resampled by the library's ``wavprep.resample`` (resampy's kaiser_best).
  * no input normalisation by default: fairseq's ``wav2vec_small`` has ``normalize=False``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional, Tuple

import numpy as np
import torch

from ._native import Handle, host_lengths, i32_ptr, on_device, stream
from ._wavnet import MAX_CONV, SAMPLING_RATE, HostEntry, WaveformNet, fill_trunk_config
from .speaker import mean_stderr  # noqa: F401  (this module's public name too)

MAX_FRAMES = 4096                  # DEX_MOS_MAX_FRAMES: the encoder frames one call takes (81 s)
MAX_LSTM = 512                     # DEX_MOS_MAX_LSTM
LSTM_ROWS = 4                      # rows one workgroup of the recurrence owns (csrc/mos.hip ROWS)
DOMAIN, JUDGE = 0, 288             # the ids the public demo scores with


@dataclasses.dataclass(frozen=True)
class MOSConfig:
    """HF ``Wav2Vec2Config`` fields of the trunk (the values of wav2vec2-base) and the widths of the UTMOS head."""
    conv_dim: Tuple[int, ...] = (512,) * 7
    conv_kernel: Tuple[int, ...] = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: Tuple[int, ...] = (5, 2, 2, 2, 2, 2, 2)
    conv_bias: bool = False
    feat_extract_norm: str = "group"
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    do_stable_layer_norm: bool = False
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    layer_norm_eps: float = 1e-5
    hidden_act: str = "gelu"
    feat_extract_activation: str = "gelu"
    num_domains: int = 3
    domain_dim: int = 128
    num_judges: int = 3000
    judge_dim: int = 128
    lstm_hidden: int = 512
    proj_hidden: int = 2048


class DexMosConfig(C.Structure):
    _fields_ = [("n_conv", C.c_int32), ("conv_dim", C.c_int32 * MAX_CONV), ("conv_kernel", C.c_int32 * MAX_CONV),
                ("conv_stride", C.c_int32 * MAX_CONV), ("conv_bias", C.c_int32), ("feat_extract_norm_group", C.c_int32),
                ("hidden", C.c_int32), ("n_layers", C.c_int32), ("n_heads", C.c_int32), ("intermediate", C.c_int32),
                ("do_stable_layer_norm", C.c_int32), ("num_conv_pos_embeddings", C.c_int32), ("num_conv_pos_embedding_groups", C.c_int32),
                ("layer_norm_eps", C.c_float), ("num_domains", C.c_int32), ("domain_dim", C.c_int32), ("num_judges", C.c_int32),
                ("judge_dim", C.c_int32), ("lstm_hidden", C.c_int32), ("proj_hidden", C.c_int32)]


def _c_config(cfg: MOSConfig) -> DexMosConfig:
    """The C struct of a config; ``NotImplementedError`` for what the struct cannot even express."""
    c = fill_trunk_config(DexMosConfig(), cfg)
    c.feat_extract_norm_group = int(cfg.feat_extract_norm == "group")
    for name in ("num_domains", "domain_dim", "num_judges", "judge_dim", "lstm_hidden", "proj_hidden"):
        setattr(c, name, int(getattr(cfg, name)))
    return c


_HOST = HostEntry("dex_mos", _c_config, MOSConfig, "MOSConfig")


def num_frames(n_samples: int, config: Optional[MOSConfig] = None) -> int:
    """Encoder frames of ``n_samples`` samples: ``floor((L - k) / s) + 1`` chained over the feature extractor.  Host integers."""
    return _HOST.num_frames(n_samples, config)


def min_samples(config: Optional[MOSConfig] = None) -> int:
    """The fewest samples a row may have: one encoder frame (400 with the default geometry).  Host integers."""
    return _HOST.min_samples(config)


def _ignored(key: str) -> bool:
    """The one training-side key ``Wav2Vec2Model`` carries."""
    return key == "wav2vec2.masked_spec_embed"


def state_dict_shapes(config: Optional[MOSConfig] = None) -> dict:
    """The keys the network of ``config`` needs, with their shapes: HF ``Wav2Vec2Model`` keys under ``wav2vec2.`` (weight norm in its
    ``weight_g`` / ``weight_v`` spelling), ``domain_embedding.weight``, ``judge_embedding.weight``, ``decoder_rnn.*_l0`` and
    ``*_l0_reverse``, ``projection.0.*`` and ``projection.3.*``; ``NotImplementedError`` naming the field for a config outside the
    family that is built.  Host only."""
    return _HOST.state_dict_shapes(config)


def check_lengths(lengths, n_samples: int, config: Optional[MOSConfig] = None, what: str = "mos") -> int:
    """What one call refuses, before anything is enqueued: a row below ``min_samples`` (``ValueError`` 'too short') and a padded
    length of more than ``MAX_FRAMES`` encoder frames.  Returns the frames of ``n_samples``.  Host only."""
    return _HOST.check_lengths(lengths, n_samples, config, what, "the feature extractor needs {need} samples for one frame", MAX_FRAMES)


_FAIRSEQ = (("self_attn_layer_norm.", "layer_norm."), ("self_attn.", "attention."), ("fc1.", "feed_forward.intermediate_dense."),
            ("fc2.", "feed_forward.output_dense."))
_SSL, _DROPPED = "feature_extractors.0.ssl_model.", ("mask_emb", "quantizer.", "project_q.", "final_proj.")
_HEAD = (("feature_extractors.1.embedding.weight", "domain_embedding.weight"),
         ("output_layers.0.judge_embedding.weight", "judge_embedding.weight"),
         ("output_layers.0.decoder_rnn.", "decoder_rnn."), ("output_layers.1.net.", "projection."))


def _fairseq_to_hf(k: str) -> str:
    """One fairseq wav2vec 2.0 key (without its model prefix) -> the HF ``Wav2Vec2Model`` key (without ``wav2vec2.``)."""
    p = k.split(".")
    if k.startswith("feature_extractor.conv_layers.") and len(p) == 5:
        if p[3] == "0":
            return ".".join(p[:3] + ["conv", p[4]])
        if p[2] == "0" and p[3] == "2":
            return ".".join(p[:3] + ["layer_norm", p[4]])
        return k
    if k.startswith("post_extract_proj."):
        return "feature_projection.projection." + k[len("post_extract_proj."):]
    if k.startswith("layer_norm."):
        return "feature_projection." + k
    if k.startswith("encoder.pos_conv.0."):
        return "encoder.pos_conv_embed.conv." + k[len("encoder.pos_conv.0."):]
    if k.startswith("encoder.layers."):
        for old, new in _FAIRSEQ:
            if f".{old}" in k:
                return k.replace(f".{old}", f".{new}", 1)
    return k


def from_utmos_checkpoint(sd) -> dict:
    """The upstream UTMOS Lightning checkpoint's ``state_dict`` -> the keys ``UTMOS.load_state_dict`` takes.  A pure rename, host only:
    ``feature_extractors.0.ssl_model.`` is stripped and fairseq's wav2vec 2.0 names become HF's under ``wav2vec2.``
    (``conv_layers.{i}.0`` -> ``{i}.conv``, ``conv_layers.0.2`` -> ``0.layer_norm``, ``post_extract_proj`` -> ``feature_projection.
    projection``, the top-level ``layer_norm`` -> ``feature_projection.layer_norm``, ``encoder.pos_conv.0`` -> ``encoder.pos_conv_embed.
    conv``, ``self_attn`` -> ``attention``, ``self_attn_layer_norm`` -> ``layer_norm``, ``fc1`` / ``fc2`` -> ``feed_forward.
    intermediate_dense`` / ``output_dense``); ``mask_emb``, ``quantizer.*``, ``project_q.*`` and ``final_proj.*`` are dropped; the head's
    ``feature_extractors.1.embedding``, ``output_layers.0.judge_embedding`` / ``decoder_rnn`` and ``output_layers.1.net`` become
    ``domain_embedding``, ``judge_embedding``, ``decoder_rnn`` and ``projection``.  Any other key is kept as it is, for ``strict`` to
    report.  The names come from a reading of the public model: this function has NOT been run on a real checkpoint."""
    out = {}
    for k, v in sd.items():
        if k.startswith(_SSL):
            k = k[len(_SSL):]
            if k.startswith(_DROPPED):
                continue
            out["wav2vec2." + _fairseq_to_hf(k)] = v
            continue
        for old, new in _HEAD:
            if k.startswith(old):
                k = new + k[len(old):]
                break
        out[k] = v
    return out


class UTMOS(WaveformNet):
    """The UTMOS22 strong learner in eval mode on one MI355X, fp32; a batch row is the row alone.  ``load_state_dict`` takes the keys
    of ``state_dict_shapes`` (``from_utmos_checkpoint`` renames the upstream checkpoint's); ``wav2vec2.masked_spec_embed`` is ignored.
    ``do_normalize``: zero mean and unit variance per row first (``asr.normalize_input``); fairseq's ``wav2vec_small`` was trained
    without it, so the default is False.  ``domain`` / ``judge`` are an int for every row or one value per row."""
    _prefix, _config_name = "dex_mos", "MOSConfig"
    _no_workspace = f"too short for one frame, or more than one call takes ({MAX_FRAMES} encoder frames)"
    _c_config = staticmethod(_c_config)
    _ignored = staticmethod(_ignored)
    _check_lengths = staticmethod(check_lengths)

    def __init__(self, config: Optional[MOSConfig] = None, device="cuda", do_normalize: bool = False):
        super().__init__(config or MOSConfig(), device)
        self.do_normalize = bool(do_normalize)

    def _ids(self, domain, judge, B: int, what: str):
        """``domain`` / ``judge`` (an int, or one value per row) -> host int32 [B] each; ``ValueError`` out of range."""
        out = []
        for name, v, hi in (("domain", domain, self.config.num_domains), ("judge", judge, self.config.num_judges)):
            a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.int64).reshape(-1)
            if a.size == 1:
                a = np.full(B, int(a[0]), dtype=np.int64)
            if a.shape != (B,):
                raise ValueError(f"{what}: {a.size} {name} ids for {B} rows")
            if (a < 0).any() or (a >= hi).any():
                raise ValueError(f"{what}: every {name} id must lie in [0, {hi}), got {a.tolist()}")
            out.append(np.ascontiguousarray(a.astype(np.int32)))
        return out

    def hidden_states(self, wav: torch.Tensor, lengths=None) -> torch.Tensor:
        """Raw 16 kHz samples [B, n] (or [n]), row b ``lengths[b]`` samples (what is stored past them reaches no result) ->
        ``Wav2Vec2Model``'s ``last_hidden_state`` [B, T, hidden] with T = ``num_frames(n)``.  Row b fills
        ``num_frames(lengths[b])`` frames and is 0 past them; it is bitwise the row alone."""
        return self._hidden(wav, lengths)

    def bilstm(self, features: torch.Tensor, lengths=None, domain=DOMAIN, judge=JUDGE) -> torch.Tensor:
        """The recurrence alone: features [B, T, hidden] (or [T, hidden]), row b ``lengths[b]`` frames, conditioned on the row's
        domain and listener embeddings -> the bidirectional LSTM's output [B, T, 2 lstm_hidden] (forward | reverse), 0 past a row's
        frames.  The reverse direction starts at the row's own last frame."""
        what = "UTMOS.bilstm"
        self._need_weights(what)
        on_device(features, what, ValueError)
        if features.dim() not in (2, 3) or features.shape[-1] != self.config.hidden_size or features.shape[-2] < 1:
            raise ValueError(f"{what}: expected [B, T, {self.config.hidden_size}] or [T, {self.config.hidden_size}], got {tuple(features.shape)}")
        one = features.dim() == 2
        f = (features[None] if one else features).to(device=self.device, dtype=torch.float32).contiguous()
        B, T = f.shape[0], f.shape[1]
        fl = host_lengths(lengths, B, T, what=what)
        dom, jud = self._ids(domain, judge, B, what)
        ctx = self._ctx
        need = int(ctx._fn("bilstm_workspace_bytes")(ctx.h, B, T))
        if need == 0:
            raise ValueError(f"{what}: {B} rows of {T} frames: more than one call takes ({MAX_FRAMES} frames)")
        ws = Handle.workspace(ctx, need)
        out = torch.empty(B, T, 2 * self.config.lstm_hidden, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = ctx._fn("bilstm")(ctx.h, f.data_ptr(), i32_ptr(fl), i32_ptr(dom), i32_ptr(jud), B, T, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                   stream(self.device))
        ctx.check(rc, "dex_mos_bilstm")
        return out[0] if one else out

    def _head(self, name: str, wav, lengths, domain, judge, what: str, per_frame: bool):
        x, ln, one, T = self._inputs(wav, lengths, what)
        B, n = x.shape
        dom, jud = self._ids(domain, judge, B, what)
        out = torch.empty((B, T) if per_frame else (B,), dtype=torch.float32, device=self.device)
        ctx = self._ctx
        ws = ctx.workspace(B, n)
        with torch.cuda.device(self.device):
            rc = ctx._fn(name)(ctx.h, x.data_ptr(), i32_ptr(ln), i32_ptr(dom), i32_ptr(jud), B, n, int(self.do_normalize), out.data_ptr(),
                               ws.data_ptr(), ws.numel(), stream(self.device))
        ctx.check(rc, f"dex_mos_{name}")
        return out[0] if one else out

    def frame_scores(self, wav: torch.Tensor, lengths=None, domain=DOMAIN, judge=JUDGE) -> torch.Tensor:
        """[B, n] (or [n]) -> the projection's score of every frame, [B, T] (or [T]); 0 past a row's frames."""
        return self._head("frames", wav, lengths, domain, judge, "UTMOS.frame_scores", True)

    def forward(self, wav: torch.Tensor, lengths=None, domain=DOMAIN, judge=JUDGE) -> torch.Tensor:
        """[B, n] (or [n]) raw 16 kHz samples -> the predicted MOS of every row alone, [B] (or a 0-d tensor):
        ``mean_t(frame score) * 2 + 3`` over the row's own frames.  Every row needs ``min_samples()`` samples."""
        return self._head("score", wav, lengths, domain, judge, "UTMOS.forward", False)

    __call__ = forward

    def score_utterances(self, wavs, lengths=None, sr: int = SAMPLING_RATE, domain=DOMAIN, judge=JUDGE) -> torch.Tensor:
        """``wavs`` [B, n] with ``lengths``, or a list of wavs (float, or int16 scaled by 1 / 32768), at ``sr`` Hz -> MOS [B] in one
        network call.  Where ``sr`` is not 16000 the wavs are resampled by ``wavprep.resample`` (kaiser_best)."""
        x, ln = self._utterances(wavs, lengths, sr, "UTMOS.score_utterances")
        return self.forward(x, ln, domain, judge)


def mos_score(wavs, lengths=None, source_sr: Optional[int] = 22050, model: Optional[UTMOS] = None, domain=DOMAIN, judge=JUDGE):
    """(mean, stderr) of the predicted MOS of ``wavs`` ([B, n] with ``lengths``, or a list) at ``source_sr`` Hz, the stderr as
    ``speaker.asv_score`` defines it (population std over sqrt(n))."""
    return mean_stderr(UTMOS._model(model, "mos_score").score_utterances(wavs, lengths, source_sr or SAMPLING_RATE, domain, judge))


def score_synthesis(model, audio, sr: int = 22050, domain=DOMAIN, judge=JUDGE):
    """``synthesize.synthesize_tokens``' list of int16 waveforms (``sr`` Hz) -> (MOS [B] on the device, mean, stderr)."""
    if len(audio) < 1:
        raise ValueError("score_synthesis: no waveforms")
    mos = UTMOS._model(model, "score_synthesis").score_utterances(list(audio), None, sr, domain, judge)
    return (mos,) + mean_stderr(mos)
