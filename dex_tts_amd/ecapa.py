"""WavLM-large + ECAPA-TDNN speaker similarity on the device: the SIM (SIM-o) column of seed-tts-eval, VALL-E, F5-TTS, E2-TTS and most
zero-shot TTS tables.  A wav at 16 kHz goes through the WavLM-large trunk (HF's ``WavLMModel``, all 25 hidden states), the
ECAPA-TDNN head of the UniSpeech speaker-verification recipe (``wavlm_large_finetune.pth``) in eval mode, and two utterances are
compared by the cosine of their embeddings.

    EcapaConfig(...)                                      HF ``WavLMConfig`` names for the trunk, and the head's widths
    WavLMEcapa(config=None, device='cuda', do_normalize=True):  load_state_dict, hidden_states -> [B, T, hidden] (the instance-normed
                                                          layer mix), forward -> embeddings [B, emb_dim], embed_utterances(wavs, ...),
                                                          res2 (one block's Res2 chain alone)
    num_frames(n_samples, config=None), min_samples(config=None), state_dict_shapes(config=None), route_state_dict(sd, want),
    check_lengths(lengths, n)                             the host half, usable without a device
    from_unispeech_checkpoint(sd)                         the fine-tuned checkpoint's keys -> ``load_state_dict``'s
    similarity(syn, trg, ..., model=) -> cos [B];  sim_score(...) -> (mean, stderr);  score_synthesis(...)

The network runs in libdexamd.so (``csrc/ecapa.hip``, C ABI ``dex_ecapa_*``), fp32 throughout.  Nothing downloads: weights come from a
dict or a local file the caller names, and the library ships no checkpoint.  Only this family is built (layer-norm feature extractor,
stable-layer-norm encoder, head_dim 64, erf GELU, ``ECAPA_TDNN`` with ``scale=8`` and ``channels`` 256 or 512, dilations up to 4);
any other config raises ``NotImplementedError`` naming the field.

The network, as this library defines it (eval mode; the spec it was written from):
  * input: ``do_normalize`` is s3prl's ``F.layer_norm(wav, wav.shape)``: zero mean, biased variance, **eps 1e-5** (``asr.normalize_input``
    is ``Wav2Vec2FeatureExtractor``'s, eps 1e-7).  The default True is WavLM-large's fairseq config (``normalize=True``) as remembered
    from the public config; nothing here can check it.
  * trunk: ``WavLMModel`` with ``feat_extract_norm="layer"``, ``conv_bias=True``, ``do_stable_layer_norm=True``.  The hidden states are
    the inputs of layers 0 .. L - 1 and ``encoder.layer_norm`` of the last layer's output: L + 1 tensors.
  * head: ``x = sum_l softmax(feature_weight)[l] hidden[l]``; ``InstanceNorm1d(x + 1e-6)``; ``layer1 = BN(ReLU(Conv1d(k=5, pad=2)))``;
    three ``SE_Res2Block`` (1x1 conv, the Res2 chain of 7 dilated k = 3 convolutions over 8 channel slices, 1x1 conv, squeeze-excitation,
    residual); ``ReLU(Conv1d 1x1)`` of their concatenation; attentive statistics pooling (optionally with the global context);
    ``Linear(BN(pool))``.  Every ``Conv1dReluBn`` is ``bn(relu(conv(x)))``: the BatchNorm follows the ReLU.

What a caller comparing numbers must know:
  * NOT checked against the real checkpoint.  The head and the checkpoint's key names were written down from a reading of the public
    UniSpeech / s3prl code; there is no copy of either here.  What the device is held to is its own float64 restatement
    (tests/ecapa_ref.py), itself held to ``transformers.WavLMModel`` and a ``torch.nn`` transcription of the head in double precision.
  * batching: row b of any batch is the network applied to row b ALONE at its own length - the instance norm, the squeeze-excitation
    means, the pooling's softmax, the attention keys and every convolution's zero padding end at the row's own frames.  The upstream
    pads a batch and masks.
  * where a wav is not at 16 kHz it is resampled by the library's ``wavprep.resample`` (resampy's kaiser_best); the upstream uses
    torchaudio's resampler.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional, Tuple

import torch

from ._native import device_rows, host_lengths, i32_ptr, on_device, pad_wavs, resample_to_16k, stream
from ._wavnet import MAX_CONV, SAMPLING_RATE, HostEntry, WaveformNet, fill_trunk_config, route_hf_state_dict
from .speaker import mean_stderr, paired_cosine  # noqa: F401  (mean_stderr is this module's public name too)

MAX_FRAMES = 4096                  # DEX_ECAPA_MAX_FRAMES: the encoder frames one call takes (81 s)
BLOCKS = 3                         # DEX_ECAPA_BLOCKS
RES2_TILE = 72                     # DEX_ECAPA_RES2_TILE: frames one workgroup of the Res2 chain stores (csrc/ecapa.hip R2_TILE)


@dataclasses.dataclass(frozen=True)
class EcapaConfig:
    """HF ``WavLMConfig`` fields of the trunk (the values of microsoft/wavlm-large) and the arguments of ``ECAPA_TDNN``."""
    conv_dim: Tuple[int, ...] = (512,) * 7
    conv_kernel: Tuple[int, ...] = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: Tuple[int, ...] = (5, 2, 2, 2, 2, 2, 2)
    conv_bias: bool = True
    feat_extract_norm: str = "layer"
    hidden_size: int = 1024
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    intermediate_size: int = 4096
    do_stable_layer_norm: bool = True
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    layer_norm_eps: float = 1e-5
    num_buckets: int = 320
    max_bucket_distance: int = 800
    hidden_act: str = "gelu"
    feat_extract_activation: str = "gelu"
    channels: int = 512
    emb_dim: int = 256
    res2_scale: int = 8
    se_bottleneck_dim: int = 128
    attention_channels: int = 128
    global_context_att: bool = False
    dilations: Tuple[int, ...] = (2, 3, 4)


class DexEcapaConfig(C.Structure):
    _fields_ = [("n_conv", C.c_int32), ("conv_dim", C.c_int32 * MAX_CONV), ("conv_kernel", C.c_int32 * MAX_CONV),
                ("conv_stride", C.c_int32 * MAX_CONV), ("conv_bias", C.c_int32), ("feat_extract_norm_layer", C.c_int32),
                ("hidden", C.c_int32), ("n_layers", C.c_int32), ("n_heads", C.c_int32), ("intermediate", C.c_int32),
                ("do_stable_layer_norm", C.c_int32), ("num_conv_pos_embeddings", C.c_int32), ("num_conv_pos_embedding_groups", C.c_int32),
                ("layer_norm_eps", C.c_float), ("num_buckets", C.c_int32), ("max_bucket_distance", C.c_int32),
                ("channels", C.c_int32), ("emb_dim", C.c_int32), ("res2_scale", C.c_int32), ("se_bottleneck_dim", C.c_int32),
                ("attention_channels", C.c_int32), ("global_context_att", C.c_int32), ("dilations", C.c_int32 * BLOCKS)]


def _c_config(cfg: EcapaConfig) -> DexEcapaConfig:
    """The C struct of a config; ``NotImplementedError`` for what the struct cannot even express."""
    c = fill_trunk_config(DexEcapaConfig(), cfg)
    c.feat_extract_norm_layer = int(cfg.feat_extract_norm == "layer")
    c.num_buckets, c.max_bucket_distance = int(cfg.num_buckets), int(cfg.max_bucket_distance)
    if len(cfg.dilations) != BLOCKS:
        raise NotImplementedError(f"dilations: {BLOCKS} SE-Res2 blocks are built, got {len(cfg.dilations)}")
    if int(cfg.res2_scale) < 1 or int(cfg.channels) % int(cfg.res2_scale) or int(cfg.channels) // int(cfg.res2_scale) not in (32, 64):
        raise NotImplementedError(f"channels / scale = {cfg.channels} / {cfg.res2_scale}: only slices of 32 or 64 channels are built")
    for name in ("channels", "emb_dim", "res2_scale", "se_bottleneck_dim", "attention_channels"):
        setattr(c, name, int(getattr(cfg, name)))
    c.global_context_att = int(bool(cfg.global_context_att))
    for i in range(BLOCKS):
        c.dilations[i] = int(cfg.dilations[i])
    return c


_HOST = HostEntry("dex_ecapa", _c_config, EcapaConfig, "EcapaConfig")


def num_frames(n_samples: int, config: Optional[EcapaConfig] = None) -> int:
    """Encoder frames of ``n_samples`` samples: ``floor((L - k) / s) + 1`` chained over the feature extractor.  Host integers."""
    return _HOST.num_frames(n_samples, config)


def min_samples(config: Optional[EcapaConfig] = None) -> int:
    """The fewest samples a row may have: two encoder frames (720 with the default geometry), since torch refuses an instance norm
    over one.  Host integers."""
    return _HOST.min_samples(config)


def _ignored(key: str) -> bool:
    """``WavLMModel``'s training-side key, and the counters of the eval-mode batch norms."""
    return key == "wavlm.masked_spec_embed" or key.endswith(".num_batches_tracked")


def state_dict_shapes(config: Optional[EcapaConfig] = None) -> dict:
    """The keys the network of ``config`` needs, with their shapes: HF ``WavLMModel`` keys under ``wavlm.`` (weight norm in its
    ``weight_g`` / ``weight_v`` spelling), then the head's UniSpeech names (``feature_weight``, ``layer1.conv.*`` / ``layer1.bn.*``,
    ``layerN.Conv1dReluBn1.*``, ``layerN.Res2Conv1dReluBn.{convs,bns}.i.*``, ``layerN.Conv1dReluBn2.*``, ``layerN.SE_Connect.linear{1,2}.*``,
    ``conv.*``, ``pooling.linear{1,2}.*``, ``bn.*``, ``linear.*``); ``NotImplementedError`` naming the field for a config outside the
    family that is built.  Host only."""
    return _HOST.state_dict_shapes(config)


def route_state_dict(sd, want: dict, strict: bool = True):
    """A state dict against the inventory ``want`` (``state_dict_shapes``) -> ({key: tensor} of what arrived, missing keys).  The
    positional convolution is taken in either weight-norm spelling; ``wavlm.masked_spec_embed`` and ``*.num_batches_tracked`` are
    dropped.  A wrong shape or (``strict``) a missing or unexpected key raises ``RuntimeError``.  Host only."""
    return route_hf_state_dict(sd, want, strict, _ignored)


def check_lengths(lengths, n_samples: int, config: Optional[EcapaConfig] = None, what: str = "ecapa") -> int:
    """What one call refuses, before anything is enqueued: a row below ``min_samples`` (``ValueError`` 'too short') and a padded
    length of more than ``MAX_FRAMES`` encoder frames.  Returns the frames of ``n_samples``.  Host only."""
    return _HOST.check_lengths(lengths, n_samples, config, what, "the instance norm needs two frames ({need} samples)", MAX_FRAMES)


_FAIRSEQ = (("self_attn_layer_norm.", "layer_norm."), ("self_attn.grep_linear.", "attention.gru_rel_pos_linear."),
            ("self_attn.grep_a", "attention.gru_rel_pos_const"), ("self_attn.relative_attention_bias.", "attention.rel_attn_embed."),
            ("self_attn.", "attention."), ("fc1.", "feed_forward.intermediate_dense."), ("fc2.", "feed_forward.output_dense."))
_TRUNK = "feature_extract.model."
_DROPPED = ("mask_emb", "label_embs_concat", "final_proj.", "quantizer.", "project_q.")


def _fairseq_to_hf(k: str) -> str:
    """One fairseq WavLM key (without its model prefix) -> the HF ``WavLMModel`` key (without ``wavlm.``)."""
    p = k.split(".")
    if k.startswith("feature_extractor.conv_layers.") and len(p) >= 5:
        if p[3] == "0":
            return ".".join(p[:3] + ["conv"] + p[4:])
        if p[3] == "2" and len(p) == 6 and p[4] == "1":                                    # Sequential(TransposeLast, LayerNorm, TransposeLast)
            return ".".join(p[:3] + ["layer_norm", p[5]])
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


def from_unispeech_checkpoint(sd) -> dict:
    """The UniSpeech speaker-verification checkpoint (``wavlm_large_finetune.pth``: the dict itself or nested under ``['model']``) ->
    the keys ``WavLMEcapa.load_state_dict`` takes.  A pure rename, host only: the trunk under ``feature_extract.model.`` loses that
    prefix and fairseq's WavLM names become HF's under ``wavlm.`` (``conv_layers.{i}.0`` -> ``{i}.conv``, ``conv_layers.{i}.2.1`` ->
    ``{i}.layer_norm``, the top-level ``layer_norm`` -> ``feature_projection.layer_norm``, ``post_extract_proj`` -> ``feature_projection.
    projection``, ``encoder.pos_conv.0`` -> ``encoder.pos_conv_embed.conv``, ``self_attn.{q,k,v,out}_proj`` -> ``attention.*``,
    ``self_attn.grep_linear`` / ``grep_a`` / ``relative_attention_bias`` -> ``attention.gru_rel_pos_linear`` / ``gru_rel_pos_const`` /
    ``rel_attn_embed``, ``self_attn_layer_norm`` -> ``layer_norm``, ``fc1`` / ``fc2`` -> ``feed_forward.intermediate_dense`` /
    ``output_dense``; ``final_layer_norm`` and ``encoder.layer_norm`` keep their names); ``mask_emb``, label embeddings and the
    pre-training heads are dropped; the head's keys are the library's already.  Any other key is kept as it is, for ``strict`` to
    report.  The names come from a reading of the public code: this function has NOT been run on the real checkpoint."""
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    out = {}
    for k, v in sd.items():
        if k.startswith(_TRUNK):
            k = k[len(_TRUNK):]
            if k.startswith(_DROPPED):
                continue
            out["wavlm." + _fairseq_to_hf(k)] = v
        else:
            out[k] = v
    return out


class WavLMEcapa(WaveformNet):
    """WavLM-large + ECAPA-TDNN in eval mode on one MI355X, fp32; a batch row is the row alone.  ``load_state_dict`` takes the keys of
    ``state_dict_shapes`` (``from_unispeech_checkpoint`` renames the fine-tuned checkpoint's); ``wavlm.masked_spec_embed`` and the
    batch norms' ``num_batches_tracked`` are ignored.  ``do_normalize``: the upstream's ``F.layer_norm(wav, wav.shape)`` on every row
    first (eps 1e-5).  The default True is what WavLM-large's fairseq config says (``normalize=True``) as remembered from the public
    config; the library reads no such file and nothing here can check it."""
    _prefix, _config_name = "dex_ecapa", "EcapaConfig"
    _no_workspace = f"too short for two frames, or more than one call takes ({MAX_FRAMES} encoder frames)"
    _c_config = staticmethod(_c_config)
    _ignored = staticmethod(_ignored)
    _check_lengths = staticmethod(check_lengths)

    def __init__(self, config: Optional[EcapaConfig] = None, device="cuda", do_normalize: bool = True):
        super().__init__(config or EcapaConfig(), device)
        self.do_normalize = bool(do_normalize)

    def hidden_states(self, wav: torch.Tensor, lengths=None) -> torch.Tensor:
        """Raw 16 kHz samples [B, n] (or [n]), row b ``lengths[b]`` samples (what is stored past them reaches no result) -> what the
        head's first convolution reads, [B, T, hidden] with T = ``num_frames(n)``: the softmax(``feature_weight``)-weighted sum of
        the trunk's L + 1 hidden states after ``InstanceNorm1d(x + 1e-6)`` over the row's own frames.  Row b fills
        ``num_frames(lengths[b])`` frames and is 0 past them; it is bitwise the row alone."""
        return self._hidden(wav, lengths)

    def forward(self, input_values: torch.Tensor, lengths=None) -> torch.Tensor:
        """[B, n] (or [n]) raw 16 kHz samples -> the speaker embedding of every row alone, [B, emb_dim] (or [emb_dim]).  Every row
        needs ``min_samples()`` samples."""
        x, ln, one, _ = self._inputs(input_values, lengths, "WavLMEcapa.forward")
        out = torch.empty(x.shape[0], self.config.emb_dim, dtype=torch.float32, device=self.device)
        return self._run("embed", x, ln, out, int(self.do_normalize), out.data_ptr(), one=one)

    __call__ = forward

    def embed_utterances(self, wavs, lengths=None, sr: int = SAMPLING_RATE) -> torch.Tensor:
        """``wavs`` [B, n] with ``lengths``, or a list of wavs (float, or int16 scaled by 1 / 32768), at ``sr`` Hz -> embeddings
        [B, emb_dim] in one network call.  Where ``sr`` is not 16000 the wavs are resampled by ``wavprep.resample`` (kaiser_best)."""
        return self.forward(*self._utterances(wavs, lengths, sr, "WavLMEcapa.embed_utterances"))

    def res2(self, block: int, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """The Res2 chain of SE-Res2 block ``block`` (0 .. 2) alone, one launch: x [B, T, channels] (or [T, channels]), row b
        ``lengths[b]`` frames -> [B, T, channels]: ``sp = bn_i(relu(conv_i(sp + slice_i)))`` over the first seven slices of
        ``channels / 8``, each convolution zero-padded at the row's own ends, the eighth slice copied; 0 past a row's frames."""
        what = "WavLMEcapa.res2"
        self._need_weights(what)
        on_device(x, what, ValueError)
        C_ = self.config.channels
        if x.dim() not in (2, 3) or x.shape[-1] != C_ or x.shape[-2] < 1:
            raise ValueError(f"{what}: expected [B, T, {C_}] or [T, {C_}], got {tuple(x.shape)}")
        if not 0 <= int(block) < BLOCKS:
            raise ValueError(f"{what}: block must lie in [0, {BLOCKS}), got {block}")
        one = x.dim() == 2
        f = (x[None] if one else x).to(device=self.device, dtype=torch.float32).contiguous()
        B, T = f.shape[0], f.shape[1]
        if T > MAX_FRAMES:
            raise ValueError(f"{what}: {T} frames; one call takes at most {MAX_FRAMES}")
        fl = host_lengths(lengths, B, T, what=what)
        out = torch.empty_like(f)
        ctx = self._ctx
        with torch.cuda.device(self.device):
            rc = ctx._fn("res2")(ctx.h, int(block), f.data_ptr(), i32_ptr(fl), B, T, out.data_ptr(), stream(self.device))
        ctx.check(rc, "dex_ecapa_res2")
        return out[0] if one else out


def _pair(what, model, syn, syn_lengths, syn_sr, trg, trg_lengths, trg_sr) -> torch.Tensor:
    """Both sides at 16 kHz, stacked as 2 B rows, embedded in ONE call -> cos [B] (``dex_spk_cosine``)."""
    model = WavLMEcapa._model(model, what)

    def at_16k(x, ln, sr):
        x, ln, _ = device_rows(x, ln, what, refuse=ValueError)
        return resample_to_16k(x.to(model.device), ln, sr)
    return paired_cosine(what, at_16k, model.forward, (syn, syn_lengths, syn_sr), (trg, trg_lengths, trg_sr))


def similarity(syn: torch.Tensor, trg: torch.Tensor, syn_lengths=None, trg_lengths=None, source_sr: Optional[int] = 22050,
               model: Optional[WavLMEcapa] = None) -> torch.Tensor:
    """SIM for a batch: syn, trg [B, n] (or [n]) at ``source_sr`` Hz, rows of ``*_lengths`` samples -> the cosine of each pair's
    embeddings, [B] on the device."""
    return _pair("similarity", model, syn, syn_lengths, source_sr, trg, trg_lengths, source_sr)


def sim_score(syn, trg, syn_lengths=None, trg_lengths=None, source_sr: Optional[int] = 22050, model: Optional[WavLMEcapa] = None):
    """(mean, stderr) of ``similarity``'s cosines, the stderr as ``speaker.asv_score`` defines it."""
    return mean_stderr(similarity(syn, trg, syn_lengths, trg_lengths, source_sr, model))


def score_synthesis(model, audio, ref_wavs, sr: int = 22050, ref_sr: Optional[int] = None):
    """``synthesize.synthesize_tokens``' list of int16 waveforms (``sr`` Hz) against the reference wavs in the same order (``ref_sr``
    Hz, default ``sr``) -> (cos [B] on the device, mean, stderr)."""
    if len(audio) != len(ref_wavs) or len(audio) < 1:
        raise ValueError(f"score_synthesis: {len(audio)} waveforms against {len(ref_wavs)} reference wavs")
    model = WavLMEcapa._model(model, "score_synthesis")
    syn, sl = pad_wavs(audio, model.device, scale_int16=True)
    trg, tl = pad_wavs(ref_wavs, model.device, scale_int16=True)
    cos = _pair("score_synthesis", model, syn, sl, sr, trg, tl, ref_sr or sr)
    return (cos,) + mean_stderr(cos)
