"""WavLM x-vector speaker similarity (SIM) on the device: the score zero-shot TTS work commonly reports.  A wav at 16 kHz goes through
HF's ``WavLMForXVector`` (microsoft/wavlm-base-plus-sv, wavlm-base-sv) in eval mode, and two utterances are compared by the cosine of
their ``embeddings``.

    WavLMConfig(...)                                      the fields of HF's config the network reads; defaults = wavlm-base-plus-sv
    WavLMXVector(config=None, device='cuda', do_normalize=False):  load_state_dict (HF keys), hidden_states -> [B, T, hidden],
                                                          forward -> embeddings [B, xvector_output_dim], embed_utterances(wavs, ...)
    num_frames(n_samples, config=None), min_samples(config=None), relative_position_buckets(n, config=None)
    state_dict_shapes(config=None), route_state_dict(sd, want), check_lengths(lengths, n)      the host half, usable without a device
    similarity(syn, trg, ..., model=) -> cos [B];  sim_score(...) -> (mean, stderr);  mean_stderr(cos)

The network runs in libdexamd.so (``csrc/wavlm.hip``, C ABI ``dex_wavlm_*``), fp32 throughout: a metric has no reduced-precision mode.
Nothing downloads: weights come from a dict or a local file the caller names, and the library ships no checkpoint.  Only this model
family is built (group-norm feature extractor, post-layer-norm encoder, head_dim 64, erf GELU, at most 8 convolution and 8 TDNN
layers); any other config raises ``NotImplementedError`` naming the field.  The WavLM-large + ECAPA-TDNN verification model
most SIM-o tables use is another network: ``dex_tts_amd/ecapa.py``.

What a caller comparing numbers must know:
  * batching: row b of any batch is the network applied to row b ALONE at its own length.  HF with a zero-padded batch and no
    attention mask gives something else (its group norm sees the padding); the row alone is what this library defines as the result.
  * where a wav is not at 16 kHz it is resampled by the library's ``wavprep.resample`` (resampy's kaiser_best); ``librosa.load(path,
    sr=16000)`` resamples with soxr.  The same note as the other two scores'.
  * ``do_normalize`` (``Wav2Vec2FeatureExtractor``'s zero-mean unit-variance step) is the caller's to set from the checkpoint's
    ``preprocessor_config.json``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._native import device_rows, pad_wavs, resample_to_16k
from ._wavnet import MAX_CONV, SAMPLING_RATE, HostEntry, WaveformNet, fill_trunk_config, route_hf_state_dict
from .speaker import mean_stderr, paired_cosine  # noqa: F401  (mean_stderr is this module's public name too)

MAX_TDNN = 8
MAX_FRAMES = 4096                  # DEX_WAVLM_MAX_FRAMES: the encoder frames one call takes (81 s)


@dataclasses.dataclass(frozen=True)
class WavLMConfig:
    """HF ``WavLMConfig`` fields the forward pass reads, with the values of microsoft/wavlm-base-plus-sv."""
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
    num_buckets: int = 320
    max_bucket_distance: int = 800
    use_weighted_layer_sum: bool = True
    tdnn_dim: Tuple[int, ...] = (512, 512, 512, 512, 1500)
    tdnn_kernel: Tuple[int, ...] = (5, 3, 3, 1, 1)
    tdnn_dilation: Tuple[int, ...] = (1, 2, 3, 1, 1)
    xvector_output_dim: int = 512
    hidden_act: str = "gelu"
    feat_extract_activation: str = "gelu"


class DexWavlmConfig(C.Structure):
    _fields_ = [("n_conv", C.c_int32), ("conv_dim", C.c_int32 * MAX_CONV), ("conv_kernel", C.c_int32 * MAX_CONV),
                ("conv_stride", C.c_int32 * MAX_CONV), ("conv_bias", C.c_int32), ("feat_extract_norm_group", C.c_int32),
                ("hidden", C.c_int32), ("n_layers", C.c_int32), ("n_heads", C.c_int32), ("intermediate", C.c_int32),
                ("do_stable_layer_norm", C.c_int32), ("num_conv_pos_embeddings", C.c_int32), ("num_conv_pos_embedding_groups", C.c_int32),
                ("layer_norm_eps", C.c_float), ("num_buckets", C.c_int32), ("max_bucket_distance", C.c_int32),
                ("use_weighted_layer_sum", C.c_int32), ("n_tdnn", C.c_int32), ("tdnn_dim", C.c_int32 * MAX_TDNN),
                ("tdnn_kernel", C.c_int32 * MAX_TDNN), ("tdnn_dilation", C.c_int32 * MAX_TDNN), ("xvector_output_dim", C.c_int32)]


def _c_config(cfg: WavLMConfig) -> DexWavlmConfig:
    """The C struct of a config; ``NotImplementedError`` for what the struct cannot even express."""
    c = fill_trunk_config(DexWavlmConfig(), cfg)
    m = len(cfg.tdnn_dim)
    if not (1 <= m <= MAX_TDNN) or len(cfg.tdnn_kernel) != m or len(cfg.tdnn_dilation) != m:
        raise NotImplementedError(f"tdnn_dim / tdnn_kernel / tdnn_dilation: 1 .. {MAX_TDNN} layers of equal count, got "
                                  f"{m} / {len(cfg.tdnn_kernel)} / {len(cfg.tdnn_dilation)}")
    c.feat_extract_norm_group = int(cfg.feat_extract_norm == "group")
    c.num_buckets, c.max_bucket_distance = int(cfg.num_buckets), int(cfg.max_bucket_distance)
    c.use_weighted_layer_sum = int(bool(cfg.use_weighted_layer_sum))
    c.n_tdnn = m
    for i in range(m):
        c.tdnn_dim[i], c.tdnn_kernel[i], c.tdnn_dilation[i] = int(cfg.tdnn_dim[i]), int(cfg.tdnn_kernel[i]), int(cfg.tdnn_dilation[i])
    c.xvector_output_dim = int(cfg.xvector_output_dim)
    return c


_HOST = HostEntry("dex_wavlm", _c_config, WavLMConfig, "WavLMConfig")


def num_frames(n_samples: int, config: Optional[WavLMConfig] = None) -> int:
    """Encoder frames of ``n_samples`` samples: ``floor((L - k) / s) + 1`` chained over the feature extractor.  Host integers."""
    return _HOST.num_frames(n_samples, config)


def min_samples(config: Optional[WavLMConfig] = None) -> int:
    """The fewest samples a row may have: two frames must be left after the TDNN layers, since statistics pooling takes the unbiased
    deviation over them (one frame: NaN in torch).  5200 samples = 16 encoder frames with the default geometry.  Host integers."""
    return _HOST.min_samples(config)


def relative_position_buckets(n: int, config: Optional[WavLMConfig] = None) -> np.ndarray:
    """``WavLMAttention._relative_positions_bucket`` of the distances ``key - query`` = -(n - 1) .. n - 1 -> int32 [2 n - 1] (entry
    ``d + n - 1``): signed, exact below ``num_buckets / 4``, logarithmic up to ``max_bucket_distance``, clamped past it.  The table
    the device gathers ``rel_attn_embed`` through; computed on the host in float64."""
    c = _c_config(config or WavLMConfig())
    if int(n) < 1:
        raise ValueError(f"relative_position_buckets: n must be >= 1, got {n}")
    out = np.zeros(2 * int(n) - 1, dtype=np.int32)
    rc = _lib.load().dex_wavlm_rel_buckets(C.byref(c), int(n), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != _lib.DEX_OK:
        raise ValueError(f"relative_position_buckets: bad arguments (n = {n}, num_buckets = {c.num_buckets}, "
                         f"max_bucket_distance = {c.max_bucket_distance})")
    return out


def _ignored(key: str) -> bool:
    """Training-side keys of the checkpoint: the classifier and the AM-softmax objective make logits and the loss."""
    return key.startswith("classifier.") or key in ("objective.weight", "wavlm.masked_spec_embed")


def state_dict_shapes(config: Optional[WavLMConfig] = None) -> dict:
    """The HF state-dict keys the network of ``config`` needs, with their shapes (weight norm in its ``weight_g`` / ``weight_v``
    spelling); ``NotImplementedError`` naming the field for a config outside the family that is built.  Host only."""
    return _HOST.state_dict_shapes(config)


def route_state_dict(sd, want: dict, strict: bool = True):
    """An HF state dict against the inventory ``want`` (``state_dict_shapes``) -> ({key: tensor} of what arrived, missing keys).  The
    positional convolution is taken in either weight-norm spelling; training-side keys are dropped.  A wrong shape or (``strict``)
    a missing or unexpected key raises ``RuntimeError``.  Host only."""
    return route_hf_state_dict(sd, want, strict, _ignored)


def check_lengths(lengths, n_samples: int, config: Optional[WavLMConfig] = None, what: str = "wavlm") -> int:
    """What one call refuses, before anything is enqueued: a row below ``min_samples`` (``ValueError`` 'too short') and a padded
    length of more than ``MAX_FRAMES`` encoder frames.  Returns the frames of ``n_samples``.  Host only."""
    return _HOST.check_lengths(lengths, n_samples, config, what, "statistics pooling needs two TDNN frames ({need} samples)", MAX_FRAMES)


class WavLMXVector(WaveformNet):
    """HF's ``WavLMForXVector`` in eval mode on one MI355X, fp32, ``attention_mask=None``; a batch row is the row alone.
    ``load_state_dict`` takes the HF checkpoint's state dict; ``classifier.*``, ``objective.weight`` and ``wavlm.masked_spec_embed``
    are ignored.  ``do_normalize``: apply ``Wav2Vec2FeatureExtractor``'s normalisation (``asr.normalize_input``) to every row first.
    It must match the checkpoint's ``preprocessor_config.json``; the library reads no such file and nothing here can check what the
    published value is, so the default is False and the caller sets it."""
    _prefix, _config_name = "dex_wavlm", "WavLMConfig"
    _no_workspace = f"too short for two TDNN frames, or more than one call takes ({MAX_FRAMES} encoder frames)"
    _c_config = staticmethod(_c_config)
    _ignored = staticmethod(_ignored)
    _check_lengths = staticmethod(check_lengths)

    def __init__(self, config: Optional[WavLMConfig] = None, device="cuda", do_normalize: bool = False):
        super().__init__(config or WavLMConfig(), device)
        self.do_normalize = bool(do_normalize)

    def hidden_states(self, wav: torch.Tensor, lengths=None) -> torch.Tensor:
        """Raw 16 kHz samples [B, n] (or [n]), row b ``lengths[b]`` samples (what is stored past them reaches no result) -> the hidden
        states the x-vector head reads, [B, T, hidden] with T = ``num_frames(n)``: the softmax(``layer_weights``)-weighted sum of
        the encoder's L + 1 hidden states (``use_weighted_layer_sum``) or the last one.  Row b fills ``num_frames(lengths[b])``
        frames and is 0 past them; it is bitwise the row alone."""
        return self._hidden(wav, lengths)

    def forward(self, input_values: torch.Tensor, lengths=None) -> torch.Tensor:
        """``WavLMForXVector.forward(input_values).embeddings`` of every row alone: [B, n] (or [n]) -> [B, xvector_output_dim] (or
        [xvector_output_dim]).  Every row needs ``min_samples()`` samples."""
        x, ln, one, _ = self._inputs(input_values, lengths, "WavLMXVector.forward")
        out = torch.empty(x.shape[0], self.config.xvector_output_dim, dtype=torch.float32, device=self.device)
        return self._run("embed", x, ln, out, int(self.do_normalize), out.data_ptr(), one=one)

    __call__ = forward

    def embed_utterances(self, wavs, lengths=None, sr: int = SAMPLING_RATE) -> torch.Tensor:
        """``wavs`` [B, n] with ``lengths``, or a list of wavs (float, or int16 scaled by 1 / 32768), at ``sr`` Hz -> embeddings
        [B, xvector_output_dim] in one network call.  Where ``sr`` is not 16000 the wavs are resampled by ``wavprep.resample``
        (kaiser_best; librosa uses soxr)."""
        return self.forward(*self._utterances(wavs, lengths, sr, "WavLMXVector.embed_utterances"))


def _pair(what, model, syn, syn_lengths, syn_sr, trg, trg_lengths, trg_sr) -> torch.Tensor:
    """Both sides at 16 kHz, stacked as 2 B rows, embedded in ONE call -> cos [B] (``dex_spk_cosine``)."""
    model = WavLMXVector._model(model, what)

    def at_16k(x, ln, sr):
        x, ln, _ = device_rows(x, ln, what, refuse=ValueError)
        return resample_to_16k(x.to(model.device), ln, sr)
    return paired_cosine(what, at_16k, model.forward, (syn, syn_lengths, syn_sr), (trg, trg_lengths, trg_sr))


def similarity(syn: torch.Tensor, trg: torch.Tensor, syn_lengths=None, trg_lengths=None, source_sr: Optional[int] = 22050,
               model: Optional[WavLMXVector] = None) -> torch.Tensor:
    """SIM for a batch: syn, trg [B, n] (or [n]) at ``source_sr`` Hz, rows of ``*_lengths`` samples -> the cosine of each pair's
    x-vector embeddings, [B] on the device."""
    return _pair("similarity", model, syn, syn_lengths, source_sr, trg, trg_lengths, source_sr)


def sim_score(syn, trg, syn_lengths=None, trg_lengths=None, source_sr: Optional[int] = 22050, model: Optional[WavLMXVector] = None):
    """(mean, stderr) of ``similarity``'s cosines, the stderr as ``speaker.asv_score`` defines it."""
    return mean_stderr(similarity(syn, trg, syn_lengths, trg_lengths, source_sr, model))


def score_synthesis(model, audio, ref_wavs, sr: int = 22050, ref_sr: Optional[int] = None):
    """``synthesize.synthesize_tokens``' list of int16 waveforms (``sr`` Hz) against the reference wavs in the same order (``ref_sr``
    Hz, default ``sr``) -> (cos [B] on the device, mean, stderr)."""
    if len(audio) != len(ref_wavs) or len(audio) < 1:
        raise ValueError(f"score_synthesis: {len(audio)} waveforms against {len(ref_wavs)} reference wavs")
    model = WavLMXVector._model(model, "score_synthesis")
    syn, sl = pad_wavs(audio, model.device, scale_int16=True)
    trg, tl = pad_wavs(ref_wavs, model.device, scale_int16=True)
    cos = _pair("score_synthesis", model, syn, sl, sr, trg, tl, ref_sr or sr)
    return (cos,) + mean_stderr(cos)
