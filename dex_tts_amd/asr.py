"""The ASR score on the device: the intelligibility half of the reference's ``Evaluater`` (src/metric.py:21-67, ``transcribe`` /
``calculate_wer_cer`` / ``calculate_asr_score``).  A synthesised wav at 16 kHz goes through HF's ``Wav2Vec2ForCTC``
(facebook/wav2vec2-large-960h-lv60-self), the argmax per frame is decoded as CTC, and the transcript is scored against the input
text as character and word error rates.

    Wav2Vec2Config(...)                                   the fields of HF's config the network reads; defaults = large-lv60-self
    Wav2Vec2CTC(config=None, device='cuda', vocab=None):  load_state_dict (HF keys), forward -> logits [B, T, V], transcribe -> [str]
    normalize_input(wav, lengths=None)                    Wav2Vec2FeatureExtractor's do_normalize
    num_frames(n_samples, config=None)                    floor((L - k) / s) + 1 chained over the feature extractor
    ctc_greedy(logits, frames) -> [[int]];  decode(ids, vocab=None) -> str
    normalize_sentence, wer, cer                          metric.py:97-110 normalize_sentence and jiwer's two rates (host strings)
    asr_score(texts, wavs, sr=16000, model=) -> (cer_mean, cer_stderr, wer_mean, wer_stderr)

The network and the CTC kernel run in libdexamd.so (``csrc/asr.hip``, C ABI ``dex_asr_*``), fp32 throughout: a metric has no
reduced-precision mode.  Only ids and counts travel to the host; edit distance and string work stay there (tens of characters).
Nothing downloads: weights come from a dict or a local file the caller names.  Only this model family is built (layer-norm feature
extractor, stable layer norm, head_dim 64, erf GELU); any other config raises ``NotImplementedError`` naming the field.

One departure from the reference's number: where a wav is not at 16 kHz it is resampled by the library's ``wavprep.resample``
(resampy's kaiser_best); ``librosa.load(path, sr=16000)`` resamples with soxr.  The same note as the speaker score's.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import unicodedata
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._native import (Handle, device_index, device_rows, host_lengths, i32_ptr, on_device, pad_wavs, per_device, resample_to_16k, stream,
                      upload_weights)

SAMPLING_RATE = 16000
VOCAB = ("<pad>", "<s>", "</s>", "<unk>", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M", "W", "C", "F", "G", "Y", "P",
         "B", "V", "K", "'", "X", "J", "Q", "Z")
MAX_CONV = 8


@dataclasses.dataclass(frozen=True)
class Wav2Vec2Config:
    """HF ``Wav2Vec2Config`` fields the forward pass reads, with the values of facebook/wav2vec2-large-960h-lv60-self."""
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
    vocab_size: int = 32
    hidden_act: str = "gelu"
    feat_extract_activation: str = "gelu"


class DexAsrConfig(C.Structure):
    _fields_ = [("n_conv", C.c_int32), ("conv_dim", C.c_int32 * MAX_CONV), ("conv_kernel", C.c_int32 * MAX_CONV),
                ("conv_stride", C.c_int32 * MAX_CONV), ("conv_bias", C.c_int32), ("feat_extract_norm_layer", C.c_int32),
                ("hidden", C.c_int32), ("n_layers", C.c_int32), ("n_heads", C.c_int32), ("intermediate", C.c_int32),
                ("do_stable_layer_norm", C.c_int32), ("num_conv_pos_embeddings", C.c_int32), ("num_conv_pos_embedding_groups", C.c_int32),
                ("layer_norm_eps", C.c_float), ("vocab", C.c_int32)]


def _c_config(cfg: Wav2Vec2Config) -> DexAsrConfig:
    """The C struct of a config; ``NotImplementedError`` for what the struct cannot even express."""
    for name in ("hidden_act", "feat_extract_activation"):
        if getattr(cfg, name) != "gelu":
            raise NotImplementedError(f"{name}={getattr(cfg, name)!r}: only 'gelu' (erf) is built")
    n = len(cfg.conv_dim)
    if not (1 <= n <= MAX_CONV) or len(cfg.conv_kernel) != n or len(cfg.conv_stride) != n:
        raise NotImplementedError(f"conv_dim / conv_kernel / conv_stride: 1 .. {MAX_CONV} layers of equal count, got "
                                  f"{n} / {len(cfg.conv_kernel)} / {len(cfg.conv_stride)}")
    c = DexAsrConfig()
    c.n_conv = n
    for i in range(n):
        c.conv_dim[i], c.conv_kernel[i], c.conv_stride[i] = int(cfg.conv_dim[i]), int(cfg.conv_kernel[i]), int(cfg.conv_stride[i])
    c.conv_bias = int(bool(cfg.conv_bias))
    c.feat_extract_norm_layer = int(cfg.feat_extract_norm == "layer")
    c.hidden, c.n_layers, c.n_heads, c.intermediate = int(cfg.hidden_size), int(cfg.num_hidden_layers), int(cfg.num_attention_heads), int(cfg.intermediate_size)
    c.do_stable_layer_norm = int(bool(cfg.do_stable_layer_norm))
    c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups = int(cfg.num_conv_pos_embeddings), int(cfg.num_conv_pos_embedding_groups)
    c.layer_norm_eps, c.vocab = float(cfg.layer_norm_eps), int(cfg.vocab_size)
    return c


def num_frames(n_samples: int, config: Optional[Wav2Vec2Config] = None) -> int:
    """Frames the feature extractor makes of ``n_samples`` samples: ``floor((L - k) / s) + 1`` chained over its layers, 0 below the
    receptive field (400 samples in the default config).  Host integers."""
    c = _c_config(config or Wav2Vec2Config())
    n = int(_lib.load().dex_asr_num_frames(C.byref(c), int(n_samples)))
    if n < 0:
        raise ValueError(f"num_frames: bad arguments ({n_samples} samples)")
    return n


_HF_PARAM = {"parametrizations.weight.original0": "weight_g", "parametrizations.weight.original1": "weight_v"}
_IGNORED = ("wav2vec2.masked_spec_embed",)


class _Asr(Handle):
    """One DexAsr handle (the config, and once loaded the packed weights); its workspace is the network's."""

    def __init__(self, cfg: Wav2Vec2Config, device):
        super().__init__("dex_asr", device, C.byref(_c_config(cfg)))

    def create_failed(self, rc):
        return NotImplementedError(f"Wav2Vec2Config.{self.lib.dex_asr_last_error(None).decode()}")

    def shapes(self) -> dict:
        out = {}
        key, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        for i in range(self.lib.dex_asr_num_weights(self.h)):
            self.lib.dex_asr_weight_info(self.h, i, C.byref(key), shape, C.byref(nd))
            out[key.value.decode()] = tuple(int(shape[k]) for k in range(nd.value))
        return out

    def workspace(self, B: int, n: int) -> torch.Tensor:
        need = int(self.lib.dex_asr_workspace_bytes(self.h, B, n))
        if need == 0:
            raise ValueError(f"{B} rows of {n} samples: too short for one frame, or more than one call takes")
        return super().workspace(need)


_default_context = per_device(lambda device: _Asr(Wav2Vec2Config(), device))


def normalize_input(wav: torch.Tensor, lengths=None) -> torch.Tensor:
    """``Wav2Vec2FeatureExtractor`` with ``do_normalize``: per row over its own length ``(x - mean) / sqrt(var + 1e-7)`` with the
    biased variance; the statistics are fp64, the result is rounded to fp32 once; 0 past a row's length.  wav [n] or [B, n]."""
    x, ln, one = device_rows(wav, lengths, "normalize_input", refuse=ValueError)
    ctx = _default_context(x.device)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = ctx.lib.dex_asr_normalize(ctx.h, x.data_ptr(), i32_ptr(ln), x.shape[0], x.shape[1], out.data_ptr(), stream(x.device))
    ctx.check(rc, "dex_asr_normalize")
    return out[0] if one else out


def ctc_greedy(logits: torch.Tensor, frames=None):
    """Greedy CTC of logits [B, T, V] (or [T, V]) on the device, row b over its first ``frames[b]`` frames (default T): per frame the
    first index of the maximum (``torch.argmax``'s tie rule), repeats collapsed, blank (id 0) dropped -> a list of id lists.  One
    device-to-host copy carries ids and counts."""
    on_device(logits, "ctc_greedy", ValueError)
    if logits.dim() not in (2, 3):
        raise ValueError(f"ctc_greedy: expected logits [T, V] or [B, T, V], got {tuple(logits.shape)}")
    one = logits.dim() == 2
    x = (logits[None] if one else logits).to(torch.float32).contiguous()
    B, T, V = x.shape
    if B < 1 or T < 1 or V < 1:
        raise ValueError(f"ctc_greedy: empty logits {tuple(logits.shape)}")
    fr = host_lengths(frames, B, T, lo=0, what="ctc_greedy")
    ctx = _default_context(x.device)
    buf = torch.empty(B * T + B, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        rc = ctx.lib.dex_asr_ctc(ctx.h, x.data_ptr(), i32_ptr(fr), B, T, V, buf.data_ptr(), buf.data_ptr() + 4 * B * T, stream(x.device))
    ctx.check(rc, "dex_asr_ctc")
    out = _unpack(buf, B, T)
    return out[0] if one else out


def _unpack(buf: torch.Tensor, B: int, T: int):
    host = buf.cpu().numpy()
    ids, counts = host[: B * T].reshape(B, T), host[B * T:]
    return [ids[b, : int(counts[b])].tolist() for b in range(B)]


def decode(ids: Sequence[int], vocab: Optional[Sequence[str]] = None) -> str:
    """CTC-collapsed ids -> text, as ``Wav2Vec2CTCTokenizer.convert_tokens_to_string`` ends: the symbols joined, the word delimiter
    ``'|'`` as a space, stripped."""
    vocab = VOCAB if vocab is None else vocab
    return "".join(" " if vocab[int(i)] == "|" else vocab[int(i)] for i in ids).strip()


def normalize_sentence(text: str) -> str:
    """metric.py:97-110 ``normalize_sentence``: upper case; ``jiwer.RemovePunctuation`` (every character whose Unicode category
    starts with ``P``, the apostrophe included); ``jiwer.RemoveWhiteSpace(replace_by_space=True)``: ``\\n \\t \\r \\x0b \\x0c`` (Python's
    ``string.whitespace``) -> space; runs of spaces collapsed; stripped."""
    text = "".join(ch for ch in text.upper() if not unicodedata.category(ch).startswith("P"))
    for ch in "\n\t\r\x0b\x0c":
        text = text.replace(ch, " ")
    return " ".join(t for t in text.split(" ") if t)


def _levenshtein(a: Sequence, b: Sequence) -> int:
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def wer(gt: str, pred: str) -> float:
    """``jiwer.wer``: the word-level Levenshtein distance over the reference's word count; an empty reference raises."""
    ref = gt.split()
    if not ref:
        raise ValueError("wer: the reference has no words")
    return _levenshtein(ref, pred.split()) / len(ref)


def cer(gt: str, pred: str) -> float:
    """``jiwer.cer``: the character-level Levenshtein distance (spaces count) over the reference's length; an empty reference raises."""
    if not gt:
        raise ValueError("cer: the reference is empty")
    return _levenshtein(gt, pred) / len(gt)


class Wav2Vec2CTC:
    """HF's ``Wav2Vec2ForCTC`` in eval mode on one MI355X, fp32.  ``load_state_dict`` takes the HF checkpoint's state dict."""

    def __init__(self, config: Optional[Wav2Vec2Config] = None, device="cuda", vocab: Optional[Sequence[str]] = None):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("Wav2Vec2CTC runs on an MI355X only (no CPU path)")
        self.config = config or Wav2Vec2Config()
        self.vocab = tuple(VOCAB if vocab is None else vocab)
        if len(self.vocab) != self.config.vocab_size:
            raise ValueError(f"Wav2Vec2CTC: {len(self.vocab)} symbols for vocab_size {self.config.vocab_size}")
        self.device = torch.device("cuda", device_index(device))
        self._ctx = _Asr(self.config, self.device)
        self._loaded = False

    def state_dict_shapes(self) -> dict:
        """The HF state-dict keys the network needs, with their shapes (weight norm in its ``weight_g`` / ``weight_v`` spelling)."""
        return self._ctx.shapes()

    def load_state_dict(self, sd, strict: bool = True):
        """HF keys.  The positional convolution is taken as ``...conv.weight_g`` / ``weight_v`` or as ``...conv.parametrizations.
        weight.original0`` / ``original1``; ``wav2vec2.masked_spec_embed`` is ignored.  A wrong shape or (``strict``) a missing or
        unexpected key raises ``RuntimeError`` before anything is uploaded; with ``strict=False`` the network stays unusable until
        every key has arrived."""
        want = self.state_dict_shapes()
        routed = {}
        for k, v in sd.items():
            for old, new in _HF_PARAM.items():
                if k.endswith(old):
                    k = k[: -len(old)] + new
            routed[k] = v
        missing = [k for k in want if k not in routed]
        extra = [k for k in routed if k not in want and k not in _IGNORED]
        if strict and missing:
            raise RuntimeError(f"missing keys {missing[:4]}")
        if strict and extra:
            raise RuntimeError(f"unexpected keys {sorted(extra)[:4]}")
        tensors = {}
        for k, shape in want.items():
            if k in routed:
                v = torch.as_tensor(routed[k])
                if tuple(v.shape) != shape:
                    raise RuntimeError(f"{k}: expected shape {shape}, got {tuple(v.shape)}")
                tensors[k] = v
        self._loaded = False
        upload_weights(self._ctx, self._ctx.lib.dex_asr_load, tensors, self.device)
        if not missing:
            self.finalize()
            torch.cuda.current_stream(self.device).synchronize()        # the operands are packed when this returns
        return self

    def finalize(self):
        """Pack the operands (``dex_asr_finalize``); ``ValueError`` naming the first key that was never loaded."""
        ctx = self._ctx
        with torch.cuda.device(self.device):
            ctx.check(ctx.lib.dex_asr_finalize(ctx.h, stream(self.device)), "dex_asr_finalize")
        self._loaded = True
        return self

    def _need_weights(self, what: str):
        if not self._loaded:
            raise ValueError(f"{what}: the network's weights are not loaded (load_state_dict)")

    def _inputs(self, wav, lengths, what: str):
        self._need_weights(what)
        x, ln, one = device_rows(wav, lengths, what, refuse=ValueError)
        short = [v for v in ln if num_frames(v, self.config) < 1]
        if short:
            raise ValueError(f"{what}: {short[0]} samples are too short for one frame of the feature extractor")
        return x.to(self.device), ln, one

    def forward(self, input_values: torch.Tensor, lengths=None) -> torch.Tensor:
        """Raw 16 kHz samples [B, n] (or [n]), row b ``lengths[b]`` samples (what is stored past them is not read into any result)
        -> logits [B, T, V] with T = ``num_frames(n)``; row b fills ``num_frames(lengths[b])`` frames and is 0 past them.  The input
        normalisation is part of the call.  A row's logits are bitwise those of the row alone."""
        x, ln, one = self._inputs(input_values, lengths, "Wav2Vec2CTC.forward")
        B, n = x.shape
        ctx = self._ctx
        ws = ctx.workspace(B, n)
        out = torch.empty(B, num_frames(n, self.config), self.config.vocab_size, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = ctx.lib.dex_asr_logits(ctx.h, x.data_ptr(), i32_ptr(ln), B, n, out.data_ptr(), ws.data_ptr(), ws.numel(), stream(self.device))
        ctx.check(rc, "dex_asr_logits")
        return out[0] if one else out

    __call__ = forward

    def transcribe_ids(self, wavs: torch.Tensor, lengths=None):
        """forward + greedy CTC in one stream-ordered sequence -> a list of id lists; one device-to-host copy of ids and counts."""
        x, ln, _ = self._inputs(wavs, lengths, "Wav2Vec2CTC.transcribe")
        B, n = x.shape
        T = num_frames(n, self.config)
        ctx = self._ctx
        ws = ctx.workspace(B, n)
        buf = torch.empty(B * T + B, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = ctx.lib.dex_asr_transcribe(ctx.h, x.data_ptr(), i32_ptr(ln), B, n, buf.data_ptr(), buf.data_ptr() + 4 * B * T, ws.data_ptr(),
                                            ws.numel(), stream(self.device))
        ctx.check(rc, "dex_asr_transcribe")
        return _unpack(buf, B, T)

    def transcribe(self, wavs, lengths=None, sr: int = SAMPLING_RATE):
        """metric.py:24-35 for a batch: ``wavs`` [B, n] (or [n]) with ``lengths``, or a list of wavs, at ``sr`` Hz -> a list of
        transcripts.  Where ``sr`` is not 16000 the wavs are resampled by ``wavprep.resample`` (kaiser_best; librosa uses soxr)."""
        if int(sr) <= 0:
            raise ValueError(f"Wav2Vec2CTC.transcribe: sr must be positive, got {sr}")
        if not isinstance(wavs, torch.Tensor):
            wavs, lengths = pad_wavs(wavs, self.device, scale_int16=True)
        if int(sr) != SAMPLING_RATE:
            x, ln, _ = device_rows(wavs, lengths, "Wav2Vec2CTC.transcribe", refuse=ValueError)
            wavs, lengths = resample_to_16k(x, ln, sr)
        return [decode(ids, self.vocab) for ids in self.transcribe_ids(wavs, lengths)]


def asr_score(texts: Sequence[str], wavs, sr: int = SAMPLING_RATE, model: Optional[Wav2Vec2CTC] = None, lengths=None):
    """calculate_asr_score (metric.py:46-67): every wav transcribed, CER and WER of ``normalize_sentence(transcript)`` against
    ``normalize_sentence(text)`` -> (cer_mean, cer_stderr, wer_mean, wer_stderr), the errors ``np.std / sqrt(n)``."""
    if not isinstance(model, Wav2Vec2CTC):
        raise ValueError("asr_score: pass model=Wav2Vec2CTC(...) with the checkpoint's weights loaded (the library ships none)")
    preds = model.transcribe(wavs, lengths, sr)
    if len(preds) != len(texts) or not preds:
        raise ValueError(f"asr_score: {len(texts)} texts against {len(preds)} wavs")
    return score_transcripts(texts, preds)


def score_transcripts(texts: Sequence[str], preds: Sequence[str]):
    """The four numbers of calculate_asr_score from the transcripts (host only)."""
    c = [cer(normalize_sentence(t), normalize_sentence(p)) for t, p in zip(texts, preds)]
    w = [wer(normalize_sentence(t), normalize_sentence(p)) for t, p in zip(texts, preds)]
    n = len(c)
    return float(sum(c) / n), float(np.std(c) / np.sqrt(n)), float(sum(w) / n), float(np.std(w) / np.sqrt(n))
