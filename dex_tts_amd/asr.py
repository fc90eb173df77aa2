"""The ASR score on the device: the intelligibility half of the reference's ``Evaluater`` (src/metric.py:21-67, ``transcribe`` /
``calculate_wer_cer`` / ``calculate_asr_score``).  A synthesised wav at 16 kHz goes through HF's ``Wav2Vec2ForCTC``
(facebook/wav2vec2-large-960h-lv60-self), the argmax per frame is decoded as CTC, and the transcript is scored against the input
text as character and word error rates.

    Wav2Vec2Config(...)                                   the fields of HF's config the network reads; defaults = large-lv60-self
    Wav2Vec2CTC(config=None, device='cuda', vocab=None):  load_state_dict (HF keys), forward -> logits [B, T, V], transcribe -> [str]
    normalize_input(wav, lengths=None)                    Wav2Vec2FeatureExtractor's do_normalize
    num_frames(n_samples, config=None)                    floor((L - k) / s) + 1 chained over the feature extractor
    ctc_greedy(logits, frames) -> [[int]];  decode(ids, vocab=None) -> str
    Wav2Vec2CTC.align(wavs, texts) / .text_nll(wavs, texts)   word and character timings, the text's likelihood (ctc_align.py)
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

from ._native import device_rows, host_lengths, i32_ptr, on_device, per_device, stream
from ._wavnet import MAX_CONV, SAMPLING_RATE, HostEntry, NetHandle, WaveformNet, fill_trunk_config

VOCAB = ("<pad>", "<s>", "</s>", "<unk>", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M", "W", "C", "F", "G", "Y", "P",
         "B", "V", "K", "'", "X", "J", "Q", "Z")


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
    c = fill_trunk_config(DexAsrConfig(), cfg)
    c.feat_extract_norm_layer = int(cfg.feat_extract_norm == "layer")
    c.vocab = int(cfg.vocab_size)
    return c


_HOST = HostEntry("dex_asr", _c_config, Wav2Vec2Config, "Wav2Vec2Config")


def num_frames(n_samples: int, config: Optional[Wav2Vec2Config] = None) -> int:
    """Frames the feature extractor makes of ``n_samples`` samples: ``floor((L - k) / s) + 1`` chained over its layers, 0 below the
    receptive field (400 samples in the default config).  Host integers."""
    return _HOST.num_frames(n_samples, config)


def _check_lengths(lengths, n_samples: int, config, what: str) -> int:
    """``ValueError`` for a row below one frame; the frames of ``n_samples``."""
    short = [v for v in lengths if num_frames(v, config) < 1]
    if short:
        raise ValueError(f"{what}: {short[0]} samples are too short for one frame of the feature extractor")
    return num_frames(n_samples, config)


_NO_WORKSPACE = "too short for one frame, or more than one call takes"

# the handle the stateless entry points run on (no weights)
_default_context = per_device(lambda device: NetHandle("dex_asr", _c_config(Wav2Vec2Config()), device, "Wav2Vec2Config", _NO_WORKSPACE))


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


class Wav2Vec2CTC(WaveformNet):
    """HF's ``Wav2Vec2ForCTC`` in eval mode on one MI355X, fp32.  ``load_state_dict`` takes the HF checkpoint's state dict;
    ``wav2vec2.masked_spec_embed`` is ignored."""
    _prefix, _config_name, _no_workspace = "dex_asr", "Wav2Vec2Config", _NO_WORKSPACE
    _c_config = staticmethod(_c_config)
    _ignored = staticmethod(lambda key: key == "wav2vec2.masked_spec_embed")
    _check_lengths = staticmethod(_check_lengths)

    def __init__(self, config: Optional[Wav2Vec2Config] = None, device="cuda", vocab: Optional[Sequence[str]] = None):
        super().__init__(config or Wav2Vec2Config(), device)
        self.vocab = tuple(VOCAB if vocab is None else vocab)
        if len(self.vocab) != self.config.vocab_size:
            raise ValueError(f"Wav2Vec2CTC: {len(self.vocab)} symbols for vocab_size {self.config.vocab_size}")

    def forward(self, input_values: torch.Tensor, lengths=None) -> torch.Tensor:
        """Raw 16 kHz samples [B, n] (or [n]), row b ``lengths[b]`` samples (what is stored past them is not read into any result)
        -> logits [B, T, V] with T = ``num_frames(n)``; row b fills ``num_frames(lengths[b])`` frames and is 0 past them.  The input
        normalisation is part of the call.  A row's logits are bitwise those of the row alone."""
        x, ln, one, T = self._inputs(input_values, lengths, "Wav2Vec2CTC.forward")
        out = torch.empty(x.shape[0], T, self.config.vocab_size, dtype=torch.float32, device=self.device)
        return self._run("logits", x, ln, out, out.data_ptr(), one=one)

    __call__ = forward

    def transcribe_ids(self, wavs: torch.Tensor, lengths=None):
        """forward + greedy CTC in one stream-ordered sequence -> a list of id lists; one device-to-host copy of ids and counts."""
        x, ln, _, T = self._inputs(wavs, lengths, "Wav2Vec2CTC.transcribe")
        B = x.shape[0]
        buf = torch.empty(B * T + B, dtype=torch.int32, device=self.device)
        return _unpack(self._run("transcribe", x, ln, buf, buf.data_ptr(), buf.data_ptr() + 4 * B * T), B, T)

    def transcribe(self, wavs, lengths=None, sr: int = SAMPLING_RATE):
        """metric.py:24-35 for a batch: ``wavs`` [B, n] (or [n]) with ``lengths``, or a list of wavs, at ``sr`` Hz -> a list of
        transcripts.  Where ``sr`` is not 16000 the wavs are resampled by ``wavprep.resample`` (kaiser_best; librosa uses soxr)."""
        wavs, lengths = self._at_16k(wavs, lengths, sr, "Wav2Vec2CTC.transcribe")
        return [decode(ids, self.vocab) for ids in self.transcribe_ids(wavs, lengths)]

    def _text_inputs(self, wavs, texts, lengths, sr, unknown: str, what: str):
        """The checked inputs of the calls that take a text per wav: (rows, host lengths, T, (ids, words) per row, frames, targets,
        target lengths); ``ValueError`` for a text outside the vocabulary or one that does not fit its row's frames."""
        from .ctc_align import check_targets, text_to_targets
        wavs, lengths = self._at_16k(wavs, lengths, sr, what)
        x, ln, _, T = self._inputs(wavs, lengths, what)
        texts = [texts] if isinstance(texts, str) else list(texts)
        if len(texts) != x.shape[0]:
            raise ValueError(f"{what}: {len(texts)} texts against {x.shape[0]} wavs")
        pairs = [text_to_targets(t, self.vocab, unknown=unknown) for t in texts]
        frames = [num_frames(int(v), self.config) for v in ln]
        fr, tg, tl = check_targets(x.shape[0], T, self.config.vocab_size, frames, [p[0] for p in pairs], None, 0, True, what)
        return x, ln, T, pairs, fr, tg, tl

    def align(self, wavs, texts, lengths=None, sr: int = SAMPLING_RATE, unknown: str = "error"):
        """Forced alignment of each wav to its text (``ctc_align.py`` holds the definitions): forward, the Viterbi pass and the
        likelihood in one stream-ordered sequence, one device-to-host copy.  ``wavs`` as for ``transcribe``; ``texts`` one string per
        wav, turned into targets by ``text_to_targets`` (``unknown`` as there).  Per row ``{"words": [{"word", "start", "end",
        "score"}], "chars": [{"char", "start", "end", "score"}], "score", "nll", "frames"}``: times in seconds (frame t starts at
        sample ``t * prod(conv_stride)``; an end is clipped to the row's length), ``chars`` without the word delimiters, a word from
        its first character's start to its last character's end with the frame-weighted mean of its characters' scores.
        ``ValueError`` naming a row that cannot be aligned (too few frames, or -inf / NaN logits)."""
        from .ctc_align import AlignBuffers, ctc_workspace, word_alignment
        what = "Wav2Vec2CTC.align"
        x, ln, T, pairs, fr, tg, tl = self._text_inputs(wavs, texts, lengths, sr, unknown, what)
        B, Lm = x.shape[0], tg.shape[1]
        cws = ctc_workspace(self.device, B, T, self.config.vocab_size, Lm)
        out = AlignBuffers(B, T, Lm, self.device)
        self._run("align", x, ln, out.buf, i32_ptr(tg), i32_ptr(tl), Lm, *out.pointers(), cws.data_ptr(), cws.numel())
        host = {k: v.numpy() for k, v in out.views(out.buf.cpu()).items()}
        stride = int(np.prod(self.config.conv_stride))
        rows = []
        for b, (ids, words) in enumerate(pairs):
            if not np.isfinite(host["score"][b]):
                raise ValueError(f"{what}: row {b} has no alignment (score {host['score'][b]}): its logits hold -inf or NaN")
            rows.append(word_alignment(ids, words, host["spans"][b], host["token_scores"][b], host["score"][b], host["nll"][b], int(fr[b]),
                                       int(ln[b]), stride, self.vocab))
        return rows

    def text_nll(self, wavs, texts, lengths=None, sr: int = SAMPLING_RATE, unknown: str = "error") -> torch.Tensor:
        """The recogniser's negative log-likelihood of each wav's text: ``ctc_nll`` of ``forward``'s logits -> [B] fp64 on the device."""
        from .ctc_align import ctc_nll
        x, ln, _, _, fr, tg, tl = self._text_inputs(wavs, texts, lengths, sr, unknown, "Wav2Vec2CTC.text_nll")
        return ctc_nll(self.forward(x, ln), fr, tg, tl, 0)


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
