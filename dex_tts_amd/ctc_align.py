"""CTC forced alignment and text likelihood on the device: where each symbol of a known text sits in the frames of a CTC recogniser
(word and character timings), and the recogniser's negative log-likelihood of that text.  The practice of WhisperX and of
torchaudio's ``forced_align``: a wav2vec 2.0 CTC model (``asr.Wav2Vec2CTC``) plus a Viterbi pass over the CTC trellis of the text.

    ctc_nll(logits, frames, targets, target_lengths=None, blank=0)    -> [B] fp64 on the device
    ctc_align(logits, frames, targets, target_lengths=None, blank=0)  -> {"states", "spans", "token_scores", "score", "nll"}
    text_to_targets(text, vocab=asr.VOCAB, delimiter="|", unknown="error") -> (ids, words)       host only
    check_targets(B, T, V, frames, targets, target_lengths=None, blank=0, feasible=False)       host only: the refusals
    word_alignment(...), alignment_score(texts, wavs, sr, model=, lengths=), speaking_rate(alignment)

Definitions, for row b.  Logits ``x[t, v]`` in fp32 for ``t < T_b`` frames; a target ``y[0..L)`` of ids in ``[0, V)``, none equal to
``blank`` (default 0), ``L >= 0``.

Trellis.  States ``s = 0 .. S-1`` with ``S = 2L + 1``; ``lab(s)`` is ``blank`` for even s and ``y[(s-1)/2]`` for odd s.  Transitions
into ``(t, s)`` come from ``(t-1, s)`` ("stay") and ``(t-1, s-1)`` ("step"); for odd ``s >= 3`` with ``lab(s) != lab(s-2)`` they also
come from ``(t-1, s-2)`` ("skip").  Start: ``a[0][0] = e(0, 0)`` and ``a[0][1] = e(0, 1)``; every other state starts at -inf.  ``R`` is
the number of adjacent equal target ids; the row is feasible by count if ``L + R <= T_b``.

Likelihood (``ctc_nll``).  ``e(t, s) = (double)x[t, lab(s)] - lse_t``, where ``lse_t`` is the fp64 log-sum-exp of the frame's V fp32
logits in a fixed order (lane v % 64 sums its logits in ascending order, then an xor butterfly over the 64 lanes), so that a row is
bitwise the row alone.  ``a[t][s] = logsumexp(stay, step, skip) + e(t, s)`` in fp64; a term of -inf contributes nothing, a state with
all three terms at -inf stays -inf, and no NaN comes from ``-inf - -inf``.  ``nll = -logsumexp(a[T-1][S-1], a[T-1][S-2])``; for
``L = 0`` it is ``-a[T-1][0]``.  This is ``F.ctc_loss(log_softmax(x), ..., reduction='none', zero_infinity=False)``; an infeasible
row gives ``+inf``, as torch does.

Viterbi (``ctc_align``).  The path is decided on the raw logits, ``e'(t, s) = (double)x[t, lab(s)]``: every path to a cell carries
the same sum of ``lse``, so the normaliser cannot change a decision; this is mathematically the log-probability Viterbi and makes the
path independent of any ``log`` / ``exp``.  ``a'[t][s] = max3 + e'(t, s)`` is one fp64 add, with no contraction or reassociation.
Candidates are taken in the order stay, step, skip and the first maximal one wins: stay wins ties, then step.  The final state is
``S-1`` unless ``a'[T-1][S-2] > a'[T-1][S-1]`` strictly; for ``L = 0`` it is 0.  Every operation is one IEEE fp64 add or compare in a
stated order, so the device path equals the numpy restatement (tests/ctc_ref.py) bit for bit, ties included.  ``score = a'_end -
sum_t lse_t``, the sum in fp64 in frame order.  The tie rule is this library's own: modelled on torchaudio's ``forced_align``, not
pinned to it.

Outputs of the alignment.  ``states [B, T]`` int32: the state per frame, -1 past ``T_b``.  ``spans [B, Lmax, 2]`` int32: first frame
and one past the last frame of each target position's state (every target position owns at least one frame on a valid path); -1 past
``L_b``.  ``token_scores [B, Lmax]`` fp64: the mean over the span's frames, in frame order, of ``exp((double)x[t, y_l] - lse_t)``; NaN
past ``L_b``.  ``score [B]`` and ``nll [B]`` fp64.

Rows without an alignment.  A row has no alignment if its score is -inf or NaN (from -inf or NaN logits): its states and spans are -1
and its token scores NaN; the backtrace never indexes outside ``[0, S)`` whatever the back-pointers hold.  A row infeasible by count
is refused on the host with ``ValueError`` naming the row (``ctc_nll`` takes it and returns ``+inf``).

Times.  Frame t of the wav2vec 2.0 feature extractor starts at sample ``t * stride``, ``stride = prod(conv_stride)`` (320).  A span
``[t0, t1)`` is ``t0 * stride / 16000`` to ``min(t1 * stride, n_b) / 16000`` seconds, in float64.

The kernels are ``csrc/ctc_align.hip`` (C ABI ``dex_ctc_*``, ``dex_asr_align``), fp64, stateless.  Targets and lengths are host
arrays, validated before anything is launched: ids in ``[0, V)``, none equal to ``blank``, ``0 <= L <= Lmax <= 1023``,
``1 <= T_b <= T <= 4096``, ``B <= 1024``.
"""
from __future__ import annotations

import unicodedata
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._native import check, host_lengths, i32_ptr, on_device, per_device, stream

MAX_FRAMES, MAX_TARGET, MAX_ROWS, MAX_VOCAB = 4096, 1023, 1024, 65536


# ---------------------------------------------------------------------------------------------------------------- host side
def text_to_targets(text: str, vocab: Optional[Sequence[str]] = None, delimiter: str = "|", unknown: str = "error"):
    """The text as CTC target ids of ``vocab`` (default ``asr.VOCAB``) -> ``(ids, words)``; host only.  The text is upper-cased, runs of
    whitespace become one ``delimiter``, leading and trailing delimiters are dropped.  A character in ``vocab`` is kept, the
    apostrophe included; a character whose Unicode category starts with ``P`` and which is not in the vocabulary is dropped; any other
    character (digits, letters outside the vocabulary) raises ``ValueError`` naming the character and its position, or is dropped
    with ``unknown="drop"``.  A word left empty disappears.  ``words`` are the kept words, ``ids`` their symbols joined by the
    delimiter.  Note: the score functions (``asr_score``) compare through ``normalize_sentence``, which deletes the apostrophe; the
    alignment keeps it, since the recogniser emits it."""
    if unknown not in ("error", "drop"):
        raise ValueError(f"text_to_targets: unknown must be 'error' or 'drop', got {unknown!r}")
    if vocab is None:
        from .asr import VOCAB as vocab
    index = {s: i for i, s in enumerate(vocab)}
    if delimiter not in index:
        raise ValueError(f"text_to_targets: the delimiter {delimiter!r} is not in the vocabulary")
    words, cur = [], []
    for pos, ch in enumerate(text.upper()):
        if ch.isspace():
            if cur:
                words.append("".join(cur))
            cur = []
        elif ch in index and ch != delimiter and len(ch) == 1:
            cur.append(ch)
        elif unicodedata.category(ch).startswith("P"):
            continue
        elif unknown == "error":
            raise ValueError(f"text_to_targets: character {ch!r} at position {pos} is not in the vocabulary (spell it out, or unknown='drop')")
    if cur:
        words.append("".join(cur))
    ids = []
    for i, w in enumerate(words):
        if i:
            ids.append(index[delimiter])
        ids.extend(index[c] for c in w)
    return ids, words


def _host_targets(targets, target_lengths, B: int, what: str):
    """``targets`` (a list of id lists, or a padded host array / tensor [B, Lmax] with ``target_lengths``) -> (int64 [B, Lmax'],
    int64 [B]) with Lmax' >= 1."""
    if torch.is_tensor(targets):
        targets = targets.detach().cpu().numpy()
    if isinstance(targets, np.ndarray) and targets.ndim == 2:
        tg = targets.astype(np.int64)
        tl = np.full(tg.shape[0], tg.shape[1], dtype=np.int64) if target_lengths is None else \
            np.asarray(target_lengths.detach().cpu() if torch.is_tensor(target_lengths) else target_lengths, dtype=np.int64).reshape(-1)
        if tl.shape != (tg.shape[0],) or (tl < 0).any() or (tl > tg.shape[1]).any():
            raise ValueError(f"{what}: target_lengths must hold one value in [0, {tg.shape[1]}] per row")
    else:
        if target_lengths is not None:
            raise ValueError(f"{what}: target_lengths goes with a padded [B, Lmax] array, not with a list of id lists")
        rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in targets]
        tl = np.array([len(r) for r in rows], dtype=np.int64)
        tg = np.zeros((len(rows), max(1, int(tl.max()) if len(rows) else 1)), dtype=np.int64)
        for b, r in enumerate(rows):
            tg[b, : len(r)] = r
    if tg.shape[0] != B:
        raise ValueError(f"{what}: {tg.shape[0]} targets for {B} rows")
    if tg.shape[1] < 1:
        tg = np.zeros((B, 1), dtype=np.int64)
    return tg, tl


def check_targets(B: int, T: int, V: int, frames, targets, target_lengths=None, blank: int = 0, feasible: bool = False, what: str = "ctc_align"):
    """What is refused before anything is launched, host only -> (frames int32 [B], targets int32 [B, Lmax], target lengths int32 [B]).
    ``ValueError`` for B outside [1, 1024], T outside [1, 4096], V outside [1, 65536], a blank outside [0, V), a target longer than 1023
    symbols, an id outside [0, V) or equal to the blank and, with ``feasible``, the first row whose ``L + R`` exceeds its frames."""
    if not 1 <= B <= MAX_ROWS:
        raise ValueError(f"{what}: {B} rows; one call takes 1 .. {MAX_ROWS}")
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError(f"{what}: {T} frames; one call takes 1 .. {MAX_FRAMES}")
    if not 1 <= V <= MAX_VOCAB:
        raise ValueError(f"{what}: {V} symbols; the vocabulary holds 1 .. {MAX_VOCAB}")
    if not 0 <= int(blank) < V:
        raise ValueError(f"{what}: blank {blank} outside [0, {V})")
    fr = host_lengths(frames, B, T, lo=1, what=what)
    tg, tl = _host_targets(targets, target_lengths, B, what)
    if int(tl.max()) > MAX_TARGET:
        raise ValueError(f"{what}: row {int(tl.argmax())} has {int(tl.max())} target symbols; one row takes at most {MAX_TARGET}")
    for b in range(B):
        y = tg[b, : tl[b]]
        if ((y < 0) | (y >= V)).any():
            raise ValueError(f"{what}: row {b} holds the id {int(y[(y < 0) | (y >= V)][0])} outside [0, {V})")
        if (y == blank).any():
            raise ValueError(f"{what}: row {b} holds the blank ({blank}) in its target")
        if feasible:
            need = int(tl[b]) + (int((y[1:] == y[:-1]).sum()) if tl[b] > 1 else 0)
            if need > fr[b]:
                raise ValueError(f"{what}: row {b} cannot be aligned: {int(tl[b])} symbols with {need - int(tl[b])} repeats need {need} frames, "
                                 f"the row has {int(fr[b])}")
    width = max(1, int(tl.max()))
    tg = tg[:, :width] if tg.shape[1] >= width else np.pad(tg, ((0, 0), (0, width - tg.shape[1])))
    return fr, np.ascontiguousarray(tg.astype(np.int32)), np.ascontiguousarray(tl.astype(np.int32))


def speaking_rate(alignment) -> float:
    """Words per second between the first word's start and the last word's end of one row of ``Wav2Vec2CTC.align``."""
    words = alignment["words"]
    if not words:
        raise ValueError("speaking_rate: the alignment has no words")
    span = float(words[-1]["end"]) - float(words[0]["start"])
    if not span > 0.0:
        raise ValueError("speaking_rate: the words span no time")
    return len(words) / span


# ---------------------------------------------------------------------------------------------------------------- device side
class _Workspace:
    def __init__(self, device):
        self.device, self.buf = device, None

    def get(self, need: int) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < need:
            self.buf = None
            self.buf = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.buf


_workspace = per_device(_Workspace)


def ctc_workspace(device, B: int, T: int, V: int, Lmax: int) -> torch.Tensor:
    """The device's growing CTC workspace, at least ``dex_ctc_workspace_bytes`` long."""
    need = int(_lib.load().dex_ctc_workspace_bytes(B, T, V, Lmax))
    if need == 0:
        raise ValueError(f"ctc workspace: (B, T, V, Lmax) = {(B, T, V, Lmax)} is outside what one call takes")
    return _workspace(device).get(need)


class AlignBuffers:
    """The outputs of one alignment call in ONE device buffer, so that they travel to the host in one copy: fp64 token_scores
    [B, Lmax], score [B], nll [B], then int32 states [B, T], spans [B, Lmax, 2]."""

    def __init__(self, B: int, T: int, Lmax: int, device):
        self.B, self.T, self.Lmax = B, T, Lmax
        self.n64 = B * Lmax + 2 * B
        self.n32 = B * T + 2 * B * Lmax
        self.buf = torch.empty(self.n64 + (self.n32 + 1) // 2, dtype=torch.float64, device=device)

    def views(self, buf=None):
        buf = self.buf if buf is None else buf
        B, T, Lm = self.B, self.T, self.Lmax
        d, i = buf[: self.n64], buf[self.n64:].view(torch.int32)
        return {"token_scores": d[: B * Lm].view(B, Lm), "score": d[B * Lm: B * Lm + B], "nll": d[B * Lm + B:],
                "states": i[: B * T].view(B, T), "spans": i[B * T: B * T + 2 * B * Lm].view(B, Lm, 2)}

    def pointers(self):
        v = self.views()
        return [v[k].data_ptr() for k in ("states", "spans", "token_scores", "score", "nll")]


def _logits(logits, what: str):
    on_device(logits, what, ValueError)
    if logits.dim() not in (2, 3):
        raise ValueError(f"{what}: expected logits [T, V] or [B, T, V], got {tuple(logits.shape)}")
    one = logits.dim() == 2
    x = (logits[None] if one else logits).to(torch.float32).contiguous()
    if min(x.shape) < 1:
        raise ValueError(f"{what}: empty logits {tuple(logits.shape)}")
    return x, one


def ctc_nll(logits: torch.Tensor, frames=None, targets=(), target_lengths=None, blank: int = 0) -> torch.Tensor:
    """The negative log-likelihood of each row's target under logits [B, T, V] (or [T, V]), row b over its first ``frames[b]`` frames
    (default T) -> [B] fp64 on the device (a scalar tensor for [T, V]); ``+inf`` where the target does not fit the frames.
    ``targets`` is a list of id lists or a padded host array with ``target_lengths``."""
    x, one = _logits(logits, "ctc_nll")
    B, T, V = x.shape
    fr, tg, tl = check_targets(B, T, V, frames, [targets] if one and _is_flat(targets) else targets, target_lengths, blank, False, "ctc_nll")
    ws = ctc_workspace(x.device, B, T, V, tg.shape[1])
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().dex_ctc_nll(x.data_ptr(), i32_ptr(fr), B, T, V, i32_ptr(tg), i32_ptr(tl), tg.shape[1], int(blank), out.data_ptr(),
                                     ws.data_ptr(), ws.numel(), stream(x.device))
    check(rc, "dex_ctc_nll")
    return out[0] if one else out


def _is_flat(targets) -> bool:
    """A single id list (for [T, V] logits) rather than a list of them."""
    if isinstance(targets, np.ndarray) or torch.is_tensor(targets):
        return targets.ndim == 1
    return len(targets) == 0 or not hasattr(targets[0], "__len__")


def ctc_align(logits: torch.Tensor, frames=None, targets=(), target_lengths=None, blank: int = 0):
    """The Viterbi alignment of each row's target to logits [B, T, V] (or [T, V]) and its likelihood -> a dict of device tensors:
    ``states`` [B, T] int32, ``spans`` [B, Lmax, 2] int32, ``token_scores`` [B, Lmax] fp64, ``score`` [B] fp64, ``nll`` [B] fp64 (the
    module docstring defines them; without the leading B for [T, V]).  ``ValueError`` naming the first row that is infeasible by
    count.  The tensors are views of one buffer."""
    x, one = _logits(logits, "ctc_align")
    B, T, V = x.shape
    fr, tg, tl = check_targets(B, T, V, frames, [targets] if one and _is_flat(targets) else targets, target_lengths, blank, True, "ctc_align")
    Lm = tg.shape[1]
    ws = ctc_workspace(x.device, B, T, V, Lm)
    out = AlignBuffers(B, T, Lm, x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().dex_ctc_align(x.data_ptr(), i32_ptr(fr), B, T, V, i32_ptr(tg), i32_ptr(tl), Lm, int(blank), *out.pointers(),
                                       ws.data_ptr(), ws.numel(), stream(x.device))
    check(rc, "dex_ctc_align")
    v = out.views()
    return {k: t[0] for k, t in v.items()} if one else v


# ---------------------------------------------------------------------------------------------------------------- words and times
def word_alignment(ids: Sequence[int], words: Sequence[str], spans, token_scores, score: float, nll: float, frames: int, n_samples: int,
                   stride: int, vocab: Sequence[str], delimiter: str = "|", sr: int = 16000):
    """One row of ``Wav2Vec2CTC.align`` from the host copies of its spans [L, 2] and token scores [L]: characters (delimiters left
    out) and words with start / end in seconds and a score; a word runs from its first character's start to its last character's end
    and scores the frame-weighted mean of its characters' scores."""
    def seconds(t0, t1):
        return float(np.float64(int(t0) * stride) / np.float64(sr)), float(np.float64(min(int(t1) * stride, int(n_samples))) / np.float64(sr))

    chars, out_words, cur, w = [], [], [], 0
    for l, i in enumerate(ids):
        sym = vocab[int(i)]
        if sym == delimiter:
            continue
        t0, t1 = int(spans[l][0]), int(spans[l][1])
        start, end = seconds(t0, t1)
        chars.append({"char": sym, "start": start, "end": end, "score": float(token_scores[l])})
        cur.append((t0, t1, float(token_scores[l])))
        if l + 1 == len(ids) or vocab[int(ids[l + 1])] == delimiter:
            n = sum(b - a for a, b, _ in cur)
            start, end = seconds(cur[0][0], cur[-1][1])
            out_words.append({"word": words[w], "start": start, "end": end, "score": float(sum((b - a) * p for a, b, p in cur) / n)})
            cur, w = [], w + 1
    return {"words": out_words, "chars": chars, "score": float(score), "nll": float(nll), "frames": int(frames)}


def alignment_score(texts: Sequence[str], wavs, sr: int = 16000, model=None, lengths=None, unknown: str = "error"):
    """Every wav aligned to its text -> ``(alignments, nll_per_char_mean, nll_per_char_stderr)``: per row ``nll / max(L, 1)`` with L the
    target's symbols (delimiters included), the error ``np.std / sqrt(n)`` like the other scores."""
    from .asr import Wav2Vec2CTC
    model = Wav2Vec2CTC._model(model, "alignment_score")
    if not len(texts):
        raise ValueError("alignment_score: no texts")
    alignments = model.align(wavs, texts, lengths=lengths, sr=sr, unknown=unknown)
    v = [a["nll"] / max(len(text_to_targets(t, model.vocab, unknown=unknown)[0]), 1) for a, t in zip(alignments, texts)]
    return alignments, float(sum(v) / len(v)), float(np.std(v) / np.sqrt(len(v)))
