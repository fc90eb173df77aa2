"""Restatement of fallback decoding of dex_tts_amd/whisper.py (``DecodingPolicy``) in float64 numpy, on top of tests/whisper_ref.py and
tests/whisper_long_ref.py (imported, not edited): Philox4x32-10 (``philox``), the Gumbel noise of an id (``gumbel``), one step's
masked row, sample and log-probability (``step``), the no-speech probability, HF's compression ratio and ``_need_fallback``
(``decision``), one attempt (``attempt``), the attempts of one window (``window``) and both loops (``short_form``, ``long_form``).
tests/test_whisper_policy_cpu.py holds it to ``transformers``' own ``generate`` with the thresholds in double precision."""
import math
import types
import zlib

import numpy as np

from tests import whisper_long_ref as L
from tests import whisper_ref as R

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox(counter, key):
    """Philox4x32-10: ``counter`` four uint32 words (arrays broadcast), ``key`` two -> the four output words, uint64 arrays below 2^32."""
    c = [np.asarray(x, np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def policy(**kw):
    base = dict(temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None,
                no_speech_token_id=None, seed=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def library_policy(po):
    from dex_tts_amd.whisper import DecodingPolicy
    return DecodingPolicy(**vars(po))


def uniform(ids, step, attempt, seek, row_key, seed):
    """u = (w + 0.5) 2^-32 of the ids: w word id & 3 of Philox at counter (id >> 2, step, attempt + 16 seek, row key), key seed."""
    ids = np.asarray(ids, np.uint64)
    words = np.stack(philox((ids >> np.uint64(2), step, attempt + 16 * seek, row_key), (seed & 0xFFFFFFFF, seed >> 32)))
    w = words[(ids & np.uint64(3)).astype(np.int64), np.arange(len(ids))]
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def gumbel(ids, step, attempt, seek, row_key, seed):
    return -np.log(-np.log(uniform(ids, step, attempt, seek, row_key, seed)))


def perturbed(x, T, step, attempt, seek, row_key, seed):
    """The masked float64 row ``x`` -> what the argmax is taken of: ``x`` at T = 0, else x / T + g (masked ids stay -inf)."""
    x = np.asarray(x, np.float64)
    if T == 0:
        return x
    return np.where(np.isneginf(x), -np.inf, x / T + gumbel(np.arange(len(x)), step, attempt, seek, row_key, seed))


def log_prob(x, tok):
    """log_softmax over the surviving ids of the masked row at ``tok``."""
    x = np.asarray(x, np.float64)
    return float(x[tok] - L.logsumexp(x[np.isfinite(x)]))


def no_speech_prob(raw, ns):
    raw = np.asarray(raw, np.float64)
    e = np.exp(raw - raw.max())
    return float(e[ns] / e.sum())


def compression_ratio(tokens, V):
    width = int(math.log2(V) / 8) + 1
    raw = b"".join(int(t).to_bytes(width, "little") for t in tokens)
    return len(raw) / len(zlib.compress(raw))


def decision(po, ratio, avg, nsp):
    """HF's ``_need_fallback`` -> (needs a retry, skipped)."""
    need = skip = False
    if po.compression_ratio_threshold is not None and ratio > po.compression_ratio_threshold:
        need = True
    if po.logprob_threshold is not None and avg < po.logprob_threshold:
        need = True
    if po.no_speech_threshold is not None and avg < po.logprob_threshold and nsp > po.no_speech_threshold:
        need, skip = False, True
    return need, skip


def masked_row(logits, sp, seq, timestamps):
    """-> (the masked row, the rule's gap: inf in the plain form)."""
    if timestamps:
        return L.masked_ts(logits, sp, seq)
    return R.masked(logits, sp, len(seq)), np.inf


def fp32(logits):
    """The logits are fp32 values (the device's are; HF rounds its own to fp32 before the processors): rounded once, then float64."""
    return np.asarray(logits, np.float64).astype(np.float32).astype(np.float64)


def attempt(cfg, sd, enc, sp, T, index, seek, row_key, seed, timestamps, max_new=None, w=None):
    """One attempt on one row from the encoder output ``enc`` -> a namespace: ``ids`` (every step until eos, the cap or ``max_new``, eos
    included), ``rows`` (masked float64), ``scores`` (what the argmax was taken of), ``gaps`` (the rule's), ``raw`` (unmasked logits of
    the steps, rounded to fp32 as every row here is), ``first`` (the unmasked logits at prompt position 0), ``sum_logprob``, ``n_scored``, ``avg_logprob``."""
    dec = R.Decoder(cfg, sd, enc, w or R._f64(sd))
    room = cfg.max_target_positions - len(sp.prompt_ids)
    n_new = room if max_new is None else min(max_new, room)
    first = None
    for p, t in enumerate(sp.prompt_ids[:-1]):
        lg = fp32(dec.step_logits(int(t), p))
        first = lg if p == 0 else first
    tok, ids, rows, scores, gaps, raw, total = int(sp.prompt_ids[-1]), [], [], [], [], [], 0.0
    for i in range(n_new):
        lg = fp32(dec.step_logits(tok, len(sp.prompt_ids) - 1 + i))
        first = lg if first is None else first
        x, gap = masked_row(lg, sp, ids, timestamps)
        y = perturbed(x, T, i, index, seek, row_key, seed)
        tok = int(np.argmax(y))
        total += log_prob(x, tok)
        ids.append(tok); rows.append(x); scores.append(y); gaps.append(gap); raw.append(lg)
        if tok == sp.eos_token_id:
            break
    return types.SimpleNamespace(ids=ids, rows=np.stack(rows), scores=np.stack(scores), gaps=np.asarray(gaps), raw=np.stack(raw), first=first,
                                 sum_logprob=total, n_scored=len(ids), avg_logprob=total / len(ids), temperature=T)


def window(cfg, sd, feat, sp, po, seek, row_key, timestamps, max_new=None):
    """The attempts of one window of features -> (result, attempts): result has ``tokens`` (no eos; [] when skipped), ``temperature``,
    ``avg_logprob``, ``compression_ratio``, ``no_speech_prob``, ``skipped``; every attempt carries its own statistics and decision."""
    w = R._f64(sd)
    enc = R.encode(cfg, sd, feat, w)
    attempts, nsp = [], float("nan")
    for index, T in enumerate(po.temperatures):
        a = attempt(cfg, sd, enc, sp, T, index, seek, row_key, po.seed, timestamps, max_new, w)
        if index == 0 and po.no_speech_token_id is not None:
            nsp = no_speech_prob(a.first, po.no_speech_token_id)
        a.compression_ratio = compression_ratio(a.ids, cfg.vocab_size)
        a.need, a.skip = decision(po, a.compression_ratio, a.avg_logprob, nsp)
        attempts.append(a)
        if not a.need:
            break
    a = attempts[-1]
    tokens = a.ids[:-1] if a.ids[-1] == sp.eos_token_id else a.ids
    return types.SimpleNamespace(tokens=[] if a.skip else tokens, temperature=a.temperature, avg_logprob=a.avg_logprob, compression_ratio=a.compression_ratio,
                                 no_speech_prob=nsp, skipped=a.skip), attempts


def short_form(cfg, sd, feat, sp, po, row_key=0, max_new=None):
    return window(cfg, sd, feat, sp, po, 0, row_key, False, max_new)


def long_form(cfg, sd, wav, sp, po, row_key=0, max_new=None):
    """The window loop under a policy on one row -> (segments with the four numbers, windows [(seek, n, features, result, attempts)])."""
    feat, F = L.log_mel_long(cfg, wav)
    feat = feat.astype(np.float32)
    tb = sp.no_timestamps_token_id + 1
    seek, segments, windows = 0, [], []
    while seek < F:
        n = min(F - seek, 2 * cfg.max_source_positions)
        wf = L.window(cfg, feat, seek, n)
        res, attempts = window(cfg, sd, wf, sp, po, seek, row_key, True, max_new)
        windows.append((seek, n, wf, res, attempts))
        if res.skipped:
            seek += n
            continue
        segs, advance = L.retrieve_segments(res.tokens, tb, seek, n)
        extra = dict(temperature=res.temperature, avg_logprob=res.avg_logprob, compression_ratio=res.compression_ratio, no_speech_prob=res.no_speech_prob)
        segments += [dict(s, **extra) for s in segs]
        seek += advance
    return segments, windows
