"""Restatement of the long form of dex_tts_amd/whisper.py in float64 numpy, on top of tests/whisper_ref.py (imported, not edited): the
timestamp rule of ``WhisperTimeStampLogitsProcessor`` (``timestamp_rule``), the cut of a window's ids into segments of
``WhisperGenerationMixin._retrieve_segment`` (``retrieve_segments``), the front end of ``WhisperFeatureExtractor(truncation=False)``
(``log_mel_long``), greedy decoding of one window under the rule (``greedy_ts``) and the window loop (``long_form``).
tests/test_whisper_long_cpu.py holds each to ``transformers``' own code in double precision.

The geometries are whisper_ref's TINY (1 s windows) and WIDE (3 s windows) with a vocabulary laid out as the real one: text ids, eos,
specials, ``no_timestamps``, then ``max_source_positions + 1`` timestamps up to the end of the vocabulary."""
import types

import numpy as np

from tests import whisper_ref as R

N_FFT, HOP = R.N_FFT, R.HOP
TINY, WIDE = R.TINY, R.WIDE


def layout(cfg, n_special=3):
    """(eos, the special ids, no_timestamps, timestamp_begin) of ``cfg``'s vocabulary: the last max_source_positions + 1 ids are the
    timestamps, no_timestamps sits before them, ``n_special`` specials before it and eos before those."""
    tb = cfg.vocab_size - (cfg.max_source_positions + 1)
    nots = tb - 1
    eos = nots - n_special - 1
    return eos, tuple(range(eos + 1, nots)), nots, tb


def spec(cfg, suppress=(), begin_suppress=(), max_initial=None):
    """The long-form spec of ``cfg``: the prompt is the three specials (sot, language, task) and ends before ``no_timestamps``."""
    eos, special, nots, _ = layout(cfg)
    return types.SimpleNamespace(prompt_ids=tuple(special), suppress_tokens=tuple(suppress), begin_suppress_tokens=tuple(begin_suppress),
                                 eos_token_id=eos, no_timestamps_token_id=nots, max_initial_timestamp_index=max_initial)


def library_spec(sp):
    from dex_tts_amd.whisper import GenerationSpec
    return GenerationSpec(**vars(sp))


def logsumexp(x):
    x = np.asarray(x, np.float64)
    m = x.max() if x.size else -np.inf
    return m + np.log(np.exp(x - m).sum()) if np.isfinite(m) else -np.inf


def rule_ranges(scores, seq, sp):
    """The rule's parts that depend on ``seq`` alone (no_timestamps, pairing, monotonicity, the first step) -> the row with -inf there."""
    x = np.array(scores, np.float64)
    tb, eos = sp.no_timestamps_token_id + 1, sp.eos_token_id
    x[sp.no_timestamps_token_id] = -np.inf
    last_ts = len(seq) >= 1 and seq[-1] >= tb
    pen_ts = len(seq) < 2 or seq[-2] >= tb
    if last_ts:
        if pen_ts:
            x[tb:] = -np.inf
        else:
            x[:eos] = -np.inf
    stamps = [t for t in seq if t >= tb]
    if stamps:
        x[tb: stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1] = -np.inf
    if len(seq) == 0:
        x[:tb] = -np.inf
        if sp.max_initial_timestamp_index is not None:
            x[tb + sp.max_initial_timestamp_index + 1:] = -np.inf
    return x


def rule_gap(x, sp):
    """|logsumexp(timestamps) - max(text)| of a row that ``rule_ranges`` has masked (inf where either side is empty)."""
    tb = sp.no_timestamps_token_id + 1
    a, b = logsumexp(x[tb:]), x[:tb].max()
    return abs(a - b) if np.isfinite(a) and np.isfinite(b) else np.inf


def timestamp_rule(scores, seq, sp):
    """One row of scores under the timestamp rule, ``seq`` the row's new tokens so far -> the row with -inf where the rule masks."""
    x = rule_ranges(scores, seq, sp)
    tb = sp.no_timestamps_token_id + 1
    if logsumexp(x[tb:]) > x[:tb].max():
        x[:tb] = -np.inf
    return x


def masked_ts(logits, sp, seq):
    """The logits of new-token step len(seq) under the spec's masks and the rule -> (the masked row, the gap |logsumexp(ts) -
    max(text)| its last part decided on)."""
    x = R.masked(logits, sp, len(seq))
    return timestamp_rule(x, seq, sp), rule_gap(rule_ranges(x, seq, sp), sp)


def greedy_ts(cfg, sd, feat, sp, max_new=None, step_fn=None):
    """Greedy decoding of one window under the rule -> (ids of every step until eos, the cap or ``max_new``, eos included; the masked
    float64 rows; each step's gap |logsumexp(ts) - max(text)|; the unmasked float64 logits)."""
    if step_fn is None:
        w = R._f64(sd)
        step_fn = R.Decoder(cfg, sd, R.encode(cfg, sd, feat, w), w).step_logits
    room = cfg.max_target_positions - len(sp.prompt_ids)
    n_new = room if max_new is None else min(max_new, room)
    for p, t in enumerate(sp.prompt_ids[:-1]):
        step_fn(int(t), p)
    tok, ids, rows, gaps, raw = int(sp.prompt_ids[-1]), [], [], [], []
    for i in range(n_new):
        lg = step_fn(tok, len(sp.prompt_ids) - 1 + i)
        x, gap = masked_ts(lg, sp, ids)
        tok = int(np.argmax(x))
        ids.append(tok)
        rows.append(x)
        gaps.append(gap)
        raw.append(lg)
        if tok == sp.eos_token_id:
            break
    return ids, np.stack(rows), np.asarray(gaps), np.stack(raw)


def retrieve_segments(tokens, tb, seek, n):
    """A window's new ids without the trailing eos, decoded at frame ``seek`` over ``n`` frames -> (segments {"start", "end", "tokens"},
    the frames ``seek`` advances by)."""
    tokens = [int(t) for t in tokens]
    is_ts = [t >= tb for t in tokens]
    t0 = seek * 0.01
    pairs = [i for i in range(1, len(tokens)) if is_ts[i - 1] and is_ts[i]]          # index of a pair's second timestamp
    if not pairs:
        stamps = [t for t in tokens if t >= tb]
        if stamps and stamps[-1] != tb:
            end = float(stamps[-1] - tb)
        else:
            end = int(np.float32(n) * np.float32(0.01) / np.float32(0.02))
        return [dict(start=t0, end=t0 + end * 0.02, tokens=tokens)], n
    single = len(tokens) >= 2 and not is_ts[-2] and is_ts[-1]
    segments, start = [], 0
    for k, i in enumerate(pairs):
        final = k == len(pairs) - 1 and not single
        piece = tokens[start: i + 1 if final else i]                                   # the last piece keeps the pair's second stamp
        end = piece[-2] if final else piece[-1]
        segments.append(dict(start=t0 + float(piece[0] - tb) * 0.02, end=t0 + float(end - tb) * 0.02, tokens=piece))
        start = i
    if single:
        piece = tokens[start:]
        segments.append(dict(start=t0 + float(piece[0] - tb) * 0.02, end=t0 + float(piece[-1] - tb) * 0.02, tokens=piece))
        return segments, n
    return segments, (tokens[pairs[-1] - 1] - tb) * 2


def log_mel_long(cfg, wav, dtype=np.float64):
    """One row of 16 kHz samples -> ([num_mel_bins, F], F): at most one chunk, whisper_ref.log_mel; longer, the row reflected at its
    own ends, len // 160 frames, the floor at the whole row's maximum - 8; every step in ``dtype``."""
    if len(wav) <= R.n_samples(cfg):
        f = R.log_mel(cfg, wav, dtype)
        return f, f.shape[1]
    x = np.pad(np.asarray(wav, dtype), N_FFT // 2, mode="reflect")
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)
    T = len(wav) // HOP
    frames = x[np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]] * win
    k = np.arange(N_FFT // 2 + 1)
    ang = 2.0 * np.pi * ((k[:, None] * np.arange(N_FFT)[None, :]) % N_FFT) / N_FFT
    re, im = frames @ np.cos(ang).T.astype(dtype), frames @ np.sin(ang).T.astype(dtype)
    mel = (re * re + im * im) @ R.mel_filters(cfg.num_mel_bins).astype(dtype)
    ls = np.log10(np.maximum(mel, dtype(1e-10)))
    ls = np.maximum(ls, ls.max() - dtype(8.0))
    return ((ls + dtype(4.0)) / dtype(4.0)).T, T


def window(cfg, feat, seek, n):
    """Frames [seek, seek + n) of ``feat`` [n_mels, F], followed by 0.0 up to the full window."""
    W = 2 * cfg.max_source_positions
    out = np.zeros((feat.shape[0], W), feat.dtype)
    out[:, :n] = feat[:, seek: seek + n]
    return out


def long_form(cfg, sd, wav, sp, max_new=None):
    """The window loop on one row -> (segments, the windows [(seek, n, the window's fp32 features, ids without the trailing eos, masked
    float64 rows, gaps, unmasked float64 logits)])."""
    feat, F = log_mel_long(cfg, wav)
    feat = feat.astype(np.float32)                                                    # the front end rounds once
    tb = sp.no_timestamps_token_id + 1
    seek, segments, windows = 0, [], []
    while seek < F:
        n = min(F - seek, 2 * cfg.max_source_positions)
        wf = window(cfg, feat, seek, n)
        ids, rows, gaps, raw = greedy_ts(cfg, sd, wf, sp, max_new)
        tokens = ids[:-1] if ids[-1] == sp.eos_token_id else ids
        segs, advance = retrieve_segments(tokens, tb, seek, n)
        windows.append((seek, n, wf, ids, rows, gaps, raw))
        segments += segs
        assert advance >= 2 or seek + advance >= F
        seek += advance
    return segments, windows
