"""GPU: the long form of dex_tts_amd/whisper.py (csrc/whisper.hip: the step tail under the timestamp rule, the front end of a long
row, the window gather, the window loop) against its float64 restatement (tests/whisper_long_ref.py, itself held to transformers by
tests/test_whisper_long_cpu.py).  Tolerances are whisper_ref.tolerance's: 8 x the distance of the fp32 CPU evaluation from the float64
restatement.  Ids are compared through the first step whose decision the device's logit error could turn: the smaller of the float64
top-2 gap of the masked logits and |logsumexp(timestamps) - max(text)| below 4 x the bound of the row's logits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import whisper_long_ref as L
from tests import whisper_ref as R

pytestmark = pytest.mark.gpu

CFG = {"TINY": L.TINY, "WIDE": L.WIDE}
SUPPRESS = (0, 3)
# One window, B = 3: feature seeds (whisper_ref.make_features) and the cap of the first timestamp, chosen on the CPU so that the
# restatement leaves out no step.  Smallest of (top-2 gap, rule gap) over a row's steps against 4 x the bound measured with the fp32 CPU
# yardstick: TINY 2.5e-2 / 4.0e-2 / 5.1e-2 against 7.8e-3 / 4.9e-3 / 4.1e-3, WIDE 2.7e-2 / 5.8e-2 / 2.7e-2 against 4.8e-3 / 5.3e-3 /
# 6.5e-3 (the yardstick's fp32 sums depend on the host's BLAS; up to 8.9e-3 was seen).  The cap bites: without it the rows' first timestamps lie above it.
ONE = {"TINY": dict(seeds=(4, 17, 27), max_initial=5), "WIDE": dict(seeds=(4, 11, 13), max_initial=10)}
# Long form at TINY (1 s windows): (samples, whisper_ref.synth_wav seed) of the three rows, checked on the CPU.  Row 0 (2.5 s) takes
# three windows at seeks 0, 72, 170: two end in a mid-window pair with ids behind it that are discarded, the last (80 frames) ends
# "... text, timestamp, eos": a single timestamp ending.  Row 1 (1.5 s) takes two windows, a mid-window pair and a single timestamp
# ending.  Row 2 (9000 samples, a short row: log_mel's features) takes two, both cut at a mid-window pair.  Smallest (gap / 4 x bound)
# over all steps of a row: 5.9, 12.3, 7.3 - no step is left out.
LONG = ((40000, 323), (24000, 331), (9000, 309))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SD, _MODEL, _LONG = {}, {}, {}


def weights(name):
    if name not in _SD:
        _SD[name] = R.make_weights(CFG[name], 0)
    return _SD[name]


def model(name):
    if name not in _MODEL:
        from dex_tts_amd import whisper
        m = whisper.Whisper(R.library_config(CFG[name]), "cuda")
        _MODEL[name] = m.load_state_dict({k: torch.from_numpy(v) for k, v in weights(name).items()})
    return _MODEL[name]


def bound_of(cfg, sd, sp, wf, ids, raw):
    """4 x the bound of a window's logits: the fp32 CPU evaluation of the same positions against the float64 restatement."""
    P = len(sp.prompt_ids)
    seq = (list(sp.prompt_ids) + ids)[: cfg.max_target_positions]
    yard = R.torch_forward_fp32(cfg, sd, wf, seq)[1][P - 1: P - 1 + len(ids)]
    return 4 * R.tolerance(yard, raw[: len(yard)])[0]


def compared(what, rows, gaps, bound):
    """The number of leading steps whose decision the bound cannot turn, and the print of the margins next to it."""
    margin = np.minimum(R.top2_margin(rows), gaps)
    low = np.nonzero(margin < bound)[0]
    n = len(margin) if len(low) == 0 else int(low[0]) + 1
    print(f"{what}: {len(margin)} steps, smallest top-2 gap {R.top2_margin(rows).min():.3e}, smallest rule gap {gaps.min():.3e}, 4 x bound {bound:.3e}, compared {n}")
    return n


# ---------------------------------------------------------------------------------------------------- the rule tail alone
MSP = {96: 50, 1031: 150, 51866: 1500}


def _pick_ts(logits, mask, sp, seqs, finished):
    """dex_whisper_pick_ts on rows with the new-token histories ``seqs`` -> (ids, finished, lengths, count, last timestamps, new-token counts)."""
    from dex_tts_amd import _lib
    B, V = logits.shape
    tb = sp.no_timestamps_token_id + 1
    hist = np.full((B, 4), -7, np.int32)
    for b, seq in enumerate(seqs):
        hist[b, 2 - min(len(seq), 2): 2] = seq[-2:] if seq else []
    last = [max([t for t in seq if t >= tb], default=-1) for seq in seqs]
    lg, fin, ids = cuda(logits.astype(np.float32)), cuda(np.asarray(finished, np.int32)), cuda(hist)
    mk = cuda(np.asarray(mask, np.uint8))
    lens, count = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    lts, nn = cuda(np.asarray(last, np.int32)), cuda(np.asarray([len(s) for s in seqs], np.int32))
    cap = -1 if sp.max_initial_timestamp_index is None else sp.max_initial_timestamp_index
    rc = _lib.load().dex_whisper_pick_ts(lg.data_ptr(), B, V, mk.data_ptr(), sp.eos_token_id, sp.no_timestamps_token_id, cap, fin.data_ptr(), lens.data_ptr(),
                                         count.data_ptr(), ids.data_ptr(), 4, 2, lts.data_ptr(), nn.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    ids = ids.cpu().numpy()
    assert np.array_equal(ids[:, [0, 1, 3]], hist[:, [0, 1, 3]])
    return ids[:, 2].tolist(), fin.cpu().tolist(), lens.cpu().tolist(), int(count.item()), lts.cpu().tolist(), nn.cpu().tolist()


def rule_cases(V, sp):
    """(name, logits row, new-token history, finished flag) of every branch of the rule."""
    tb, eos = sp.no_timestamps_token_id + 1, sp.eos_token_id
    t = lambda i: tb + i                                                                   # noqa: E731

    def row(**spikes):
        x = -20.0 + 0.5 * np.linspace(-1.0, 1.0, V)              # the timestamps' sum without a spike: below -12, under every spike
        for k, v in spikes.items():
            x[int(k[1:])] = v
        return x

    many = row(**{f"i{7}": 2.0})
    many[t(10): t(30)] = 0.0                                      # 20 timestamps at 0: none beats 2.0, their sum (log 20 = 3.0) does
    tie = row(**{"i9": 4.0, "i5": 4.0, f"i{t(3)}": 1.0})
    return [
        ("first step: text masked, the best timestamp", row(**{"i5": 9.0, f"i{t(40)}": 3.0, f"i{t(2)}": 2.0}), [], 0),
        ("a single leading timestamp: every timestamp masked, the maximum sits on one", row(**{f"i{t(9)}": 9.0, "i6": 1.0}), [t(2)], 0),
        ("text after a timestamp: text wins", row(**{"i8": 5.0, f"i{t(9)}": 1.0}), [t(2), 5], 0),
        ("text after a timestamp: the timestamp wins", row(**{"i8": 1.0, f"i{t(9)}": 5.0}), [t(2), 5], 0),
        ("a suppressed id holds the maximum", row(**{"i3": 9.0, "i8": 5.0}), [t(2), 5], 0),
        ("a timestamp after text: text below eos masked, the partner may repeat", row(**{"i8": 9.0, f"i{t(7)}": 3.0, f"i{t(6)}": 8.0}), [t(2), 5, t(7)], 0),
        ("a timestamp after text: eos ends the row", row(**{"i8": 9.0, f"i{eos}": 6.0, f"i{t(7)}": 3.0}), [t(2), 5, t(7)], 0),
        ("a pair: text next", row(**{f"i{t(30)}": 9.0, "i6": 1.0}), [t(2), 5, t(7), t(7)], 0),
        ("timestamps never decrease", row(**{f"i{t(5)}": 9.0, f"i{t(7)}": 8.0, f"i{t(8)}": 6.0, "i4": 0.0}), [t(2), 5, t(7), t(7), 4], 0),
        ("the sum beats text where no single timestamp does; the tie of 20 at its lowest index", many, [t(2), 5], 0),
        ("a tie of two text ids at the lower index", tie, [t(2), 5], 0),
        ("a finished row emits eos", row(**{"i8": 9.0}), [t(2), 5], 1),
        ("a row of NaN", np.full(V, np.nan), [t(2), 5], 0),
    ]


def expect(x, mask, sp, seq, finished):
    if finished:
        return sp.eos_token_id
    if np.isnan(x).all():
        return 0
    y = np.where(mask != 0, -np.inf, x.astype(np.float32).astype(np.float64))
    return int(np.argmax(L.timestamp_rule(y, seq, sp)))


@pytest.mark.parametrize("max_initial", [None, 5])
@pytest.mark.parametrize("V", [96, 1031, 51866])
def test_rule_tail_kernel(V, max_initial):
    """The step tail under the rule alone on crafted logits, exact, every case as a row of its own (B = 1) and in batches of 3 at every
    batch position: the id, the finished flag, the length, the finished count, the last timestamp and the new-token count."""
    cfg = types_cfg(V)
    sp = L.spec(cfg, max_initial=max_initial)
    tb, eos = sp.no_timestamps_token_id + 1, sp.eos_token_id
    mask = np.zeros(V, np.uint8)
    mask[list(SUPPRESS)] = 1
    cases = rule_cases(V, sp)
    want = [expect(x, mask, sp, seq, fin) for _, x, seq, fin in cases]
    by_name = {c[0]: w for c, w in zip(cases, want)}
    # the crafted rows do what their names say
    assert by_name["first step: text masked, the best timestamp"] == (tb + 2 if max_initial is not None else tb + 40)
    assert by_name["a single leading timestamp: every timestamp masked, the maximum sits on one"] == 6
    assert by_name["text after a timestamp: text wins"] == 8 and by_name["text after a timestamp: the timestamp wins"] == tb + 9
    assert by_name["a suppressed id holds the maximum"] == 8
    assert by_name["a timestamp after text: text below eos masked, the partner may repeat"] == tb + 7
    assert by_name["a timestamp after text: eos ends the row"] == eos and by_name["a pair: text next"] == 6
    assert by_name["timestamps never decrease"] == tb + 8
    assert by_name["the sum beats text where no single timestamp does; the tie of 20 at its lowest index"] == tb + 10
    assert by_name["a tie of two text ids at the lower index"] == 5
    alone = []
    for (what, x, seq, fin), w in zip(cases, want):
        ids, f, lens, count, lts, nn = _pick_ts(x[None], mask, sp, [seq], [fin])
        assert ids == [w], (what, ids, w)
        ended = not fin and w == eos
        assert f == [1 if fin or ended else 0] and lens == [0 if fin or ended else 1] and count == int(ended), what
        prev = max([t for t in seq if t >= tb], default=-1)
        assert lts == [w if (w >= tb and not fin) else prev] and nn == [len(seq) + 1], what
        alone.append((ids[0], f[0], lens[0], lts[0], nn[0]))
    for shift in range(3):                                        # batches of 3: every case at every batch position
        order = [(i + shift) % len(cases) for i in range(len(cases) + (-len(cases)) % 3)]
        for k in range(0, len(order), 3):
            pick = order[k: k + 3]
            ids, f, lens, count, lts, nn = _pick_ts(np.stack([cases[i][1] for i in pick]), mask, sp, [cases[i][2] for i in pick], [cases[i][3] for i in pick])
            assert [(ids[j], f[j], lens[j], lts[j], nn[j]) for j in range(3)] == [alone[i] for i in pick]
            assert count == sum(int(not cases[i][3] and want[i] == eos) for i in pick)


def types_cfg(V):
    """A config that only carries the vocabulary's layout: V ids, the last MSP[V] + 1 of them timestamps."""
    return R._cfg(vocab_size=V, max_source_positions=MSP[V])


# ---------------------------------------------------------------------------------------------------- long front end, gather
@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_log_mel_long_ragged_rows(name):
    """Rows of chunk + 1 samples, exactly 2 chunks, 2.37 chunks, one chunk + 160 (one frame more than a window) and a short row, with
    garbage past each length: each meets the float64 restatement under the fp32 yardstick, has its own frame count, is 0.0 behind it
    and is BITWISE the row alone; the short row is ``log_mel``'s."""
    cfg, m = CFG[name], model(name)
    N = R.n_samples(cfg)
    lens = [N + 1, 2 * N, int(2.37 * N), N + 160, 4001]
    x = (10.0 * np.random.default_rng(3).standard_normal((len(lens), max(lens)))).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = R.synth_wav(n, 50 + b)
    got, frames = m.log_mel_long(cuda(x), lens)
    got = got.cpu().numpy()
    assert frames.tolist() == [n // 160 if n > N else N // 160 for n in lens] and got.shape == (len(lens), cfg.num_mel_bins, max(frames))
    for b, n in enumerate(lens):
        F = int(frames[b])
        ref, yard = L.log_mel_long(cfg, x[b, :n])[0], L.log_mel_long(cfg, x[b, :n], np.float32)[0]
        tol, d = R.tolerance(yard, ref)
        err = float(np.abs(got[b, :, :F].astype(np.float64) - ref).max())
        print(f"log_mel_long {name} n={n}: {F} frames, device err {err:.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}")
        assert np.isfinite(got[b]).all() and err <= tol and (got[b, :, F:] == 0.0).all()
        alone, fa = m.log_mel_long(cuda(x[b, :n]))
        assert fa.tolist() == [F] and np.array_equal(alone.cpu().numpy()[0], got[b, :, :F])
    assert np.array_equal(got[4, :, : N // 160], m.log_mel(cuda(x[4, :4001])).cpu().numpy())
    with pytest.raises(ValueError, match="longer than one chunk"):
        m.log_mel(cuda(x[0, : N + 1]))


def test_gather_windows():
    """Exact: seek 0, an odd seek, a last window shorter than the window with zeros behind it, rows at different seeks in one call."""
    cfg, m = L.TINY, model("TINY")
    W, F = 2 * cfg.max_source_positions, 257
    feats = np.random.default_rng(5).standard_normal((3, cfg.num_mel_bins, F)).astype(np.float32)
    rows, seeks, ns = [0, 2, 1, 2, 0], [0, 37, F - 31, 157, F - 1], [W, W, 31, W, 1]
    got = m._gather(cuda(feats), rows, seeks, ns).cpu().numpy()
    assert got.shape == (5, cfg.num_mel_bins, W)
    for a, (r, s, n) in enumerate(zip(rows, seeks, ns)):
        assert np.array_equal(got[a], L.window(cfg, feats[r], s, n)), (r, s, n)
    assert (got[2, :, 31:] == 0.0).all() and np.array_equal(m._gather(cuda(feats), [1], [F - 31], [31]).cpu().numpy()[0], got[2])
    with pytest.raises(ValueError, match="window"):
        m._gather(cuda(feats), [0], [F - 30], [31])


# ---------------------------------------------------------------------------------------------------- one window under the rule
@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_generate_under_the_rule(name):
    """B = 3 windows with different inputs: device ids equal the restatement's through the first low-margin step (with these seeds:
    every step, see ONE); at most 10 % of steps are left out; each row is the row alone."""
    cfg, m, sd, one = CFG[name], model(name), weights(name), ONE[name]
    sp = L.spec(cfg, SUPPRESS, (), one["max_initial"])
    lib_sp = L.library_spec(sp)
    feats = np.stack([R.make_features(cfg, s) for s in one["seeds"]])
    ids, lens = m.generate(cuda(feats), lib_sp, timestamps=True)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    total = left_out = 0
    tb = sp.no_timestamps_token_id + 1
    for b in range(3):
        ref_ids, rows, gaps, raw = L.greedy_ts(cfg, sd, feats[b], sp)
        n = compared(f"rule generate {name} row {b}", rows, gaps, bound_of(cfg, sd, sp, feats[b], ref_ids, raw))
        total, left_out = total + len(ref_ids), left_out + len(ref_ids) - n
        assert ids[b, :n].tolist() == ref_ids[:n]
        assert tb <= ref_ids[0] <= tb + one["max_initial"] and ref_ids[1] < tb
        if n == len(ref_ids):
            assert lens[b] == len([t for t in ref_ids if t != sp.eos_token_id])
        a_ids, a_lens = m.generate(cuda(feats[b:b + 1]), lib_sp, timestamps=True)
        a_ids = a_ids.cpu().numpy()[0]
        assert int(a_lens[0]) == lens[b] and np.array_equal(a_ids, ids[b, : len(a_ids)])
    assert left_out * 10 <= total, (left_out, total)


# ---------------------------------------------------------------------------------------------------- long form end to end
def long_case():
    """The three rows of LONG, computed once and shared, never changed: (wav, the restatement's segments, its windows)."""
    if not _LONG:
        sp = L.spec(L.TINY, SUPPRESS)
        _LONG["rows"] = []
        for n, seed in LONG:
            wav = R.synth_wav(n, seed)
            _LONG["rows"].append((wav, *L.long_form(L.TINY, weights("TINY"), wav, sp)))
    return _LONG["rows"]


def test_long_form_end_to_end():
    """Three rows in one batch (three windows, two windows, a short row): every window's ids equal the restatement's through the first
    low-margin step (none with these seeds, see LONG) and then its seek and segments do; each row equals the row alone; the rows reach
    a single timestamp ending, a mid-window pair and discarded ids; ``transcribe_long`` and ``whisper_scores(long_form=True)`` are
    their pieces; a row of chunk + 1 samples scores while ``log_mel`` refuses it."""
    from dex_tts_amd import synthesize, whisper
    from dex_tts_amd.asr import score_transcripts
    cfg, m, sd = L.TINY, model("TINY"), weights("TINY")
    sp = L.spec(cfg, SUPPRESS)
    lib_sp, tb = L.library_spec(sp), sp.no_timestamps_token_id + 1
    rows = long_case()
    # what the seeds were chosen for
    assert [len(r[2]) for r in rows] == [3, 2, 2] and [w[0] for w in rows[0][2]] == [0, 72, 170]
    ends = set()
    for _, _, windows in rows:
        for seek, n, wf, ids, *_ in windows:
            tok = ids[:-1] if ids[-1] == sp.eos_token_id else ids
            ts = [t >= tb for t in tok]
            pairs = [i for i in range(1, len(tok)) if ts[i - 1] and ts[i]]
            if ts[-2:] == [False, True]:
                ends.add("single")
            elif pairs:
                ends.add("pair")
                if pairs[-1] < len(tok) - 1:
                    ends.add("discarded")
    assert ends == {"single", "pair", "discarded"}
    wavs = [r[0] for r in rows]
    trace = []
    got = m.generate_segments([torch.from_numpy(w) for w in wavs], lib_sp, _trace=trace)
    seen = {b: [] for b in range(3)}
    for call in trace:
        assert len({b for b, *_ in call}) == len(call)
        for b, seek, n, tokens in call:
            seen[b].append((seek, n, tokens))
    total = left_out = 0
    for b, (wav, segments, windows) in enumerate(rows):
        exact = True
        for k, (seek, n, wf, ids, masked, gaps, raw) in enumerate(windows):
            assert exact and seen[b][k][:2] == (seek, n), (b, k, seen[b][k][:2], (seek, n))
            c = compared(f"long form row {b} window {k} (seek {seek}, {n} frames)", masked, gaps, bound_of(cfg, sd, sp, wf, ids, raw))
            total, left_out = total + len(ids), left_out + len(ids) - c
            tok = ids[:-1] if ids[-1] == sp.eos_token_id else ids
            assert seen[b][k][2][: min(c, len(tok))] == tok[: min(c, len(tok))]
            exact = c == len(ids) and seen[b][k][2] == tok
            if not exact:
                break                                             # the later windows of this row start elsewhere: left out
        if exact:
            assert len(seen[b]) == len(windows) and got[b] == segments
        alone = m.generate_segments(cuda(wav), lib_sp)
        assert alone == [got[b]]
    assert left_out * 10 <= total, (left_out, total)
    vocab = [f"Ġw{i}" for i in range(cfg.vocab_size)]
    texts = m.transcribe_long([torch.from_numpy(w) for w in wavs], lib_sp, vocab)
    assert texts == [whisper.decode([t for s in segs for t in s["tokens"]], vocab, sp.eos_token_id) for segs in got] and all(t.startswith(" w") for t in texts)
    audio = [(w * 32767.0).astype(np.int16) for w in wavs]
    refs = ["w1 w2 w3", "w4, w5!", "w6"]
    preds, *score = synthesize.whisper_scores(m, lib_sp, vocab, audio, refs, sr=16000, long_form=True)
    assert preds == m.transcribe_long(audio, lib_sp, vocab) and tuple(score) == score_transcripts(refs, preds)
    N = R.n_samples(cfg)
    one_more = cuda(R.synth_wav(N + 1, 9))
    with pytest.raises(ValueError, match="longer than one chunk"):
        m.log_mel(one_more)
    with pytest.raises(ValueError, match="longer than one chunk"):
        whisper.whisper_score(one_more[None], ["w1"], model=m, spec=lib_sp, vocab=vocab)
    preds, *_ = whisper.whisper_score(one_more[None], ["w1"], model=m, spec=lib_sp, vocab=vocab, long_form=True)
    assert len(preds) == 1 and preds[0].startswith(" w")


# ---------------------------------------------------------------------------------------------------- errors
def test_errors():
    from dex_tts_amd import whisper
    cfg, m = L.TINY, model("TINY")
    sp = L.library_spec(L.spec(cfg, SUPPRESS))
    wav = cuda(R.synth_wav(20000, 1))
    plain = whisper.GenerationSpec(sp.prompt_ids, SUPPRESS, (), sp.eos_token_id)
    vocab = [f"Ġw{i}" for i in range(cfg.vocab_size)]
    for call in (lambda: m.generate_segments(wav, plain), lambda: m.transcribe_long(wav, plain, vocab),
                 lambda: whisper.whisper_score(wav[None], ["w1"], model=m, spec=plain, vocab=vocab, long_form=True)):
        with pytest.raises(ValueError, match="no_timestamps_token_id"):
            call()
    import dataclasses
    few = dataclasses.replace(sp, no_timestamps_token_id=sp.no_timestamps_token_id + 1)      # one timestamp id short of a window's 51
    with pytest.raises(ValueError, match="timestamp ids"):
        m.generate_segments(wav, few)
    with pytest.raises(ValueError, match="above the cap"):
        m.log_mel_long(torch.zeros(whisper.MAX_LONG_SAMPLES + 1, device="cuda"))
    with pytest.raises(ValueError, match="CUDA"):
        m.generate_segments(torch.zeros(20000), sp)
    empty = whisper.Whisper(R.library_config(cfg), "cuda")
    with pytest.raises(ValueError, match="not loaded"):
        empty.generate_segments(wav, sp)
    # the C ABI refuses what the wrapper refuses, before anything is enqueued
    ctx = m._ctx
    ws, st = ctx.workspace(1), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    prompt = np.asarray(sp.prompt_ids, np.int32)
    buf, steps = torch.zeros(8, dtype=torch.int32, device="cuda"), C.c_int(0)
    rc = ctx.lib.dex_whisper_generate_ts(ctx.h, prompt.ctypes.data_as(C.POINTER(C.c_int32)), 3, None, None, sp.eos_token_id, few.no_timestamps_token_id, -1, 1, 4, 0,
                                         buf.data_ptr(), buf[4:].data_ptr(), C.byref(steps), ws.data_ptr(), ws.numel(), st)
    assert rc != 0 and "timestamp ids" in ctx.lib.dex_whisper_last_error(ctx.h).decode()
