"""GPU: fallback decoding of dex_tts_amd/whisper.py (csrc/whisper.hip: the policy step tail, the no-speech probe, the attempt loop that
decodes retried rows from the encoder output already computed) against its float64 restatement (tests/whisper_policy_ref.py, itself
held to transformers by tests/test_whisper_policy_cpu.py).  The tail alone is exact on the same fp32 logits.  In the loops the logits
carry the network's error: tolerances are whisper_ref.tolerance's, ids are compared through the first step whose decision 4 x the
bound of the row's logits could turn (at temperature T the perturbed scores carry bound / T), and every threshold lies at least 16 x
the bound from every statistic it is compared with (asserted), so no decision hangs on the error."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import whisper_long_ref as L
from tests import whisper_policy_ref as P
from tests import whisper_ref as R

pytestmark = pytest.mark.gpu

CFG = {"TINY": L.TINY, "WIDE": L.WIDE}
SUPPRESS = (0, 3)
TEMPS = (0.0, 0.4, 0.8)
MSP = {96: 50, 1031: 150, 2048 + 37: 150, 51866: 1500}
_SD, _MODEL, _CASE = {}, {}, {}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------- the tail alone
def tail_spec(V, max_initial=None):
    return L.spec(R._cfg(vocab_size=V, max_source_positions=MSP[V]), max_initial=max_initial)


def pick_policy(logits, mask, sp, timestamps, T, seed, attempt, keys, seeks, seqs, finished, step):
    """dex_whisper_pick_policy on fp32 rows -> (ids, finished, lengths, count, sum_logprob, n_scored)."""
    from dex_tts_amd import _lib
    B, V = logits.shape
    tb = sp.no_timestamps_token_id + 1
    hist = np.full((B, step + 2), -7, np.int32)
    for b, seq in enumerate(seqs):
        hist[b, step - min(len(seq), 2): step] = seq[-2:] if seq else []
    last = [max([t for t in seq if t >= tb], default=-1) for seq in seqs]
    lg, fin, ids, mk = cuda(logits), cuda(np.asarray(finished, np.int32)), cuda(hist), cuda(np.asarray(mask, np.uint8))
    lens, count = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    lts, nn = cuda(np.asarray(last, np.int32)), cuda(np.asarray([len(s) for s in seqs], np.int32))
    slp, ns = torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    kk, sk = np.asarray(keys, np.uint32), np.asarray(seeks, np.int32)
    cap = -1 if sp.max_initial_timestamp_index is None else sp.max_initial_timestamp_index
    rc = _lib.load().dex_whisper_pick_policy(lg.data_ptr(), B, V, mk.data_ptr(), sp.eos_token_id, int(timestamps), sp.no_timestamps_token_id, cap, float(T), seed, attempt,
                                             kk.ctypes.data_as(C.POINTER(C.c_uint32)), sk.ctypes.data_as(C.POINTER(C.c_int32)), fin.data_ptr(), lens.data_ptr(),
                                             count.data_ptr(), ids.data_ptr(), step + 2, step, lts.data_ptr(), nn.data_ptr(), slp.data_ptr(), ns.data_ptr(), stream())
    assert rc == 0
    got = ids.cpu().numpy()
    keep = [c for c in range(step + 2) if c != step]
    assert np.array_equal(got[:, keep], hist[:, keep])
    return got[:, step].tolist(), fin.cpu().tolist(), lens.cpu().tolist(), int(count.item()), slp.cpu().numpy(), ns.cpu().tolist()


def plain_pick(logits, mask, sp, timestamps, seqs, finished, step):
    """The ids of dex_whisper_pick / dex_whisper_pick_ts on the same rows."""
    from dex_tts_amd import _lib
    B, V = logits.shape
    tb = sp.no_timestamps_token_id + 1
    hist = np.full((B, step + 2), -7, np.int32)
    for b, seq in enumerate(seqs):
        hist[b, step - min(len(seq), 2): step] = seq[-2:] if seq else []
    lg, fin, ids, mk = cuda(logits), cuda(np.asarray(finished, np.int32)), cuda(hist), cuda(np.asarray(mask, np.uint8))
    lens, count = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    if timestamps:
        lts = cuda(np.asarray([max([t for t in seq if t >= tb], default=-1) for seq in seqs], np.int32))
        nn = cuda(np.asarray([len(s) for s in seqs], np.int32))
        cap = -1 if sp.max_initial_timestamp_index is None else sp.max_initial_timestamp_index
        rc = lib.dex_whisper_pick_ts(lg.data_ptr(), B, V, mk.data_ptr(), sp.eos_token_id, sp.no_timestamps_token_id, cap, fin.data_ptr(), lens.data_ptr(), count.data_ptr(),
                                     ids.data_ptr(), step + 2, step, lts.data_ptr(), nn.data_ptr(), stream())
    else:
        rc = lib.dex_whisper_pick(lg.data_ptr(), B, V, mk.data_ptr(), sp.eos_token_id, fin.data_ptr(), lens.data_ptr(), count.data_ptr(), ids.data_ptr(), step + 2, step,
                                  stream())
    assert rc == 0
    return ids.cpu().numpy()[:, step].tolist()


def tail_rows(V, sp, timestamps):
    """(logits fp32 [3, V], the rows' new-token histories, finished flags): standard deviation 3 - the timestamps' summed probability
    wins in some rows and loses in others; row 1 has finished."""
    tb = sp.no_timestamps_token_id + 1
    rng = np.random.default_rng(V + int(timestamps))
    x = (3.0 * rng.standard_normal((3, V))).astype(np.float32)
    x[2, :tb] += 4.0                                             # text far ahead in row 2: the rule does not force a timestamp there
    seqs = [[tb + 2, 5], [tb + 2, 5, 6], [tb + 1, 5, tb + 7, tb + 7, 4]] if timestamps else [[5, 6], [5], [7, 8, 9]]
    return x, seqs, [0, 1, 0]


def tail_expect(x, mask, sp, timestamps, T, seed, attempt, key, seek, seq, fin, step):
    """The restatement on one fp32 row -> (id, the perturbed top-2 gap, the log-probability of the id or None for a finished row)."""
    y = np.where(np.asarray(mask) != 0, -np.inf, x.astype(np.float64))
    y = L.timestamp_rule(y, seq, sp) if timestamps else y
    if fin:
        return sp.eos_token_id, np.inf, None
    s = P.perturbed(y, T, step, attempt, seek, key, seed)
    top = np.sort(s[np.isfinite(s)])
    gap = top[-1] - top[-2] if len(top) > 1 else np.inf
    tok = int(np.argmax(s))
    return tok, gap, P.log_prob(y, tok)


@pytest.mark.parametrize("timestamps", [False, True], ids=["plain", "rule"])
@pytest.mark.parametrize("V", [96, 1031, 2048 + 37, 51866])
def test_policy_tail_kernel(V, timestamps):
    """The tail alone at T = 0, 0.2 and 1.0: B = 3 with a finished row (one row at V = 51866), and a row with everything but one id
    masked.  Ids equal the restatement's on the same fp32 logits wherever the perturbed top-2 gap exceeds 1e-9 (with these seeds: every
    row, asserted); the chosen id's log-probability lies within 2 V 2^-53 + 1e-15; at T = 0 the ids are those of dex_whisper_pick /
    dex_whisper_pick_ts; each row is the row alone under its own key."""
    sp = tail_spec(V)
    tb, eos = sp.no_timestamps_token_id + 1, sp.eos_token_id
    x, seqs, fins = tail_rows(V, sp, timestamps)
    if V == 51866:
        x, seqs, fins = x[:1], seqs[:1], fins[:1]
    B = len(x)
    mask = np.zeros(V, np.uint8)
    mask[list(SUPPRESS)] = 1
    lonely = np.ones(V, np.uint8)                                # everything but one id masked
    lonely[7] = 0
    tol, step, seed, attempt = 2 * V * 2.0 ** -53 + 1e-15, 4, (9 << 32) | 77, 2
    keys, seeks = [11, 12, 13][:B], [0, 170, 98][:B]
    for T in (0.0, 0.2, 1.0):
        ids, fin, lens, count, slp, ns = pick_policy(x, mask, sp, timestamps, T, seed, attempt, keys, seeks, seqs, fins, step)
        want = [tail_expect(x[b], mask, sp, timestamps, T, seed, attempt, keys[b], seeks[b], seqs[b], fins[b], step) for b in range(B)]
        for b, (tok, gap, lp) in enumerate(want):
            print(f"V {V} rule {timestamps} T {T} row {b}: id {ids[b]} want {tok}, perturbed top-2 gap {gap:.3e}, logprob {slp[b]:.12f} want {lp}")
            assert gap > 1e-9, "the seeds were chosen so that no row is left out"
            assert ids[b] == tok
            if fins[b]:
                assert ns[b] == 0 and slp[b] == 0.0 and fin[b] == 1 and lens[b] == 0
            else:
                assert ns[b] == 1 and abs(slp[b] - lp) <= tol, (slp[b], lp, tol)
                assert fin[b] == int(tok == eos) and lens[b] == int(tok != eos)
        assert count == sum(int(not f and w[0] == eos) for f, w in zip(fins, want))
        if T == 0.0:
            assert ids == plain_pick(x, mask, sp, timestamps, seqs, fins, step)
        for b in range(B):                                        # the row alone, under its own key and seek
            a = pick_policy(x[b:b + 1], mask, sp, timestamps, T, seed, attempt, keys[b:b + 1], seeks[b:b + 1], seqs[b:b + 1], fins[b:b + 1], step)
            assert a[0] == [ids[b]] and a[4][0] == slp[b] and a[5] == [ns[b]]
        # everything but id 7 masked: the id is 7 at every temperature and its log-probability is 0
        seq = [tb + 2, 5] if timestamps else [5, 6]
        ids1, _, _, _, slp1, ns1 = pick_policy(x[:1], lonely, sp, timestamps, T, seed, attempt, keys[:1], seeks[:1], [seq], [0], step)
        assert ids1 == [7] and ns1 == [1] and abs(slp1[0]) <= tol
        if T == 0.0:
            assert plain_pick(x[:1], lonely, sp, timestamps, [seq], [0], step) == [7]


# ---------------------------------------------------------------------------------------------------- the loops
# The fixtures, chosen on the CPU from the restatement's own statistics (each test prints them).  Short form: whisper_ref.make_features
# seeds, B = 3, the timestamp ids suppressed.  Long form: B = 2 rows of whisper_ref.synth_wav, 2.5 and 1.3 windows.  Thresholds are
# (logprob, compression ratio, no-speech); `seeds` are policy seeds, each a run of its own.
# Measured on the CPU (the fp32 yardstick's bound is 1e-3 .. 3e-3): the short rows are accepted at T = 0 (avg -1.219 / -2.663),
# exhaust the temperatures (-1.409, -1.702, -2.041 / -2.813, -3.114, -4.981) and are skipped (avg -1.475, no-speech 8.1e-3 / -2.750,
# 1.15e-3); no step is low-margin.  TINY long, seed 5: first, first, accepted after the second retry | exhausted, first; seed 11: first,
# first, skipped on the second retry | accepted after one retry, first; no step is low-margin and every statistic lies >= 30 bounds
# from its threshold.  WIDE long: exhausted, exhausted, first | skipped, first, 11 low-margin steps of 330 left out.
SHORT = {"TINY": dict(features=(4, 8, 12), thresholds=(-1.31, 2.4, 8e-4), seeds=(5,)),
         "WIDE": dict(features=(2, 15, 10), thresholds=(-2.72, 2.4, 6e-4), seeds=(5,))}
LONG = {"TINY": dict(rows=((40000, 350), (20800, 340)), thresholds=(-1.45, 0.84, 1.6e-3), seeds=(5, 11)),
        "WIDE": dict(rows=((120000, 309), (62400, 340)), thresholds=(-2.45, 0.95, 2.6e-4), seeds=(5,))}


def make_policy(cfg, thresholds, seed):
    nots = L.layout(cfg)[2]
    return P.policy(temperatures=TEMPS, logprob_threshold=thresholds[0], compression_ratio_threshold=thresholds[1], no_speech_threshold=thresholds[2],
                    no_speech_token_id=nots - 1, seed=seed)


def short_spec(cfg):
    eos, special, nots, tb = L.layout(cfg)
    return R.spec(tuple(special) + (nots,), SUPPRESS + tuple(range(tb, cfg.vocab_size)), (), eos)


def branch(attempts):
    last = attempts[-1]
    return "skipped" if last.skip else "exhausted" if last.need else ("first", "retry", "second retry")[len(attempts) - 1]


def window_bound(cfg, sd, sp, wf, attempts):
    """The bound of a window's logits: the fp32 CPU evaluation of every attempt's positions (and of prompt position 0) against the
    float64 restatement, the largest over the attempts."""
    P0, bound = len(sp.prompt_ids), 0.0
    for a in attempts:
        seq = (list(sp.prompt_ids) + a.ids)[: cfg.max_target_positions]
        yard = R.torch_forward_fp32(cfg, sd, wf, seq)[1]
        ref = np.concatenate([a.first[None], a.raw[: len(yard) - (P0 - 1)]]) if P0 > 1 else a.raw[: len(yard)]
        yard = np.concatenate([yard[:1], yard[P0 - 1: P0 - 1 + len(a.raw)]]) if P0 > 1 else yard[: len(a.raw)]
        bound = max(bound, R.tolerance(yard, ref[: len(yard)])[0])
    return bound


def check_margins(what, po, attempts, nsp, bound):
    """Every statistic a threshold is compared with lies at least 16 x the bound from it: the average of log-softmax values moves by
    at most 2 x the logits' error, the no-speech probability by at most 2 x error x itself (<= 2 x error)."""
    for a in attempts:
        d = abs(a.avg_logprob - po.logprob_threshold)
        print(f"{what} T {a.temperature}: avg {a.avg_logprob:.4f} ({d / bound:.1f} bounds from the threshold), ratio {a.compression_ratio:.4f}, need {a.need} skip {a.skip}")
        assert d >= 16 * bound, (what, a.avg_logprob, po.logprob_threshold, bound)
    d = abs(nsp - po.no_speech_threshold)
    print(f"{what}: no-speech {nsp:.3e}, threshold {po.no_speech_threshold:.1e}: {d / (nsp * bound):.1f} bounds of its own error")
    assert d >= 16 * bound * nsp, (what, nsp, po.no_speech_threshold, bound)


def compared(what, a, bound):
    """The number of leading steps of an attempt whose decision 4 x the bound cannot turn."""
    scale = 4 * bound / (a.temperature if a.temperature > 0 else 1.0)
    margin = np.minimum(R.top2_margin(a.scores), np.where(np.isfinite(a.gaps), a.gaps, np.inf))
    low = np.nonzero(margin < scale)[0]
    n = len(margin) if len(low) == 0 else int(low[0]) + 1
    print(f"{what} T {a.temperature}: {len(margin)} steps, smallest margin {margin.min():.3e}, 4 x bound (/ T) {scale:.3e}, compared {n}")
    return n


def short_case(name, seed):
    key = ("short", name, seed)
    if key not in _CASE:
        cfg, fx = CFG[name], SHORT[name]
        po, sp = make_policy(cfg, fx["thresholds"], seed), short_spec(cfg)
        feats = np.stack([R.make_features(cfg, s) for s in fx["features"]])
        _CASE[key] = (po, sp, feats, [P.short_form(cfg, weights(name), feats[b], sp, po, row_key=40 + b) for b in range(len(feats))])
    return _CASE[key]


def long_case(name, seed):
    key = ("long", name, seed)
    if key not in _CASE:
        cfg, fx = CFG[name], LONG[name]
        po, sp = make_policy(cfg, fx["thresholds"], seed), L.spec(cfg, SUPPRESS)
        wavs = [R.synth_wav(n, s) for n, s in fx["rows"]]
        _CASE[key] = (po, sp, wavs, [P.long_form(cfg, weights(name), w, sp, po, row_key=70 + b) for b, w in enumerate(wavs)])
    return _CASE[key]


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_short_form_and_no_speech_probe(name):
    """B = 3 under a policy: the no-speech probability within twice the bound of the row's logits; every attempt's ids through the
    first low-margin step, at most 10 % of steps left out; where nothing was left out the statistics, the temperature the row ended on,
    the skip and the branch equal the restatement's; each row is the row alone bitwise; one encoder call whatever the attempts;
    ``policy=None`` is the existing path bitwise; beams with a policy raise."""
    cfg, m, sd = CFG[name], model(name), weights(name)
    for seed in SHORT[name]["seeds"]:
        po, sp, feats, ref = short_case(name, seed)
        lib_po, lib_sp = P.library_policy(po), L.library_spec(types_spec(sp))
        keys = [40 + b for b in range(len(feats))]
        calls = getattr(m, "encoder_calls", 0)
        ids, lens, info = m.generate(cuda(feats), lib_sp, policy=lib_po, row_keys=keys)
        assert m.encoder_calls - calls == 1
        ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
        total = left_out = 0
        branches = {}
        for b, (res, attempts) in enumerate(ref):
            bound = window_bound(cfg, sd, sp, feats[b], attempts)
            check_margins(f"short {name} row {b}", po, attempts, res.no_speech_prob, bound)
            err = abs(info["no_speech_prob"][b] - res.no_speech_prob)
            print(f"short {name} row {b}: no-speech device {info['no_speech_prob'][b]:.6e} restatement {res.no_speech_prob:.6e}, err {err:.3e}, 2 x bound {2 * bound:.3e}")
            assert err <= 2 * bound
            alone = m.generate(cuda(feats[b:b + 1]), lib_sp, policy=lib_po, row_keys=keys[b:b + 1])
            a_ids = alone[0].cpu().numpy()[0]
            assert int(alone[1][0]) == lens[b] and np.array_equal(a_ids[: lens[b]], ids[b, : lens[b]])
            for k in info:
                assert np.array_equal(alone[2][k], info[k][b:b + 1], equal_nan=True), (k, alone[2][k], info[k][b])
            exact = True
            for a in attempts:
                n = compared(f"short {name} row {b}", a, bound)
                total, left_out = total + len(a.ids), left_out + len(a.ids) - n
                exact = exact and n == len(a.ids)
            final = attempts[-1]
            n = compared(f"short {name} row {b} (final)", final, bound) if info["attempts"][b] == len(attempts) else 0
            tokens = res.tokens
            if exact:
                assert info["attempts"][b] == len(attempts) and info["temperature"][b] == res.temperature and bool(info["skipped"][b]) == res.skipped
                assert ids[b, : lens[b]].tolist() == tokens
                assert abs(info["avg_logprob"][b] - res.avg_logprob) <= 2 * bound and info["compression_ratio"][b] == res.compression_ratio
                branches[branch(attempts)] = branches.get(branch(attempts), 0) + 1
            elif not res.skipped and n:
                assert ids[b, : min(n, lens[b])].tolist() == tokens[: min(n, lens[b])]
        print(f"short {name} seed {seed}: branches {branches}, left out {left_out} of {total}")
        assert left_out * 10 <= total, (left_out, total)
        want = {}
        for res, attempts in ref:
            want[branch(attempts)] = want.get(branch(attempts), 0) + 1
        if left_out == 0:
            assert branches == want
    # policy=None: the existing entry points, bitwise, in the same process
    po, sp, feats, _ = short_case(name, SHORT[name]["seeds"][0])
    lib_sp = L.library_spec(types_spec(sp))
    a, b = m.generate(cuda(feats), lib_sp, policy=None), m.generate(cuda(feats), lib_sp)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and len(a) == 2
    # at T = 0 alone and no threshold the policy path emits the greedy ids
    only = P.library_policy(P.policy(temperatures=(0.0,)))
    c = m.generate(cuda(feats), lib_sp, policy=only)
    for r in range(len(feats)):
        n = int(b[1][r])
        assert int(c[1][r]) == n and torch.equal(c[0][r, :n], b[0][r, :n])
    assert np.isnan(c[2]["no_speech_prob"]).all() and (c[2]["temperature"] == 0.0).all()
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(cuda(feats), lib_sp, policy=P.library_policy(po), num_beams=2)
    with pytest.raises(ValueError, match="num_beams"):
        from dex_tts_amd import whisper
        whisper.whisper_score(cuda(R.synth_wav(8000, 1))[None], ["w1"], model=m, spec=lib_sp, vocab=[f"Ġw{i}" for i in range(cfg.vocab_size)],
                              policy=P.library_policy(po), num_beams=2)


def types_spec(sp):
    """whisper_ref's plain spec carries no timestamp fields: give it the two the library's dataclass has."""
    import types
    d = dict(vars(sp))
    d.setdefault("no_timestamps_token_id", None)
    d.setdefault("max_initial_timestamp_index", None)
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("name,seed", [("TINY", 5), ("TINY", 11), ("WIDE", 5)])
def test_long_form_under_a_policy(name, seed):
    """B = 2 rows of 2.5 and 1.3 windows: every window's attempts through the first low-margin step, at most 10 % of steps left out;
    where nothing was left out the seeks, the segments with their four numbers, the skipped windows and the branch counts equal the
    restatement's (TINY's two seeds reach all four branches between them); each row is the row alone; the encoder runs once per window
    group; ``policy=None`` is the existing path."""
    cfg, m, sd = CFG[name], model(name), weights(name)
    po, sp, wavs, ref = long_case(name, seed)
    lib_po, lib_sp = P.library_policy(po), L.library_spec(sp)
    keys = [70, 71]
    trace = []
    calls = getattr(m, "encoder_calls", 0)
    got = m.generate_segments([torch.from_numpy(w) for w in wavs], lib_sp, _trace=trace, policy=lib_po, row_keys=keys)
    assert m.encoder_calls - calls == len(trace) and all(t["encoder_calls"] == 1 for t in trace)
    seen = {0: [], 1: []}
    for t in trace:
        assert len({b for b, _, _ in t["windows"]}) == len(t["windows"])
        for b, seek, n in t["windows"]:
            atts = [(T, tok) for att in t["attempts"] for r, T, tok in att if r == b]
            seen[b].append((seek, n, atts, (b, seek, n) in t["skipped"]))
    total = left_out = 0
    branches, want = {}, {}
    for b, (segments, windows) in enumerate(ref):
        exact = True
        for k, (seek, n, wf, res, attempts) in enumerate(windows):
            want[branch(attempts)] = want.get(branch(attempts), 0) + 1
            if not exact:
                continue                                          # the later windows of this row start elsewhere: left out
            assert seen[b][k][:2] == (seek, n), (b, k, seen[b][k][:2], (seek, n))
            bound = window_bound(cfg, sd, sp, wf, attempts)
            check_margins(f"long {name} row {b} seek {seek}", po, attempts, res.no_speech_prob, bound)
            for j, a in enumerate(attempts):
                c = compared(f"long {name} row {b} seek {seek}", a, bound)
                total, left_out = total + len(a.ids), left_out + len(a.ids) - c
                tok = a.ids[:-1] if a.ids[-1] == sp.eos_token_id else a.ids
                if j < len(seen[b][k][2]):
                    T, dev = seen[b][k][2][j]
                    assert T == a.temperature and dev[: min(c, len(tok))] == tok[: min(c, len(tok))]
                exact = exact and c == len(a.ids) and j < len(seen[b][k][2]) and seen[b][k][2][j][1] == tok
                if not exact:
                    break
            if exact:
                assert len(seen[b][k][2]) == len(attempts) and seen[b][k][3] == res.skipped
                branches[branch(attempts)] = branches.get(branch(attempts), 0) + 1
        if exact:
            assert len(seen[b]) == len(windows) and len(got[b]) == len(segments)
            for g, s in zip(got[b], segments):
                assert (g["start"], g["end"], g["tokens"], g["temperature"], g["compression_ratio"]) == (s["start"], s["end"], s["tokens"], s["temperature"], s["compression_ratio"])
                assert abs(g["avg_logprob"] - s["avg_logprob"]) <= 2 * bound and abs(g["no_speech_prob"] - s["no_speech_prob"]) <= 2 * bound
        alone = m.generate_segments(cuda(wavs[b]), lib_sp, policy=lib_po, row_keys=keys[b:b + 1])
        assert alone == [got[b]]
    print(f"long {name} seed {seed}: branches {branches} (restatement {want}), left out {left_out} of {total}")
    assert left_out * 10 <= total, (left_out, total)
    if left_out == 0:
        assert branches == want
    if name == "TINY":                                            # what the two seeds were chosen for
        assert set(want) == ({"first", "second retry", "exhausted"} if seed == 5 else {"first", "skipped", "retry"}), want
    if seed == LONG[name]["seeds"][0]:
        plain = m.generate_segments([torch.from_numpy(w) for w in wavs], lib_sp)
        assert plain == m.generate_segments([torch.from_numpy(w) for w in wavs], lib_sp, policy=None)
        vocab = [f"Ġw{i}" for i in range(cfg.vocab_size)]
        from dex_tts_amd import whisper
        texts = m.transcribe_long([torch.from_numpy(w) for w in wavs], lib_sp, vocab, policy=lib_po)       # the default keys: the rows' indices
        own = m.generate_segments([torch.from_numpy(w) for w in wavs], lib_sp, policy=lib_po)
        assert texts == [whisper.decode([t for s in segs for t in s["tokens"]], vocab, sp.eos_token_id) for segs in own]
