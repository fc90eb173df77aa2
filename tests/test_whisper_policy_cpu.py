"""CPU: the restatement of fallback decoding (tests/whisper_policy_ref.py) against ``transformers``' own ``generate`` with
``temperature=(...)``, ``logprob_threshold``, ``compression_ratio_threshold`` and ``no_speech_threshold`` in double precision at the TINY
geometry, Philox4x32-10 against its known answers, the sampler against the softmax, and the host halves of the library's policy
(``DecodingPolicy``, the compression ratio, the decision), which need the built library and no device.

What is compared with HF, and how.  HF's control flow (``generate_with_fallback``, ``_need_fallback``) runs unchanged; its
``_need_fallback`` is wrapped to record what it saw and what it decided.  HF rounds the model's logits to fp32 before its processors
even on a double-precision model; the device's logits are fp32 too, and the restatement rounds its own the same way, so all three
work on fp32 rows.  HF then takes its ``log_softmax`` in fp32 (``.float()``), a stated departure of the library, so the average
log-prob HF itself computes is fp32-born: it is held to ``FP32_BORN`` = 1e-5 (an fp32 log-softmax over 96 ids of magnitude <= 16
carries a few 1e-6).  The same statistic recomputed in float64 from the tensors HF hands to ``_need_fallback`` (its processed scores,
its tokens) is held to 1e-9 at T = 0, as are the no-speech probability, the ratio and the decisions; at T > 0 those scores have been
divided by T in fp32, so they are fp32-born as well.  For T > 0 ``torch.multinomial`` is replaced by the restatement's Gumbel-max keyed
by (step, attempt, seek), so HF's flow runs on the library's noise."""
import types

import numpy as np
import pytest
import torch

from tests import whisper_long_ref as L
from tests import whisper_policy_ref as P
from tests import whisper_ref as R

FP32_BORN = 1e-5
SUPPRESS = (0, 3)
# The fixture: rows of whisper_ref.synth_wav (samples, seed) at TINY and one set of thresholds, chosen from the restatement's own
# measured statistics (printed by the tests) so that every branch occurs: see LOGPROB.
ROWS = ((40000, 350), (56000, 340))
TEMPS = (0.0, 0.4, 0.8)


def hf_model(cfg, sd, timestamps=True):
    transformers = pytest.importorskip("transformers")
    eos, special, nots, tb = L.layout(cfg)
    hc = transformers.WhisperConfig(**vars(cfg), pad_token_id=eos, bos_token_id=eos, eos_token_id=eos, decoder_start_token_id=special[0],
                                    suppress_tokens=None, begin_suppress_tokens=None)
    m = transformers.WhisperForConditionalGeneration(hc)
    full = {k: torch.from_numpy(v) for k, v in sd.items()}
    full["proj_out.weight"] = full["model.decoder.embed_tokens.weight"]
    m.load_state_dict(full, strict=True)
    m = m.double().eval()
    g = m.generation_config
    g.no_timestamps_token_id, g.is_multilingual, g.lang_to_id, g.task_to_id = nots, True, {"<|en|>": special[1]}, {"transcribe": special[2]}
    g.suppress_tokens, g.begin_suppress_tokens, g.eos_token_id, g.pad_token_id, g.decoder_start_token_id = list(SUPPRESS), None, eos, eos, special[0]
    g.max_length, g.max_initial_timestamp_index, g.prev_sot_token_id = cfg.max_target_positions, None, None
    return m


class Recorder:
    """Wraps ``_need_fallback`` and ``generate_with_fallback`` of one HF model and, for T > 0, ``torch.multinomial``."""

    def __init__(self, m, cfg, po, row_key=0):
        self.m, self.cfg, self.po, self.key = m, cfg, po, row_key
        self.calls, self.seek, self.attempt, self.step = [], 0, 0, 0
        self.first_logits = None

    def __enter__(self):
        m, rec = self.m, self
        self.orig_need, self.orig_gwf, self.orig_multinomial = m._need_fallback, m.generate_with_fallback, torch.multinomial

        def need(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature):
            out = rec.orig_need(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature)
            from transformers.generation.logits_process import WhisperNoSpeechDetection
            scores = torch.stack(seek_outputs[index]["scores"])
            assert index == 0
            scores = scores.double()                      # HF rounds the logits to fp32 before its processors; the restatement does the same
            tokens = seek_sequence.tolist()
            T = temperature if temperature > 0 else 1.0
            x = (scores[: len(tokens)] * T).numpy()
            lp64 = sum(P.log_prob(x[i], tokens[i]) for i in range(len(tokens))) / len(tokens)
            hf_avg = float(m._retrieve_avg_logprobs(seek_outputs[index]["scores"], seek_sequence, temperature))
            nsp = [p for p in logits_processor if isinstance(p, WhisperNoSpeechDetection)]
            hf_nsp = float(nsp[0].no_speech_prob[0]) if nsp else float("nan")
            rec.calls.append(types.SimpleNamespace(seek=rec.seek, attempt=rec.attempt, temperature=float(temperature), tokens=tokens, avg64=lp64, hf_avg=hf_avg,
                                                   ratio=float(m._retrieve_compression_ratio(seek_sequence, vocab_size)), hf_nsp=hf_nsp, need=out[0], skip=out[1]))
            rec.attempt, rec.step = rec.attempt + 1, 0
            return out

        def gwf(*a, **kw):
            seek = kw["seek"] if "seek" in kw else a[3]
            rec.seek, rec.attempt, rec.step = int(seek[0]), 0, 0
            return rec.orig_gwf(*a, **kw)

        def multinomial(probs, num_samples, **kw):
            assert probs.shape[0] == 1 and num_samples == 1
            with np.errstate(divide="ignore"):
                y = np.log(probs[0].double().numpy())
            y = np.where(np.isneginf(y), -np.inf, y + P.gumbel(np.arange(len(y)), rec.step, rec.attempt, rec.seek, rec.key, rec.po.seed))
            rec.step += 1
            return torch.tensor([[int(np.argmax(y))]])

        m._need_fallback, m.generate_with_fallback, torch.multinomial = need, gwf, multinomial
        return self

    def __exit__(self, *exc):
        del self.m._need_fallback, self.m.generate_with_fallback
        torch.multinomial = self.orig_multinomial


def hf_long(m, cfg, wav, po, row_key=0):
    feat, F = L.log_mel_long(cfg, wav)
    feat = feat.astype(np.float32)
    with Recorder(m, cfg, po, row_key) as rec, torch.no_grad():
        out = m.generate(input_features=torch.from_numpy(feat).double()[None], attention_mask=torch.ones(1, F, dtype=torch.long), return_timestamps=True,
                         return_segments=True, language="en", task="transcribe", temperature=tuple(po.temperatures), condition_on_prev_tokens=False,
                         logprob_threshold=po.logprob_threshold, compression_ratio_threshold=po.compression_ratio_threshold,
                         no_speech_threshold=po.no_speech_threshold, top_k=0)       # top_k = 0: sampling from the whole masked row
    segs = [dict(start=float(s["start"]), end=float(s["end"]), tokens=s["tokens"].tolist()) for s in out["segments"][0]]
    return segs, rec.calls


def branch(attempts, n_temps):
    """The branch a window took: 'first', 'retry' (accepted after one retry), 'exhausted' or 'skipped'."""
    last = attempts[-1]
    if last.skip:
        return "skipped"
    if last.need:
        assert len(attempts) == n_temps
        return "exhausted"
    return "first" if len(attempts) == 1 else "retry" if len(attempts) == 2 else f"accepted at attempt {len(attempts)}"


def compare_windows(windows, calls, po, timestamps=True):
    """The restatement's windows against what HF's ``_need_fallback`` saw, attempt by attempt -> the branch counts."""
    k, counts = 0, {}
    for seek, n, wf, res, attempts in windows:
        for a in attempts:
            c = calls[k]
            k += 1
            print(f"seek {seek} T {a.temperature}: avg {a.avg_logprob:.12f} hf64 {c.avg64:.12f} hf {c.hf_avg:.9f}  ratio {a.compression_ratio:.6f}  "
                  f"no-speech {res.no_speech_prob:.3e} hf {c.hf_nsp:.3e}  need {a.need} skip {a.skip}")
            assert (c.seek, c.temperature, c.tokens) == (seek, a.temperature, a.ids)
            # at T > 0 HF's scores went through an fp32 division by T (and come back through an fp32 product): fp32-born too
            assert abs(a.avg_logprob - c.avg64) <= (1e-9 if a.temperature == 0 else FP32_BORN) and abs(a.avg_logprob - c.hf_avg) <= FP32_BORN
            assert abs(a.compression_ratio - c.ratio) <= 1e-9
            if po.no_speech_threshold is not None:
                assert abs(res.no_speech_prob - c.hf_nsp) <= 1e-9        # HF's fp32 softmax of a probability of a few 1e-3: 1e-10 off
            assert (a.need, a.skip) == (c.need, c.skip)
        b = branch(attempts, len(po.temperatures))
        counts[b] = counts.get(b, 0) + 1
    assert k == len(calls)
    return counts


# ---------------------------------------------------------------------------------------------------- Philox, the sampler
def test_philox_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in cases:
        assert " ".join(f"{int(w):08x}" for w in P.philox(counter, key)) == want
    # arrays broadcast: the vector form is the scalar form per element
    many = P.philox((np.arange(5), 7, 9, 11), (3, 4))
    for i in range(5):
        assert [int(w[i]) for w in many] == [int(w) for w in P.philox((i, 7, 9, 11), (3, 4))]


def test_uniform_words_and_counter():
    """u of id v is word v & 3 of the block of counter (v >> 2, step, attempt + 16 seek, row key); it depends on nothing else."""
    u = P.uniform(np.arange(11), 5, 2, 7, 13, (9 << 32) | 4)
    for v in range(11):
        w = P.philox((v >> 2, 5, 2 + 16 * 7, 13), (4, 9))[v & 3]
        assert u[v] == (float(w) + 0.5) * 2.0 ** -32 and 0.0 < u[v] < 1.0
    assert np.array_equal(P.uniform([10, 3], 5, 2, 7, 13, (9 << 32) | 4), u[[10, 3]])
    for other in (P.uniform(np.arange(11), 6, 2, 7, 13, (9 << 32) | 4), P.uniform(np.arange(11), 5, 3, 7, 13, (9 << 32) | 4),
                  P.uniform(np.arange(11), 5, 2, 8, 13, (9 << 32) | 4), P.uniform(np.arange(11), 5, 2, 7, 14, (9 << 32) | 4),
                  P.uniform(np.arange(11), 5, 2, 7, 13, (9 << 32) | 5)):
        assert not np.array_equal(other, u)


def test_gumbel_max_samples_the_softmax():
    """A 7-id row over 20 000 counter values (the step word) at T = 1: every frequency within 5 standard errors of the softmax."""
    x = np.array([0.3, -1.2, 2.0, 0.0, -np.inf, 1.1, -0.4])
    p = np.exp(x - x.max())
    p /= p.sum()
    N = 20000
    steps = np.arange(N)
    g = np.stack([P.gumbel(np.full(N, v), steps, 1, 0, 0, 1234) for v in range(7)], axis=1)
    picks = np.argmax(np.where(np.isneginf(x), -np.inf, x / 1.0 + g), axis=1)
    freq = np.bincount(picks, minlength=7) / N
    se = np.sqrt(p * (1 - p) / N)
    print("softmax", p, "frequencies", freq, "standard errors off", np.abs(freq - p) / np.maximum(se, 1e-300))
    assert freq[4] == 0.0 and (np.abs(freq - p) <= 5 * se).all()
    # perturbed() is that expression, and T = 0 leaves the row alone
    assert np.array_equal(P.perturbed(x, 1.0, 17, 1, 0, 0, 1234), np.where(np.isneginf(x), -np.inf, x + g[17]))
    assert P.perturbed(x, 0.0, 17, 1, 0, 0, 1234) is not None and np.array_equal(P.perturbed(x, 0.0, 17, 1, 0, 0, 1234), x)


# ---------------------------------------------------------------------------------------------------- the policy object, host halves
GEN = {"decoder_start_token_id": 50258, "eos_token_id": 50257, "is_multilingual": True, "no_timestamps_token_id": 50364}


def test_decoding_policy_validation():
    from dex_tts_amd.whisper import DecodingPolicy
    d = DecodingPolicy()
    assert d.temperatures == (0.0, 0.2, 0.4, 0.6, 0.8, 1.0) and d.seed == 0
    assert d.compression_ratio_threshold is None and d.logprob_threshold is None and d.no_speech_threshold is None
    p = DecodingPolicy.from_generation_config(GEN, logprob_threshold=-1.0, no_speech_threshold=0.6, compression_ratio_threshold=1.35, seed=7)
    assert p.no_speech_token_id == 50363 and p.seed == 7 and p == DecodingPolicy((0.0, 0.2, 0.4, 0.6, 0.8, 1.0), 1.35, -1.0, 0.6, 50363, 7)
    assert DecodingPolicy(temperatures=[0, 0.5]).temperatures == (0.0, 0.5)
    for bad in ((0.2, 0.4), (0.0, 0.4, 0.4), (0.0, 0.6, 0.4), (), tuple(0.1 * i for i in range(9)), (0.0, float("nan")), 0.0):
        with pytest.raises(ValueError, match="temperatures"):
            DecodingPolicy(temperatures=bad)
    with pytest.raises(ValueError, match="no_speech_threshold requires logprob_threshold"):
        DecodingPolicy(no_speech_threshold=0.6, no_speech_token_id=5)
    with pytest.raises(ValueError, match="no_speech_token_id"):
        DecodingPolicy(no_speech_threshold=0.6, logprob_threshold=-1.0)
    with pytest.raises(ValueError, match="logprob_threshold"):
        DecodingPolicy(logprob_threshold=float("inf"))
    with pytest.raises(ValueError, match="seed"):
        DecodingPolicy(seed=-1)
    with pytest.raises(ValueError, match="seed"):
        DecodingPolicy(seed=1 << 64)
    with pytest.raises(ValueError, match="no_timestamps_token_id"):
        DecodingPolicy.from_generation_config({"eos_token_id": 1})


def test_compression_ratio_and_decision():
    """28 equal one-byte ids give 2.55, 28 distinct ids 0.78; two-byte ids above 2^8 ... 2^16 - the library's host functions and the
    restatement's equal HF's ``_retrieve_compression_ratio``; the decision equals ``_need_fallback``'s table."""
    from dex_tts_amd import whisper
    pytest.importorskip("transformers")
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as G
    for tokens, V in (([5] * 28, 96), (list(range(28)), 96), ([300, 7, 300, 7, 51865], 51866), ([9], 96), ([65535] * 40, 65536), ([1, 2, 3] * 9, 255)):
        want = G._retrieve_compression_ratio(torch.tensor(tokens), V)
        assert whisper.compression_ratio(tokens, V) == want == P.compression_ratio(tokens, V)
    assert round(whisper.compression_ratio([5] * 28, 96), 2) == 2.55 and round(whisper.compression_ratio(list(range(28)), 96), 2) == 0.78
    po = P.policy(compression_ratio_threshold=1.35, logprob_threshold=-1.0, no_speech_threshold=0.6, no_speech_token_id=5)
    lib = P.library_policy(po)
    table = {(1.0, -0.5, 0.9): (False, False), (1.4, -0.5, 0.9): (True, False), (1.0, -1.5, 0.1): (True, False), (1.0, -1.5, 0.9): (False, True),
             (1.4, -1.5, 0.9): (False, True), (1.35, -1.0, 0.6): (False, False)}
    for args, want in table.items():
        assert whisper.fallback_decision(lib, *args) == want == P.decision(po, *args)
    off = P.policy()
    assert whisper.fallback_decision(P.library_policy(off), 9.0, -9.0, 1.0) == (False, False) == P.decision(off, 9.0, -9.0, 1.0)


# ---------------------------------------------------------------------------------------------------- against transformers
# Thresholds from the measured statistics of ROWS (the tests print every one of them).  Under (0.0, 0.4, 0.8), seed 11: row 0 accepts
# its first two windows at T = 0 (avg -1.216, -1.123; ratio 0.829) and its third after one retry (ratio 1.0 at T = 0, then avg -1.034,
# ratio 0.853); row 1 skips its first window (avg -1.287, no-speech 2.8e-3), skips its second on the retry (ratio 0.906 at T = 0, then
# avg -1.567, no-speech 2.0e-3), accepts two (avg -1.208, -1.098) and exhausts the temperatures on the last (avg -1.494, -1.694, -1.983).
# The nearest statistic is 0.006 from its threshold, far above the 1e-9 the comparison is held to.
LOGPROB, RATIO, NO_SPEECH = -1.25, 0.9, 0.002


def fixture(name="TINY"):
    cfg = L.TINY
    return cfg, R.make_weights(cfg, 0), L.spec(cfg, suppress=SUPPRESS), L.layout(cfg)


def test_statistics_equal_transformers():
    """``temperature=(0.0,)`` with all three thresholds on the rows of ROWS: per window the average log-prob, the ratio, the no-speech
    probability and the decisions equal what HF's ``_need_fallback`` saw and returned; the segments equal HF's."""
    cfg, sd, sp, (eos, special, nots, tb) = fixture()
    m = hf_model(cfg, sd)
    po = P.policy(temperatures=(0.0,), logprob_threshold=LOGPROB, compression_ratio_threshold=RATIO, no_speech_threshold=NO_SPEECH, no_speech_token_id=nots - 1)
    total = {}
    for n, seed in ROWS:
        wav = R.synth_wav(n, seed)
        want, calls = hf_long(m, cfg, wav, po)
        got, windows = P.long_form(cfg, sd, wav, sp, po)
        for b, c in compare_windows(windows, calls, po).items():
            total[b] = total.get(b, 0) + c
        assert [{k: s[k] for k in ("start", "end", "tokens")} for s in got] == want
    print("branches", total)
    assert total.get("first", 0) >= 1 and total.get("skipped", 0) >= 1 and total.get("exhausted", 0) >= 1         # one temperature: a refused window is exhausted


def test_fallback_flow_equals_transformers():
    """``temperatures=(0.0, 0.4, 0.8)`` and all three thresholds: HF's own fallback flow on the library's noise.  Segments, every
    attempt's tokens and statistics, and the temperature each window ended on are equal, and the four branches all occur."""
    cfg, sd, sp, (eos, special, nots, tb) = fixture()
    m = hf_model(cfg, sd)
    po = P.policy(temperatures=TEMPS, logprob_threshold=LOGPROB, compression_ratio_threshold=RATIO, no_speech_threshold=NO_SPEECH, no_speech_token_id=nots - 1,
                  seed=11)
    total = {}
    for key, (n, seed) in enumerate(ROWS):
        wav = R.synth_wav(n, seed)
        want, calls = hf_long(m, cfg, wav, po, row_key=key)
        got, windows = P.long_form(cfg, sd, wav, sp, po, row_key=key)
        for b, c in compare_windows(windows, calls, po).items():
            total[b] = total.get(b, 0) + c
        assert [{k: s[k] for k in ("start", "end", "tokens")} for s in got] == want
        ended = [c.temperature for i, c in enumerate(calls) if i + 1 == len(calls) or calls[i + 1].attempt == 0]
        assert ended == [w[3].temperature for w in windows]
    print("branches", total)
    assert total == {"first": 4, "retry": 1, "skipped": 2, "exhausted": 1}, total


def test_short_form_equals_transformers():
    """The short form (no timestamps, one window of 1 s) against HF ``generate`` with the thresholds and the temperatures: the ids, the
    statistics and the decisions of every attempt."""
    cfg, sd, sp_ts, (eos, special, nots, tb) = fixture()
    # the timestamp ids are suppressed, as a real checkpoint's never win without the rule: HF cuts at any it finds, even here
    suppress = SUPPRESS + tuple(range(tb, cfg.vocab_size))
    sp = R.spec(tuple(special) + (nots,), suppress, (), eos)
    m = hf_model(cfg, sd)
    m.generation_config.suppress_tokens = list(suppress)
    outcomes = set()
    for seed, lp in ((4, -1.0), (17, -9.0), (27, -1.0)):
        po = P.policy(temperatures=TEMPS, logprob_threshold=lp, compression_ratio_threshold=2.4, no_speech_threshold=0.9, no_speech_token_id=nots - 1, seed=3)
        feat = R.make_features(cfg, seed)
        with Recorder(m, cfg, po, row_key=seed) as rec, torch.no_grad():
            out = m.generate(input_features=torch.from_numpy(feat).double()[None], return_timestamps=False, language="en", task="transcribe",
                             temperature=tuple(po.temperatures), logprob_threshold=po.logprob_threshold, compression_ratio_threshold=po.compression_ratio_threshold,
                             no_speech_threshold=po.no_speech_threshold, top_k=0)
        res, attempts = P.short_form(cfg, sd, feat, sp, po, row_key=seed)
        counts = compare_windows([(0, 2 * cfg.max_source_positions, feat, res, attempts)], rec.calls, po)
        outcomes |= set(counts)
        seq = out[0].tolist() if torch.is_tensor(out) else out["sequences"][0].tolist()
        new = seq[len(sp.prompt_ids):] if seq[: len(sp.prompt_ids)] == list(sp.prompt_ids) else seq
        new = [t for t in new if t != eos]
        assert new == res.tokens, (seed, new, res.tokens)
    print("short form outcomes", outcomes)
    assert {"first", "exhausted"} <= outcomes
