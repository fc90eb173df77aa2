"""CPU: the restatement of the long form (tests/whisper_long_ref.py) against ``transformers``' own
``WhisperTimeStampLogitsProcessor``, ``WhisperGenerationMixin._retrieve_segment``, ``WhisperFeatureExtractor(truncation=False)`` and
``generate(return_timestamps=True)`` in double precision, and the host halves of the library's long form (the spec, the segment
cut), which need the built library and no device."""
import types

import numpy as np
import pytest
import torch

from tests import whisper_long_ref as L
from tests import whisper_ref as R

transformers = pytest.importorskip("transformers")

CFG = {"TINY": L.TINY, "WIDE": L.WIDE}


def processor(sp):
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    gc = types.SimpleNamespace(no_timestamps_token_id=sp.no_timestamps_token_id, eos_token_id=sp.eos_token_id, bos_token_id=None,
                               max_initial_timestamp_index=sp.max_initial_timestamp_index)
    return WhisperTimeStampLogitsProcessor(gc, begin_index=len(sp.prompt_ids))


def histories(cfg):
    """New-token histories that reach every branch of the rule, by name."""
    eos, _, _, tb = L.layout(cfg)
    return {"first step": [], "a single leading timestamp": [tb + 2], "text after a timestamp": [tb + 2, 5], "text after text": [tb, 5, 6],
            "a timestamp after text": [tb + 2, 5, tb + 7], "a pair": [tb + 2, 5, tb + 7, tb + 7],
            "text after a pair": [tb + 2, 5, tb + 7, tb + 9, 4], "a timestamp after a pair and text": [tb, 5, tb + 7, tb + 9, 4, tb + 20],
            "the last timestamp": [tb, 5, tb + cfg.max_source_positions], "eos": [tb + 1, 5, tb + 3, eos]}


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
@pytest.mark.parametrize("max_initial", [None, 0, 4])
def test_rule_equals_the_logits_processor(name, max_initial):
    """Random score rows (standard deviation 3: the timestamps' summed probability wins in some and loses in others) and crafted ones
    under every history: the same -inf set and the same surviving values as ``WhisperTimeStampLogitsProcessor`` on float64 scores."""
    cfg = CFG[name]
    sp = L.spec(cfg, max_initial=max_initial)
    proc, V, tb = processor(sp), cfg.vocab_size, sp.no_timestamps_token_id + 1
    rng = np.random.default_rng(7)
    forced = plain = 0
    for what, seq in histories(cfg).items():
        rows = [3.0 * rng.standard_normal(V) for _ in range(6)]
        crafted = np.full(V, -4.0)                 # no single timestamp beats the best text id, their sum does
        crafted[7], crafted[tb + 10: tb + 30] = 2.0, 0.0
        assert crafted[tb:].max() < crafted[:tb].max() < L.logsumexp(crafted[tb:])
        rows.append(crafted)
        rows.append(np.where(np.arange(V) < tb, 9.0, -9.0) + rng.standard_normal(V))       # text far ahead
        for x in rows:
            ids = torch.tensor([list(sp.prompt_ids) + seq])
            want = proc(ids, torch.from_numpy(x)[None].clone())[0].numpy()
            got = L.timestamp_rule(x, seq, sp)
            assert want.dtype == np.float64
            assert np.array_equal(np.isneginf(got), np.isneginf(want)), (what, max_initial)
            assert np.array_equal(got[~np.isneginf(got)], x[~np.isneginf(want)]) and np.array_equal(want[~np.isneginf(want)], x[~np.isneginf(want)])
            live = L.rule_ranges(x, seq, sp)
            if np.isfinite(live[:tb]).any() and np.isfinite(live[tb:]).any():
                forced, plain = forced + int(np.isneginf(got[:tb]).all()), plain + int(not np.isneginf(got[:tb]).all())
    assert forced >= 5 and plain >= 5, (forced, plain)
    # the crafted row at a step where both text and timestamps are open: the timestamp wins although id 7 has the largest logit
    got = L.timestamp_rule(crafted, [tb + 2, 5], sp)
    assert int(np.argmax(crafted)) == 7 and np.isneginf(got[:tb]).all() and int(np.argmax(got)) == tb + 10


def hf_segments(tokens, tb, seek, n, prompt=(1, 2, 3)):
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    segs, offset = WhisperGenerationMixin._retrieve_segment(
        seek_sequence=torch.tensor(tokens), seek_outputs=[None], time_offset=torch.tensor([seek * 0.02 / 2], dtype=torch.float64),
        timestamp_begin=tb, seek_num_frames=torch.tensor([n]), time_precision=0.02, time_precision_features=0.01, input_stride=2, prev_idx=0, idx=0,
        return_token_timestamps=False, decoder_input_ids=torch.tensor([list(prompt)]))
    return [dict(start=float(s["start"]), end=float(s["end"]), tokens=s["tokens"].tolist()) for s in segs], int(offset)


def test_segments_equal_retrieve_segment():
    """Crafted sequences: a pair in the middle followed by a tail, two pairs, a single timestamp ending (after a pair and alone), no
    timestamp, one lone non-initial timestamp, only the initial one, and a final partial window - starts, ends, tokens and offset
    of the restatement and of the library's host function equal ``_retrieve_segment``'s."""
    from dex_tts_amd import whisper
    tb = 45
    t = lambda i: tb + i                                                                   # noqa: E731
    cases = {"a pair in the middle and a tail": [t(0), 5, 6, t(20), t(20), 7, 8],
             "two pairs and a tail that ends in text": [t(1), 5, t(9), t(9), 6, t(30), t(31), 7],
             "a pair then a tail with a lone timestamp": [t(0), 5, t(9), t(12), 6, 7, t(40), 8],
             "a single timestamp ending after a pair": [t(0), 5, t(9), t(9), 6, 7, t(33)],
             "a single timestamp ending, no pair": [t(2), 5, 6, t(33)],
             "no timestamp": [5, 6, 7],
             "one lone non-initial timestamp": [t(0), 5, 6, t(17), 7],
             "only the initial timestamp": [t(0), 5, 6],
             "a pair at the very end": [t(0), 5, t(9), t(9)],
             "one timestamp": [t(3)]}
    for what, tokens in cases.items():
        for seek, n in ((0, 100), (98, 100), (196, 54), (242, 7), (300, 33)):             # full windows and final partial ones
            want = hf_segments(tokens, tb, seek, n)
            assert L.retrieve_segments(tokens, tb, seek, n) == want, (what, seek, n)
            assert whisper.retrieve_segments(tokens, tb, seek, n) == want, (what, seek, n)
    segs, adv = L.retrieve_segments(cases["a pair in the middle and a tail"], tb, 98, 100)
    assert adv == 40 and len(segs) == 1 and segs[0]["tokens"] == [t(0), 5, 6, t(20), t(20)] and segs[0]["end"] == 0.98 + 20 * 0.02


@pytest.mark.parametrize("name,chunk", [("TINY", 1), ("WIDE", 3)])
def test_long_log_mel_meets_the_feature_extractor(name, chunk):
    """Rows of chunk + 1 samples and of 2.37 chunks against ``WhisperFeatureExtractor`` without truncation: its double-precision path
    under the bound tests/test_whisper_cpu.py derives for it (3.2e-7), and as it is called under the float32 yardstick."""
    cfg = CFG[name]
    fe = transformers.WhisperFeatureExtractor(feature_size=cfg.num_mel_bins, sampling_rate=16000, hop_length=160, chunk_length=chunk, n_fft=400)
    N = R.n_samples(cfg)
    for n in (N + 1, int(2.37 * N)):
        wav = R.synth_wav(n, n)
        got, F = L.log_mel_long(cfg, wav)
        assert F == n // 160 and got.shape == (cfg.num_mel_bins, F)
        err = np.abs(got - fe._np_extract_fbank_features(wav[None], "cpu")[0].astype(np.float64)).max()
        print(f"{name} long log_mel n={n}: err {err:.3e} against the extractor in double precision")
        assert err <= 3.2e-7
        want = fe(wav, sampling_rate=16000, truncation=False, padding="longest", return_tensors="np").input_features[0]
        tol, d = R.tolerance(L.log_mel_long(cfg, wav, np.float32)[0], got)
        err = np.abs(got - want.astype(np.float64)).max()
        print(f"{name} long log_mel n={n}: err {err:.3e} against the extractor as called, float32 yardstick {d:.3e}, bound {tol:.3e}")
        assert want.shape == got.shape and err <= tol
    short, F = L.log_mel_long(cfg, R.synth_wav(N, 1))
    assert F == 2 * cfg.max_source_positions and np.array_equal(short, R.log_mel(cfg, R.synth_wav(N, 1)))


def test_window_loop_equals_transformers_generate():
    """``transformers``' own ``generate(return_timestamps=True)`` driven at the TINY geometry in double precision on one row of 2.5 s
    (three 1 s windows): its segments - starts, ends and tokens, which fix every window's ids and seek - equal the restatement's."""
    cfg = L.TINY
    sd = R.make_weights(cfg, 0)
    sp = L.spec(cfg, suppress=(0, 3))
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
    g.suppress_tokens, g.begin_suppress_tokens, g.eos_token_id, g.pad_token_id, g.decoder_start_token_id = [0, 3], None, eos, eos, special[0]
    g.max_length, g.max_initial_timestamp_index, g.prev_sot_token_id = cfg.max_target_positions, None, None
    wav = R.synth_wav(40000, 323)
    feat, F = L.log_mel_long(cfg, wav)
    feat = feat.astype(np.float32)
    with torch.no_grad():
        out = m.generate(input_features=torch.from_numpy(feat).double()[None], attention_mask=torch.ones(1, F, dtype=torch.long), return_timestamps=True,
                         return_segments=True, language="en", task="transcribe", temperature=0.0, condition_on_prev_tokens=False)
    want = [dict(start=float(s["start"]), end=float(s["end"]), tokens=s["tokens"].tolist()) for s in out["segments"][0]]
    got, windows = L.long_form(cfg, sd, wav, sp)
    assert len(windows) == 3 and [w[0] for w in windows] == [0, 72, 170]
    assert got == want


GEN = {"decoder_start_token_id": 50258, "eos_token_id": 50257, "is_multilingual": True, "no_timestamps_token_id": 50364,
       "lang_to_id": {"<|en|>": 50259, "<|de|>": 50261}, "task_to_id": {"transcribe": 50360, "translate": 50359},
       "suppress_tokens": [1, 2, 7], "begin_suppress_tokens": [220, 50257], "max_initial_timestamp_index": 50}


def test_generation_spec_with_timestamps():
    from dex_tts_amd.whisper import GenerationSpec
    s = GenerationSpec.from_generation_config(GEN, timestamps=True)
    assert s == GenerationSpec((50258, 50259, 50360), (1, 2, 7), (220, 50257), 50257, 50364, 50)
    assert s.timestamp_begin == 50365
    assert GenerationSpec.from_generation_config(GEN, "de", "translate", timestamps=True).prompt_ids == (50258, 50261, 50359)
    no_cap = {k: v for k, v in GEN.items() if k != "max_initial_timestamp_index"}
    assert GenerationSpec.from_generation_config(no_cap, timestamps=True).max_initial_timestamp_index is None
    # the default path is unchanged: the prompt ends in <|notimestamps|> and the new fields stay empty
    d = GenerationSpec.from_generation_config(GEN)
    assert d == GenerationSpec((50258, 50259, 50360, 50364), (1, 2, 7), (220, 50257), 50257)
    assert d.no_timestamps_token_id is None and d.max_initial_timestamp_index is None and d.timestamp_begin is None
    assert GenerationSpec((1,)) == GenerationSpec((1,), (), (), 50257, None, None)
    with pytest.raises(ValueError, match="no_timestamps_token_id"):
        GenerationSpec.from_generation_config({k: v for k, v in GEN.items() if k != "no_timestamps_token_id"} | {"no_timestamps_token_id": None},
                                              timestamps=True)
    with pytest.raises(ValueError, match="xx"):
        GenerationSpec.from_generation_config(GEN, language="xx", timestamps=True)
