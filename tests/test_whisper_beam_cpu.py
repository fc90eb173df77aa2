"""CPU: the float64 restatement of beam search (tests/whisper_beam_ref.py) against ``transformers``' own beam search, driven through
``GenerationMixin.generate`` on the double-precision model of tests/test_whisper_cpu.py, and the host-side refusals of the beam
surface of dex_tts_amd/whisper.py (they need no device).

``transformers`` accumulates the beam scores in fp32, so a case first asserts that the restatement's smallest decision gap is at
least 1e-4 - far above fp32 rounding of scores of magnitude 10 - and then asks for equal ids and scores within 1e-5.  The seeds
were picked on the CPU for that: the first seed from 19 on whose gap is >= 1e-3 (TINY K = 5 with an eos: 8.5e-4), that runs to the
cap (``cap``: the eos is never emitted) or ends by the early stop with an eos-terminated best hypothesis (``eos``: the eos is the
fourth id of the utterance's greedy path)."""
import numpy as np
import pytest
import torch

from tests import whisper_beam_ref as BR
from tests import whisper_ref as R

transformers = pytest.importorskip("transformers")

CFG = {"TINY": R.TINY, "WIDE": R.WIDE}
PROMPT = (1, 5, 7)
SUPPRESS = (0, 3)
BEGIN = {"TINY": (55, 69), "WIDE": (253, 351, 982)}
MAX_NEW = 12
# (config, K, length_penalty, kind, seed, eos)
CASES = [("TINY", 2, 1.0, "cap", 19, 91), ("TINY", 2, 1.0, "eos", 20, 94), ("TINY", 2, 0.6, "cap", 19, 91), ("TINY", 2, 0.6, "eos", 23, 94),
         ("TINY", 3, 1.0, "cap", 19, 91), ("TINY", 3, 1.0, "eos", 20, 94), ("TINY", 3, 0.6, "cap", 23, 91), ("TINY", 3, 0.6, "eos", 20, 94),
         ("TINY", 5, 1.0, "cap", 23, 91), ("TINY", 5, 1.0, "eos", 27, 94), ("TINY", 5, 0.6, "cap", 23, 91), ("TINY", 5, 0.6, "eos", 32, 94),
         ("WIDE", 2, 1.0, "cap", 20, 502), ("WIDE", 2, 1.0, "eos", 19, 288), ("WIDE", 2, 0.6, "cap", 20, 502), ("WIDE", 2, 0.6, "eos", 19, 288),
         ("WIDE", 3, 1.0, "cap", 21, 502), ("WIDE", 3, 1.0, "eos", 19, 288), ("WIDE", 3, 0.6, "cap", 21, 502), ("WIDE", 3, 0.6, "eos", 19, 288),
         ("WIDE", 5, 1.0, "cap", 28, 502), ("WIDE", 5, 1.0, "eos", 31, 978), ("WIDE", 5, 0.6, "cap", 25, 502), ("WIDE", 5, 0.6, "eos", 31, 978)]

_HF = {}


def hf(name):
    if name not in _HF:
        from tests.test_whisper_cpu import hf_model
        sd = R.make_weights(CFG[name], 0)
        _HF[name] = (sd, hf_model(CFG[name], sd))
    return _HF[name]


@pytest.mark.parametrize("name,K,lp,kind,seed,eos", CASES)
def test_restatement_is_transformers_beam_search(name, K, lp, kind, seed, eos):
    cfg = CFG[name]
    sd, m = hf(name)
    feat = R.make_features(cfg, seed)
    sp = R.spec(PROMPT, SUPPRESS, BEGIN[name], eos)
    hyp, pool, trace, gap = BR.beam_search(cfg, sd, feat, sp, K, MAX_NEW, lp)
    print(f"{name} K={K} lp={lp} {kind} seed {seed}: gap {gap:.3e}, {len(trace)} steps, pool lengths {[e['length'] for e in pool]}, score {hyp['score']:.6f}")
    assert gap >= 1e-4
    if kind == "cap":
        assert len(trace) == MAX_NEW and all(e["length"] == MAX_NEW and eos not in e["ids"] for e in pool)
    else:
        assert len(trace) < MAX_NEW and hyp["ids"][-1] == eos and hyp["length"] == len(hyp["ids"]) - 1      # the early stop fired
    procs = transformers.LogitsProcessorList([transformers.SuppressTokensLogitsProcessor(list(SUPPRESS), device="cpu"),
                                              transformers.SuppressTokensAtBeginLogitsProcessor(list(BEGIN[name]), len(PROMPT), device="cpu")])
    with torch.no_grad():
        out = transformers.GenerationMixin.generate(
            m, input_features=torch.from_numpy(feat).double()[None], decoder_input_ids=torch.tensor([PROMPT]), num_beams=K, do_sample=False,
            early_stopping=False, length_penalty=lp, max_new_tokens=MAX_NEW, logits_processor=procs, eos_token_id=eos, pad_token_id=0,
            num_return_sequences=1, return_dict_in_generate=True, output_scores=True)
    want = out.sequences[0].tolist()[len(PROMPT):]
    assert want[: len(hyp["ids"])] == hyp["ids"] and all(t == 0 for t in want[len(hyp["ids"]):])              # pad_token_id 0 behind the eos
    assert abs(float(out.sequences_scores[0]) - hyp["score"]) <= 1e-5


def test_select_rules_on_small_rows():
    """The rules of one step on rows small enough to read: step 0 is beam 0's alone, ties go to the lowest flat index, an eos of rank
    >= K is dropped, the masks are applied after the softmax (no renormalisation), the last step pools the top K."""
    sp = R.spec((1,), (7,), (6,), 5)
    x = np.zeros((2, 8), np.float32)
    x[1, 2] = 50.0                                                             # beam 1 would win everything, were it not at -1e9
    st, info = BR.select(x, BR.new_state(2, 4), sp, 0, False, pos=0)
    assert info.tokens == [0, 1] and info.parents == [0, 0] and info.gap == 0.0        # ids 0 .. 4 tie exactly; 5 is eos, 6 and 7 masked
    assert len(st.pool) == 0 and np.allclose(st.run, -np.log(8.0)) and st.anc.tolist() == [[0, 0, 0, 0], [0, 1, 1, 1]]
    y = np.zeros((2, 8), np.float32)
    y[:, 5] = -0.5                                                             # eos ranks behind the five tied ids of beam 0: rank >= K
    st2, info2 = BR.select(y, st, sp, 1, False, pos=1)
    assert info2.tokens == [0, 1] and info2.parents == [0, 0] and st2.pool == [] and st2.seqs == [[0, 0], [0, 1]]
    st3, info3 = BR.select(y, st2, sp, 2, True, pos=2)
    assert st3.done and info3.tokens is None and [e["ids"] for e in st3.pool] == [[0, 0, 0], [0, 0, 1]] and [e["length"] for e in st3.pool] == [3, 3]
    lse = np.log(7.0 + np.exp(-0.5))                                           # the masked ids 6 and 7 stay in the normaliser
    assert np.isclose(st3.pool[0]["score"], (-np.log(8.0) - 2 * lse) / 3.0, rtol=1e-14)
    again, _ = BR.select(x, st3, sp, 3, False)
    assert again is st3                                                        # done is sticky


def test_host_side_refusals():
    """Every out-of-scope argument raises ``ValueError`` naming it, before any device is touched."""
    from dex_tts_amd import whisper
    cfg = R.library_config(R.TINY)
    sp = whisper.GenerationSpec(PROMPT, SUPPRESS, BEGIN["TINY"], 91)
    assert whisper.check_beam_args(cfg, sp, 3) == 3 and whisper.check_beam_args(cfg, sp, 8, 0.6) == 8
    for bad in (0, 1, 9, -2, 2.5, True):
        with pytest.raises(ValueError, match="num_beams"):
            whisper.check_beam_args(cfg, sp, bad)
    with pytest.raises(ValueError, match="timestamps"):
        whisper.check_beam_args(cfg, sp, 3, timestamps=True)
    with pytest.raises(ValueError, match="long_form"):
        whisper.check_beam_args(cfg, sp, 3, long_form=True)
    for bad in (True, "never"):
        with pytest.raises(ValueError, match="early_stopping"):
            whisper.check_beam_args(cfg, sp, 3, early_stopping=bad)
    with pytest.raises(ValueError, match="num_return_sequences"):
        whisper.check_beam_args(cfg, sp, 3, num_return_sequences=2)
    with pytest.raises(ValueError, match="length_penalty"):
        whisper.check_beam_args(cfg, sp, 3, float("nan"))
    few = whisper.GenerationSpec(PROMPT, tuple(range(0, 80)), tuple(range(80, 91)), 91)       # 5 ids left: K = 2 fits, K = 3 does not
    assert whisper.check_beam_args(cfg, few, 2) == 2
    with pytest.raises(ValueError, match="leave 5 ids"):
        whisper.check_beam_args(cfg, few, 3)
    with pytest.raises(ValueError, match="max_source_positions"):
        whisper.check_beam_args(whisper.WhisperConfig(max_source_positions=4000), sp, 4)
    with pytest.raises(ValueError, match="model=Whisper"):
        whisper.whisper_score([np.zeros(100, np.float32)], ["a"], num_beams=3)
    assert whisper.MIN_BEAMS == 2 and whisper.MAX_BEAMS == 8 and whisper.MAX_ROWS // whisper.MAX_BEAMS == 4
