"""CPU: the float64 restatement of the Whisper path (tests/whisper_ref.py) against ``transformers``' own
``WhisperForConditionalGeneration`` and ``WhisperFeatureExtractor`` in double precision, and the host halves of
dex_tts_amd/whisper.py (the mel matrix, the key inventory, the generation spec, byte-level decoding, the refused configs), which need
the built library and no device."""
import json

import numpy as np
import pytest
import torch

from tests import whisper_ref as R

transformers = pytest.importorskip("transformers")

CFG = {"TINY": R.TINY, "WIDE": R.WIDE}
PROMPT = (1, 5, 7)


def hf_model(cfg, sd):
    hc = transformers.WhisperConfig(**vars(cfg), pad_token_id=0, bos_token_id=1, eos_token_id=2, decoder_start_token_id=1,
                                    suppress_tokens=None, begin_suppress_tokens=None)
    m = transformers.WhisperForConditionalGeneration(hc)
    full = {k: torch.from_numpy(v) for k, v in sd.items()}
    full["proj_out.weight"] = full["model.decoder.embed_tokens.weight"]
    m.load_state_dict(full, strict=True)
    return m.double().eval()


_HF = {}


def hf(name):
    if name not in _HF:
        sd = R.make_weights(CFG[name], 0)
        _HF[name] = (sd, hf_model(CFG[name], sd))
    return _HF[name]


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_restatement_meets_transformers_in_double(name):
    cfg = CFG[name]
    sd, m = hf(name)
    feat = R.make_features(cfg, 1)
    ids = np.random.default_rng(5).integers(0, cfg.vocab_size, cfg.max_target_positions)
    enc, logits = R.forward(cfg, sd, feat, ids)
    with torch.no_grad():
        f = torch.from_numpy(feat).double()[None]
        henc = m.model.encoder(f).last_hidden_state[0].numpy()
        hlog = m(input_features=f, decoder_input_ids=torch.from_numpy(ids)[None]).logits[0].numpy()
    for what, a, b in (("encoder", enc, henc), ("logits", logits, hlog)):
        err, mag = np.abs(a - b).max(), np.abs(b).max()
        print(f"{name} {what}: err {err:.3e}, largest magnitude {mag:.3f}")
        assert a.shape == b.shape and err <= 1e-9 * mag


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_greedy_is_a_loop_over_transformers_forward(name):
    cfg = CFG[name]
    sd, m = hf(name)
    feat = R.make_features(cfg, 2)
    probe, _ = R.greedy(cfg, sd, feat, R.spec(PROMPT, eos=cfg.vocab_size - 1), 6)
    masks = dict(suppress=(probe[1], 3), begin_suppress=(probe[0],))                          # masks that bite
    open_end, _ = R.greedy(cfg, sd, feat, R.spec(PROMPT, eos=cfg.vocab_size - 1, **masks), 8)
    sp = R.spec(PROMPT, eos=open_end[5], **masks)                                             # an eos that ends it
    ids, rows = R.greedy(cfg, sd, feat, sp)
    f = torch.from_numpy(feat).double()[None]
    seq, want = list(PROMPT), []
    with torch.no_grad():
        for i in range(cfg.max_target_positions - len(PROMPT)):
            lg = m(input_features=f, decoder_input_ids=torch.tensor([seq])).logits[0, -1].numpy()
            tok = int(np.argmax(R.masked(lg, sp, i)))
            want.append(tok)
            seq.append(tok)
            if tok == sp.eos_token_id:
                break
    assert ids == want and ids[0] != probe[0] and probe[1] not in ids
    assert ids[-1] == sp.eos_token_id and len(ids) < cfg.max_target_positions - len(PROMPT)


@pytest.mark.parametrize("name,chunk", [("TINY", 1), ("WIDE", 3)])
def test_log_mel_meets_the_feature_extractor(name, chunk):
    cfg = CFG[name]
    assert R.n_samples(cfg) == chunk * 16000
    fe = transformers.WhisperFeatureExtractor(feature_size=cfg.num_mel_bins, sampling_rate=16000, hop_length=160, chunk_length=chunk, n_fft=400)
    for L in (1, 399, 400, R.n_samples(cfg)):
        wav = R.synth_wav(L, L)
        got = R.log_mel(cfg, wav)
        assert got.shape == (cfg.num_mel_bins, 2 * cfg.max_source_positions)
        # the extractor's double-precision path.  It keeps the spectrum as complex64 (2 x 6e-8 of a power: 1.3e-8 here), rounds log10
        # (|.| < 16: half an ulp is 4.8e-7, a quarter of it here) and the row's maximum (the same again) to float32, and computes
        # (x + 4) / 4 in float32 (half an ulp of |.| < 8 is 2.4e-7, a quarter of it here): 3.2e-7 in all
        padded = np.zeros((1, R.n_samples(cfg)), np.float32)
        padded[0, :L] = wav
        err = np.abs(got - fe._np_extract_fbank_features(padded, "cpu")[0].astype(np.float64)).max()
        print(f"{name} log_mel L={L}: err {err:.3e} against the extractor in double precision")
        assert err <= 3.2e-7
        # the extractor as it is called (float32 torch.stft where torch is installed): the float32 restatement is the yardstick
        want = fe(wav, sampling_rate=16000, return_tensors="np").input_features[0]
        tol, d = R.tolerance(R.log_mel(cfg, wav, np.float32), got)
        err = np.abs(got - want.astype(np.float64)).max()
        print(f"{name} log_mel L={L}: err {err:.3e} against the extractor as called, float32 yardstick {d:.3e}, bound {tol:.3e}")
        assert want.shape == got.shape and err <= tol


# ---------------------------------------------------------------------------------------------------- host halves of the library
def test_mel_filters():
    from dex_tts_amd import whisper
    for n in (80, 128):
        want = transformers.audio_utils.mel_filter_bank(201, n, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney")
        assert np.abs(whisper.mel_filters(n) - want).max() <= 1e-12
        assert np.abs(R.mel_filters(n) - want).max() <= 1e-12
    with pytest.raises(ValueError):
        whisper.mel_filters(129)


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_state_dict_shapes_are_transformers_own(name):
    import ctypes as C
    from dex_tts_amd import _lib, _wavnet, whisper
    lib, h = _lib.load(), C.c_void_p()
    c = whisper._c_config(R.library_config(CFG[name]))
    assert lib.dex_whisper_create(C.byref(c), C.byref(h)) == 0
    try:
        got = _wavnet.weight_shapes(lib, "dex_whisper", h)
    finally:
        lib.dex_whisper_destroy(h)
    want = {k: tuple(v.shape) for k, v in hf(name)[1].state_dict().items() if k != "proj_out.weight"}
    assert got == want and list(got) == list(want) == list(R.state_dict_shapes(CFG[name]))


GEN = {"decoder_start_token_id": 50258, "eos_token_id": 50257, "is_multilingual": True, "no_timestamps_token_id": 50364,
       "lang_to_id": {"<|en|>": 50259, "<|de|>": 50261}, "task_to_id": {"transcribe": 50360, "translate": 50359},
       "suppress_tokens": [1, 2, 7], "begin_suppress_tokens": [220, 50257]}


def test_generation_spec(tmp_path):
    from dex_tts_amd.whisper import GenerationSpec
    s = GenerationSpec.from_generation_config(GEN)
    assert s == GenerationSpec((50258, 50259, 50360, 50364), (1, 2, 7), (220, 50257), 50257)
    assert GenerationSpec.from_generation_config(GEN, "de", "translate").prompt_ids == (50258, 50261, 50359, 50364)
    en = dict(GEN, is_multilingual=False, decoder_start_token_id=50257, eos_token_id=[50256], no_timestamps_token_id=50362)
    del en["lang_to_id"], en["task_to_id"]
    s = GenerationSpec.from_generation_config(en)
    assert s.prompt_ids == (50257, 50362) and s.eos_token_id == 50256
    with pytest.raises(ValueError, match="xx"):
        GenerationSpec.from_generation_config(GEN, language="xx")
    with pytest.raises(ValueError, match="sing"):
        GenerationSpec.from_generation_config(GEN, task="sing")
    (tmp_path / "generation_config.json").write_text(json.dumps(GEN))
    assert GenerationSpec.from_generation_config(tmp_path) == GenerationSpec.from_generation_config(GEN)


def test_decode(tmp_path):
    from dex_tts_amd import whisper
    vocab = ["Ġcaf", "Ã", "©", "Ġ!", "<|endoftext|>", "<|notimestamps|>", "a"]
    assert whisper.decode([0, 1, 2, 3], vocab) == " café !"                      # G-dot -> space, e-acute split across two tokens
    assert whisper.decode([5, 0, 4, 4], vocab) == " caf"                              # special ids (>= eos) skipped
    assert whisper.decode([6], vocab) == "" and whisper.decode([6], vocab, eos_token_id=7) == "a"
    assert whisper.decode([2], vocab) == "�"                                     # a lone continuation byte
    assert whisper.decode([], vocab) == ""
    (tmp_path / "vocab.json").write_text(json.dumps({t: i for i, t in enumerate(vocab)}))
    assert whisper.load_vocab(tmp_path) == vocab


@pytest.mark.parametrize("field,value", [("scale_embedding", True), ("activation_function", "relu"), ("num_mel_bins", 160), ("d_model", 100),
                                         ("encoder_attention_heads", 4), ("decoder_attention_heads", 1), ("encoder_ffn_dim", 100),
                                         ("decoder_ffn_dim", 0), ("encoder_layers", 0), ("decoder_layers", 99), ("vocab_size", 1),
                                         ("max_source_positions", 5000), ("max_target_positions", 0)])
def test_refused_configs_name_their_field(field, value):
    import ctypes as C
    import dataclasses
    from dex_tts_amd import _lib, whisper
    lib, h = _lib.load(), C.c_void_p()
    c = whisper._c_config(dataclasses.replace(R.library_config(R.TINY), **{field: value}))
    assert lib.dex_whisper_create(C.byref(c), C.byref(h)) == _lib.DEX_ERR_ARG and not h.value
    assert lib.dex_whisper_last_error(None).decode().startswith(field + ":")
