"""CPU: the restatement tests/asr_ref.py (which the GPU tests hold the device to) against HF's own model, and the host half of
dex_tts_amd/asr.py (normalize_sentence, wer, cer, decode, frame counts).

tests/golden/asr_tiny.npz holds a ragged batch (``input_values`` [3, 4000] float32 with garbage past each length, ``lengths``) and
``logits`` [3, 12, 32]: the float64 logits of ``transformers.Wav2Vec2ForCTC(config).double()`` (transformers 5.15, eval mode, built
from the TINY config offline, weights ``asr_ref.make_weights(TINY, 0)``) on that batch - each row normalised over its own length and
zero past it, as ``Wav2Vec2FeatureExtractor`` pads, with the ``attention_mask`` of the lengths.  It was written by

    python -m tests.test_asr_cpu

and holds no weights: they come from the seed.  ``test_restatement_matches_fixture`` needs no transformers; where transformers is
installed ``test_restatement_matches_transformers`` rebuilds the model and checks restatement and fixture against it."""
import os

import numpy as np
import pytest

from tests import asr_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "asr_tiny.npz")
LENGTHS = [4000, 400, 3000]


def ragged_batch():
    n = max(LENGTHS)
    rng = np.random.default_rng(5)
    x = (10.0 * rng.standard_normal((len(LENGTHS), n))).astype(np.float32)          # garbage past each length
    for b, L in enumerate(LENGTHS):
        x[b, :L] = R.synth_wav(L, 11 + b)
    return x


def hf_logits(cfg, sd, x, lengths):
    """transformers' Wav2Vec2ForCTC in double precision on the padded batch with its attention mask -> float64 [B, T, V]."""
    import torch
    import transformers
    hc = transformers.Wav2Vec2Config(
        vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size, hidden_act="gelu",
        layer_norm_eps=cfg.layer_norm_eps, feat_extract_norm="layer", feat_extract_activation="gelu", conv_dim=list(cfg.conv_dim),
        conv_stride=list(cfg.conv_stride), conv_kernel=list(cfg.conv_kernel), conv_bias=True,
        num_conv_pos_embeddings=cfg.num_conv_pos_embeddings, num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups,
        do_stable_layer_norm=True, apply_spec_augment=False, pad_token_id=0)
    model = transformers.Wav2Vec2ForCTC(hc).double().eval()
    own = model.state_dict()
    new = {}
    for k, v in sd.items():
        for a, b in (("weight_g", "parametrizations.weight.original0"), ("weight_v", "parametrizations.weight.original1")):
            if k.endswith(a) and k not in own:
                k = k[: -len(a)] + b
        new[k] = torch.from_numpy(np.asarray(v, np.float64))
    missing, unexpected = model.load_state_dict(new, strict=False)
    assert not unexpected and all(m == "wav2vec2.masked_spec_embed" for m in missing), (missing, unexpected)
    B, n = x.shape
    inp, mask = np.zeros((B, n), np.float64), np.zeros((B, n), np.int64)
    for b, L in enumerate(lengths):
        inp[b, :L] = R.normalize_input(x[b, :L])
        mask[b, :L] = 1
    with torch.no_grad():
        return model(torch.from_numpy(inp), attention_mask=torch.from_numpy(mask)).logits.numpy()


def restatement(x, lengths):
    sd = R.make_weights(R.TINY, 0)
    return [R.forward(R.TINY, sd, x[b, :L]) for b, L in enumerate(lengths)]


@pytest.fixture(scope="module")
def rows():
    return restatement(ragged_batch(), LENGTHS)


def test_restatement_matches_fixture(rows):
    g = np.load(GOLDEN)
    assert np.array_equal(g["input_values"], ragged_batch()) and g["lengths"].tolist() == LENGTHS
    for b, L in enumerate(LENGTHS):
        T = R.num_frames(R.TINY, L)
        assert rows[b].shape == (T, 32)
        err = float(np.abs(rows[b] - g["logits"][b, :T]).max())
        print(f"row {b} ({L} samples, {T} frames): |restatement - fixture| = {err:.2e}, |logit| max {np.abs(rows[b]).max():.2f}")
        assert err <= 1e-10


def test_restatement_matches_transformers(rows):
    pytest.importorskip("transformers")
    x = ragged_batch()
    hf = hf_logits(R.TINY, R.make_weights(R.TINY, 0), x, LENGTHS)
    g = np.load(GOLDEN)
    for b, L in enumerate(LENGTHS):
        T = R.num_frames(R.TINY, L)
        assert np.abs(rows[b] - hf[b, :T]).max() <= 1e-10
        assert np.abs(g["logits"][b, :T] - hf[b, :T]).max() <= 1e-10


def test_torch_fp32_yardstick_is_the_same_graph(rows):
    x = ragged_batch()
    sd = R.make_weights(R.TINY, 0)
    for b, L in enumerate(LENGTHS):
        yard = R.torch_forward_fp32(R.TINY, sd, x[b, :L])
        tol, d = R.tolerance(yard, rows[b])
        print(f"row {b}: fp32 yardstick {d:.2e} at |logit| {np.abs(rows[b]).max():.2f}")
        assert yard.shape == rows[b].shape and d < 1e-4


@pytest.mark.parametrize("n, frames", [(399, 0), (400, 1), (401, 1), (719, 1), (720, 2), (3000, 9), (4000, 12), (64000, 199)])
def test_frame_counts(n, frames):
    from dex_tts_amd import asr
    assert R.num_frames(R.DEFAULT, n) == frames
    assert asr.num_frames(n) == frames
    assert asr.num_frames(n, R.library_config(R.TINY)) == frames


def test_normalize_sentence():
    from dex_tts_amd import asr
    assert asr.normalize_sentence("Don't stop!") == "DONT STOP"
    assert asr.normalize_sentence("  a,\tb\nc\r\x0cd  ") == "A B C D"
    assert asr.normalize_sentence("“Quoted” — dash… (x)") == "QUOTED DASH X"
    assert asr.normalize_sentence("a\x0bb") == "A B"                        # jiwer replaces all of string.whitespace
    assert asr.normalize_sentence("...") == ""


def test_wer_cer():
    from dex_tts_amd import asr
    assert asr.wer("THE CAT SAT DOWN", "THE CAT SAT DOWN") == 0.0
    assert asr.wer("THE CAT SAT DOWN", "THE BAT SAT DOWN") == 0.25            # one substitution in four words
    assert asr.wer("THE CAT SAT DOWN", "THE CAT SAT") == 0.25                 # one deletion
    assert asr.wer("THE CAT SAT DOWN", "THE BIG CAT SAT DOWN") == 0.25        # one insertion
    assert asr.wer("A B", "X Y Z W") == 2.0                                   # above 1: two substitutions, two insertions
    assert asr.wer("THE CAT", "") == 1.0 and asr.cer("THE CAT", "") == 1.0    # an empty hypothesis
    assert asr.cer("ABCD", "ABXD") == 0.25
    assert asr.cer("AB CD", "ABCD") == 0.2                                    # the space counts: one deletion in five characters
    assert asr.cer("ABCD", "XABCD") == 0.25
    for f in (asr.wer, asr.cer):
        with pytest.raises(ValueError):
            f("", "ANYTHING")
    with pytest.raises(ValueError):
        asr.wer("   ", "X")
    assert R.levenshtein("KITTEN", "SITTING") == 3 == asr._levenshtein("KITTEN", "SITTING")


def test_score_transcripts_matches_restatement():
    from dex_tts_amd import asr
    texts = ["Don't stop!", "the cat sat down", "hello world"]
    preds = ["DONT STOP", "THE BAT SAT", "HELLO WORD"]
    got = asr.score_transcripts(texts, preds)
    ref = R.asr_score(texts, preds, asr.normalize_sentence)
    assert np.allclose(got, ref, rtol=0, atol=1e-15)
    assert got[0] > 0 and got[2] == pytest.approx((0 + 0.5 + 0.5) / 3)


def test_ctc_and_decode_restated():
    from dex_tts_amd import asr
    V = R.VOCAB
    e, t, bar = V.index("E"), V.index("T"), V.index("|")
    assert R.collapse([e, e, 0, e, t, t]) == [e, e, t]                        # a repeat across a blank survives
    assert R.collapse([0, 0, e, t, 0, 0]) == [e, t]                           # leading and trailing blanks
    assert R.collapse([0, 0, 0]) == [] and asr.decode([]) == "" == R.decode([])
    assert R.collapse([e, t, e, t]) == [e, t, e, t]
    ids = R.collapse([bar, t, t, e, 0, e, bar, bar, t, 0, bar])
    assert asr.decode(ids) == "TEE T" == R.decode(ids)                        # '|' -> space, stripped
    lg = np.zeros((3, 32))
    lg[0, [5, 7]] = 1.0                                                       # a tie: the first index wins
    lg[1, 0] = 1.0
    lg[2, 7] = 2.0
    assert R.ctc_greedy(lg) == [5, 7]
    assert asr.VOCAB == R.VOCAB and len(asr.VOCAB) == 32


def test_state_dict_inventory_is_in_the_restatement_s_order():
    """The library registers its keys in the order of the restatement's state dict: ``weight_info(i)``, ``state_dict_shapes()`` and
    the 'missing keys' texts follow that order.  Host only: a handle is created, nothing touches a device."""
    import ctypes as C
    from dex_tts_amd import _lib, _wavnet, asr
    lib = _lib.load()
    for cfg in (R.TINY, R.DEFAULT):
        h = C.c_void_p()
        assert lib.dex_asr_create(C.byref(asr._c_config(R.library_config(cfg))), C.byref(h)) == _lib.DEX_OK
        try:
            got = _wavnet.weight_shapes(lib, "dex_asr", h)
        finally:
            lib.dex_asr_destroy(h)
        assert list(got.items()) == list(R.state_dict_shapes(cfg).items())


def test_config_outside_the_family_names_the_field():
    from dex_tts_amd import asr
    with pytest.raises(NotImplementedError, match="hidden_act"):
        asr._c_config(asr.Wav2Vec2Config(hidden_act="relu"))


if __name__ == "__main__":
    x = ragged_batch()
    hf = hf_logits(R.TINY, R.make_weights(R.TINY, 0), x, LENGTHS)
    T = [R.num_frames(R.TINY, L) for L in LENGTHS]
    for b in range(len(LENGTHS)):
        hf[b, T[b]:] = 0.0                                                     # frames past a row's count carry no meaning
    np.savez_compressed(GOLDEN, input_values=x, lengths=np.asarray(LENGTHS, np.int32), logits=hf)
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes")
