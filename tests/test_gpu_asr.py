"""GPU: the ASR path of dex_tts_amd/asr.py (csrc/asr.hip) against its float64 restatement (tests/asr_ref.py, itself held to
transformers' model by tests/test_asr_cpu.py).  Tolerances are not constants: each case measures, on its own inputs, how far the
torch fp32 CPU evaluation of the same graph lies from the float64 restatement, and allows the device ``NET_FACTOR`` = 8 times that
distance, floored at 1e-6 of the largest |logit| (asr_ref.tolerance).  Every case prints the device error, the yardstick and the
bound."""
import numpy as np
import pytest
import torch

from tests import asr_ref as R

pytestmark = pytest.mark.gpu

CFG = {"TINY": R.TINY, "WIDE": R.WIDE}
RAGGED = [4000, 400, 3000]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SD, _MODEL, _CASE = {}, {}, {}


def weights(name):
    if name not in _SD:
        _SD[name] = R.make_weights(CFG[name], 0)
    return _SD[name]


def model(name):
    if name not in _MODEL:
        from dex_tts_amd import asr
        m = asr.Wav2Vec2CTC(R.library_config(CFG[name]), "cuda")
        _MODEL[name] = m.load_state_dict({k: torch.from_numpy(v) for k, v in weights(name).items()})
    return _MODEL[name]


def case(name, n, seed):
    """(wav, float64 logits, fp32 CPU yardstick logits) of one utterance: computed once and shared, never changed."""
    key = (name, n, seed)
    if key not in _CASE:
        wav = R.synth_wav(n, seed)
        _CASE[key] = (wav, R.forward(CFG[name], weights(name), wav), R.torch_forward_fp32(CFG[name], weights(name), wav))
    return _CASE[key]


def ragged(name):
    """The batch [4000, 400, 3000] with garbage past each length, and its rows' cases."""
    cases = [case(name, L, 20 + b) for b, L in enumerate(RAGGED)]
    x = (10.0 * np.random.default_rng(3).standard_normal((len(RAGGED), max(RAGGED)))).astype(np.float32)
    for b, L in enumerate(RAGGED):
        x[b, :L] = cases[b][0]
    return x, cases


def check_logits(what, got, ref, yard):
    tol, d = R.tolerance(yard, ref)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: device err {err:.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}, |logit| max {np.abs(ref).max():.2f}")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert err <= tol, (what, err, tol)
    return tol


@pytest.mark.parametrize("n", [400, 401, 720, 4000])
def test_forward_tiny(n):
    """400 samples are ONE frame: attention over one key, a positional convolution that sees nothing but its padding."""
    wav, ref, yard = case("TINY", n, n)
    got = model("TINY").forward(cuda(wav)).cpu().numpy()
    assert got.shape == (R.num_frames(R.TINY, n), 32)
    check_logits(f"forward TINY n={n}", got, ref, yard)


def test_normalize_input():
    from dex_tts_amd import asr
    x, cases = ragged("TINY")
    got = asr.normalize_input(cuda(x), RAGGED).cpu().numpy()
    for b, L in enumerate(RAGGED):
        ref = R.normalize_input(x[b, :L])
        yard = R.normalize_input(x[b, :L], np.float32)
        tol = max(R.NET_FACTOR * float(np.abs(yard - ref).max()), R.NET_FLOOR * float(np.abs(ref).max()))
        err = float(np.abs(got[b, :L] - ref).max())
        print(f"normalize_input row {b}: device err {err:.3e}, bound {tol:.3e}")
        assert err <= tol and not got[b, L:].any()


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_ragged_batch_rows_are_the_rows_alone(name):
    """[4000, 400, 3000] with garbage past each length: a row's logits are BITWISE the row alone (every launch fixes its k-split and
    summation order from the config; the two tile forms of launch_igemm walk K identically), its transcript ids are equal, frames
    past its count are 0, and every row meets the restatement.  WIDE runs the C = 512 / 1024 / 4096, 16-group, 16-head shapes."""
    m = model(name)
    x, cases = ragged(name)
    got = m.forward(cuda(x), RAGGED).cpu().numpy()
    ids = m.transcribe_ids(cuda(x), RAGGED)
    assert got.shape == (3, 12, 32)
    for b, L in enumerate(RAGGED):
        T = R.num_frames(CFG[name], L)
        wav, ref, yard = cases[b]
        check_logits(f"ragged {name} row {b}", got[b, :T], ref, yard)
        assert not got[b, T:].any()
        alone = m.forward(cuda(wav)).cpu().numpy()
        assert np.array_equal(alone, got[b, :T]), f"row {b} differs from the row alone by {np.abs(alone - got[b, :T]).max():.3e}"
        assert m.transcribe_ids(cuda(wav)) == [ids[b]]
        assert ids[b] == R.collapse(np.argmax(got[b, :T], axis=-1))


def test_wide_batch_of_16_takes_the_other_gemm_tile():
    """launch_igemm picks its 128 x 64 tile once a launch has 512 of them: at 16 utterances of 4000 samples the first strided
    convolution (399 frames, N = 512: 4 x 8 x 16 tiles) does, where every smaller case here runs the 64 x 64 form.  Both walk K in
    the same order: the rows stay bitwise the rows alone."""
    m = model("WIDE")
    x3, cases = ragged("WIDE")
    x = np.concatenate([x3] * 6)[:16]
    lens = (RAGGED * 6)[:16]
    got = m.forward(cuda(x), lens).cpu().numpy()
    for b in (0, 1, 2, 15):
        wav, ref, yard = cases[b % 3]
        T = ref.shape[0]
        check_logits(f"WIDE B=16 row {b}", got[b, :T], ref, yard)
        assert np.array_equal(m.forward(cuda(wav)).cpu().numpy(), got[b, :T])


def test_forward_wide_single():
    wav, ref, yard = case("WIDE", 4000, 20)
    got = model("WIDE").forward(cuda(wav)[None]).cpu().numpy()
    assert got.shape == (1, 12, 32)
    check_logits("forward WIDE B=1", got[0], ref, yard)


def crafted_logits():
    """Rows for the CTC kernel: ties, all-blank, every frame a new symbol (count = T), repeats across blanks, T past one 256-frame
    round of the kernel's scan."""
    T, V = 300, 32
    rng = np.random.default_rng(9)
    lg = rng.standard_normal((6, T, V)).astype(np.float32)
    lg[1] = 0.0                                                   # every frame a 32-way tie: index 0 wins, all blank
    lg[2, :, 0] = 50.0                                            # all blank by a wide margin
    lg[3] = -1.0
    lg[3, np.arange(T), 1 + np.arange(T) % 31] = 5.0              # a new symbol on every frame: count = T
    lg[4] = 0.0
    lg[4, :, 7] = 1.0
    lg[4, :, 9] = 1.0                                             # a two-way tie between 7 and 9 on every frame: one 7
    lg[4, 100:200, 0] = 2.0                                       # ... a blank stretch, and the 7 comes again
    lg[5, ::2, 0] = 60.0                                          # blanks between random symbols: repeats across a blank survive
    frames = [T, T, T, T, T, 257]
    return lg, frames


def test_ctc_kernel_is_exact():
    from dex_tts_amd import asr
    lg, frames = crafted_logits()
    got = asr.ctc_greedy(cuda(lg), frames)
    for b, F in enumerate(frames):
        assert got[b] == R.ctc_greedy(lg[b, :F]), b
    assert got[1] == [] and got[2] == [] and len(got[3]) == 300 and got[4] == [7, 7]
    one = asr.ctc_greedy(cuda(lg[3, :1]))                         # T = 1
    assert one == [1]
    assert asr.ctc_greedy(cuda(lg[:1]), [0]) == [[]]              # no frames at all


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_transcribe_end_to_end(name):
    """transcribe against the restatement.  Per frame, the device's id equals the restatement's wherever the float64 top-2 margin
    exceeds 4 x the logits' tolerance; frames below it are left out, and at most 10 % may be.  Measured on the CPU with the fp32
    yardstick in the device's place (seed 0, lm_head 6 x): the tolerance is 9.4e-5 to 1.24e-4 at |logit| 9 - 19, the smallest margin
    among these frames is 0.26 (TINY) / 0.044 (WIDE): 0 of 22 frames are left out in either config (0 %).  The transcript is the CTC
    collapse of the device's own per-frame ids, and with no frame left out it is the restatement's string."""
    m = model(name)
    x, cases = ragged(name)
    logits = m.forward(cuda(x), RAGGED).cpu().numpy()
    texts = m.transcribe(cuda(x), RAGGED)
    left_out = total = 0
    for b, L in enumerate(RAGGED):
        wav, ref, yard = cases[b]
        T = ref.shape[0]
        tol, _ = R.tolerance(yard, ref)
        sure = R.top2_margin(ref) > 4 * tol
        left_out += int((~sure).sum())
        total += T
        dev_arg, ref_arg = np.argmax(logits[b, :T], axis=-1), np.argmax(ref, axis=-1)
        assert np.array_equal(dev_arg[sure], ref_arg[sure]), (b, dev_arg, ref_arg)
        assert texts[b] == R.decode(R.collapse(dev_arg))
        if sure.all():
            assert texts[b] == R.decode(R.ctc_greedy(ref))
        print(f"transcribe {name} row {b}: {T} frames, min margin {R.top2_margin(ref).min():.3e}, 4 x bound {4 * tol:.3e}, {texts[b]!r}")
    assert left_out <= 0.1 * total, (left_out, total)


def test_errors():
    from dex_tts_amd import asr
    m = model("TINY")
    with pytest.raises(ValueError, match="too short"):
        m.forward(torch.zeros(399, device="cuda"))
    with pytest.raises(ValueError, match="too short"):
        m.transcribe(torch.zeros(2, 4000, device="cuda"), [4000, 399])
    with pytest.raises(ValueError):
        m.forward(torch.zeros(4000))                              # a CPU tensor
    for bad in (dict(do_stable_layer_norm=False), dict(feat_extract_norm="group"), dict(num_attention_heads=4),
                dict(hidden_act="relu"), dict(num_conv_pos_embeddings=129)):
        field = next(iter(bad))
        with pytest.raises(NotImplementedError, match="hidden_size" if field == "num_attention_heads" else field):
            asr.Wav2Vec2CTC(R.library_config(R._cfg(**{**vars(R.TINY), **bad})), "cuda")
    sd = {k: torch.from_numpy(v) for k, v in weights("TINY").items()}
    fresh = asr.Wav2Vec2CTC(R.library_config(R.TINY), "cuda")
    with pytest.raises(ValueError, match="not loaded"):
        fresh.forward(torch.zeros(4000, device="cuda"))
    del sd["lm_head.bias"]
    with pytest.raises(RuntimeError, match="lm_head.bias"):
        fresh.load_state_dict(sd)
    fresh.load_state_dict(sd, strict=False)
    with pytest.raises(ValueError, match="lm_head.bias"):
        fresh.finalize()
    with pytest.raises(ValueError, match="not loaded"):
        fresh.forward(torch.zeros(4000, device="cuda"))
    bad_shape = dict(sd, **{"lm_head.bias": torch.zeros(31)})
    with pytest.raises(RuntimeError, match="shape"):
        fresh.load_state_dict(bad_shape)
    # HF's newer spelling of the weight norm, and the key the network never reads
    sd = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): torch.from_numpy(v)
          for k, v in weights("TINY").items()}
    sd["wav2vec2.masked_spec_embed"] = torch.zeros(128)
    fresh.load_state_dict(sd)
    wav, ref, yard = case("TINY", 4000, 4000)
    assert np.array_equal(fresh.forward(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy())


def test_asr_score():
    from dex_tts_amd import asr
    m = model("TINY")
    texts = ["Don't stop!", "the cat sat down", "hello world"]
    lens = [4000, 3000, 2000]
    cases = [case("TINY", L, 40 + b) for b, L in enumerate(lens)]
    for wav, ref, yard in cases:
        tol, _ = R.tolerance(yard, ref)
        assert R.top2_margin(ref).min() > 4 * tol                 # the restatement's transcript is beyond fp32 noise
    want = [R.decode(R.ctc_greedy(ref)) for _, ref, _ in cases]
    wavs = [c[0] for c in cases]
    got = m.transcribe(wavs)
    print("asr_score transcripts:", got)
    assert got == want
    score = asr.asr_score(texts, wavs, 16000, model=m)
    ref = R.asr_score(texts, want, asr.normalize_sentence)
    assert np.abs(np.asarray(score) - np.asarray(ref)).max() <= 1e-12
    from dex_tts_amd import synthesize
    audio = [np.round(w * 32768.0).astype(np.int16) for w in wavs]
    preds, *four = synthesize.asr_scores(m, audio, texts, sr=16000)
    assert len(preds) == 3 and len(four) == 4 and all(np.isfinite(four))
