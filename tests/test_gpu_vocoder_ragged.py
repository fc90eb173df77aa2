"""Ragged vocoder batches on the GPU (dex_vocode_ragged through ``Generator.forward(x, lengths)``): utterance b of a batch is vocoded
exactly as if it had been passed alone at lengths[b] frames, and its waveform is zero behind lengths[b] * hop.

Geometries: HiFi-GAN V1 (wide implicit GEMMs + the transposed convs' fold), BigVGAN base (wide anti-aliased activation), and the two
small configurations of tests/test_bigvgan_22khz.py that isolate the narrow kernels (snakebeta_242: narrow conv, the k = 8 / u = 4 narrow
transposed conv, narrow activation; hifigan_v2: narrow kernels behind a leaky_relu).  Cases: B = 3, T = 40, lengths [40, 23, 1] (stage
lengths such as 184, 368 and 1472 fall inside the kernels' 32-, 64- and 256-sample tiles) and B = 2, T = 37, lengths [5, 37] (the
full-length utterance is not the first one, T is odd).

The reference is the CPU oracle run on ``mel[b:b+1, :, :n]`` ALONE in fp32, at the bounds of the existing vocoder tests: 2e-5 for
HiFi-GAN V1 (tests/test_vocoder.py), 5e-5 for BigVGAN and the narrow geometries (tests/test_bigvgan_22khz.py).  The padded call misses
those bounds by four orders of magnitude in the last frames of every shorter utterance (``test_padded_call_is_not_the_alone_result``)."""
import functools

import numpy as np
import pytest
import torch

from dex_tts_amd import synth, vocoder as V
from tests.test_bigvgan_22khz import SMALL, gpu_gen, mel_input, oracle, small_weights
from tests.test_vocoder import VOC_LOWP, bvg_weights

pytestmark = pytest.mark.gpu

# name -> (config, fp32 bound against the oracle)
GEOM = {"hifigan_v1": (V.HIFIGAN_V1, 2e-5), "bigvgan_base": (V.BIGVGAN_BASE, 5e-5),
        "snakebeta_242": (SMALL["snakebeta_242"], 5e-5), "hifigan_v2": (SMALL["hifigan_v2"], 5e-5)}
CASES = [(3, 40, (40, 23, 1)), (2, 37, (5, 37))]
ALL = [(g, c) for g in GEOM for c in range(len(CASES))]


def hop_of(name):
    return int(np.prod(GEOM[name][0]["upsample_rates"]))


@functools.lru_cache(maxsize=None)
def weights_of(name):
    return bvg_weights() if name == "bigvgan_base" else small_weights(GEOM[name][0])


@functools.lru_cache(maxsize=None)
def gen_of(name):
    return gpu_gen(GEOM[name][0], weights_of(name))


@functools.lru_cache(maxsize=None)
def mel_of(ci):
    """The padded batch: the mel of the other vocoder tests, seeded by shape; frames past each length are 0, as the decoder leaves them."""
    B, T, lengths = CASES[ci]
    mel = mel_input("ragged_mel", B, T, 91)
    for b, n in enumerate(lengths):
        mel[b, :, n:] = 0.0
    mel.setflags(write=False)
    return mel


@functools.lru_cache(maxsize=None)
def alone_oracle(name, ci, b):
    """The reference semantics: the fp32 CPU oracle on utterance b alone at its own length.  Computed once, shared, read-only."""
    n = CASES[ci][2][b]
    ref = oracle(weights_of(name), GEOM[name][0], np.array(mel_of(ci)[b:b + 1, :, :n]))[0, 0]
    ref.setflags(write=False)
    return ref


def call(gen, mel, lengths=None):
    x = torch.from_numpy(np.array(mel)).cuda()                 # (a writable, contiguous copy)
    return (gen(x) if lengths is None else gen(x, lengths)).cpu().numpy()


@functools.lru_cache(maxsize=None)
def ragged_fp32(name, ci):
    gen = gen_of(name)
    gen.precision = "fp32"
    out = call(gen, mel_of(ci), list(CASES[ci][2]))
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name,ci", ALL)
def test_ragged_matches_each_utterance_vocoded_alone_by_the_oracle(name, ci):
    from tests import gpu_util as U
    B, T, lengths = CASES[ci]
    hop, bound = hop_of(name), GEOM[name][1]
    out = ragged_fp32(name, ci)
    assert out.shape == (B, 1, T * hop) and np.isfinite(out).all()
    errs = []
    for b, n in enumerate(lengths):
        e = np.abs(out[b, 0, :n * hop] - alone_oracle(name, ci, b))
        U.record(f"voc_ragged_{name}_T{T}_n{n}:fp32:call", max=e.max(), mean=e.mean())
        print(f"{name} T={T} n={n}: max|d| = {e.max():.3e}")
        errs.append(float(e.max()))
    assert max(errs) <= bound, errs


@pytest.mark.parametrize("name", list(GEOM))
def test_padded_call_is_not_the_alone_result(name):
    """The check above is not vacuous: on the same inputs the plain padded call differs from the alone oracle by more than 1e-2 in the
    valid part of the 23-frame utterance (measured on the CPU oracles: 0.16 - 0.40)."""
    hop = hop_of(name)
    gen = gen_of(name)
    gen.precision = "fp32"
    padded = call(gen, mel_of(0))
    d = np.abs(padded[1, 0, :23 * hop] - alone_oracle(name, 0, 1)).max()
    print(f"{name}: padded call against the alone oracle, max|d| = {d:.3e}")
    assert d > 1e-2, float(d)


@pytest.mark.parametrize("name,ci", ALL)
def test_ragged_is_bitwise_the_library_s_own_alone_call(name, ci):
    """fp32: fixed K order, ksplit = 1, no atomics - the batch's utterance and the B = 1 call at its length run the same operations."""
    hop = hop_of(name)
    out = ragged_fp32(name, ci)
    gen = gen_of(name)
    gen.precision = "fp32"
    for b, n in enumerate(CASES[ci][2]):
        alone = call(gen, mel_of(ci)[b:b + 1, :, :n])[0, 0]
        assert np.array_equal(out[b, 0, :n * hop], alone), (b, n, float(np.abs(out[b, 0, :n * hop] - alone).max()))


@pytest.mark.parametrize("name,ci", ALL)
def test_zero_tail_and_ignored_padding(name, ci):
    B, T, lengths = CASES[ci]
    hop = hop_of(name)
    out = ragged_fp32(name, ci)
    for b, n in enumerate(lengths):
        assert not out[b, 0, n * hop:].any(), (b, n)                # exactly zero, not tanh(bias)
        assert n == 0 or out[b, 0, :n * hop].any()
    gen = gen_of(name)
    gen.precision = "fp32"
    mel = mel_of(ci).copy()
    for b, n in enumerate(lengths):
        mel[b, :, n:] = np.nan                                      # whatever the caller left there is never read into the result
    got = call(gen, mel, list(lengths))
    assert np.isfinite(got).all() and np.array_equal(got, out)
    # a length of 0: silence, and the other utterances do not notice; lengths outside [0, T] are clamped
    zl = [0] + list(lengths[1:])
    got = call(gen, mel, zl)
    assert not got[0].any() and np.array_equal(got[1:], out[1:])
    got = call(gen, mel_of(ci), [-3] + [T + 9] * (B - 1))
    assert not got[0].any() and np.array_equal(got[1:], call(gen, mel_of(ci), [0] + [T] * (B - 1))[1:])


@pytest.mark.parametrize("name,ci", ALL)
def test_repeatable_and_neutral_at_full_length(name, ci):
    B, T, lengths = CASES[ci]
    gen = gen_of(name)
    gen.precision = "fp32"
    assert np.array_equal(call(gen, mel_of(ci), list(lengths)), ragged_fp32(name, ci))
    assert np.array_equal(call(gen, mel_of(ci), torch.tensor(lengths, dtype=torch.int64).cuda()), ragged_fp32(name, ci))     # a device tensor
    plain = call(gen, mel_of(ci))
    assert np.array_equal(call(gen, mel_of(ci), None), plain)
    assert np.array_equal(call(gen, mel_of(ci), [T] * B), plain)


# (max|d|, RMS of d) against the fp32 oracle alone: the bounds of the existing reduced-precision tests (tests/test_vocoder.py VOC_LOWP,
# test_bigvgan_reduced_precision_mode)
LOWP = [("hifigan_v1", "bf16", VOC_LOWP["bf16"]), ("hifigan_v1", "fp16", VOC_LOWP["fp16"]), ("bigvgan_base", "bf16", (1.4e-2, 3.2e-3))]


@pytest.mark.parametrize("name,prec,bounds", LOWP, ids=[f"{n}-{p}" for n, p, _ in LOWP])
def test_ragged_reduced_precision(name, prec, bounds):
    """bf16 / fp16 operands in the wide convolutions: each utterance of the first case against the fp32 oracle alone.  (Not bitwise
    against the B = 1 call: the reduced-precision GEMM chooses its tile form by problem size.)  The one-frame utterance is held to the
    max bound only - its RMS sits on 256 samples."""
    from tests import gpu_util as U
    B, T, lengths = CASES[0]
    hop = hop_of(name)
    gen = gen_of(name)
    gen.precision = prec
    try:
        out = call(gen, mel_of(0), list(lengths))
        again = call(gen, mel_of(0), list(lengths))
    finally:
        gen.precision = "fp32"
    assert np.isfinite(out).all() and np.array_equal(out, again)
    bad = []
    for b, n in enumerate(lengths):
        assert not out[b, 0, n * hop:].any()
        e = out[b, 0, :n * hop] - alone_oracle(name, 0, b)
        mx, rms = float(np.abs(e).max()), float(np.sqrt((e * e).mean()))
        U.record(f"voc_ragged_{name}_T{T}_n{n}:{prec}:call", max=mx, mean=rms)
        print(f"{name} {prec} n={n}: max|d| = {mx:.3e}  rms = {rms:.3e}")
        if mx > bounds[0] or (n > 1 and rms > bounds[1]):
            bad.append((n, mx, rms))
    assert not bad, bad
    assert not np.array_equal(out, ragged_fp32(name, 0))


def test_synthesize_tokens_exact_lengths():
    """tests/test_tts_module.py's tokens-to-waveform case with ``exact_lengths=True``: every returned waveform is the utterance's own mel
    vocoded alone; the default is the padded call cut afterwards, as before."""
    from dex_tts_amd import synthesize as SY, tts
    from tests.test_tts_module import full_state_dict, model_cfg
    m = tts.GeDEXTTS(model_cfg("gedex_lj"))
    m.load_state_dict(full_state_dict(m, "gedex_lj"))
    m = m.cuda().eval()
    voc = V.Generator()
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_vocoder_weights(V.param_shapes(V.HIFIGAN_V1)).items()})
    voc = voc.cuda().eval()
    tok, lengths = synth.make_text_inputs(2, 21, [21, 12], 149)
    args = (m, voc, torch.from_numpy(tok).cuda(), torch.from_numpy(lengths).cuda())

    def pcm(wav):
        return (wav.clamp(-1, 1).cpu().numpy() * SY.MAX_VALUE).astype(np.int16)

    SY.seed_init(100)
    audio, y_dec, _ = SY.synthesize_tokens(*args, n_timesteps=4, exact_lengths=True)
    y_len = [int(n) for n in m.encoder._last["y_len"].cpu()]
    assert len(set(y_len)) == 2 and max(y_len) == y_dec.shape[-1]                   # a ragged batch
    assert [len(a) for a in audio] == [n * 256 for n in y_len]
    for b, n in enumerate(y_len):
        assert np.array_equal(audio[b], pcm(voc(y_dec[b:b + 1, :, :n])[0, 0])), b
    SY.seed_init(100)
    plain, y_dec2, _ = SY.synthesize_tokens(*args, n_timesteps=4)
    assert torch.equal(y_dec, y_dec2)
    padded = pcm(voc(y_dec)[:, 0])
    short = int(np.argmin(y_len))
    for b, n in enumerate(y_len):
        assert np.array_equal(plain[b], padded[b, :n * 256]), b
    assert not np.array_equal(plain[short], audio[short])                           # the padding reaches the shorter utterance's tail
