"""GPU: the speaker-similarity path of dex_tts_amd/speaker.py (csrc/speaker.hip) against its float64 restatement
(tests/speaker_ref.py).  Tolerances are not constants: each test measures, on its own inputs, how far a CPU fp32 evaluation
(torch.nn.LSTM + Linear for the network, numpy fp32 for the mel) lies from the float64 restatement, and allows the device
NET_FACTOR / MEL_FACTOR times that distance (floored; speaker_ref.py says where the factors come from)."""
import numpy as np
import pytest
import torch

from tests import speaker_ref as R
from tests import wav_prep as WP

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def sd():
    return R.make_weights(0)


@pytest.fixture(scope="module")
def enc(sd):
    from dex_tts_amd import speaker
    return speaker.VoiceEncoder("cuda").load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})


@pytest.fixture(scope="module")
def torch_net(sd):
    lstm = torch.nn.LSTM(R.N_MELS, R.H, R.LAYERS, batch_first=True)
    lin = torch.nn.Linear(R.H, R.H)
    lstm.load_state_dict({k[len("lstm."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("lstm.")})
    lin.load_state_dict({k[len("linear."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("linear.")})
    return lstm, lin


def torch_forward_fp32(net, mels):
    """resemblyzer's forward in fp32 on the CPU: the yardstick."""
    lstm, lin = net
    with torch.no_grad():
        _, (h, _) = lstm(torch.from_numpy(np.asarray(mels, np.float32)))
        raw = torch.relu(lin(h[-1]))
        return (raw / torch.norm(raw, dim=1, keepdim=True)).numpy()


def net_tolerance(yard, ref):
    d = float(np.abs(yard.astype(np.float64) - ref).max())
    return max(R.NET_FACTOR * d, R.NET_FLOOR), d


_FWD = {}


def forward_case(sd, net, P, T):
    """(mels, float64 reference, its raw norms, fp32 yardstick): computed once per shape and shared."""
    if (P, T) not in _FWD:
        mels = R.mel_like(P, T, 100 * P + T)
        _FWD[(P, T)] = (mels, R.forward(sd, mels), np.linalg.norm(R.forward_raw(sd, mels), axis=1), torch_forward_fp32(net, mels))
    return _FWD[(P, T)]


@pytest.mark.parametrize("T", [1, 7, 160])
@pytest.mark.parametrize("P", [1, 2, 17, 33])
def test_forward(enc, sd, torch_net, P, T):
    mels, ref, raw_norm, yard = forward_case(sd, torch_net, P, T)
    assert (raw_norm > R.MIN_RAW_NORM).all()
    tol, d = net_tolerance(yard, ref)
    got = enc.forward(cuda(mels)).cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"forward P={P} T={T}: device err {err:.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}")
    assert got.shape == (P, 256) and np.isfinite(got).all()
    assert err <= tol, (P, T, err, tol)
    # a row does not see its neighbours: the last row alone, bitwise
    alone = enc.forward(cuda(mels[-1:])).cpu().numpy()
    assert np.array_equal(alone[0], got[-1])


@pytest.mark.parametrize("n", [159, 160, 401, 14400])
def test_wav_to_mel_spectrogram(n):
    from dex_tts_amd import speaker
    wav = R.synth_wav(n, 7 + n)
    ref = R.wav_to_mel_spectrogram(wav)
    yard = R.wav_to_mel_spectrogram(wav, dtype=np.float32)
    scale = float(ref.max())
    d = float(np.abs(yard.astype(np.float64) - ref).max()) / scale
    tol = max(R.MEL_FACTOR * d, R.MEL_FLOOR)
    got = speaker.wav_to_mel_spectrogram(cuda(wav)).cpu().numpy()
    assert got.shape == (1 + n // 160, 40) and got.dtype == np.float32
    err = float(np.abs(got - ref).max()) / scale
    print(f"mel n={n}: device err {err:.3e} of the largest value, numpy fp32 yardstick {d:.3e}, bound {tol:.3e}")
    assert err <= tol, (n, err, tol)


def test_mel_ragged_rows_are_the_rows_alone():
    from dex_tts_amd import speaker
    ns = [401, 14400, 160]
    wavs = [R.synth_wav(n, 20 + i) for i, n in enumerate(ns)]
    batch = np.zeros((3, max(ns)), np.float32)
    for b, w in enumerate(wavs):
        batch[b, : len(w)] = w
        batch[b, len(w):] = 1.0                     # garbage past the length must not be read
    got = speaker.wav_to_mel_spectrogram(cuda(batch), ns).cpu().numpy()
    for b, w in enumerate(wavs):
        alone = speaker.wav_to_mel_spectrogram(cuda(w)).cpu().numpy()
        F = 1 + ns[b] // 160
        assert np.array_equal(got[b, :F], alone) and not got[b, F:].any()


LENGTHS = [14400, 40000, 44800]


@pytest.fixture(scope="module")
def ragged(sd, torch_net):
    """The three utterances of the slice test: wavs, float64 embeddings, fp32-yardstick embeddings, raw norms of every partial."""
    wavs = [R.synth_wav(n, 40 + i) for i, n in enumerate(LENGTHS)]
    ref, yard, raw = [], [], []
    for w in wavs:
        e, raw_partials = R.embed_utterance(sd, w, return_raw=True)
        ref.append(e)
        raw.append(np.linalg.norm(raw_partials, axis=1))
        p = torch_forward_fp32(torch_net, R.partial_mels(w).astype(np.float32))
        m = p.mean(axis=0)
        yard.append(m / np.linalg.norm(m))
    return wavs, np.stack(ref), np.stack(yard), np.concatenate(raw)


def test_embed_utterances_ragged(enc, ragged):
    wavs, ref, yard, raw = ragged
    assert len(raw) == 1 + 2 + 3 and (raw > R.MIN_RAW_NORM).all()
    tol, d = net_tolerance(yard, ref)
    batch = np.zeros((3, max(LENGTHS)), np.float32)
    for b, w in enumerate(wavs):
        batch[b, : len(w)] = w
        batch[b, len(w):] = 1.0                     # garbage past the length: the pad to the last slice must be zeros, not this
    got = enc.embed_utterances(cuda(batch), LENGTHS).cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"embed_utterances: device err {err:.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}")
    assert got.shape == (3, 256) and err <= tol, (err, tol)
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() <= 4 * EPS32
    for b, w in enumerate(wavs):
        alone = enc.embed_utterance(cuda(w)).cpu().numpy()
        assert np.array_equal(alone, got[b]), b     # bitwise: a row must not see its neighbours


def test_embed_utterance_partials(enc, sd, torch_net, ragged):
    wavs, _, _, _ = ragged
    e, partials, wav_slices = enc.embed_utterance(cuda(wavs[2]), return_partials=True)
    assert partials.shape == (3, 256) and [(s.start, s.stop) for s in wav_slices] == [(0, 25600), (12320, 37920), (24640, 50240)]
    mels = R.partial_mels(wavs[2])
    ref = R.forward(sd, mels)
    tol, d = net_tolerance(torch_forward_fp32(torch_net, mels.astype(np.float32)), ref)
    p = partials.double().cpu().numpy()
    err = float(np.abs(ref - p).max())
    print(f"partials: device err {err:.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}")
    assert err <= tol
    # the utterance embedding is the normalised mean of exactly these partials: two fp32 additions, a division, a 256-term tree of
    # squares (8 levels), a square root and a division - under 8 half-ulps of values below 1
    m = p.mean(axis=0)
    assert np.abs(m / np.linalg.norm(m) - e.double().cpu().numpy()).max() <= 4 * EPS32


def test_embed_speaker(enc, ragged):
    wavs, ref, yard, _ = ragged
    tol, _ = net_tolerance(yard, ref)
    got = enc.embed_speaker([cuda(w) for w in wavs]).double().cpu().numpy()
    m = ref.mean(axis=0)
    # every utterance embedding within tol, so the mean within tol; normalising x -> x / |x| moves by at most 2 |dx|_2 / |x|
    bound = 2 * 16 * tol / np.linalg.norm(m) + 4 * EPS32
    assert np.abs(got - m / np.linalg.norm(m)).max() <= bound


# 1.8 s and 1.6 s "at 22050 Hz": at 16 kHz each is one partial without zero padding (29024 and 26122 samples: the second slice would
# cover 0.65 / 0.54 and is dropped), so the final LSTM state sees signal to the last frame - the embeddings differ measurably
NA, NB = 40000, 36000


def test_speaker_similarity(enc, sd, torch_net):
    from dex_tts_amd import speaker
    a22, b22 = R.synth_wav(NA, 60), R.synth_wav(NB, 61)
    # a wav with itself: both rows are embedded bitwise alike, and the cosine of a vector with itself is 1 to fp32 rounding
    cos = speaker.speaker_similarity(cuda(a22), cuda(a22), encoder=enc)
    assert cos.shape == (1,) and abs(float(cos[0]) - 1.0) <= EPS32
    # two different wavs, a ragged pair batch, against the restatement
    pre = lambda w: R.normalize_volume(WP.resample(w.astype(np.float64), 22050, 16000).astype(np.float32))
    ref, yard = [], []
    for w in (a22, b22):
        x = pre(w)
        e, raw_partials = R.embed_utterance(sd, x, return_raw=True)
        assert (np.linalg.norm(raw_partials, axis=1) > R.MIN_RAW_NORM).all()
        ref.append(e)
        p = torch_forward_fp32(torch_net, R.partial_mels(x).astype(np.float32))
        yard.append(p.mean(axis=0) / np.linalg.norm(p.mean(axis=0)))
    tol, d = net_tolerance(np.stack(yard), np.stack(ref))
    want = R.cosine(ref[0], ref[1])
    syn = np.zeros((2, NA), np.float32); syn[0] = a22; syn[1, :NB] = b22
    trg = np.zeros((2, NA), np.float32); trg[0, :NB] = b22; trg[1] = a22
    cos = speaker.speaker_similarity(cuda(syn), cuda(trg), [NA, NB], [NB, NA], encoder=enc).double().cpu().numpy()
    # unit vectors: |d cos| <= |da|_2 + |db|_2 <= 2 sqrt(256) max|d|
    bound = 2 * 16 * tol + EPS32
    print(f"similarity: cos {cos}, restatement {want:.9f}, embedding yardstick {d:.3e}, bound {bound:.3e}")
    assert np.abs(cos - want).max() <= bound
    assert cos[0] == cos[1]                                   # the same pair in either order and batch position, bitwise
    assert np.abs(ref[0] - ref[1]).max() > 10 * tol          # (the two embeddings differ by far more than the bound: the comparison says something)
    mean, stderr = speaker.asv_score(cuda(syn), cuda(trg), [NA, NB], [NB, NA], encoder=enc)
    assert mean == pytest.approx(float(cos.mean()), abs=1e-12) and stderr == pytest.approx(0.0, abs=1e-12)


def test_score_synthesis_takes_int16_waveforms(enc):
    """synthesize_tokens' list of int16 waveforms scores exactly as the same waveforms passed as floats."""
    from dex_tts_amd import speaker, synthesize
    a, b = R.synth_wav(NA, 60), R.synth_wav(NB, 61)
    audio = [(a * 32768.0).astype(np.int16), (b * 32768.0).astype(np.int16)]
    cos, mean, stderr = synthesize.speaker_scores(enc, audio, [b, a])
    syn = np.zeros((2, NA), np.float32); syn[0] = audio[0] / 32768.0; syn[1, :NB] = audio[1] / 32768.0
    trg = np.zeros((2, NA), np.float32); trg[0, :NB] = b; trg[1] = a
    want = speaker.speaker_similarity(cuda(syn), cuda(trg), [NA, NB], [NB, NA], encoder=enc)
    assert cos.shape == (2,) and torch.equal(cos, want)
    c = want.double().cpu().numpy()
    assert mean == pytest.approx(float(c.mean()), abs=1e-12) and stderr == pytest.approx(float(c.std() / np.sqrt(2)), abs=1e-12)


def test_preprocess_wav_from_22050():
    from dex_tts_amd import speaker
    wavs = [R.synth_wav(26460, 70, amp=0.5), R.synth_wav(22050, 71, amp=0.002)]          # louder than -30 dBFS, and quieter
    batch = np.zeros((2, 26460), np.float32)
    for b, w in enumerate(wavs):
        batch[b, : len(w)] = w
    got, lengths = speaker.preprocess_wav(cuda(batch), 22050, [26460, 22050])
    got = got.cpu().numpy()
    for b, w in enumerate(wavs):
        res = WP.resample(w.astype(np.float64), 22050, 16000).astype(np.float32)
        ref = R.normalize_volume(res)
        assert (ref is res) == (b == 0)                       # the loud one is left alone, the quiet one raised
        assert int(lengths[b]) == len(ref) == len(w) * 16000 // 22050
        # the fp64 resamplers agree to 1e-12 (tests/test_gpu_wav_prep.py), so their fp32 roundings lie at most one ulp apart; the
        # gain, itself rounded to fp32 from a mean that moves with those ulps, and the product's rounding add one each
        assert np.abs(got[b, : len(ref)].astype(np.float64) - ref).max() <= 3 * EPS32 * np.abs(ref).max()
        assert not got[b, len(ref):].any()
    assert abs(10 * np.log10(np.mean(got[1, : lengths[1]].astype(np.float64) ** 2)) + 30.0) < 1e-4


def test_refused_arguments(enc, sd):
    from dex_tts_amd import speaker
    with pytest.raises(ValueError):
        enc.forward(torch.zeros(2, 160, 40))                                  # CPU tensor
    with pytest.raises(ValueError):
        enc.forward(torch.zeros(2, 160, 80, device="cuda"))                   # wrong mel width
    with pytest.raises(ValueError):
        enc.forward(torch.zeros(2, 0, 40, device="cuda"))                     # no frames
    with pytest.raises(ValueError):
        enc.embed_utterances(torch.zeros(2, 1000, device="cuda"), [1000, 0])  # zero length
    with pytest.raises(ValueError):
        enc.embed_utterances(torch.zeros(2, 1000, device="cuda"), [1000, 1001])
    with pytest.raises(ValueError):
        enc.embed_utterance(torch.zeros(0, device="cuda"))
    with pytest.raises(ValueError):
        speaker.wav_to_mel_spectrogram(torch.zeros(1000))
    with pytest.raises(ValueError):
        speaker.normalize_volume(torch.zeros(2, 100, device="cuda"), lengths=[100])
    empty = speaker.VoiceEncoder("cuda")
    with pytest.raises(ValueError, match="not loaded"):
        empty.forward(torch.zeros(1, 4, 40, device="cuda"))
    with pytest.raises(ValueError, match="not loaded"):
        empty.embed_utterance(torch.zeros(1000, device="cuda"))
    with pytest.raises(ValueError, match="not loaded"):
        speaker.speaker_similarity(torch.zeros(1000, device="cuda"), torch.zeros(1000, device="cuda"), encoder=empty)
    # and at the C ABI: a handle without weights refuses the network with DEX_ERR_STATE, nothing enqueued
    import ctypes as C
    ctx = empty._ctx
    x = torch.zeros(1, 4, 40, device="cuda"); out = torch.zeros(1, 256, device="cuda"); ws = ctx.workspace(1, 4)
    assert ctx.lib.dex_spk_forward(ctx.h, x.data_ptr(), 1, 4, out.data_ptr(), ws.data_ptr(), ws.numel(), None) == -2
    assert b"not loaded" in ctx.lib.dex_spk_last_error(ctx.h)
    assert ctx.lib.dex_spk_forward(enc._ctx.h, x.data_ptr(), 1, 4, out.data_ptr(), ws.data_ptr(), 16, None) == -4      # workspace too small
    bad = (C.c_int64 * 1)(255)
    assert ctx.lib.dex_spk_load(ctx.h, b"linear.bias", out.data_ptr(), bad, 1, None) == -1
    assert ctx.lib.dex_spk_load(ctx.h, b"no.such.key", out.data_ptr(), bad, 1, None) == -1
