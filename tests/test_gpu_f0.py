"""GPU (-m gpu): the f0 tracker (dex_f0_dio / dex_f0_stonemask, csrc/f0.hip) against its float64 restatement (tests/world_f0.py) on
synthetic signals and real speech at 22050 and 16000 Hz, a ragged batch (rows bitwise equal to the same utterance alone, calls
bitwise reproducible), and reference_features end to end through the style encoders.  Both sides sum directly in fp64 in different
orders: the voiced / unvoiced pattern must be identical and voiced frames agree to 1e-9 relative.  Not pinned to pyworld."""
import os

import numpy as np
import pytest
import torch

from tests import world_f0 as W

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FS = 22050.0
FP = 256.0 / 22050.0 * 1000.0
REL = 1e-9


def tone(f0, sec=2.0, fs=FS):
    n = np.arange(int(sec * fs))
    x = sum(np.sin(2 * np.pi * f0 * k * n / fs) / k for k in range(1, 8))
    return 0.3 * x / np.abs(x).max()


def glide(sec=2.0, fs=FS):
    n = np.arange(int(sec * fs))
    ph = 2 * np.pi * np.cumsum(120.0 * 2.0 ** (n / fs / sec)) / fs
    x = sum(np.sin(k * ph) / k for k in range(1, 8))
    return 0.3 * x / np.abs(x).max()


def sample1():
    return np.load(os.path.join(GOLD, "sample1_wav.npz"))["wav"]


def sample1_1s():
    return np.load(os.path.join(GOLD, "audio_mel.npz"))["sample1_1s_wav"]


def resample(x, fs_in, fs_out):
    """Band-limited resampling by zero-padding / truncating the spectrum (numpy only)."""
    n_out = int(round(len(x) * fs_out / fs_in))
    X = np.fft.rfft(np.asarray(x, np.float64))
    Y = np.zeros(n_out // 2 + 1, dtype=complex)
    k = min(len(X), len(Y))
    Y[:k] = X[:k]
    return np.fft.irfft(Y, n_out) * (n_out / len(x))


SIGNALS = {
    **{f"tone{int(f)}": (lambda f=f: tone(f)) for f in (90.0, 130.0, 220.0, 400.0, 650.0)},
    "glide": glide,
    "noise": lambda: np.random.default_rng(0).normal(0.0, 0.1, int(2 * FS)),
    "silence": lambda: np.zeros(int(FS)),
    "sample1_1s": sample1_1s,
    "sample1": sample1,
}


def _agree(got, ref, tag):
    vg, vr = got > 0, ref > 0
    flips = np.nonzero(vg != vr)[0]
    assert len(flips) == 0, f"{tag}: voicing differs at frames {flips.tolist()} (gpu {got[flips].tolist()}, restatement {ref[flips].tolist()})"
    if vr.any():
        rel = np.abs(got[vr] / ref[vr] - 1).max()
        assert rel <= REL, (tag, float(rel))


def _track(x32, fs, fp):
    from dex_tts_amd import f0 as F0
    xd = torch.from_numpy(x32).cuda()
    f, t = F0.dio(xd, fs, frame_period=fp)
    return xd, f.cpu().numpy(), t.cpu().numpy()


def _check_signal(x, fs, fp, tag):
    from dex_tts_amd import f0 as F0
    x32 = np.asarray(x, np.float32)
    x64 = x32.astype(np.float64)                       # the device promotes the fp32 wav exactly: the restatement sees the same samples
    xd, fg, t = _track(x32, fs, fp)
    fr, tr = W.dio(x64, fs, frame_period=fp)
    assert fg.shape == fr.shape and np.array_equal(t, tr)
    _agree(fg, fr, f"{tag}:dio")
    sg = F0.stonemask(xd, torch.from_numpy(fr).cuda(), tr, fs).cpu().numpy()      # the same input f0 on both sides
    sr = W.stonemask(x64, fr, tr, fs)
    _agree(sg, sr, f"{tag}:stonemask")
    return fr, sr


@pytest.mark.parametrize("name", list(SIGNALS))
def test_matches_restatement(name):
    fr, sr = _check_signal(SIGNALS[name](), FS, FP, name)
    if name.startswith("tone"):
        assert (fr[3:-3] > 0).all()
    if name in ("noise", "silence"):
        assert not (sr > 0).any()


@pytest.mark.parametrize("name", ["tone220", "speech"])
def test_matches_restatement_at_16k(name):
    x = tone(220.0, fs=16000.0) if name == "tone220" else resample(sample1_1s().astype(np.float64), FS, 16000.0)
    fr, _ = _check_signal(x, 16000.0, 5.0, f"{name}@16k")
    assert (fr > 0).sum() > 20


def test_ragged_batch_rows_equal_single_runs():
    from dex_tts_amd import f0 as F0
    lengths = [89082, 3328, 26624, 700, 22050]
    src = [sample1(), tone(220.0).astype(np.float32), glide().astype(np.float32), tone(130.0).astype(np.float32),
           sample1_1s()]
    L = max(lengths)
    xb = np.zeros((len(lengths), L), np.float32)
    for b, (n, s) in enumerate(zip(lengths, src)):
        xb[b, :n] = s[:n]
    xbd = torch.from_numpy(xb).cuda()
    f, t = F0.dio(xbd, FS, frame_period=FP, lengths=lengths)
    s = F0.stonemask(xbd, f, t, FS, lengths=lengths)
    f2, _ = F0.dio(xbd, FS, frame_period=FP, lengths=lengths)
    s2 = F0.stonemask(xbd, f2, t, FS, lengths=lengths)
    f, s, f2, s2 = (a.cpu().numpy() for a in (f, s, f2, s2))
    assert f.shape == (5, W.frames(L, FS, FP))
    assert np.array_equal(f, f2) and np.array_equal(s, s2)                        # two identical calls: bitwise
    for b, n in enumerate(lengths):
        Fb = W.frames(n, FS, FP)
        assert not f[b, Fb:].any() and not s[b, Fb:].any()                          # past the row's F: 0
        x1 = torch.from_numpy(np.ascontiguousarray(xb[b, :n])).cuda()
        f1, t1 = F0.dio(x1, FS, frame_period=FP)
        s1 = F0.stonemask(x1, f1, t1, FS)
        assert np.array_equal(f[b, :Fb], f1.cpu().numpy()), b                      # bitwise: independent of the batch
        assert np.array_equal(s[b, :Fb], s1.cpu().numpy()), b
        _agree(f[b, :Fb], W.dio(xb[b, :n].astype(np.float64), FS, frame_period=FP)[0], f"row{b}")
    assert W.frames(700, FS, FP) <= 3 and not f[3].any()
    assert W.frames(3328, FS, FP) == 13 and W.frames(26624, FS, FP) == 104


def test_peak_normalize_and_argument_errors():
    from dex_tts_amd import f0 as F0
    x = np.zeros((2, 1000), np.float32)
    x[0] = 0.25 * np.sin(np.arange(1000) / 7.0)
    x[1, :600] = -0.5 * np.cos(np.arange(600) / 3.0)
    got = F0.peak_normalize(torch.from_numpy(x).cuda(), lengths=[1000, 600]).cpu().numpy()
    for b, n in enumerate((1000, 600)):
        r = x[b, :n].astype(np.float64)
        assert np.array_equal(got[b, :n], (r / np.abs(r).max()).astype(np.float32)) and not got[b, n:].any()
    with pytest.raises(ValueError):
        F0.dio(torch.zeros(1000).cuda(), FS, speed=2)
    with pytest.raises(ValueError):
        F0.dio(torch.zeros(1000).cuda(), FS, f0_floor=900.0)
    with pytest.raises(ValueError):
        F0.reference_features(torch.zeros(1000).cuda(), sr=16000)
    with pytest.raises(RuntimeError):
        F0.dio(torch.zeros(1000), FS)                                               # no CPU path


def test_reference_features_through_style_encoders():
    from dex_tts_amd import f0 as F0, style as S, synth
    from dex_tts_amd.audio import TacotronSTFT, lf0_from_f0
    w = sample1()
    feats = F0.reference_features(torch.from_numpy(w).cuda())
    mel_frames = len(w) // 256 + 1
    tlen = min(W.frames(len(w), FS, FP), mel_frames)
    assert feats["ref"].shape == (1, 80, mel_frames) and int(feats["ref_lengths"][0]) == mel_frames
    assert feats["lf0"].shape == (1, tlen) and int(feats["lf0_lengths"][0]) == tlen
    # the same chain with the restatement's f0 (synthesize.py:46-58)
    w64 = w.astype(np.float64)
    wn = w64 / np.abs(w64).max()
    wn32 = wn.astype(np.float32)
    f, t = W.dio(wn32.astype(np.float64), FS, frame_period=FP)
    f = W.stonemask(wn32.astype(np.float64), f, t, FS)
    stft = TacotronSTFT()
    mel = stft.mel_spectrogram(torch.from_numpy(wn32).reshape(1, -1).cuda())[0]
    lf0 = lf0_from_f0(torch.from_numpy(f[:tlen].astype(np.float32)).cuda())[None]
    assert torch.equal(mel, feats["ref"])
    ln = torch.tensor([mel_frames]).cuda()
    m = S.StyleEncoders()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_style_weights(S.param_shapes(S.VCTK)).items()})
    m = m.cuda().eval()
    a = m(feats["ref"], feats["ref_lengths"], feats["sty"], feats["sty_lengths"], feats["lf0"], feats["lf0_lengths"], return_indices=True)
    b = m(mel, ln, mel, ln, lf0, torch.tensor([tlen]).cuda(), return_indices=True)
    assert torch.equal(a[3], b[3])                                                  # identical VQ indices
    for x, y, tag in ((a[1], b[1], "sty_dec"), (a[2], b[2], "sty_enc"), (torch.stack(a[0]), torch.stack(b[0]), "ref_skips")):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        err = np.abs(x - y).max()
        assert np.isfinite(x).all() and err <= 2e-4 * max(1.0, np.abs(y).max()), (tag, float(err))     # tests/test_style.py's bound


def test_reference_features_ragged_batch():
    from dex_tts_amd import f0 as F0
    w = sample1()
    lengths = [len(w), 22050, 3328]
    xb = np.zeros((3, len(w)), np.float32)
    for b, n in enumerate(lengths):
        xb[b, :n] = w[:n]
    feats = F0.reference_features(torch.from_numpy(xb).cuda(), lengths=lengths)
    for b, n in enumerate(lengths):
        one = F0.reference_features(torch.from_numpy(xb[b, :n]).cuda())
        T = int(one["ref_lengths"][0]); Tl = int(one["lf0_lengths"][0])
        assert int(feats["ref_lengths"][b]) == T and int(feats["lf0_lengths"][b]) == Tl
        assert torch.equal(feats["ref"][b, :, :T], one["ref"][0]) and torch.equal(feats["lf0"][b, :Tl], one["lf0"][0])
