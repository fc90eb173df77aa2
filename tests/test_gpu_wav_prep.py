"""GPU (-m gpu): the wav preparation (dex_wav_trim / dex_wav_resample / dex_wav_peak_normalize_f64, csrc/wavprep.hip) against its
float64 restatement (tests/wav_prep.py), a ragged mixed-rate batch (rows bitwise equal to the same row alone), and preprocess_wav
end to end through the style encoders.  The signals are built here from tests/golden/sample1_wav.npz: padded with low noise and
silence, and resampled by the restatement to 16 / 24 / 44.1 / 48 kHz.  Not pinned to librosa or resampy."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from tests import wav_prep as P
from tests import world_f0 as W

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FS = 22050.0
FP = 256.0 / 22050.0 * 1000.0
RATES = (16000, 24000, 44100, 48000)


def sample1():
    return np.load(os.path.join(GOLD, "sample1_wav.npz"))["wav"]


def padded(x, sr, seed=0):
    """x (fp32-exact) with 0.3 s of -70 dB noise and 0.1 s of digital silence before it, 0.2 s of noise after it -> fp32."""
    rng = np.random.default_rng(seed)
    amp = np.abs(x).max() * 10 ** (-70 / 20)
    return np.concatenate([amp * rng.standard_normal(int(0.3 * sr)), np.zeros(int(0.1 * sr)), x,
                           amp * rng.standard_normal(int(0.2 * sr))]).astype(np.float32)


_AT = {}
SEG = (0.35, 3.35)      # seconds of sample1 cut at loud points: every frame next to the trim bounds lies >= 15 dB from -30 dB


def segment(sr):
    """sample1 resampled by the restatement to sr, cut to SEG: fp32."""
    w = sample1().astype(np.float64)
    y = w if sr == 22050 else P.resample(w, 22050, sr)
    return y[int(SEG[0] * sr): int(SEG[1] * sr)].astype(np.float32)


def sample1_at(sr):
    """segment(sr), padded: fp32."""
    if sr not in _AT:
        _AT[sr] = padded(segment(sr), sr)
    return _AT[sr]


def robust_bounds(x, pad_mode="constant"):
    """The restatement's bounds, with the test's precondition: every frame outside them is below -31 dB and the first and last
    frame inside are above -29 dB, so a last-bit difference in a frame's mse cannot move them."""
    x64 = x.astype(np.float64)
    s, e = P.trim_bounds(x64, pad_mode=pad_mode)
    db = P.frame_db(x64, pad_mode=pad_mode)
    first, last = s // 512, -(-e // 512) - 1
    outside = np.r_[db[:first], db[last + 1:]]
    assert (outside < -31).all() and db[first] > -29 and db[last] > -29, "test signal too close to the threshold"
    return s, e


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- trim
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_trim_matches_restatement(pad_mode):
    from dex_tts_amd import wavprep as WP
    short = (0.4 * np.sin(np.arange(700) / 5.0)).astype(np.float32)                   # shorter than one frame
    rows = [sample1_at(sr) for sr in (22050,) + RATES] + [short, np.zeros(3000, np.float32)]
    L = max(len(r) for r in rows)
    xb = np.zeros((len(rows), L), np.float32)
    for b, r in enumerate(rows):
        xb[b, : len(r)] = r
    lengths = [len(r) for r in rows]
    got = WP.trim(cuda(xb), lengths, pad_mode=pad_mode).cpu().numpy()
    for b, r in enumerate(rows[:-1]):
        assert tuple(got[b]) == robust_bounds(r, pad_mode), (b, got[b])
        one = WP.trim(cuda(r), pad_mode=pad_mode).cpu().numpy()
        assert np.array_equal(one, got[b])
    assert tuple(got[-1]) == P.trim_bounds(np.zeros(3000)) == (0, 3000)                # all zero: kept whole
    assert tuple(got[-2]) == (0, 700)
    for b, sr in enumerate((22050,) + RATES):
        lead, n = int(0.3 * sr) + int(0.1 * sr), len(segment(sr))
        assert lead - 2048 <= got[b, 0] <= lead and lead + n <= got[b, 1] <= lead + n + 2048, (sr, got[b])


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_trim_frame_mse_short_rows(pad_mode):
    """Rows shorter than the 1024-sample pad (reflect repeats with period 2 (L - 1) there) and around it: every frame's mean square
    against the restatement's, not only the bounds."""
    from dex_tts_amd import wavprep as WP
    rng = np.random.default_rng(7)
    lengths = [1, 2, 3, 5, 700, 1023, 1024, 1025, 3000]
    rows = [(rng.standard_normal(n) * np.linspace(1.0, 0.01, n)).astype(np.float32) for n in lengths]
    L = max(lengths)
    xb = np.zeros((len(rows), L), np.float32)
    for b, r in enumerate(rows):
        xb[b, : len(r)] = r
    bounds, mse = WP.trim(cuda(xb), lengths, pad_mode=pad_mode, return_mse=True)
    bounds, mse = bounds.cpu().numpy(), mse.cpu().numpy()
    for b, r in enumerate(rows):
        want = P.frame_mse(r.astype(np.float64), pad_mode=pad_mode)
        F = len(want)
        assert np.allclose(mse[b, :F], want, rtol=1e-12, atol=0), (lengths[b], mse[b, :F], want)
        assert not mse[b, F:].any()
    if pad_mode == "reflect":                      # the two pad modes must differ where the pad reflects: here they do
        const = P.frame_mse(rows[4].astype(np.float64), pad_mode="constant")
        assert not np.allclose(mse[4, : len(const)], const, rtol=1e-3)


# ---- resample
@pytest.mark.parametrize("sr_in,sr_out", [(48000, 22050), (44100, 22050), (24000, 22050), (16000, 22050), (22050, 48000), (8000, 22050)])
def test_resample_matches_restatement(sr_in, sr_out):
    from dex_tts_amd import wavprep as WP
    x = sample1_at(sr_in)[: int(1.5 * sr_in)]                                         # 1.5 s: the restatement's loop stays short
    y, lo = WP.resample(cuda(x), sr_in, sr_out)
    ref = P.resample(x.astype(np.float64), sr_in, sr_out)
    assert y.dtype == torch.float64 and int(lo[0]) == len(ref) == P.resampled_length(len(x), sr_in, sr_out)
    err = np.abs(y.cpu().numpy() - ref).max()
    assert err <= 1e-12 * np.abs(x).max(), (sr_in, sr_out, float(err))


@pytest.mark.parametrize("sr_in", [24 * 22050, 32 * 22050])
def test_resample_high_rates_read_global_memory(sr_in):
    """Above about 21 x 22050 Hz a tile's input span (255 / ratio + 2 wings of taps) no longer fits in LDS and the taps read the wav
    from global memory: the same arithmetic, the same results."""
    from dex_tts_amd import wavprep as WP
    w = sample1()[int(1.0 * 22050): int(1.15 * 22050)].astype(np.float64)
    x = P.resample(w, 22050, sr_in).astype(np.float32)
    y, lo = WP.resample(cuda(x), sr_in, 22050)
    ref = P.resample(x.astype(np.float64), sr_in, 22050)
    assert int(lo[0]) == len(ref)
    err = np.abs(y.cpu().numpy() - ref).max()
    assert err <= 1e-12 * np.abs(x).max(), (sr_in, float(err))


def test_resample_offsets_read_in_place():
    from dex_tts_amd import wavprep as WP
    x = sample1_at(48000)
    y, lo = WP.resample(cuda(x), 48000, 22050, lengths=[30000], offsets=[12345])
    y1, _ = WP.resample(cuda(x[12345:42345]), 48000, 22050)
    assert int(lo[0]) == 30000 * 22050 // 48000 and torch.equal(y, y1)


# ---- peak normalisation
def test_peak_normalize_f64_bitwise():
    from dex_tts_amd import wavprep as WP
    rng = np.random.default_rng(5)
    lengths = [5000, 4097, 2048, 1, 3000]
    x = np.zeros((5, 5000))
    for b, n in enumerate(lengths):
        x[b, :n] = rng.normal(0, 0.1 * (b + 1), n)
    x[4] = 0.0                                                                        # silent row
    got = WP.peak_normalize_f64(cuda(x), lengths).cpu().numpy()
    for b, n in enumerate(lengths):
        want = (x[b, :n] / np.abs(x[b, :n]).max()).astype(np.float32) if b != 4 else np.zeros(n, np.float32)
        assert np.array_equal(got[b, :n], want), b
        assert not got[b, n:].any()


# ---- ragged, mixed-rate batch
def test_ragged_mixed_rate_batch_rows_equal_single_rows():
    from dex_tts_amd import wavprep as WP
    rows = [sample1_at(48000), sample1_at(16000)[:30000], sample1_at(22050)[:50000], sample1_at(44100), sample1_at(24000)[:7000]]
    srs = [48000, 16000, 22050, 44100, 24000]
    L = max(len(r) for r in rows)
    xb = np.zeros((len(rows), L), np.float32)
    for b, r in enumerate(rows):
        xb[b, : len(r)] = r
    lengths = [len(r) for r in rows]
    xn, lo = WP.prepare(cuda(xb), srs, lengths)
    xn2, lo2 = WP.prepare(cuda(xb), srs, lengths)
    assert torch.equal(xn, xn2) and np.array_equal(lo, lo2)                            # two identical calls: bitwise
    xn = xn.cpu().numpy()
    for b, (r, sr) in enumerate(zip(rows, srs)):
        one, l1 = WP.prepare(cuda(r), sr)
        n = int(lo[b])
        assert n == int(l1[0]) and np.array_equal(xn[b, :n], one.cpu().numpy()[0]), b   # bitwise: independent of the batch
        assert not xn[b, n:].any()
    feats = WP.preprocess_wav(cuda(xb), srs, lengths)
    for b in (0, 2):
        one = WP.preprocess_wav(cuda(rows[b]), srs[b])
        T, Tl = int(one["ref_lengths"][0]), int(one["lf0_lengths"][0])
        assert int(feats["ref_lengths"][b]) == T and int(feats["lf0_lengths"][b]) == Tl
        assert torch.equal(feats["ref"][b, :, :T], one["ref"][0]) and torch.equal(feats["lf0"][b, :Tl], one["lf0"][0])


# ---- end to end
def test_preprocess_wav_48k_end_to_end():
    from dex_tts_amd import style as S, synth, wavprep as WP
    from dex_tts_amd.audio import TacotronSTFT, lf0_from_f0
    x = sample1_at(48000)
    xn, lo = WP.prepare(cuda(x), 48000)
    wd = xn[0, : int(lo[0])]
    w32 = wd.cpu().numpy()
    ref32, (s, e) = P.prepare(x.astype(np.float64), 48000)
    assert len(w32) == len(ref32)
    ulps = np.abs(w32.view(np.int32).astype(np.int64) - ref32.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, int(ulps.max())                                            # within 1 fp32 ulp of the restatement chain
    feats = WP.preprocess_wav(cuda(x), 48000)
    mel = TacotronSTFT().mel_spectrogram(wd.reshape(1, -1))[0]
    Tm = mel.shape[-1]
    assert feats["ref"].shape == (1, 80, Tm) and torch.equal(feats["ref"], mel) and torch.equal(feats["sty"], mel)
    w64 = w32.astype(np.float64)
    f, t = W.dio(w64, FS, frame_period=FP)
    f = W.stonemask(w64, f, t, FS)
    tlen = min(len(f), Tm)
    assert int(feats["lf0_lengths"][0]) == tlen
    lf0_ref = lf0_from_f0(cuda(f[:tlen].astype(np.float32)))[None]
    got, want = feats["lf0"][0].cpu().numpy(), lf0_ref[0].cpu().numpy()
    vg, vr = got != 0, want != 0
    flips = np.nonzero(vg != vr)[0]
    assert len(flips) == 0, f"voicing differs at frames {flips.tolist()} (f0 there {f[flips].tolist()})"
    assert np.abs(got[vr] - want[vr]).max() <= 1e-6
    ln = torch.tensor([Tm]).cuda()
    m = S.StyleEncoders()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_style_weights(S.param_shapes(S.VCTK)).items()})
    m = m.cuda().eval()
    a = m(feats["ref"], feats["ref_lengths"], feats["sty"], feats["sty_lengths"], feats["lf0"], feats["lf0_lengths"], return_indices=True)
    b = m(mel, ln, mel, ln, lf0_ref, torch.tensor([tlen]).cuda(), return_indices=True)
    assert torch.equal(a[3], b[3])
    for u, v, tag in ((a[1], b[1], "sty_dec"), (a[2], b[2], "sty_enc"), (torch.stack(a[0]), torch.stack(b[0]), "ref_skips")):
        u, v = u.cpu().numpy(), v.cpu().numpy()
        err = np.abs(u - v).max()
        assert np.isfinite(u).all() and err <= 2e-4 * max(1.0, np.abs(v).max()), (tag, float(err))


def test_preprocess_wav_from_files(tmp_path):
    from dex_tts_amd import wavprep as WP
    paths, rows, srs = [], [], []
    for sr in (48000, 16000):
        x = sample1_at(sr)
        pcm = np.round(x / np.abs(x).max() * 0.5 * 32767).astype(np.int16)
        p = tmp_path / f"ref{sr}.wav"
        wavfile.write(p, sr, pcm)
        paths.append(str(p)); rows.append((pcm / 32768.0).astype(np.float32)); srs.append(sr)
    feats = WP.preprocess_wav(paths)
    for b, (r, sr) in enumerate(zip(rows, srs)):
        one = WP.preprocess_wav(cuda(r), sr)
        T, Tl = int(one["ref_lengths"][0]), int(one["lf0_lengths"][0])
        assert torch.equal(feats["ref"][b, :, :T], one["ref"][0]) and torch.equal(feats["lf0"][b, :Tl], one["lf0"][0])


def test_preprocess_wav_at_22050_is_reference_features():
    from dex_tts_amd import f0 as F0, wavprep as WP
    w = cuda(sample1())
    a = WP.preprocess_wav(w, 22050)
    b = F0.reference_features(w)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_errors(tmp_path):
    from dex_tts_amd import wavprep as WP
    with pytest.raises(RuntimeError):
        WP.peak_normalize_f64(torch.ones(2, 100, dtype=torch.float64), [100, 50])      # CPU tensor: refused before any launch
    with pytest.raises(ValueError):
        WP.peak_normalize_f64(torch.ones(2, 100, dtype=torch.float64).cuda(), [100, 101])
    x32 = torch.linspace(-0.3, 0.7, 1000).cuda()                                     # float32 rows are promoted, not read as doubles
    assert torch.equal(WP.peak_normalize_f64(x32), WP.peak_normalize_f64(x32.double()))
    with pytest.raises(RuntimeError):
        WP.preprocess_wav(torch.zeros(1000), 22050)                                   # no CPU path
    with pytest.raises(RuntimeError):
        WP.trim(torch.zeros(1000))
    for bad in (0, -16000, [48000, 0]):
        with pytest.raises(ValueError):
            WP.preprocess_wav(torch.zeros(2, 1000).cuda(), bad)
    with pytest.raises(ValueError):
        WP.resample(torch.zeros(1000).cuda(), 48000, 0)
    with pytest.raises(ValueError):
        WP.resample(torch.zeros(2).cuda(), 48000, 22050)                               # no output sample
    with pytest.raises(ValueError):
        WP.preprocess_wav(torch.zeros(1000).cuda())                                    # rate missing
    p = tmp_path / "stereo.wav"
    wavfile.write(p, 16000, np.zeros((100, 2), np.int16))
    with pytest.raises(ValueError):
        WP.read_wav(str(p))
    with pytest.raises(ValueError):
        WP.preprocess_wav(str(p))
