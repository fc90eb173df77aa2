"""CPU: the wav preparation's host-side entry points (resampled length, workspace plans, argument validation - no device is touched),
read_wav, and the float64 restatement of its contract (tests/wav_prep.py) held to signals with known answers."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.io import wavfile

from dex_tts_amd import _lib
from tests import wav_prep as P

RATES = (16000, 22050, 24000, 44100, 48000)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dex_tts_amd import build
        build.build(verbose=False)
    return _lib.load()


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def test_resampled_length_matches_integer_division(lib):
    lengths = list(range(1, 300)) + [511, 512, 513, 4095, 22050, 44100, 88200, 89082, 192000, 1 << 22]
    for a in RATES:
        for b in RATES:
            for n in lengths:
                want = n * b // a
                got = lib.dex_wav_resampled_length(n, a, b)
                assert got == (want if want >= 1 else -1), (n, a, b, got)
                if want >= 1:
                    assert P.resampled_length(n, a, b) == want
    assert lib.dex_wav_resampled_length(0, 48000, 22050) == -1
    assert lib.dex_wav_resampled_length(100, 0, 22050) == -1
    assert lib.dex_wav_resampled_length(100, 48000, -1) == -1
    assert lib.dex_wav_resampled_length(1 << 30, 1000, 48000) == -1             # above INT32_MAX


def test_workspace_plans(lib):
    o = _lib.DexWavTrimOpts(30.0, 2048, 512, 0)
    one = [lib.dex_wav_trim_workspace_bytes(1, i32(n), C.byref(o)) for n in (1, 700, 89082, 192000)]
    assert all(v > 0 for v in one) and all(a < b for a, b in zip(one, one[1:]))
    assert lib.dex_wav_trim_workspace_bytes(1, i32(89082), None) == lib.dex_wav_trim_workspace_bytes(1, i32(89082), C.byref(o))
    assert lib.dex_wav_trim_workspace_bytes(1, i32(89082), None) == (89082 // 512 + 4) * 8
    assert lib.dex_wav_resample_table_bytes(None) == (512 * 64 + 1) * 16
    assert lib.dex_wav_peak_workspace_bytes(3, 5000) == 3 * 3 * 8
    for bad in (_lib.DexWavTrimOpts(30.0, 2048, 500, 0), _lib.DexWavTrimOpts(30.0, 2048, 0, 0), _lib.DexWavTrimOpts(30.0, 256, 512, 0),
                _lib.DexWavTrimOpts(30.0, 2048, 512, 2), _lib.DexWavTrimOpts(float("nan"), 2048, 512, 0)):
        assert lib.dex_wav_trim_workspace_bytes(1, i32(89082), C.byref(bad)) == 0
    assert lib.dex_wav_trim_workspace_bytes(1, i32(0), None) == 0
    for bad in (_lib.DexWavResampleOpts(0, 9, 14.0, 0.9), _lib.DexWavResampleOpts(64, 0, 14.0, 0.9), _lib.DexWavResampleOpts(64, 9, -1.0, 0.9),
                _lib.DexWavResampleOpts(64, 9, 14.0, 0.0), _lib.DexWavResampleOpts(64, 9, 14.0, 1.5), _lib.DexWavResampleOpts(1 << 20, 9, 14.0, 0.9)):
        assert lib.dex_wav_resample_table_bytes(C.byref(bad)) == 0
    assert lib.dex_wav_peak_workspace_bytes(0, 100) == 0 and lib.dex_wav_peak_workspace_bytes(1, 0) == 0


def test_bad_arguments_rejected_without_a_device(lib):
    """Every check runs on the host before anything is enqueued: dummy (never dereferenced) device pointers suffice."""
    fake, out = C.c_void_p(0x1000), C.c_void_p(0x2000)
    ERR, WS = -1, -4
    ws = lib.dex_wav_trim_workspace_bytes(1, i32(1000), None)
    assert lib.dex_wav_trim(None, i32(1000), 1, 1000, None, out, None, fake, ws, None) == ERR
    assert lib.dex_wav_trim(fake, i32(1000), 1, 1000, None, None, None, fake, ws, None) == ERR
    assert lib.dex_wav_trim(fake, i32(1000), 1, 1000, None, out, None, None, ws, None) == ERR
    assert lib.dex_wav_trim(fake, i32(1001), 1, 1000, None, out, None, fake, 1 << 30, None) == ERR      # length past the row
    assert lib.dex_wav_trim(fake, i32(0), 1, 1000, None, out, None, fake, 1 << 30, None) == ERR
    assert lib.dex_wav_trim(fake, i32(1000), 0, 1000, None, out, None, fake, 1 << 30, None) == ERR
    bad = _lib.DexWavTrimOpts(30.0, 2048, 500, 0)
    assert lib.dex_wav_trim(fake, i32(1000), 1, 1000, C.byref(bad), out, None, fake, 1 << 30, None) == ERR
    assert lib.dex_wav_trim(fake, i32(1000), 1, 1000, None, out, None, fake, ws - 1, None) == WS

    rws = lib.dex_wav_resample_table_bytes(None)
    assert lib.dex_wav_resample_table(None, None, rws, None) == ERR
    assert lib.dex_wav_resample_table(None, C.c_void_p(0x1008), rws, None) == ERR                # not 16-byte aligned
    assert lib.dex_wav_resample_table(None, fake, rws - 1, None) == WS
    assert lib.dex_wav_resample_table(C.byref(_lib.DexWavResampleOpts(64, 9, 14.0, 2.0)), fake, rws, None) == ERR

    def rs(off=0, n=48000, sr=48000, B=1, stride=48000, sr_new=22050, out_stride=22050, ws=rws, x=fake, y=out, w=fake, opts=None):
        return lib.dex_wav_resample(x, stride, i32(off), i32(n), i32(sr), B, sr_new, opts, y, out_stride, w, ws, None)

    assert rs(sr=0) == ERR and rs(sr=-48000) == ERR and rs(sr_new=0) == ERR
    assert rs(n=0) == ERR and rs(off=-1) == ERR and rs(off=1) == ERR and rs(n=48001) == ERR       # spans outside the row
    assert rs(n=2, sr=48000, stride=48000) == ERR                                                  # L_out = 0
    assert rs(out_stride=22049) == ERR                                                              # row does not fit the output
    assert rs(sr=48000 * 600, n=48000) == ERR                                                       # ratio below 1 / 512
    assert rs(x=None) == ERR and rs(y=None) == ERR and rs(w=None) == ERR and rs(B=0) == ERR and rs(w=C.c_void_p(0x1008)) == ERR
    assert rs(ws=rws - 1) == WS
    assert rs(opts=C.byref(_lib.DexWavResampleOpts(64, 9, 14.0, 2.0))) == ERR
    assert lib.dex_wav_resample(fake, 48000, None, i32(48000), i32(48000), 1, 22050, None, out, 22050, fake, rws, None) == ERR

    pws = lib.dex_wav_peak_workspace_bytes(1, 1000)
    assert lib.dex_wav_peak_normalize_f64(None, i32(1000), 1, 1000, out, fake, pws, None) == ERR
    assert lib.dex_wav_peak_normalize_f64(fake, i32(1000), 1, 1000, None, fake, pws, None) == ERR
    assert lib.dex_wav_peak_normalize_f64(fake, i32(1001), 1, 1000, out, fake, pws, None) == ERR
    assert lib.dex_wav_peak_normalize_f64(fake, i32(1000), 1, 1000, out, None, pws, None) == ERR
    assert lib.dex_wav_peak_normalize_f64(fake, i32(1000), 1, 1000, out, fake, pws - 1, None) == WS


# ---- the restatement against known answers
def _tone_error(sr, f=1000.0, sec=2.0, edge=300):
    n = np.arange(int(sec * sr))
    y = P.resample(np.sin(2 * np.pi * f * n / sr), sr, 22050)
    assert len(y) == P.resampled_length(len(n), sr, 22050)
    ref = np.sin(2 * np.pi * f * np.arange(len(y)) / 22050)
    return np.abs(y - ref)[edge:-edge].max()


def test_restatement_tone_48k_and_16k():
    assert _tone_error(48000) <= 1e-3              # resampy's own gain error: int(0.459375 * 512) = 235, not 235.2 (about 8.6e-4)
    assert _tone_error(16000) <= 1e-6


def test_restatement_rejects_aliases():
    sr = 48000
    n = np.arange(2 * sr)
    y = P.resample(np.sin(2 * np.pi * 15000.0 * n / sr), sr, 22050)            # above 11025 Hz: must not fold back
    assert 20 * np.log10(np.abs(y[300:-300]).max()) <= -70.0


def test_restatement_constant():
    for sr in (48000, 44100, 16000):
        y = P.resample(np.ones(sr), sr, 22050)
        assert np.abs(y[300:-300] - 1.0).max() <= 1e-3, sr


def test_restatement_window_and_identity():
    w = P.kaiser_best_window()
    assert len(w) == 512 * 64 + 1 and w[0] == pytest.approx(P.ROLLOFF, rel=1e-15)
    assert abs(w[-1]) < 1e-6 * w[0]                                  # the kaiser taper ends near 1 / i0(beta)
    x = np.random.default_rng(0).normal(size=1000)
    assert np.array_equal(P.resample(x, 22050, 22050), x)


def _silence_padded(sig, lead, tail, noise_db=-80.0, seed=0):
    rng = np.random.default_rng(seed)
    amp = np.abs(sig).max() * 10 ** (noise_db / 20)
    return np.concatenate([amp * rng.standard_normal(lead), sig, amp * rng.standard_normal(tail)])


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_restatement_trim_known_bounds(pad_mode):
    sr = 22050
    n = np.arange(sr)
    tone = 0.5 * np.sin(2 * np.pi * 440.0 * n / sr)
    x = _silence_padded(tone, 8192, 10240)                           # the tone is samples [8192, 30242), noise at -80 dB around it
    # frame f covers samples [512 f - 1024, 512 f + 1024): f = 15 is the first to reach the tone (512 of its samples: -6 dB), f = 61
    # the last (34 samples: -18 dB); every other frame holds noise only (-77 dB)
    assert P.trim_bounds(x, pad_mode=pad_mode) == (15 * 512, 62 * 512)
    db = P.frame_db(x, pad_mode=pad_mode)
    assert np.abs(db + 30).min() > 1.0                               # no frame within 1 dB of the threshold


def test_restatement_trim_edge_rows():
    assert P.trim_bounds(np.zeros(5000)) == (0, 5000)                 # every frame is 0 dB below the (zero) maximum
    assert P.trim_bounds(np.array([0.3])) == (0, 1)
    x = np.random.default_rng(1).normal(size=700)
    for m in ("constant", "reflect"):
        assert P.trim_bounds(x, pad_mode=m) == (0, 700)
    with pytest.raises(ValueError):
        P.trim_bounds(x, pad_mode="edge")


# ---- read_wav
@pytest.mark.parametrize("kind", ["int16", "int32", "uint8", "float32"])
def test_read_wav_round_trip(tmp_path, kind):
    from dex_tts_amd.wavprep import read_wav
    rng = np.random.default_rng(3)
    if kind == "int16":
        d = rng.integers(-32768, 32768, 1000).astype(np.int16); want = d / 32768.0
    elif kind == "int32":
        d = rng.integers(-(1 << 31), 1 << 31, 1000).astype(np.int32); want = d / 2.0 ** 31
    elif kind == "uint8":
        d = rng.integers(0, 256, 1000).astype(np.uint8); want = (d.astype(np.float64) - 128.0) / 128.0
    else:
        d = rng.uniform(-1, 1, 1000).astype(np.float32); want = d.astype(np.float64)
    p = tmp_path / f"{kind}.wav"
    wavfile.write(p, 44100, d)
    x, sr = read_wav(str(p))
    assert sr == 44100 and x.dtype == np.float64 and np.array_equal(x, want)
    assert np.abs(x).max() <= 1.0


def test_read_wav_rejects_multichannel(tmp_path):
    from dex_tts_amd.wavprep import read_wav
    p = tmp_path / "stereo.wav"
    wavfile.write(p, 16000, np.zeros((100, 2), np.int16))
    with pytest.raises(ValueError):
        read_wav(str(p))
