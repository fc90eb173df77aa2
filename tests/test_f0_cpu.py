"""CPU: the f0 tracker's host-side entry points (frame count, workspace plan, argument validation - no device is touched) and the
float64 restatement of its contract (tests/world_f0.py) held to signals whose f0 is known analytically."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from dex_tts_amd import _lib
from tests import world_f0 as W

FS = 22050.0
FP = 256.0 / 22050.0 * 1000.0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dex_tts_amd import build
        build.build(verbose=False)
    return _lib.load()


def opts(**kw):
    d = dict(fs=FS, frame_period_ms=FP, f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0, allowed_range=0.1)
    d.update(kw)
    return _lib.DexF0Opts(*(float(d[k]) for k in ("fs", "frame_period_ms", "f0_floor", "f0_ceil", "channels_in_octave", "allowed_range")))


def lens(*v):
    return (C.c_int32 * len(v))(*v)


def tone(f0, sec=2.0, fs=FS):
    n = np.arange(int(sec * fs))
    x = sum(np.sin(2 * np.pi * f0 * k * n / fs) / k for k in range(1, 8))
    return 0.3 * x / np.abs(x).max()


def glide(sec=2.0, fs=FS, f_lo=120.0):
    """Exponential glide f_lo -> 2 f_lo over `sec` seconds, 7 partials; -> (x, f(t))."""
    n = np.arange(int(sec * fs))
    ph = 2 * np.pi * np.cumsum(f_lo * 2.0 ** (n / fs / sec)) / fs
    x = sum(np.sin(k * ph) / k for k in range(1, 8))
    return 0.3 * x / np.abs(x).max(), (lambda t: f_lo * 2.0 ** (t / sec))


def test_frames_match_the_contract(lib):
    L = np.arange(1, 400001)
    got = np.array([lib.dex_f0_frames(int(n), None) for n in L])
    want = np.array([int(1000.0 * int(n) / 22050 / FP) + 1 for n in L])
    assert np.array_equal(got, want)
    short = L[got == L // 256]                        # one frame fewer than the mel's L // 256 + 1
    assert len(short) == 60 and 3328 in short and 26624 in short
    assert lib.dex_f0_frames(3328, None) == 13 and lib.dex_f0_frames(26624, None) == 104
    assert lib.dex_f0_frames(16000, C.byref(opts(fs=16000.0, frame_period_ms=5.0))) == 201
    assert W.frames(3328, FS, FP) == 13


def test_workspace_is_positive_and_monotone(lib):
    o = C.byref(opts())
    one = [lib.dex_f0_workspace_bytes(1, lens(n), o) for n in (1, 700, 3328, 22050, 89082)]
    assert all(v > 0 for v in one) and all(a < b for a, b in zip(one, one[1:]))
    byB = [lib.dex_f0_workspace_bytes(b, lens(*([22050] * b)), o) for b in (1, 2, 5, 32)]
    assert all(a < b for a, b in zip(byB, byB[1:]))
    assert lib.dex_f0_workspace_bytes(2, lens(700, 22050), o) == lib.dex_f0_workspace_bytes(2, lens(22050, 22050), o)
    assert lib.dex_f0_workspace_bytes(1, lens(22050), None) == lib.dex_f0_workspace_bytes(1, lens(22050), o)


def test_bad_arguments_rejected_without_a_device(lib):
    """Every check runs on the host before anything is enqueued: a dummy (never dereferenced) device pointer suffices."""
    fake = C.c_void_p(0x1000)
    ERR = -1
    for bad in (opts(f0_floor=0.0), opts(f0_floor=800.0), opts(f0_floor=900.0), opts(frame_period_ms=0.0), opts(frame_period_ms=-5.0),
                opts(fs=0.0), opts(channels_in_octave=0.0), opts(f0_floor=1.0, f0_ceil=1e6, channels_in_octave=8.0)):
        assert lib.dex_f0_frames(22050, C.byref(bad)) == ERR
        assert lib.dex_f0_workspace_bytes(1, lens(22050), C.byref(bad)) == 0
        assert lib.dex_f0_dio(fake, lens(22050), 1, 22050, C.byref(bad), fake, fake, 1 << 30, None) == ERR
        assert lib.dex_f0_stonemask(fake, lens(22050), 1, 22050, C.byref(bad), fake, C.c_void_p(0x2000), None, 0, None) == ERR
    o = C.byref(opts())
    assert lib.dex_f0_frames(0, o) == ERR
    for B, ln, n in ((0, lens(10), 10), (1, lens(0), 10), (1, lens(11), 10), (2, lens(10, -1), 10), (1, lens(5), 0)):
        assert lib.dex_f0_dio(fake, ln, B, n, o, fake, fake, 1 << 30, None) == ERR
        assert lib.dex_f0_stonemask(fake, ln, B, n, o, fake, C.c_void_p(0x2000), None, 0, None) == ERR
        assert lib.dex_f0_peak_normalize(fake, ln, B, n, fake, None) == ERR
    assert lib.dex_f0_dio(fake, None, 1, 10, o, fake, fake, 1 << 30, None) == ERR                    # no lengths
    assert lib.dex_f0_dio(None, lens(10), 1, 10, o, fake, fake, 1 << 30, None) == ERR                # no wav
    assert lib.dex_f0_dio(fake, lens(10), 1, 10, o, fake, None, 1 << 30, None) == ERR                # no workspace
    assert lib.dex_f0_dio(fake, lens(22050), 1, 22050, o, fake, fake, 64, None) == -4                # workspace too small
    assert lib.dex_f0_stonemask(fake, lens(10), 1, 10, o, fake, fake, None, 0, None) == ERR          # in place


@pytest.mark.parametrize("f0", [90.0, 130.0, 220.0, 400.0, 650.0])
def test_restatement_tracks_harmonic_tones(f0):
    x = tone(f0)
    f, t = W.dio(x, FS, frame_period=FP)
    inner = slice(3, len(f) - 3)                      # the 4th through the 4th-last frame
    assert (f[inner] > 0).all()
    e = np.abs(f / f0 - 1)
    # DIO: <= 1e-5 from the 5th through the 5th-last frame; the 4th frames are rebuilt by the fix steps' walks from the band
    # candidates next to the signal's ends (the filters' zero padding reaches them), measured up to 1.3e-5 at 90 Hz
    assert e[4:-4].max() <= 1e-5, e[4:-4].max()
    assert e[inner].max() <= 2e-5, e[inner].max()
    s = W.stonemask(x, f, t, FS)
    assert np.abs(s[inner] / f0 - 1).max() <= 1e-3


def test_restatement_follows_a_glide():
    x, ftrue = glide()
    f, t = W.dio(x, FS, frame_period=FP)
    s = W.stonemask(x, f, t, FS)
    v = s > 0
    assert v.sum() >= len(s) - 6
    assert np.abs(s[v] / ftrue(t[v]) - 1).max() <= 2e-2


def test_restatement_noise_and_silence_unvoiced():
    x = np.random.default_rng(0).normal(0.0, 0.1, int(2 * FS))
    f, t = W.dio(x, FS, frame_period=FP)
    assert not (f > 0).any() and not (W.stonemask(x, f, t, FS) > 0).any()
    f, _ = W.dio(np.zeros(int(2 * FS)), FS, frame_period=FP)
    assert not f.any()


def test_restatement_short_input_all_zero():
    for L in (1, 300, 700, 767):
        f, _ = W.dio(tone(220.0)[:L], FS, frame_period=FP)
        assert len(f) <= 3 and not f.any()


def test_restatement_on_real_speech(golden_dir):
    x = np.load(os.path.join(golden_dir, "audio_mel.npz"))["sample1_1s_wav"].astype(np.float64)
    f, t = W.dio(x, FS, frame_period=FP)
    v = f > 0
    assert len(f) == 87 and 50 <= v.sum() <= 70 and 180 < np.median(f[v]) < 260
    s = W.stonemask(x, f, t, FS)
    assert np.array_equal(s > 0, v) or (s > 0).sum() >= v.sum() - 2
    assert math.isclose(np.median(s[s > 0]), np.median(f[v]), rel_tol=0.05)


def test_sample1_fixture_is_the_reference_utterance(golden_dir):
    g = np.load(os.path.join(golden_dir, "sample1_wav.npz"))
    w = g["wav"]
    a = np.load(os.path.join(golden_dir, "audio_mel.npz"))
    assert w.dtype == np.float32 and len(w) == int(a["n_total"]) == 89082 and int(g["sr"]) == 22050
    assert np.array_equal(w[: len(a["sample1_1s_wav"])], a["sample1_1s_wav"])
