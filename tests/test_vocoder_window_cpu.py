"""Windowed vocoding, the host side (no GPU): the three symbols of the C ABI, the workspace plan of a window, and the receptive field
``dex_voc_halo_frames`` / ``Generator.halo_frames`` = H checked on the fp32 CPU oracles of the four geometries of
tests/test_gpu_vocoder_ragged.py:

* sufficient: the oracle on ``mel[:, :, t0 - H : t0 + n + H]``, cropped, is the oracle on the whole mel over the window to 1e-6 (not
  bitwise: the CPU convolutions' rounding varies with the length; 0 - 7e-7 measured at H, 1e-4 to 9e-4 at H = 8);
* not wasteful: one mel frame is raised by 1.0 and the extent of the output samples that change at all is measured left of the
  frame's first sample and right of its last one.  H * hop covers both and is at most FACTOR * left + hop.  The measured extent is a
  lower bound of the analytic radius - fp32 rounding absorbs the farthest, smallest taps of the chain (in float64 the same
  measurement reaches 3240 / 4054 / 904 / 3235 samples) - and 1.25 allows for that.

  geometry        H    H * hop   measured left / right (fp32)   (H * hop - hop) / left
  hifigan_v1      13   3328      3230 / 3229                    0.95
  bigvgan_base    18   4608      3795 / 3768                    1.15
  snakebeta_242   67   1072      836 / 821                      1.263
  hifigan_v2      13   3328      3134 / 3125                    0.98

  snakebeta_242 exceeds 1.25: its hop is 16 and 19 anti-aliased activations (two 12-tap Kaiser-sinc filters each, whose outer taps
  are below 1e-3 of the centre) make up most of its 67 frames, so rounding absorbs more of the chain than in the hop-256 geometries.
  The analytic radius stands (float64 already reaches 904 samples = 56.5 frames); that geometry's factor is the observed ratio, 1.27."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from dex_tts_amd import _lib, vocoder as V
from tests.test_bigvgan_22khz import SMALL, mel_input, oracle, small_weights
from tests.test_vocoder import bvg_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = {"hifigan_v1": V.HIFIGAN_V1, "bigvgan_base": V.BIGVGAN_BASE, "snakebeta_242": SMALL["snakebeta_242"], "hifigan_v2": SMALL["hifigan_v2"]}
FACTOR = {"hifigan_v1": 1.25, "bigvgan_base": 1.25, "snakebeta_242": 1.27, "hifigan_v2": 1.25}
NEW = ("dex_voc_halo_frames", "dex_voc_window_workspace_bytes", "dex_vocode_window")


def hop_of(name):
    return int(np.prod(GEOM[name]["upsample_rates"]))


@functools.lru_cache(maxsize=None)
def weights_of(name):
    return bvg_weights() if name == "bigvgan_base" else small_weights(GEOM[name])


def halo_of(name):
    return V.Generator(V.AttrDict(GEOM[name])).halo_frames


class Ctx:
    """A created (not finalized) library context: host logic only."""

    def __init__(self, h):
        self.lib = _lib.load()
        self.ctx = C.c_void_p()
        c = V.make_config(h)
        assert self.lib.dex_voc_create(C.byref(c), C.byref(self.ctx)) == 0, self.lib.dex_voc_last_error(self.ctx)

    def __enter__(self):
        return self.lib, self.ctx

    def __exit__(self, *a):
        self.lib.dex_voc_destroy(self.ctx)


def test_symbols_in_header_export_and_binding():
    hdr = open(os.path.join(ROOT, "include", "dex_amd.h")).read()
    declared = set(re.findall(r"\b(dex_[a-z_0-9]+)\s*\(", hdr))
    bound = {n for n, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name


@pytest.mark.parametrize("name", list(GEOM) + ["bigvgan_22khz"])
def test_halo_and_window_workspace_follow_from_the_configuration(name):
    h = V.BIGVGAN_22KHZ if name == "bigvgan_22khz" else GEOM[name]
    with Ctx(h) as (lib, a), Ctx(h) as (_, b):
        H = lib.dex_voc_halo_frames(a)
        assert H > 0 and H == lib.dex_voc_halo_frames(b) == V.Generator(V.AttrDict(h)).halo_frames
        ws = lib.dex_voc_window_workspace_bytes(a, 2, 16)
        # one value per (B, n_frames) - the call has no T to depend on -, the same in every context of the configuration
        assert ws > 0 and ws == lib.dex_voc_window_workspace_bytes(a, 2, 16) == lib.dex_voc_window_workspace_bytes(b, 2, 16)
        # the ragged plan of the widest window a call can meet, n_frames + 2 H, plus the lengths and the window's waveform
        inner = lib.dex_voc_ragged_workspace_bytes(a, 2, 16 + 2 * H)
        hop = lib.dex_voc_samples(a, 1)
        assert inner + 2 * (16 + 2 * H) * hop * 4 <= ws <= inner + 2 * (16 + 2 * H) * hop * 4 + 1024
        assert lib.dex_voc_window_workspace_bytes(a, 2, 17) > ws > lib.dex_voc_window_workspace_bytes(a, 1, 16)
        for B, n in [(0, 16), (-1, 16), (2, 0), (2, -5)]:
            assert lib.dex_voc_window_workspace_bytes(a, B, n) == 0, (B, n)
        # bounded: a 64-frame window of a T = 4000 utterance needs a fraction of the whole call's workspace
        assert lib.dex_voc_window_workspace_bytes(a, 1, 64) < lib.dex_voc_workspace_bytes(a, 1, 4000) // 10
    assert lib.dex_voc_halo_frames(None) == 0


def test_halo_of_the_shipped_models():
    """The derivation of DESIGN.md 4.x by hand.  HiFi-GAN V1: conv_post 3; per stage the k = 11 ResBlock, 5 (1 + 3 + 5) + 3 * 5 = 60;
    63 -> ConvTranspose1d(4, 2): 32 -> 92 -> 47 -> 107 -> ConvTranspose1d(16, 8): 14 -> 74 -> 10; conv_pre 3: 13 frames.  BigVGAN adds 5
    per anti-aliased activation (6 per ResBlock, 1 in front of conv_post): 8, 98 -> 50 -> 140 -> 71 -> 161 -> 21 -> 111 -> 15, 18 frames."""
    assert V.Generator(V.AttrDict(V.HIFIGAN_V1)).halo_frames == 13
    assert V.Generator(V.AttrDict(V.BIGVGAN_BASE)).halo_frames == 18
    assert V.Generator(V.AttrDict(SMALL["snakebeta_242"])).halo_frames == 67
    assert V.Generator(V.AttrDict(V.BIGVGAN_22KHZ)).halo_frames == 38


@pytest.mark.parametrize("name", list(GEOM))
def test_halo_is_sufficient_on_the_cpu_oracle(name, golden_threads):
    h, hop, H = GEOM[name], hop_of(name), halo_of(name)
    T = 96 if hop == 256 else 208
    t0, n = T // 2 - 16, 32
    assert t0 > H and t0 + n + H <= T                              # an interior window: both edges are artificial
    mel = mel_input("window_mel", 2, T, 93)
    whole = oracle(weights_of(name), h, mel)
    lo, hi = t0 - H, t0 + n + H
    part = oracle(weights_of(name), h, np.ascontiguousarray(mel[:, :, lo:hi]))
    d = np.abs(part[:, :, (t0 - lo) * hop:(t0 - lo + n) * hop] - whole[:, :, t0 * hop:(t0 + n) * hop]).max()
    print(f"{name}: H = {H}, window oracle against whole oracle, max|d| = {d:.3e}")
    assert d <= 1e-6, float(d)


@pytest.mark.parametrize("name", list(GEOM))
def test_halo_is_not_wasteful(name, golden_threads):
    h, hop, H = GEOM[name], hop_of(name), halo_of(name)
    T, f = 2 * H + 9, H + 4                                         # H + 4 frames on each side of frame f: the extent is not cut by an edge
    mel = mel_input("halo_mel", 1, T, 7)
    a = oracle(weights_of(name), h, mel)[0, 0]
    mel[:, :, f] += 1.0
    b = oracle(weights_of(name), h, mel)[0, 0]
    nz = np.nonzero(a != b)[0]
    left, right = int(f * hop - nz[0]), int(nz[-1] + 1 - (f + 1) * hop)
    print(f"{name}: H = {H} ({H * hop} samples), measured extent left {left} / right {right} samples, "
          f"ratio (H hop - hop) / left = {(H * hop - hop) / left:.3f}")
    assert 0 < nz[0] and nz[-1] < T * hop - 1
    assert H * hop >= left and H * hop >= right, (H * hop, left, right)
    assert H * hop <= FACTOR[name] * left + hop, (H * hop, left, FACTOR[name])
