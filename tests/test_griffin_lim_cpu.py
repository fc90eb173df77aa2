"""CPU: the float64 restatement of the reference's Griffin-Lim path (tests/griffin_lim.py) against the reference's goldens
(tests/golden/griffin_lim.npz, tools/make_golden_griffin_lim.py), the new C ABI bindings, and the refusals that happen before any
device work (configuration, frame counts, CPU tensors)."""
import os

import numpy as np
import pytest
import torch

from dex_tts_amd import _lib
from dex_tts_amd import griffin_lim as G
from tests import griffin_lim as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "griffin_lim.npz")))


@pytest.fixture(scope="module")
def mels(golden_dir):
    d = np.load(os.path.join(golden_dir, "audio_mel.npz"))
    return {"s1": d["sample1_1s_mel"], "chirp": d["chirp_mel"]}


@pytest.mark.parametrize("frames", [86, 62])
def test_window_sumsquare_bitwise(gold, frames):
    np.testing.assert_array_equal(R.window_sumsquare(frames), gold[f"wss_{frames}"])


@pytest.mark.parametrize("name", ["s1", "chirp"])
def test_spec_from_mel_to_fp32_rounding(gold, mels, name):
    ref = gold[f"spec_{name}"].astype(np.float64)
    got = R.spec_from_mel(mels[name])
    assert np.abs(got - ref).max() <= 4 * np.finfo(np.float32).eps * np.abs(ref).max()
    nz = np.abs(ref) > 1e-3 * np.abs(ref).max()
    assert (np.abs(got - ref)[nz] / np.abs(ref)[nz]).max() <= 4 * np.finfo(np.float32).eps


@pytest.mark.parametrize("name,n", [("s1", 0), ("s1", 1), ("chirp", 0)])
def test_griffin_lim_restatement_matches_reference(gold, name, n):
    np.random.seed(int(gold["seed"]))
    drawn = np.angle(np.exp(2j * np.pi * np.random.rand(*gold[f"angles_{name}"].shape))).astype(np.float32)
    np.testing.assert_array_equal(drawn, gold[f"angles_{name}"])            # the recorded angles are the seeded draw
    x = R.griffin_lim(gold[f"spec_{name}"][:, :-1], gold[f"angles_{name}"], n)[0]
    assert x.shape == gold[f"gl{n}_{name}"].shape
    assert np.abs(x - gold[f"gl{n}_{name}"]).max() <= 1e-5


def test_transform_and_round_trip_restatement(gold):
    mag, phase = R.transform(gold["wav"])
    assert np.abs(mag[0] - gold["wav_mag"]).max() <= 1e-5 * gold["wav_mag"].max()
    inv = R.inverse(mag, phase)[0]
    assert inv.shape == gold["wav_inv"].shape == (256 * (gold["wav"].size // 256),)
    assert np.abs(inv - gold["wav_inv"]).max() <= 1e-5


def test_sixty_iterations_converge_like_reference(gold):
    S = gold["spec_s1"][:, :-1]
    x = R.griffin_lim(S, gold["angles_s1"], 60)[0]
    sc = R.spectral_convergence(S, x)
    assert abs(sc - float(gold["sc60_s1"])) <= 0.01 * float(gold["sc60_s1"])


def test_symbols_bound():
    names = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("dex_gl_create", "dex_gl_destroy", "dex_gl_last_error", "dex_gl_workspace_bytes", "dex_stft_transform", "dex_stft_inverse",
              "dex_griffin_lim", "dex_mel_to_linear"):
        assert n in names, n
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.dex_gl_workspace_bytes(0, 10) == 0 and lib.dex_gl_workspace_bytes(2, 0) == 0
        assert lib.dex_gl_workspace_bytes(2, 100) >= 2 * 100 * (1024 + 513) * 4
        assert lib.dex_griffin_lim(None, None, None, None, 1, 4, 0, None, None, 0, None) == -1


@pytest.mark.parametrize("cfg", [(2048, 256, 1024, "hann"), (1024, 512, 1024, "hann"), (1024, 256, 800, "hann"), (1024, 256, 1024, "hamming")])
def test_other_configurations_refused(cfg):
    with pytest.raises(ValueError):
        G.STFT(*cfg)


def test_refusals_before_device_work():
    stft = G.STFT(1024, 256, 1024)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError):                                  # fewer than 4 frames: the reference's reflect pad fails there
        G.griffin_lim(torch.ones(1, 513, 3), stft, 1)
    with pytest.raises(ValueError):
        G.griffin_lim(torch.ones(1, 513, 8), stft, -1)
    with pytest.raises(ValueError):
        G.mel_to_wav(torch.zeros(1, 80, 4))
    with pytest.raises(ValueError):
        G.mel_to_wav(torch.zeros(2, 80, 20), lengths=[20, 21])
    np.testing.assert_array_equal(np.random.get_state()[1], state)   # nothing drawn
    with pytest.raises(RuntimeError):
        G.griffin_lim(torch.ones(1, 513, 8), stft, 1)
    with pytest.raises(RuntimeError):
        stft.transform(torch.zeros(1, 2048))
    with pytest.raises(RuntimeError):
        stft.inverse(torch.ones(1, 513, 8), torch.zeros(1, 513, 8))
    with pytest.raises(RuntimeError):
        G.mel_to_wav(torch.zeros(1, 80, 20))
    with pytest.raises(RuntimeError):
        G.mel_to_linear(torch.zeros(1, 80, 20))
    np.testing.assert_array_equal(np.random.get_state()[1], state)
