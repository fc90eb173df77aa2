"""CPU: the float64 restatement of the speaker-similarity path (tests/speaker_ref.py) is what it says it is, and the host side of
dex_tts_amd/speaker.py (slice arithmetic, checkpoint key handling, the C ABI's host-only entry points) needs no device."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from dex_tts_amd import _lib, speaker
from tests import speaker_ref as R


@pytest.fixture(scope="module")
def sd():
    return R.make_weights(0)


def _torch_net(sd, dtype):
    lstm = torch.nn.LSTM(R.N_MELS, R.H, R.LAYERS, batch_first=True).to(dtype)
    lin = torch.nn.Linear(R.H, R.H).to(dtype)
    lstm.load_state_dict({k[len("lstm."):]: torch.from_numpy(v).to(dtype) for k, v in sd.items() if k.startswith("lstm.")})
    lin.load_state_dict({k[len("linear."):]: torch.from_numpy(v).to(dtype) for k, v in sd.items() if k.startswith("linear.")})
    return lstm, lin


def test_restated_network_is_torch_lstm(sd):
    """Same weights, float64: the hand-written LSTM + Linear + ReLU + L2 norm against torch.nn.LSTM + Linear to 1e-12 - the gate order
    i | f | g | o and both biases are right."""
    lstm, lin = _torch_net(sd, torch.float64)
    mels = R.mel_like(5, 23, 1)
    with torch.no_grad():
        _, (h, _) = lstm(torch.from_numpy(mels).double())
        raw = torch.relu(lin(h[-1]))
        want = (raw / torch.norm(raw, dim=1, keepdim=True)).numpy()
    got = R.forward(sd, mels)
    assert np.linalg.norm(R.forward_raw(sd, mels), axis=1).min() > R.MIN_RAW_NORM
    assert np.abs(got - want).max() <= 1e-12


def test_synthetic_weights_give_well_conditioned_embeddings(sd):
    raw = R.forward_raw(sd, R.mel_like(4, 160, 2))
    norms = np.linalg.norm(raw, axis=1)
    assert (norms > R.MIN_RAW_NORM).all()
    assert 0.2 < (raw > 0).mean() < 0.8


@pytest.mark.parametrize("n, n_slices, last_cov, padded", [(14400, 1, 0.5625, 25600), (40000, 2, None, 40000), (44800, 3, 0.79, 50240)])
def test_partial_slices_by_hand(n, n_slices, last_cov, padded):
    """14 400 samples: 91 frames -> steps 9 -> one slice [0, 160), kept although it covers 0.56 (it is the only one), wav padded to
    25 600.  40 000: 251 frames -> steps 169 -> starts 0, 77, 154; the last covers (40000 - 24640) / 25600 = 0.60 < 0.75 and is
    dropped; the second ends at 37 920 <= 40 000: no padding.  44 800: 281 frames -> steps 199 -> starts 0, 77, 154; the last covers
    (44800 - 24640) / 25600 = 0.7875 and stays, ending at 50 240."""
    for fn in (speaker.compute_partial_slices, R.compute_partial_slices):
        wav_slices, mel_slices = fn(n)
        as_pair = lambda s: (s.start, s.stop) if isinstance(s, slice) else tuple(s)
        wav_slices, mel_slices = [as_pair(s) for s in wav_slices], [as_pair(s) for s in mel_slices]
        assert len(mel_slices) == n_slices
        assert mel_slices == [(77 * i, 77 * i + 160) for i in range(n_slices)]
        assert wav_slices == [(160 * a, 160 * b) for a, b in mel_slices]
        assert max(n, wav_slices[-1][1]) == padded
        if last_cov is not None:
            assert abs((n - wav_slices[-1][0]) / 25600 - last_cov) < 5e-3
    assert int(round(16000 / 1.3 / 160)) == 77


def test_slices_refuse_bad_arguments():
    for bad in (dict(n_samples=0), dict(n_samples=100, min_coverage=0.0), dict(n_samples=100, rate=0.1)):
        with pytest.raises(ValueError):
            speaker.compute_partial_slices(**bad)


def test_mel_of_a_tone_peaks_in_its_band_and_obeys_parseval():
    n = 16000
    t = np.arange(n) / R.SR
    f = 1000.0
    wav = (0.3 * np.sin(2 * np.pi * f * t)).astype(np.float32)
    mel = R.wav_to_mel_spectrogram(wav)
    assert mel.shape == (1 + n // 160, 40)
    basis = R.mel_basis()
    want_band = int(np.argmax(basis[:, int(round(f * R.N_FFT / R.SR))]))
    assert (np.argmax(mel[5:-5], axis=1) == want_band).all()
    # Parseval per frame: sum_k' |X_k'|^2 over all 400 bins = 400 sum_n x_n^2; the one-sided spectrum counts 1 .. 199 twice
    fr = R.frames(wav)
    pw = R.power_spectrogram(wav)
    two_sided = pw[:, 0] + pw[:, 200] + 2.0 * pw[:, 1:200].sum(axis=1)
    energy = R.N_FFT * (fr ** 2).sum(axis=1)
    assert np.abs(two_sided - energy).max() <= 1e-9 * energy.max()


def test_mel_frame_count_and_zero_padding():
    for n in (159, 160, 401):
        assert R.wav_to_mel_spectrogram(np.ones(n, np.float32)).shape == (1 + n // 160, 40)
    wav = R.synth_wav(1000, 3)
    a = R.wav_to_mel_spectrogram(wav, n_frames=12)
    b = R.wav_to_mel_spectrogram(np.concatenate([wav, np.zeros(1000, np.float32)]))[:12]
    assert np.abs(a - b).max() <= 1e-13 * a.max()            # (two matrix products of different heights: BLAS may order the sums differently)


def test_normalize_volume():
    loud = R.synth_wav(8000, 4, amp=0.5)
    assert 10 * np.log10(np.mean(loud.astype(np.float64) ** 2)) > -30
    out = R.normalize_volume(loud)
    assert out.dtype == np.float32 and np.array_equal(out, loud)                      # bit-identical
    quiet = R.synth_wav(8000, 5, amp=0.001)
    out = R.normalize_volume(quiet)
    assert out.dtype == np.float32
    assert abs(10 * np.log10(np.mean(out.astype(np.float64) ** 2)) + 30.0) < 1e-5


def test_asv_score_is_mean_and_population_stderr():
    cos = np.array([0.5, 0.7, 0.9, 0.7])
    m, se = R.asv_score(cos)
    assert m == pytest.approx(0.7) and se == pytest.approx(math.sqrt(0.02) / 2)


def test_state_dict_routing(sd):
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    want = set(speaker.state_dict_shapes())
    assert want == set(sd) and len(want) == 14
    assert set(speaker.route_state_dict(tsd)) == want
    with_loss = dict(tsd, similarity_weight=torch.tensor([10.0]), similarity_bias=torch.tensor([-5.0]))
    assert set(speaker.route_state_dict(with_loss)) == want                            # the training loss's parameters are ignored
    assert set(speaker.route_state_dict({"model_state": with_loss, "step": 3, "optimizer_state": {}})) == want
    missing = dict(tsd); del missing["lstm.bias_hh_l2"]
    with pytest.raises(RuntimeError, match="missing"):
        speaker.route_state_dict(missing)
    with pytest.raises(RuntimeError, match="unexpected"):
        speaker.route_state_dict(dict(tsd, **{"lstm.weight_ih_l3": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="shape"):
        speaker.route_state_dict(dict(tsd, **{"linear.bias": torch.zeros(255)}))


def test_cpu_tensors_are_refused_without_a_device():
    wav = torch.zeros(1000)
    for fn in (speaker.normalize_volume, speaker.wav_to_mel_spectrogram, speaker.preprocess_wav):
        with pytest.raises(ValueError, match="CUDA"):
            fn(wav)
    with pytest.raises(ValueError, match="CUDA"):
        speaker.cosine(torch.zeros(2, 256), torch.zeros(2, 256))
    with pytest.raises(ValueError):
        speaker.speaker_similarity(wav, wav)                                             # no encoder
    with pytest.raises(ValueError):
        speaker.VoiceEncoder("cpu")


def test_cabi_host_side():
    """The dex_spk_* entry points that need no device: the workspace plan, and the refusal of a null handle by every compute call."""
    if not os.path.exists(_lib.LIB_PATH):
        from dex_tts_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    for name in ("dex_spk_create", "dex_spk_destroy", "dex_spk_last_error", "dex_spk_load", "dex_spk_workspace_bytes",
                 "dex_spk_forward_workspace_bytes", "dex_spk_mel", "dex_spk_forward", "dex_spk_embed", "dex_spk_normalize_volume",
                 "dex_spk_cosine"):
        assert hasattr(lib, name), name
    assert lib.dex_spk_forward_workspace_bytes(0, 160) == 0 and lib.dex_spk_forward_workspace_bytes(4, 0) == 0
    assert lib.dex_spk_forward_workspace_bytes(1 << 20, 160) == 0                        # more rows x frames than one call takes
    assert lib.dex_spk_workspace_bytes(4, 0) == 0
    one = lib.dex_spk_forward_workspace_bytes(1, 160)
    assert one >= 160 * (64 + 1024 + 512) * 4
    assert lib.dex_spk_workspace_bytes(10, 64000) == lib.dex_spk_forward_workspace_bytes(10, 160)
    assert 9 * one < lib.dex_spk_workspace_bytes(10, 64000) <= 10 * one
    assert lib.dex_spk_create(None) == -1
    assert b"null" in lib.dex_spk_last_error(None)
    ln = (C.c_int32 * 1)(100)
    assert lib.dex_spk_mel(None, None, ln, 1, 100, None, None) == -1
    assert lib.dex_spk_forward(None, None, 1, 1, None, None, 0, None) == -1
    assert lib.dex_spk_embed(None, None, ln, 1, 100, ln, ln, 1, None, None, None, 0, None) == -1
    assert lib.dex_spk_normalize_volume(None, None, ln, 1, 100, -30.0, None, None) == -1
    assert lib.dex_spk_cosine(None, None, None, 1, 256, None, None) == -1
    assert lib.dex_spk_load(None, b"linear.bias", None, None, 1, None) == -1
    lib.dex_spk_destroy(None)
