"""CPU: the host layer the waveform-side wrappers share (dex_tts_amd/_native.py): ``host_lengths``, ``pad_wavs``, and the refusal of
a CPU tensor by every public wav-taking entry point, under its own name and before the library is looked for.  (``audio``'s
``TacotronSTFT.mel_spectrogram`` / ``get_mel_from_wav`` take host wavs by design and ``align`` takes no wav: neither has a case.)"""
import re

import numpy as np
import pytest
import torch

from dex_tts_amd import _lib, _native, asr, f0, griffin_lim, speaker, wavprep

B, HI = 3, 7
WANT = np.array([2, 7, 1], dtype=np.int32)


@pytest.mark.parametrize("lengths", [[2, 7, 1], (2, 7, 1), np.array([2, 7, 1]), np.array([2, 7, 1], dtype=np.int16), torch.tensor([2, 7, 1]),
                                     torch.tensor([2, 7, 1], dtype=torch.int32), torch.tensor([2, 7, 1], dtype=torch.int64)],
                         ids=["list", "tuple", "ndarray", "int16", "tensor", "int32", "int64"])
def test_host_lengths_spellings_agree(lengths):
    got = _native.host_lengths(lengths, B, HI)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.flags.c_contiguous and got.shape == (B,)
    assert np.array_equal(got, WANT)


def test_host_lengths_default_and_refusals():
    got = _native.host_lengths(None, B, HI)
    assert got.dtype == np.int32 and got.flags.c_contiguous and np.array_equal(got, [HI] * B)
    for bad in ([2, 7], [2, 7, 1, 1], []):                                   # a wrong count
        with pytest.raises(ValueError, match="wav_rows"):
            _native.host_lengths(bad, B, HI, what="wav_rows")
    with pytest.raises(ValueError):
        _native.host_lengths([2, 0, 1], B, HI)                               # lo - 1
    with pytest.raises(ValueError):
        _native.host_lengths([2, HI + 1, 1], B, HI)                          # hi + 1
    assert np.array_equal(_native.host_lengths([2, 0, 1], B, HI, lo=0), [2, 0, 1])
    with pytest.raises(ValueError):
        _native.host_lengths([2, -1, 1], B, HI, lo=0)                        # lo - 1 again
    with pytest.raises(ValueError):
        _native.host_lengths(None, B, HI, lo=HI + 1)                         # the default is held to the range too
    with pytest.raises(ValueError):
        _native.host_lengths([2, 2 ** 32 + 1, 1], B, HI)                     # not wrapped into range by the int32 cast


ROWS = (np.array([0.5], dtype=np.float32), torch.tensor([0.1, -0.2, 0.3, -0.4, 1 / 3], dtype=torch.float64), np.array([-32768, 16384, 1], dtype=np.int16))


@pytest.mark.parametrize("scale", [False, True])
def test_pad_wavs(scale):
    x, ln = _native.pad_wavs(list(ROWS), "cpu", scale)
    assert x.dtype == torch.float32 and x.device.type == "cpu" and tuple(x.shape) == (3, 5)
    assert isinstance(ln, np.ndarray) and ln.dtype == np.int32 and np.array_equal(ln, [1, 5, 3])
    got = x.numpy()
    assert np.array_equal(got[0, :1], ROWS[0]) and not got[0, 1:].any()
    assert np.array_equal(got[1], ROWS[1].numpy().astype(np.float32))       # fp64 is rounded to fp32 once
    i16 = ROWS[2].astype(np.float32)
    assert np.array_equal(got[2, :3], i16 / 32768 if scale else i16) and not got[2, 3:].any()
    if scale:
        assert got[2, 0] == -1.0 and got[2, 1] == 0.5


def test_pad_wavs_refuses_empty_rows():
    with pytest.raises(ValueError):
        _native.pad_wavs([np.zeros(4, np.float32), np.zeros(0, np.float32)], "cpu")
    with pytest.raises(ValueError):
        _native.pad_wavs([], "cpu")


WAV = torch.zeros(2048)
T4 = torch.arange(4, dtype=torch.float64) * 0.005
# module, the name the message carries, the call, the class of the refusal
CASES = [
    (speaker, "normalize_volume", lambda: speaker.normalize_volume(WAV), ValueError),
    (speaker, "wav_to_mel_spectrogram", lambda: speaker.wav_to_mel_spectrogram(WAV), ValueError),
    (speaker, "preprocess_wav", lambda: speaker.preprocess_wav(WAV, 22050), ValueError),
    (asr, "normalize_input", lambda: asr.normalize_input(WAV), ValueError),
    (griffin_lim, "STFT.transform", lambda: griffin_lim.STFT().transform(WAV[None]), RuntimeError),
    (wavprep, "trim", lambda: wavprep.trim(WAV), RuntimeError),
    (wavprep, "resample", lambda: wavprep.resample(WAV, 48000, 22050), RuntimeError),
    (wavprep, "peak_normalize_f64", lambda: wavprep.peak_normalize_f64(WAV.double()), RuntimeError),
    (wavprep, "prepare", lambda: wavprep.prepare(WAV, 22050), RuntimeError),
    (wavprep, "preprocess_wav", lambda: wavprep.preprocess_wav(WAV, 22050), RuntimeError),
    (f0, "dio", lambda: f0.dio(WAV, 22050), RuntimeError),
    (f0, "stonemask", lambda: f0.stonemask(WAV, torch.zeros(4), T4, 22050), RuntimeError),
    (f0, "peak_normalize", lambda: f0.peak_normalize(WAV), RuntimeError),
    (f0, "reference_features", lambda: f0.reference_features(WAV), RuntimeError),
]


@pytest.mark.parametrize("module,name,call,refusal", CASES, ids=[f"{m.__name__.split('.')[-1]}.{n}" for m, n, _, _ in CASES])
def test_cpu_tensor_is_refused_under_the_entry_points_own_name(module, name, call, refusal, monkeypatch):
    def no_library():
        raise AssertionError("the library was looked for before the CPU tensor was refused")
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(refusal, match="CUDA") as e:
        call()
    assert type(e.value) is refusal
    msg = str(e.value)
    assert msg.startswith(name + " "), msg
    others = {n for m, n, _, _ in CASES if m is not module and n != name}
    named = [n for n in others if re.search(rf"(?<![\w.]){re.escape(n)}(?!\w)", msg)]
    assert not named and "f0 tracker" not in msg and "alignment search" not in msg, msg
