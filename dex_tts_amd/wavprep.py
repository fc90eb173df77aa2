"""The reference wav preparation of DEX-TTS/synthesize.py:40-62 (``preprocess_wav``) on the device: ``read_wav`` (sf.read), ``trim``
(librosa.effects.trim, top_db = 30), ``resample`` (resampy.resample with kaiser_best) and ``preprocess_wav``, the whole function for
a ragged, mixed-rate batch: wav(s) at any sample rate -> the style inputs of ``DeXTTS.forward``.  The arithmetic runs in
libdexamd.so (``dex_wav_trim`` / ``dex_wav_resample`` / ``dex_wav_peak_normalize_f64``, csrc/wavprep.hip), fp64, then the mel and
the f0 tracker of dex_tts_amd.f0.  The contract is the docstring of tests/wav_prep.py; parity with librosa 0.9.2 and resampy
themselves is not measured.  There is no CPU path.

Wavs reach the kernels as fp32 CUDA tensors, as in the f0 ABI: exact for 8-, 16- and 24-bit PCM; 32-bit PCM and float64 files are
rounded to fp32 once on the way in."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from . import f0 as F0
from ._native import check, device_rows, host_lengths, i32_ptr, pad_wavs, per_device, stream

SR = F0.SR


def read_wav(path):
    """sf.read(path) for a mono WAV -> (float64 ndarray, sample rate), scaled as soundfile scales a float64 read: int16 / 2^15,
    int32 (scipy's left-justified 24-bit included) / 2^31, uint8 (v - 128) / 128, float passed through."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.ndim != 1:
        raise ValueError(f"{path}: {data.shape[1]} channels; only mono wavs are supported")
    if data.dtype == np.int16:
        x = data.astype(np.float64) / 32768.0
    elif data.dtype == np.int32:
        x = data.astype(np.float64) / 2147483648.0
    elif data.dtype == np.uint8:
        x = (data.astype(np.float64) - 128.0) / 128.0
    elif data.dtype in (np.float32, np.float64):
        x = data.astype(np.float64)
    else:
        raise ValueError(f"{path}: unsupported sample type {data.dtype}")
    return x, int(sr)


def _trim_opts(top_db, frame_length, hop_length, pad_mode):
    if pad_mode not in _lib.WAV_PAD:
        raise ValueError(f"pad_mode must be one of {sorted(_lib.WAV_PAD)}, got {pad_mode!r}")
    return _lib.DexWavTrimOpts(float(top_db), int(frame_length), int(hop_length), _lib.WAV_PAD[pad_mode])


def _rates(sr, B):
    """One sample rate, or one per row -> host int32 [B] of positive rates."""
    return host_lengths(np.full(B, sr) if np.ndim(sr) == 0 else sr, B, np.iinfo(np.int32).max, what="sample rates")


def trim(wav, lengths=None, top_db=30.0, frame_length=2048, hop_length=512, pad_mode="constant", return_mse=False):
    """librosa.effects.trim(wav, top_db)[1] per row: wav [L] or [B, L] (a CUDA tensor; rows of ``lengths`` samples) -> bounds
    [2] or [B, 2] int32 on the device, (start, end) of the non-silent part.  return_mse: also each frame's mean square, float64
    [F] or [B, F] with F = 1 + L // hop_length (0 past a row's own frames)."""
    x, ln, one = device_rows(wav, lengths, "trim")
    lib = _lib.load()
    B, L = x.shape
    o = _trim_opts(top_db, frame_length, hop_length, pad_mode)
    need = int(lib.dex_wav_trim_workspace_bytes(B, i32_ptr(ln), C.byref(o)))
    if need == 0:
        raise ValueError("dex_wav_trim_workspace_bytes rejected the arguments")
    with torch.cuda.device(x.device):
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        bounds = torch.empty(B, 2, dtype=torch.int32, device=x.device)
        mse = torch.empty(B, 1 + L // int(hop_length), dtype=torch.float64, device=x.device) if return_mse else None
        check(lib.dex_wav_trim(x.data_ptr(), i32_ptr(ln), B, L, C.byref(o), bounds.data_ptr(),
                               mse.data_ptr() if return_mse else None, ws.data_ptr(), need, stream(x.device)), "dex_wav_trim")
    if return_mse:
        return (bounds[0], mse[0]) if one else (bounds, mse)
    return bounds[0] if one else bounds


def resampled_length(n_samples, sr_orig, sr_new):
    """(n_samples * sr_new) div sr_orig; ValueError if that is < 1."""
    n = _lib.load().dex_wav_resampled_length(int(n_samples), int(sr_orig), int(sr_new))
    if n < 1:
        raise ValueError(f"{n_samples} samples at {sr_orig} Hz give no sample at {sr_new} Hz")
    return n


@per_device
def _table(dev):
    """The kaiser_best window table of one device, built once (dex_wav_resample_table) and kept."""
    lib = _lib.load()
    need = int(lib.dex_wav_resample_table_bytes(None))
    with torch.cuda.device(dev):
        tab = torch.empty(need, dtype=torch.uint8, device=dev)
        check(lib.dex_wav_resample_table(None, tab.data_ptr(), need, stream(dev)), "dex_wav_resample_table")
        torch.cuda.current_stream(dev).synchronize()          # ready for calls on any stream
    return tab


def _resample(x, offsets, lengths, srs, sr_new):
    """x fp32 [B, Ls] (device), host int32 offsets / lengths / rates -> (fp64 [B, max L_out] on the device, host int32 L_out)."""
    lib = _lib.load()
    B, Ls = x.shape
    lo = np.array([resampled_length(int(n), int(s), sr_new) for n, s in zip(lengths, srs)], dtype=np.int32)
    Lm = int(lo.max())
    tab = _table(x.device)
    with torch.cuda.device(x.device):
        y = torch.empty(B, Lm, dtype=torch.float64, device=x.device)
        check(lib.dex_wav_resample(x.data_ptr(), Ls, i32_ptr(offsets), i32_ptr(lengths), i32_ptr(srs), B, int(sr_new), None, y.data_ptr(), Lm,
                                   tab.data_ptr(), tab.numel(), stream(x.device)), "dex_wav_resample")
    return y, lo


def resample(wav, sr_orig, sr_new, lengths=None, offsets=None):
    """resampy.resample(wav, sr_orig, sr_new) (kaiser_best) per row, in fp64: wav [L] or [B, L] (a CUDA tensor); row b reads
    ``lengths[b]`` samples from ``offsets[b]`` (default 0) at ``sr_orig`` Hz (an int or one per row) -> (y, lengths_out): y [L_out]
    or [B, max L_out] float64 on the device (0 past a row's length), lengths_out a host int32 array.  A row already at sr_new is
    copied."""
    x, ln, one = device_rows(wav, lengths, "resample")
    B, L = x.shape
    off = np.zeros(B, np.int32) if offsets is None else host_lengths(offsets, B, L - 1, lo=0, what="resample offsets")
    if (off.astype(np.int64) + ln > L).any():
        raise ValueError(f"resample: offsets / lengths must describe B = {B} non-empty spans inside rows of {L} samples")
    if int(sr_new) <= 0:
        raise ValueError(f"sr_new must be positive, got {sr_new}")
    y, lo = _resample(x, off, ln, _rates(sr_orig, B), int(sr_new))
    return (y[0], lo) if one else (y, lo)


def peak_normalize_f64(y, lengths=None):
    """synthesize.py:46 on fp64 rows: y [L] or [B, L] (a CUDA tensor; promoted to float64 if it is not), rows of ``lengths`` samples
    -> float(y / max|y|) fp32 of y's shape (0 past a row's length and for a silent row)."""
    y, ln, one = device_rows(y, lengths, "peak_normalize_f64", dtype=torch.float64)
    lib = _lib.load()
    B, L = y.shape
    need = int(lib.dex_wav_peak_workspace_bytes(B, L))
    with torch.cuda.device(y.device):
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=y.device)
        out = torch.empty(B, L, dtype=torch.float32, device=y.device)
        check(lib.dex_wav_peak_normalize_f64(y.data_ptr(), i32_ptr(ln), B, L, out.data_ptr(), ws.data_ptr(), need, stream(y.device)),
              "dex_wav_peak_normalize_f64")
    return out[0] if one else out


def _load(paths):
    rows, srs = zip(*(read_wav(p) for p in paths))
    x, ln = pad_wavs(rows, torch.device("cuda", torch.cuda.current_device()))
    return x, ln, list(srs)


def _prepare(wav, sr, lengths, top_db, pad_mode, what):
    if isinstance(wav, (str, os.PathLike)) or (isinstance(wav, (list, tuple)) and wav and isinstance(wav[0], (str, os.PathLike))):
        wav, lengths, sr = _load([wav] if isinstance(wav, (str, os.PathLike)) else list(wav))
    elif sr is None:
        raise ValueError(f"{what}: pass the sample rate of the tensor's rows")
    x, ln, _ = device_rows(wav, lengths, what)
    B = x.shape[0]
    srs = _rates(sr, B)
    bounds = trim(x, ln, top_db=top_db, pad_mode=pad_mode).cpu().numpy().reshape(B, 2)
    y, lo = _resample(x, np.ascontiguousarray(bounds[:, 0]), bounds[:, 1] - bounds[:, 0], srs, SR)
    return peak_normalize_f64(y, lo), lo


def prepare(wav, sr=None, lengths=None, top_db=30.0, pad_mode="constant"):
    """synthesize.py:41-46 on the device: ``wav`` as for ``preprocess_wav`` -> (xn, lengths): the trimmed, resampled (to 22050 Hz
    where the rate differs) and peak-normalised rows as fp32 [B, max length] on the device (computed in fp64, rounded once; 0 past a
    row's length) and their host int32 lengths.  The one host synchronisation reads the trim bounds back."""
    return _prepare(wav, sr, lengths, top_db, pad_mode, "prepare")


def preprocess_wav(wav, sr=None, lengths=None, stft=None, top_db=30.0, pad_mode="constant"):
    """synthesize.py:40-62 (preprocess_wav) on the device for a ragged, mixed-rate batch.  ``wav`` is a path, a list of paths (mono
    WAVs, read with ``read_wav``; their rates are the files') or a CUDA tensor [L] / [B, L] of rows of ``lengths`` samples at ``sr``
    Hz (an int or one per row).  Trim at the source rate, resample to 22050 Hz in fp64 where the rate differs, peak-normalise in fp64,
    round to fp32 once (``prepare``), then the mel and the f0 tracker -> the dict of ``dex_tts_amd.f0.reference_features`` (which
    DeXTTS.forward / synthesize_tokens(style=...) take)."""
    return F0.features(*_prepare(wav, sr, lengths, top_db, pad_mode, "preprocess_wav"), stft)
