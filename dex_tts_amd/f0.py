"""The DEX f0 front-end on the device: pyworld's call surface for WORLD's DIO + StoneMask (``dio`` / ``stonemask``, the arguments
DEX-TTS/synthesize.py:50-52 passes) and ``reference_features``, synthesize.py's ``preprocess_wav`` (:41-60) without the trim and the
resampler: a 22050 Hz reference wav -> the style inputs of ``DeXTTS.forward``.  The arithmetic runs in libdexamd.so
(``dex_f0_dio`` / ``dex_f0_stonemask`` / ``dex_f0_peak_normalize``, csrc/f0.hip), fp64, for a ragged batch in one call.  The
contract is the docstring of tests/world_f0.py; parity with pyworld itself is not measured.  There is no CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._native import check, device_rows, i32_ptr, per_device, stream
from .audio import TacotronSTFT, lf0_from_f0

SR = 22050
HOP = 256


def _opts(fs, frame_period, f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0, allowed_range=0.1):
    return _lib.DexF0Opts(float(fs), float(frame_period), float(f0_floor), float(f0_ceil), float(channels_in_octave), float(allowed_range))


def frames(n_samples, fs=SR, frame_period=HOP / SR * 1000.0):
    """F of the contract: int(1000 L / fs / frame_period) + 1."""
    return int(_lib.load().dex_f0_frames(int(n_samples), C.byref(_opts(fs, frame_period))))


def dio(x, fs, f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0, frame_period=5.0, speed=1, allowed_range=0.1, lengths=None):
    """pw.dio on the device: x [L] or [B, L] (a CUDA tensor; fp32 on the device, promoted to fp64 exactly) -> (f0, t), f0 [F] or
    [B, F] float64 with F = frames(L), 0 past each row's own frame count; t [F] float64 = i * frame_period / 1000."""
    if speed != 1:
        raise ValueError("only speed = 1 is built (DIO's decimation is not)")
    x, ln, one = device_rows(x, lengths, "dio")
    lib = _lib.load()
    B, L = x.shape
    o = _opts(fs, frame_period, f0_floor, f0_ceil, channels_in_octave, allowed_range)
    F = lib.dex_f0_frames(L, C.byref(o))
    check(F if F < 0 else 0, "dex_f0_frames")
    need = int(lib.dex_f0_workspace_bytes(B, i32_ptr(ln), C.byref(o)))
    if need == 0:
        raise ValueError("dex_f0_workspace_bytes rejected the arguments")
    with torch.cuda.device(x.device):
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        f0 = torch.empty(B, F, dtype=torch.float64, device=x.device)
        check(lib.dex_f0_dio(x.data_ptr(), i32_ptr(ln), B, L, C.byref(o), f0.data_ptr(), ws.data_ptr(), need, stream(x.device)),
              "dex_f0_dio")
    t = torch.from_numpy(np.arange(F) * float(frame_period) / 1000.0).to(x.device)    # the contract's t_i, rounded as on the host
    return (f0[0] if one else f0), t


def stonemask(x, f0, t, fs, lengths=None, frame_period=None):
    """pw.stonemask on the device: x as for ``dio``, f0 [F] / [B, F] from ``dio``, t its frame times (i * frame_period / 1000;
    frame_period is taken from t unless given) -> refined f0 of f0's shape, float64."""
    x, ln, one = device_rows(x, lengths, "stonemask")
    lib = _lib.load()
    B, L = x.shape
    t = torch.as_tensor(t, dtype=torch.float64).cpu().reshape(-1)
    if frame_period is None:
        if t.numel() < 2:
            raise ValueError("pass frame_period when t has fewer than 2 frames")
        frame_period = float(t[1]) * 1000.0
    if not torch.allclose(t, torch.arange(t.numel(), dtype=torch.float64) * frame_period / 1000.0, rtol=1e-12, atol=1e-12):
        raise ValueError("t must be the uniform frame times i * frame_period / 1000 that dio returns")
    o = _opts(fs, frame_period)
    F = lib.dex_f0_frames(L, C.byref(o))
    check(F if F < 0 else 0, "dex_f0_frames")
    f0 = torch.as_tensor(f0)
    f0 = (f0.reshape(1, -1) if f0.dim() == 1 else f0).to(device=x.device, dtype=torch.float64).contiguous()
    if f0.shape != (B, F):
        raise ValueError(f"f0 must be [{B}, {F}] for {L} samples, got {tuple(f0.shape)}")
    with torch.cuda.device(x.device):
        out = torch.empty_like(f0)
        check(lib.dex_f0_stonemask(x.data_ptr(), i32_ptr(ln), B, L, C.byref(o), f0.data_ptr(), out.data_ptr(), None, 0,
                                   stream(x.device)), "dex_f0_stonemask")
    return out[0] if one else out


def peak_normalize(x, lengths=None):
    """synthesize.py:46 ``wav / max(abs(wav))`` per row, in fp64 on the device, rounded to fp32 (0 past a row's length)."""
    x, ln, one = device_rows(x, lengths, "peak_normalize")
    lib = _lib.load()
    B, L = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty_like(x)
        check(lib.dex_f0_peak_normalize(x.data_ptr(), i32_ptr(ln), B, L, out.data_ptr(), stream(x.device)), "dex_f0_peak_normalize")
    return out[0] if one else out


_stft = per_device(lambda dev: TacotronSTFT(device=dev))     # one mel front-end per device (its DFT basis and filterbank are built once)


def reference_features(wav, lengths=None, sr=SR, stft: TacotronSTFT = None):
    """synthesize.py:41-60 (preprocess_wav) after the trim and the resampler, which stay the caller's: wav [L] or [B, L] (a CUDA
    tensor, trimmed, at 22050 Hz; rows of ``lengths`` samples) -> the dict DeXTTS.forward / synthesize_tokens(style=...) take:
    ref / sty [B, 80, Tr] (the mel of the peak-normalised wav), ref_lengths / sty_lengths [B] (L // 256 + 1), lf0 [B, Tl]
    (normalize_lf0(log f0[:tlen]) with tlen = min(F, mel frames)) and lf0_lengths [B]; lengths are int64 on the device.
    dex_tts_amd.wavprep.preprocess_wav does the trim and the resampler too."""
    if sr != SR:
        raise ValueError(f"reference_features needs {SR} Hz audio (there is no resampler), got {sr}")
    x, ln, _ = device_rows(wav, lengths, "reference_features")
    return features(peak_normalize(x, ln), ln, stft)


def features(xn, ln, stft: TacotronSTFT = None):
    """The mel / f0 / lf0 tail of preprocess_wav (synthesize.py:47-60) on peak-normalised fp32 rows xn [B, L] (a CUDA tensor) of host
    int32 lengths ln -> the dict reference_features returns."""
    B, L = xn.shape
    dev = xn.device
    stft = stft if stft is not None else _stft(dev)
    lib = _lib.load()
    fp = HOP / SR * 1000.0
    f0, t = dio(xn, SR, frame_period=fp, lengths=ln)
    f0 = stonemask(xn, f0, t, SR, lengths=ln, frame_period=fp)
    mel_frames = [lib.dex_mel_frames(int(n)) for n in ln]
    tlen = [min(frames(int(n), SR, fp), m) for n, m in zip(ln, mel_frames)]
    Tr, Tl = max(mel_frames), max(tlen)
    with torch.cuda.device(dev):
        mel = torch.zeros(B, 80, Tr, dtype=torch.float32, device=dev)
        for n in sorted(set(int(v) for v in ln)):          # the mel's reflect padding is per utterance: one pass per length
            rows = torch.from_numpy(np.nonzero(ln == n)[0]).to(dev)
            mel[rows, :, : lib.dex_mel_frames(n)] = stft._run(xn[rows, :n])[0]
        mask = torch.arange(Tl, device=dev)[None, :] < torch.tensor(tlen, device=dev)[:, None]
        f0c = torch.where(mask, f0[:, :Tl], torch.zeros((), dtype=f0.dtype, device=dev)).to(torch.float32).contiguous()
        lf0_len = torch.tensor(tlen, dtype=torch.int64, device=dev)
        lf0 = lf0_from_f0(f0c, lf0_len)
        mel_len = torch.tensor(mel_frames, dtype=torch.int64, device=dev)
    return {"ref": mel, "ref_lengths": mel_len, "sty": mel, "sty_lengths": mel_len.clone(), "lf0": lf0, "lf0_lengths": lf0_len}
