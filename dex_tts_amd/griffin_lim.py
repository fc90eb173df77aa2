"""Griffin-Lim mel inversion on the device: the reference's only mel -> waveform path that needs no vocoder checkpoint
(audio/tools.py:18-34 ``inv_mel_spec`` -> audio/audio_processing.py:66-82 ``griffin_lim`` -> audio/stft.py:52-121 ``STFT``).

    STFT(filter_length, hop_length, win_length, window="hann")   transform(y) -> (magnitude, phase), inverse(magnitude, phase), forward
    griffin_lim(magnitudes, stft_fn, n_iters=30, angles=None)
    inv_mel_spec(mel, out_filename, _stft, griffin_iters=60)       writes the wav with scipy.io.wavfile.write, as the reference does
    mel_to_linear(mel, lengths=None)                                spec_from_mel[:, :, :-1] of inv_mel_spec for a ragged batch
    mel_to_wav(mel, lengths=None, n_iters=60, angles=None)          inv_mel_spec's waveform for a ragged batch

Every frame is a 1024-point real FFT in LDS (``csrc/griffin_lim.hip``, C ABI ``dex_gl_*``, ``dex_stft_*``, ``dex_griffin_lim``,
``dex_mel_to_linear``).  Only the reference configuration is built: filter_length 1024, hop 256, win_length 1024, periodic Hann,
80 Slaney mels at 22050 Hz; anything else raises ``ValueError``.  Tensors must be on an MI355X: CPU tensors raise ``RuntimeError``
(there is no CPU path).  Arguments are checked before anything touches the device or the random stream.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._native import Handle, device_rows, host_lengths, i32_ptr, on_device, per_device, stream

FILTER_LENGTH, HOP_LENGTH, WIN_LENGTH, N_BINS, N_MELS, SAMPLING_RATE = 1024, 256, 1024, 513, 80, 22050
MIN_FRAMES = 4            # the transform's reflect pad needs 256 (F - 1) > 512 samples (the reference's F.pad fails below)


_context = per_device(lambda device: Handle("dex_gl", device))     # one DexGl handle (FFT twiddles, window, mel basis) per device


def _workspace(ctx: Handle, B: int, max_frames: int) -> torch.Tensor:
    return ctx.workspace(int(ctx.lib.dex_gl_workspace_bytes(B, max_frames)))


def _random_angles(shape) -> np.ndarray:
    """audio_processing.py:74-75: the reference's host draw, so a numpy-seeded run stays on the reference's random stream."""
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


def _check_spec(S: torch.Tensor, what: str, min_frames: int = MIN_FRAMES):
    if S.dim() != 3 or S.shape[1] != N_BINS:
        raise ValueError(f"{what}: expected a spectrogram [B, {N_BINS}, frames], got {tuple(S.shape)}")
    if S.shape[2] < min_frames:
        raise ValueError(f"{what}: a spectrogram needs at least {min_frames} frames, got {S.shape[2]}")


def _griffin_lim(S: torch.Tensor, angles: torch.Tensor, frames: np.ndarray, n_iters: int) -> torch.Tensor:
    """S, angles [B, 513, F] on one device, row b frames[b] frames (host int32) -> [B, 256 (F - 1)] fp32, 0 past 256 (frames[b] - 1)."""
    ctx = _context(S.device)
    B, _, F = S.shape
    S = S.to(torch.float32).contiguous()
    angles = angles.to(device=S.device, dtype=torch.float32).contiguous()
    out = torch.empty(B, HOP_LENGTH * (F - 1), dtype=torch.float32, device=S.device)
    ws = _workspace(ctx, B, F)
    with torch.cuda.device(S.device):
        rc = ctx.lib.dex_griffin_lim(ctx.h, S.data_ptr(), angles.data_ptr(), i32_ptr(frames), B, F, int(n_iters), out.data_ptr(),
                                     ws.data_ptr(), ws.numel(), stream(S.device))
    ctx.check(rc, "dex_griffin_lim")
    return out


class STFT:
    """audio/stft.py:16-125 on the device: ``transform(y [B, L]) -> (magnitude, phase) [B, 513, L // 256 + 1]`` (reflect pad 512,
    windowed rFFT, atan2 phase), ``inverse(magnitude, phase) -> [B, 1, 256 (F - 1)]`` (irFFT, window, overlap-add, divided by
    window_sumsquare where it is > tiny(float32), times 4, 512 samples cropped at each end), ``forward(y) = inverse(transform(y))``."""

    def __init__(self, filter_length=FILTER_LENGTH, hop_length=HOP_LENGTH, win_length=WIN_LENGTH, window="hann"):
        got = (filter_length, hop_length, win_length, window)
        if got != (FILTER_LENGTH, HOP_LENGTH, WIN_LENGTH, "hann"):
            raise ValueError(f"only the reference configuration (1024, 256, 1024, 'hann') is built into the HIP STFT, got {got}")
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        self.magnitude = self.phase = None

    def transform(self, input_data: torch.Tensor):
        if input_data.dim() != 2:
            raise ValueError(f"STFT.transform: expected [B, samples], got {tuple(input_data.shape)}")
        B, L = input_data.shape
        if L <= FILTER_LENGTH // 2:
            raise ValueError(f"STFT.transform: the reflect pad needs more than {FILTER_LENGTH // 2} samples, got {L}")
        y, ln, _ = device_rows(input_data, None, "STFT.transform")
        self.num_samples = L
        ctx = _context(y.device)
        F = L // HOP_LENGTH + 1
        mag = torch.empty(B, N_BINS, F, dtype=torch.float32, device=y.device)
        phase = torch.empty_like(mag)
        with torch.cuda.device(y.device):
            rc = ctx.lib.dex_stft_transform(ctx.h, y.data_ptr(), i32_ptr(ln), B, L, mag.data_ptr(), phase.data_ptr(), stream(y.device))
        ctx.check(rc, "dex_stft_transform")
        return mag, phase

    def inverse(self, magnitude: torch.Tensor, phase: torch.Tensor) -> torch.Tensor:
        _check_spec(magnitude, "STFT.inverse", 2)
        if tuple(phase.shape) != tuple(magnitude.shape):
            raise ValueError(f"STFT.inverse: phase {tuple(phase.shape)} does not match magnitude {tuple(magnitude.shape)}")
        S = on_device(magnitude, "STFT.inverse").to(torch.float32).contiguous()
        ph = on_device(phase, "STFT.inverse").to(device=S.device, dtype=torch.float32).contiguous()
        ctx = _context(S.device)
        B, _, F = S.shape
        out = torch.empty(B, HOP_LENGTH * (F - 1), dtype=torch.float32, device=S.device)
        ws = _workspace(ctx, B, F)
        with torch.cuda.device(S.device):
            rc = ctx.lib.dex_stft_inverse(ctx.h, S.data_ptr(), ph.data_ptr(), i32_ptr(host_lengths(None, B, F)), B, F, out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), stream(S.device))
        ctx.check(rc, "dex_stft_inverse")
        return out.unsqueeze(1)

    def forward(self, input_data: torch.Tensor) -> torch.Tensor:
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)

    __call__ = forward


def griffin_lim(magnitudes: torch.Tensor, stft_fn: STFT, n_iters: int = 30, angles: Optional[torch.Tensor] = None) -> torch.Tensor:
    """audio_processing.py:66-82: magnitudes [B, 513, F] -> signal [B, 256 (F - 1)].  Without ``angles`` the initial phases are drawn
    on the host with ``np.random.rand(*magnitudes.size())`` exactly as the reference draws them; ``angles`` [B, 513, F] gives them
    explicitly.  The loop (signal = inverse(S, angles), then n_iters x signal = inverse(S, phase(transform(signal)))) runs on the
    device, two launches per iteration."""
    if not isinstance(stft_fn, STFT):
        raise TypeError("griffin_lim: stft_fn must be a dex_tts_amd.griffin_lim.STFT")
    _check_spec(magnitudes, "griffin_lim")
    if int(n_iters) < 0:
        raise ValueError(f"griffin_lim: n_iters must be >= 0, got {n_iters}")
    if angles is not None and tuple(angles.shape) != tuple(magnitudes.shape):
        raise ValueError(f"griffin_lim: angles {tuple(angles.shape)} do not match magnitudes {tuple(magnitudes.shape)}")
    S = on_device(magnitudes, "griffin_lim")
    if angles is None:
        angles = torch.from_numpy(_random_angles(magnitudes.size()))
    elif not isinstance(angles, torch.Tensor):
        angles = torch.as_tensor(np.asarray(angles, dtype=np.float32))
    return _griffin_lim(S, angles, host_lengths(None, S.shape[0], S.shape[2]), n_iters)


def mel_to_linear(mel: torch.Tensor, lengths=None) -> torch.Tensor:
    """tools.py:19-26 for a ragged batch: mel [B, 80, T] (log mel, as the sampler / TacotronSTFT produce) -> 1000 exp(mel)^T mel_basis
    without its last frame, [B, 513, T - 1]; row b keeps lengths[b] - 1 frames and is 0 past them.  The mel basis is the Slaney table
    of the library's mel front-end."""
    one = mel.dim() == 2
    m = mel[None] if one else mel
    if m.dim() != 3 or m.shape[1] != N_MELS:
        raise ValueError(f"mel_to_linear: expected a mel [B, {N_MELS}, T], got {tuple(mel.shape)}")
    B, _, T = m.shape
    n = host_lengths(lengths, B, T, lo=2, what="mel_to_linear")
    m = on_device(m, "mel_to_linear").to(torch.float32).contiguous()
    ctx = _context(m.device)
    spec = torch.empty(B, N_BINS, T - 1, dtype=torch.float32, device=m.device)
    with torch.cuda.device(m.device):
        rc = ctx.lib.dex_mel_to_linear(ctx.h, m.data_ptr(), i32_ptr(n), B, T, spec.data_ptr(), stream(m.device))
    ctx.check(rc, "dex_mel_to_linear")
    return spec[0] if one else spec


def mel_to_wav(mel: torch.Tensor, lengths=None, n_iters: int = 60, angles: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inv_mel_spec's waveform for a ragged batch: mel [B, 80, T] (or [80, T]), row b lengths[b] mel frames (5 .. T; default T)
    -> fp32 waveforms [B, 256 (T - 2)], row b 256 (lengths[b] - 2) samples long and 0 past them.

    Without ``angles`` each row's initial phases are drawn on the host per row, in row order, as ``np.random.rand(513, lengths[b] - 1)``
    mapped through the reference's ``np.angle(np.exp(2j pi .))``: the draws of consecutive ``inv_mel_spec`` calls.  A batch run under a
    numpy seed therefore equals those calls, one row after the other, under the same seed.  ``angles`` [B, 513, T - 1] gives them."""
    one = mel.dim() == 2
    m = mel[None] if one else mel
    if m.dim() != 3 or m.shape[1] != N_MELS:
        raise ValueError(f"mel_to_wav: expected a mel [B, {N_MELS}, T], got {tuple(mel.shape)}")
    B, _, T = m.shape
    n = host_lengths(lengths, B, T, lo=MIN_FRAMES + 1, what="mel_to_wav")
    if int(n_iters) < 0:
        raise ValueError(f"mel_to_wav: n_iters must be >= 0, got {n_iters}")
    if angles is not None and tuple(angles.shape) != (B, N_BINS, T - 1):
        raise ValueError(f"mel_to_wav: angles must be [{B}, {N_BINS}, {T - 1}], got {tuple(angles.shape)}")
    m = on_device(m, "mel_to_wav")
    S = mel_to_linear(m, n)
    if angles is None:
        a = np.zeros((B, N_BINS, T - 1), dtype=np.float32)
        for b in range(B):
            a[b, :, : n[b] - 1] = _random_angles((N_BINS, n[b] - 1))
        angles = torch.from_numpy(a)
    wav = _griffin_lim(S, angles, n - 1, n_iters)
    return wav[0] if one else wav


def inv_mel_spec(mel: torch.Tensor, out_filename: str, _stft, griffin_iters: int = 60):
    """tools.py:18-34: mel [80, T] -> Griffin-Lim waveform of 256 (T - 2) samples, written as float32 with
    ``scipy.io.wavfile.write(out_filename, _stft.sampling_rate, audio)``.  ``_stft`` is an ``audio.TacotronSTFT``: its ``_stft_fn``
    (an alias of ``stft_fn``) runs the loop, as the reference reads it.  The initial phases come from ``np.random.rand`` as in the
    reference's griffin_lim."""
    from scipy.io.wavfile import write

    if mel.dim() != 2 or mel.shape[0] != N_MELS:
        raise ValueError(f"inv_mel_spec: expected a mel [{N_MELS}, T], got {tuple(mel.shape)}")
    if mel.shape[1] < MIN_FRAMES + 1:
        raise ValueError(f"inv_mel_spec: a mel needs at least {MIN_FRAMES + 1} frames, got {mel.shape[1]}")
    spec = mel_to_linear(on_device(mel, "inv_mel_spec")[None])
    audio = griffin_lim(spec, _stft._stft_fn, griffin_iters).squeeze()
    write(out_filename, _stft.sampling_rate, audio.cpu().numpy())
