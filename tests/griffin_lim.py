"""CPU restatement of the reference's Griffin-Lim mel inversion (DEX-TTS audio/tools.py:18-34 inv_mel_spec, audio/audio_processing.py
:7-82 window_sumsquare / griffin_lim, audio/stft.py:52-121 STFT.transform / STFT.inverse) in float64 numpy, with rfft / irfft in
place of the reference's dense conv1d / conv_transpose1d bases.  Test infrastructure only: it is held to the reference's goldens
(tests/golden/griffin_lim.npz, tests/test_griffin_lim_cpu.py) and the product never imports it.

Configuration: filter_length N = 1024, hop 256, win_length 1024, window = scipy's periodic Hann, which general_cosine evaluates as
0.5 + 0.5 cos(linspace(-pi, pi, 1025)[:1024]).

transform(y [B, L]):  reflect-pad 512 on both sides, F = L // 256 + 1 frames x_f[n] = ypad[256 f + n], X_f = rfft(window x_f)
                      (the reference's forward basis is [Re; Im] of fft(eye(N))[:513] times the window) -> |X|, atan2(Im X, Re X).
inverse(mag, phase):  the reference's inverse basis pinv(4 [Re; Im]).T is irfft / 4 (1/N on DC and Nyquist, 2/N elsewhere, the
                      imaginary parts of DC and Nyquist ignored): frame_f = window irfft(mag e^{i phase}) / 4; overlap-add at hop
                      256 (length N + 256 (F - 1)); divide by window_sumsquare where it is > tiny(float32); times 4; crop 512 each end.
window_sumsquare:     a float32 array; frame by frame, ascending, the float64 squared window is added and the sum rounded to float32.
griffin_lim(S, angles, n): signal = inverse(S, angles); n times signal = inverse(S, angle(transform(signal))).
spec_from_mel(mel [80, T]):  1000 exp(mel)^T mel_basis (librosa's Slaney table, float32), [513, T]; griffin_lim gets [:, :-1].
"""
import numpy as np

N, HOP, PAD, NB = 1024, 256, 512, 513


def _rows(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.float64)
    return a[None] if a.ndim == 2 else a


def window() -> np.ndarray:
    return 0.5 + 0.5 * np.cos(np.linspace(-np.pi, np.pi, N + 1)[:N])


def window_sumsquare(n_frames: int) -> np.ndarray:
    n = N + HOP * (n_frames - 1)
    x = np.zeros(n, dtype=np.float32)
    wsq = window() ** 2
    for i in range(n_frames):
        s = i * HOP
        x[s:min(n, s + N)] += wsq[:max(0, min(N, n - s))]
    return x


def transform(y: np.ndarray):
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    L = y.shape[1]
    yp = np.pad(y, ((0, 0), (PAD, PAD)), mode="reflect")
    F = L // HOP + 1
    idx = np.arange(F)[:, None] * HOP + np.arange(N)[None, :]
    X = np.fft.rfft(yp[:, idx] * window(), axis=-1)             # [B, F, 513]
    X = np.swapaxes(X, 1, 2)
    return np.abs(X), np.arctan2(X.imag, X.real)


def inverse(mag: np.ndarray, phase: np.ndarray) -> np.ndarray:
    mag, phase = _rows(mag), _rows(phase)
    B, _, F = mag.shape
    frames = np.fft.irfft(np.swapaxes(mag * np.exp(1j * phase), 1, 2), n=N, axis=-1) * window() / 4.0    # [B, F, N]
    n = N + HOP * (F - 1)
    out = np.zeros((B, n))
    for f in range(F):
        out[:, f * HOP:f * HOP + N] += frames[:, f]
    wss = window_sumsquare(F)
    nz = wss > np.finfo(np.float32).tiny
    out[:, nz] /= wss[nz]
    out *= 4.0
    return out[:, PAD:n - PAD]


def griffin_lim(S: np.ndarray, angles: np.ndarray, n_iters: int) -> np.ndarray:
    S = _rows(S)
    signal = inverse(S, np.asarray(angles, dtype=np.float64).reshape(S.shape))
    for _ in range(n_iters):
        _, angles = transform(signal)
        signal = inverse(S, angles)
    return signal


def mel_basis() -> np.ndarray:
    from oracle.dex_oracle import slaney_mel_basis            # librosa 0.9.2's filters.mel, float32 as librosa returns it
    return slaney_mel_basis(22050, N, 80, 0.0, 8000.0).astype(np.float32)


def spec_from_mel(mel: np.ndarray) -> np.ndarray:
    return 1000.0 * (np.exp(np.asarray(mel, dtype=np.float64)).T @ mel_basis().astype(np.float64)).T


def spectral_convergence(S: np.ndarray, x: np.ndarray) -> float:
    mag, _ = transform(x)
    S = _rows(S)
    return float(np.linalg.norm(S - mag) / np.linalg.norm(S))
