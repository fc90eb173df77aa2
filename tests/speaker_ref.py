"""Float64 restatement, in numpy, of the speaker-similarity path the library runs on the device (dex_tts_amd/speaker.py): resemblyzer's
audio front end and VoiceEncoder as the reference's src/metric.py:69-95, 115-142 uses them, minus the VAD.  resemblyzer and librosa are not
importable here, so - as for pyworld, librosa's trim and resampy elsewhere in this suite - the definition is written out:

    rates     16 kHz, n_fft = win = 400 (25 ms), hop 160 (10 ms), 40 mels, partials of 160 frames
    normalize_volume(wav, -30, increase_only=True)   dBFS = 10 log10(mean(wav^2)); change = target - dBFS; unchanged if change < 0,
                                                     else wav * float32(10^(change / 20)) (numpy: float32 array times a scalar)
    wav_to_mel_spectrogram    librosa.feature.melspectrogram(y, sr, n_fft=400, hop_length=160, n_mels=40).T: center=True with zero
                              padding of 200, periodic Hann, |X|^2 of 201 bins, Slaney mel scale with Slaney normalisation (the basis
                              rounded to float32, as librosa returns it), fmin 0, fmax 8000, no logarithm; 1 + n // 160 frames
    compute_partial_slices, embed_utterance, forward (LSTM(40, 256, 3) with gates i | f | g | o and both biases -> Linear -> ReLU ->
    L2 normalisation), cosine, asv_score

The LSTM is written out by hand and does not use torch.nn.LSTM; tests/test_speaker_cpu.py holds it against torch's in float64.
Every function takes ``dtype``: np.float64 is the definition, np.float32 the same arithmetic in single precision - the yardstick
of the device tolerances below."""
import math

import numpy as np

SR, N_FFT, HOP, N_MELS, PARTIAL, H, LAYERS = 16000, 400, 160, 40, 160, 256, 3

# ---- tolerances of tests/test_gpu_speaker.py (each a factor on a distance the test measures on its own inputs) ----
# the device runs the same fp32 sums as a CPU fp32 evaluation in another order: 8 x covers the reordering of a 256-term dot product
NET_FACTOR = 8.0
# never below 1e-6 on a unit-norm embedding: a yardstick that happens to land near 0 on some input must not demand the impossible
NET_FLOOR = 1e-6
# the mel: the same rule, against this file's fp32 evaluation, relative to the utterance's largest mel value
MEL_FACTOR = 8.0
MEL_FLOOR = 1e-6
# an all-zero ReLU output must never be what makes a comparison pass: every row's raw (pre-normalisation) norm must exceed this
MIN_RAW_NORM = 0.1


# ------------------------------------------------------------------ weights
def make_weights(seed=0):
    """Synthetic weights with torch's default init for LSTM and Linear of width 256: U(-1/16, 1/16), float32."""
    rng = np.random.RandomState(seed)
    k = 1.0 / math.sqrt(H)
    u = lambda *shape: rng.uniform(-k, k, size=shape).astype(np.float32)
    sd = {}
    for l in range(LAYERS):
        sd[f"lstm.weight_ih_l{l}"] = u(4 * H, N_MELS if l == 0 else H)
        sd[f"lstm.weight_hh_l{l}"] = u(4 * H, H)
        sd[f"lstm.bias_ih_l{l}"] = u(4 * H)
        sd[f"lstm.bias_hh_l{l}"] = u(4 * H)
    sd["linear.weight"] = u(H, H)
    sd["linear.bias"] = u(H)
    return sd


# ------------------------------------------------------------------ audio
def normalize_volume(wav, target_dbfs=-30.0, dtype=np.float64):
    wav = np.asarray(wav)
    dbfs = 10.0 * np.log10(np.mean(wav.astype(np.float64) ** 2))
    change = target_dbfs - dbfs
    if change < 0:
        return wav
    return wav * np.float32(10.0 ** (change / 20.0)) if wav.dtype == np.float32 else wav * (10.0 ** (change / 20.0))


def _hz_to_mel(f):
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return min_log_mel + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp


def _mel_to_hz(m):
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return min_log_hz * math.exp(logstep * (m - min_log_mel)) if m >= min_log_mel else f_sp * m


def mel_basis():
    """librosa.filters.mel(sr=16000, n_fft=400, n_mels=40): [40, 201], float32 values held in float64."""
    lo, hi = _hz_to_mel(0.0), _hz_to_mel(SR / 2.0)
    pts = np.array([_mel_to_hz(lo + (hi - lo) * i / (N_MELS + 1)) for i in range(N_MELS + 2)])
    freqs = np.arange(N_FFT // 2 + 1) * (SR / N_FFT)
    w = np.zeros((N_MELS, N_FFT // 2 + 1))
    for m in range(N_MELS):
        lower = (freqs - pts[m]) / (pts[m + 1] - pts[m])
        upper = (pts[m + 2] - freqs) / (pts[m + 2] - pts[m + 1])
        w[m] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[m + 2] - pts[m]))
    return w.astype(np.float32).astype(np.float64)


def hann():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def dft_basis():
    """[400, 201] cos and -sin of 2 pi k n / 400, the angle reduced mod 400 exactly."""
    kn = np.outer(np.arange(N_FFT), np.arange(N_FFT // 2 + 1)) % N_FFT
    a = 2.0 * np.pi * kn / N_FFT
    return np.cos(a), -np.sin(a)


def frames(wav, n_frames=None):
    """The windowed frames of the zero-padded wav: [F, 400], F = 1 + n // 160 (or n_frames, the wav counting as 0 past its end)."""
    wav = np.asarray(wav, np.float64)
    F = 1 + len(wav) // HOP if n_frames is None else n_frames
    pad = np.zeros(N_FFT // 2 + max(len(wav), (F - 1) * HOP + N_FFT) + N_FFT)
    pad[N_FFT // 2: N_FFT // 2 + len(wav)] = wav
    idx = np.arange(F)[:, None] * HOP + np.arange(N_FFT)[None, :]
    return pad[idx] * hann()[None, :]


def power_spectrogram(wav, n_frames=None, dtype=np.float64):
    fr = frames(wav, n_frames).astype(dtype)
    c, s = dft_basis()
    re, im = fr @ c.astype(dtype), fr @ s.astype(dtype)
    return re * re + im * im                                  # [F, 201]


def wav_to_mel_spectrogram(wav, n_frames=None, dtype=np.float64):
    return (power_spectrogram(wav, n_frames, dtype) @ mel_basis().T.astype(dtype)).astype(dtype)      # [F, 40]


def compute_partial_slices(n_samples, rate=1.3, min_coverage=0.75):
    n_frames = int(math.ceil((n_samples + 1) / HOP))
    frame_step = int(round((SR / rate) / HOP))
    steps = max(1, n_frames - PARTIAL + frame_step + 1)
    mel_slices = [(i, i + PARTIAL) for i in range(0, steps, frame_step)]
    wav_slices = [(a * HOP, b * HOP) for a, b in mel_slices]
    coverage = (n_samples - wav_slices[-1][0]) / (wav_slices[-1][1] - wav_slices[-1][0])
    if coverage < min_coverage and len(mel_slices) > 1:
        mel_slices, wav_slices = mel_slices[:-1], wav_slices[:-1]
    return wav_slices, mel_slices


# ------------------------------------------------------------------ network
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm(sd, x, dtype=np.float64):
    """x [P, T, 40] -> the top layer's final hidden state [P, 256]."""
    x = np.asarray(x, dtype)
    for l in range(LAYERS):
        w_ih, w_hh = sd[f"lstm.weight_ih_l{l}"].astype(dtype), sd[f"lstm.weight_hh_l{l}"].astype(dtype)
        b_ih, b_hh = sd[f"lstm.bias_ih_l{l}"].astype(dtype), sd[f"lstm.bias_hh_l{l}"].astype(dtype)
        P, T, _ = x.shape
        h, c = np.zeros((P, H), dtype), np.zeros((P, H), dtype)
        out = np.empty((P, T, H), dtype)
        for t in range(T):
            g = x[:, t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
            i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
            c = f * c + i * gg
            h = o * np.tanh(c)
            out[:, t] = h
        x = out
    return x[:, -1]


def forward_raw(sd, mels, dtype=np.float64):
    """The embeddings before the L2 normalisation: relu(linear(h_T))."""
    h = lstm(sd, mels, dtype)
    return np.maximum(h @ sd["linear.weight"].astype(dtype).T + sd["linear.bias"].astype(dtype), 0)


def forward(sd, mels, dtype=np.float64):
    raw = forward_raw(sd, mels, dtype)
    return raw / np.linalg.norm(raw, axis=1, keepdims=True)


def partial_mels(wav, dtype=np.float64):
    """The [n_partials, 160, 40] mel partials of embed_utterance (the wav zero-padded to the last slice's end)."""
    wav_slices, mel_slices = compute_partial_slices(len(wav))
    n = max(len(wav), wav_slices[-1][1])
    padded = np.zeros(n, np.asarray(wav).dtype)
    padded[: len(wav)] = wav
    mel = wav_to_mel_spectrogram(padded, dtype=dtype)
    return np.stack([mel[a:b] for a, b in mel_slices])


def embed_utterance(sd, wav, dtype=np.float64, return_raw=False):
    mels = partial_mels(wav, dtype)
    raw_partials = forward_raw(sd, mels, dtype)
    partials = raw_partials / np.linalg.norm(raw_partials, axis=1, keepdims=True)
    raw = partials.mean(axis=0)
    e = raw / np.linalg.norm(raw)
    return (e, raw_partials) if return_raw else e


def cosine(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sum(a * b, axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def asv_score(cos):
    cos = np.asarray(cos, np.float64)
    return float(np.mean(cos)), float(np.std(cos) / np.sqrt(len(cos)))


# ------------------------------------------------------------------ test inputs
def synth_wav(n, seed, amp=0.1):
    """A voiced-speech-like wav: a few harmonics of a gliding pitch under a slow envelope, plus noise.  float32."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / SR
    f0 = 110.0 + 40.0 * rng.rand() + 30.0 * np.sin(2 * np.pi * (0.7 + rng.rand()) * t)
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = sum(rng.rand() / (k + 1) * np.sin((k + 1) * ph + 2 * np.pi * rng.rand()) for k in range(8))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t + rng.rand())) + 0.05 * rng.randn(n)
    return (amp * x / np.abs(x).max()).astype(np.float32)


def mel_like(P, T, seed):
    """Power-mel-like network inputs: non-negative, a few orders of magnitude of spread, float32 [P, T, 40]."""
    rng = np.random.RandomState(seed)
    return (np.exp(rng.randn(P, T, N_MELS) * 1.5 - 3.0)).astype(np.float32)
