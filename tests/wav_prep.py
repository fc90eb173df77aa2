"""CPU restatement of the reference wav preparation that precedes the mel and the f0 tracker (DEX-TTS/synthesize.py:40-62,
``preprocess_wav``): silence trim, resampling to 22050 Hz and peak normalisation, float64 numpy, as the library's kernels
(dex_tts_amd/csrc/wavprep.hip) are specified.  Test infrastructure only: it is the oracle of tests/test_gpu_wav_prep.py and is itself
held to signals with known answers (tests/test_wavprep_cpu.py).  The product never imports it.

It is NOT pinned to librosa 0.9.2 (DEX-TTS/requirements.txt) or to resampy: neither package is available to this project, so parity
with them is unmeasured.  The text below was written from their published source and documentation and is the contract both this
file and the GPU follow.

Trim  (librosa.effects.trim(y, top_db=30), ref = max, frame_length = 2048, hop_length = 512)
  L samples, pad = frame_length // 2, F = 1 + L // hop_length frames.  The signal is centred: padded by `pad` samples on each side,
  with zeros (pad mode "constant", the default here) or by numpy's "reflect" (np.pad mode="reflect", which for pad >= L keeps
  reflecting: a period of 2 (L - 1) samples, a constant for L = 1).  Which of the two librosa 0.9.2's feature.rms used by default is
  not verified; both are offered.
  mse_f = mean of x^2 over padded samples [f hop, f hop + frame_length).
  db_f = 10 log10(max(1e-10, mse_f)) - 10 log10(max(1e-10, max_f mse_f)); frame f is non-silent iff db_f > -top_db.
  start = first non-silent frame * hop; end = min(L, (last non-silent frame + 1) * hop).  No non-silent frame gives (0, 0)
  (only for L = 0, which the API rejects).  An all-zero row has every db_f = 0: it is kept whole, (0, L).

Resample  (resampy 0.4 resample(x, sr_orig, sr_new), filter "kaiser_best")
  Table: sinc_window(num_zeros = 64, precision = 9, window = kaiser(beta = 14.769656459379492), rolloff = 0.9475937167399596):
    N = 512 * 64, nwin = N + 1; win[j] = kaiser(2N + 1, beta)[N + j] * (rolloff * sinc(rolloff * j / 512)), j = 0..N, with
    kaiser[N + j] = i0(beta sqrt(1 - (j / N)^2)) / i0(beta) and sinc(u) = sin(pi u) / (pi u), sinc(0) = 1.
  ratio = sr_new / sr_orig (double).  If ratio < 1 the window is scaled: win <- ratio * win.  delta[j] = win[j+1] - win[j], delta[N] = 0.
  L_out = (L * sr_new) div sr_orig in integer arithmetic (L_out < 1 is rejected).  sr_orig == sr_new returns x unchanged
  (synthesize.py resamples only when fs != 22050).
  t_out[t] = t * (1.0 / ratio); scale = min(1, ratio); index_step = int(scale * 512).  Per output t:
    n = int(t_out[t]); frac = scale * (t_out[t] - n); index_frac = frac * 512; offset = int(index_frac); eta = index_frac - offset
    left wing:  i = 0 .. min(n + 1, (nwin - offset) // index_step) - 1:  y += (win[o] + eta * delta[o]) * x[n - i],  o = offset + i index_step
    frac = scale - frac, and offset / eta again from it
    right wing: k = 0 .. min(L - n - 1, (nwin - offset) // index_step) - 1:  y += (win[o] + eta * delta[o]) * x[n + k + 1]
  y starts at 0 and accumulates sequentially in fp64, one rounding per operation.  (index_step truncates 235.2 to 235 at 48 kHz ->
  22.05 kHz, a gain error of about 8.6e-4 when downsampling: that is resampy's behaviour, reproduced, not corrected.)

Peak normalisation (synthesize.py:46): x / max|x| per row in fp64 (a silent row stays 0).

The chain (``preprocess_wav`` as the device runs it): trim at the source rate -> resample to 22050 in fp64 if sr != 22050 ->
peak-normalise in fp64 -> round to fp32 once -> the mel and the f0 tracker of that fp32 wav.  The reference's mel also sees an fp32
wav (torch.FloatTensor); its DIO / StoneMask see the fp64 one (DESIGN §4 reports the difference this makes).
"""
from __future__ import annotations

import numpy as np

TOP_DB = 30.0
FRAME = 2048
HOP = 512

NUM_ZEROS = 64
PRECISION = 9
NUM_TABLE = 1 << PRECISION          # 512
BETA = 14.769656459379492
ROLLOFF = 0.9475937167399596
SR = 22050


# ---- trim
def _pad(x, pad, mode):
    if mode == "constant":
        return np.concatenate([np.zeros(pad), x, np.zeros(pad)])
    if mode == "reflect":
        return np.pad(x, pad, mode="reflect")
    raise ValueError(f"pad_mode must be 'constant' or 'reflect', got {mode!r}")


def frame_mse(x, frame_length=FRAME, hop_length=HOP, pad_mode="constant"):
    """mse_f, f = 0..F-1 (F = 1 + L // hop_length)."""
    x = np.asarray(x, np.float64)
    L = len(x)
    xp = _pad(x, frame_length // 2, pad_mode)
    F = 1 + L // hop_length
    return np.array([np.mean(xp[f * hop_length: f * hop_length + frame_length] ** 2) for f in range(F)])


def frame_db(x, frame_length=FRAME, hop_length=HOP, pad_mode="constant"):
    mse = frame_mse(x, frame_length, hop_length, pad_mode)
    return 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))


def trim_bounds(x, top_db=TOP_DB, frame_length=FRAME, hop_length=HOP, pad_mode="constant"):
    """(start, end) of librosa.effects.trim as stated above."""
    L = len(x)
    if L == 0:
        return 0, 0
    nz = np.nonzero(frame_db(x, frame_length, hop_length, pad_mode) > -top_db)[0]
    if len(nz) == 0:
        return 0, 0
    return int(nz[0]) * hop_length, min(L, (int(nz[-1]) + 1) * hop_length)


# ---- resample
def kaiser_best_window():
    """win[j], j = 0..N (float64, unscaled)."""
    n = NUM_TABLE * NUM_ZEROS
    j = np.arange(n + 1, dtype=np.float64)
    u = ROLLOFF * (j * (NUM_ZEROS / n))                # np.linspace(0, num_zeros, n + 1): j * 2^-9, exact
    y = np.pi * np.where(u == 0, 1.0e-20, u)            # np.sinc
    sinc_win = ROLLOFF * (np.sin(y) / y)
    taper = np.i0(BETA * np.sqrt(1.0 - (j / n) ** 2.0)) / np.i0(BETA)
    return taper * sinc_win


_WIN = None


def _window():
    global _WIN
    if _WIN is None:
        _WIN = kaiser_best_window()
    return _WIN


def resampled_length(L, sr_orig, sr_new):
    return (int(L) * int(sr_new)) // int(sr_orig)


def resample(x, sr_orig, sr_new):
    """resampy.resample(x, sr_orig, sr_new, filter='kaiser_best') as stated above, float64."""
    x = np.asarray(x, np.float64)
    if sr_orig <= 0 or sr_new <= 0:
        raise ValueError("sample rates must be positive")
    if sr_orig == sr_new:
        return x.copy()
    L = len(x)
    L_out = resampled_length(L, sr_orig, sr_new)
    if L_out < 1:
        raise ValueError(f"{L} samples at {sr_orig} Hz give no sample at {sr_new} Hz")
    ratio = float(sr_new) / float(sr_orig)
    win = _window()
    if ratio < 1:
        win = ratio * win
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    nwin = len(win)
    scale = min(1.0, ratio)
    step = int(scale * NUM_TABLE)
    if step < 1:
        raise ValueError("sr_new / sr_orig below 1 / 512 is not supported")
    t_out = np.arange(L_out, dtype=np.float64) * (1.0 / ratio)
    n = t_out.astype(np.int64)
    y = np.zeros(L_out)

    def wing(frac, count, src):
        nonlocal y
        index_frac = frac * NUM_TABLE
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        cnt = np.minimum(count, (nwin - offset) // step)
        for i in range(int(cnt.max(initial=0))):
            m = i < cnt
            o = np.where(m, offset + i * step, 0)
            w = win[o] + eta * delta[o]
            idx = np.where(m, src(i), 0)
            y = np.where(m, y + w * x[idx], y)

    frac = scale * (t_out - n)
    wing(frac, n + 1, lambda i: n - i)
    wing(scale - frac, L - n - 1, lambda i: n + i + 1)
    return y


# ---- peak normalisation and the chain
def peak_normalize(x):
    x = np.asarray(x, np.float64)
    pk = np.abs(x).max() if len(x) else 0.0
    return x / pk if pk > 0 else np.zeros_like(x)


def prepare(x, sr, sr_out=SR, top_db=TOP_DB, pad_mode="constant"):
    """The chain up to the fp32 wav the mel and the f0 tracker read: -> (float32 wav, (start, end))."""
    x = np.asarray(x, np.float64)
    s, e = trim_bounds(x, top_db=top_db, pad_mode=pad_mode)
    y = x[s:e]
    if sr != sr_out:
        y = resample(y, sr, sr_out)
    return peak_normalize(y).astype(np.float32), (s, e)
