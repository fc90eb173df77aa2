"""CPU restatement of WORLD's DIO + StoneMask f0 tracker (M. Morise), float64 numpy, as the library's f0 kernels
(dex_tts_amd/csrc/f0.hip) are specified.  Test infrastructure only: it is the oracle of tests/test_gpu_f0.py and is itself held
to synthetic signals whose f0 is known analytically (tests/test_f0_cpu.py).

It is NOT pinned to pyworld: pyworld is not available to this project, so parity with pyworld itself is unmeasured.  The text
below was written from WORLD's published description and is the contract both this file and the GPU follow.

Arguments are those of DEX-TTS/synthesize.py: ``pw.dio(x, fs, frame_period=fp)`` with pyworld's defaults f0_floor = 71,
f0_ceil = 800, channels_in_octave = 2, speed = 1, allowed_range = 0.1, then ``pw.stonemask(x, f0, t, fs)``.  round(v) is
MATLAB's: int(v + 0.5) for v > 0, else int(v - 0.5).  L = number of samples, eps = 1e-12.

DIO
  Frames: F = int(1000.0 * L / fs / fp) + 1 (in that order, in double); t_i = i * fp / 1000.
  Bands: nb = 1 + int(log2(f0_ceil / f0_floor) * cio); boundary_b = f0_floor * 2^((b+1) / cio).
  Signal: y = x followed by one zero (L + 1 samples), minus mean(y) over all L + 1 samples.
  Low-cut: N = 2 round(fs / 50) + 1, w_k = 0.5 - 0.5 cos(2 pi k / (N + 1)) for k = 1..N, h = delta - w / sum(w), centred.
  Band b: hl = round(fs / boundary_b / 2); an unnormalised Nuttall window of length 4 hl,
    0.355768 - 0.487396 cos(2 pi u) + 0.144232 cos(4 pi u) - 0.012604 cos(6 pi u), u = n / (4 hl - 1), applied causally, the
    output advanced by 2 hl.  Both filters are direct linear convolutions (WORLD uses an FFT long enough to be linear; equal in
    exact arithmetic, and digital silence stays exactly 0).  s_b has L + 1 samples.
  Events: on s, -s, d, -d with d_i = s_i - s_{i+1} (L samples): an event at i + 1 wherever v_i > 0 and v_{i+1} <= 0, fine position
    e = (i + 1) - v_i / (v_{i+1} - v_i).  Consecutive events give the interval fs / (e_{k+1} - e_k) located at (e_k + e_{k+1}) / 2 / fs.
  Candidates: if one of the four sequences has fewer than 3 events the band gives candidate 0, score 1e5 on every frame.  Otherwise
    each interval sequence is interpolated linearly at t_i, extrapolating from the first / last segment (interp1 + histc);
    cand = (I0 + I1 + I2 + I3) / 4, score = sqrt(sum (Ik - cand)^2 / 3); cand > boundary_b, cand < boundary_b / 2, cand > f0_ceil
    or cand < f0_floor gives cand = 0, score = 1e5.  Finally score /= cand + eps.
  Best: the per-frame arg-min of score over bands (strict >: the lowest band wins a tie).
  Fix: vrm = int(0.5 + 1000 / fp / f0_floor) * 2 + 1; F <= vrm gives all zeros.
    1. Zero the first and last vrm frames; for i >= vrm keep f_i iff |(f_i - f_{i-1}) / (eps + f_i)| < allowed_range.
    2. c = (vrm - 1) / 2: frame i (c <= i < F - c) becomes 0 if a step-1 value in [i - c, i + c] is 0.
    3. For each voiced -> unvoiced boundary n (last voiced index), walk j = n .. limit - 1 (limit: the next such boundary, F - 1 for
       the last) setting f[j+1] = select(f[j], f[j-1], j+1); stop at the first 0.
    4. For each unvoiced -> voiced boundary p (first voiced index), last to first, walk j = p .. limit + 1 downwards (limit: the
       previous p, 1 for the first) setting f[j-1] = select(f[j], f[j+1], j-1); stop at the first 0.
    select(cur, past, j): ref = (3 cur - past) / 2; the band candidate of frame j nearest to ref (first band on a tie), or 0 if
    |1 - best / ref| > allowed_range.  (A neighbour past the last frame reads as the current frame; the walks never reach it.)

StoneMask, per frame with 40 < f0 <= fs / 12 (others give 0):
  hw = int(1.5 fs / f0 + 1), W = (2 hw + 1) / fs, nfft = 2^(2 + int(log2(2 hw + 1))).
  r_k = round((t + (k - hw) / fs) * fs), k = 0..2hw; the window reads x[clamp(r_k - 1, 0, L - 1)].
  Main window (Blackman at tau = (r_k - 1) / fs - t): 0.42 + 0.5 cos(2 pi tau / W) + 0.08 cos(4 pi tau / W).
  Difference window: dw_0 = -mw_1 / 2, dw_k = -(mw_{k+1} - mw_{k-1}) / 2, dw_last = mw_{last-1} / 2.
  M, D = nfft-point DFTs of x mw and x dw; P = |M|^2; num = Re M Im D - Im M Re D.
  fix(f, nh): for k = 1..nh, bin j = round(f nfft / fs k) (taken modulo nfft); if_k = j fs / nfft + num_j / P_j fs / (2 pi)
    (0 if P_j == 0), a_k = sqrt(P_j); returns sum a_k if_k / (sum a_k k + eps).
  f1 = fix(f0, 2); f1 <= 0 or f1 > 2 f0 gives 0; else f2 = fix(f1, min(int(fs / 2 / f0), 6)); |f2 - f0| > 0.2 f0 gives f0.
"""
from __future__ import annotations

import math

import numpy as np

EPS = 1e-12


def mround(v):
    return int(v + 0.5) if v > 0 else int(v - 0.5)


def frames(L, fs=22050.0, frame_period=256.0 / 22050.0 * 1000.0):
    return int(1000.0 * L / fs / frame_period) + 1


def _fir(sig, h, off):
    """out[n] = sum_m h[m] sig[n + off - m], n = 0..len(sig)-1, sig zero outside."""
    full = np.convolve(sig, h)                     # full[k] = sum_m h[m] sig[k - m]
    return full[off:off + len(sig)]


def _events(v, fs):
    i = np.nonzero((v[:-1] > 0) & (v[1:] <= 0))[0]
    e = (i + 1) - v[i] / (v[i + 1] - v[i])
    return e


def _interp(e, fs, t):
    """Intervals fs / de at (e_k + e_k+1) / 2 / fs, linearly interpolated / extrapolated at t."""
    x = (e[:-1] + e[1:]) / 2.0 / fs
    y = fs / (e[1:] - e[:-1])
    k = np.clip(np.searchsorted(x, t, side="right") - 1, 0, len(x) - 2)
    return y[k] + (t - x[k]) * (y[k + 1] - y[k]) / (x[k + 1] - x[k])


def band_candidates(x, fs, frame_period=5.0, f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0):
    """-> (cand [nb, F], score [nb, F]) after the range check and the final division."""
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    F = frames(L, fs, frame_period)
    t = np.arange(F) * frame_period / 1000.0
    nb = 1 + int(math.log2(f0_ceil / f0_floor) * channels_in_octave)
    y = np.concatenate([x, [0.0]])
    y = y - np.mean(y)
    N = 2 * mround(fs / 50.0) + 1
    w = 0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(1, N + 1) / (N + 1))
    h = -w / np.sum(w)
    h[(N - 1) // 2] += 1.0
    z = _fir(y, h, (N - 1) // 2)
    cand = np.zeros((nb, F))
    score = np.zeros((nb, F))
    for b in range(nb):
        bnd = f0_floor * 2.0 ** ((b + 1) / channels_in_octave)
        hl = mround(fs / bnd / 2.0)
        u = np.arange(4 * hl) / (4 * hl - 1)
        g = 0.355768 - 0.487396 * np.cos(2 * math.pi * u) + 0.144232 * np.cos(4 * math.pi * u) - 0.012604 * np.cos(6 * math.pi * u)
        s = _fir(z, g, 2 * hl)
        d = s[:-1] - s[1:]
        ev = [_events(v, fs) for v in (s, -s, d, -d)]
        if min(len(e) for e in ev) < 3:
            c = np.zeros(F)
            sc = np.full(F, 1e5)
        else:
            I = [_interp(e, fs, t) for e in ev]
            c = (I[0] + I[1] + I[2] + I[3]) / 4.0
            sc = np.sqrt(((I[0] - c) ** 2 + (I[1] - c) ** 2 + (I[2] - c) ** 2 + (I[3] - c) ** 2) / 3.0)
            bad = (c > bnd) | (c < bnd / 2.0) | (c > f0_ceil) | (c < f0_floor)
            c = np.where(bad, 0.0, c)
            sc = np.where(bad, 1e5, sc)
        cand[b], score[b] = c, sc / (c + EPS)
    return cand, score


def _select(cand, cur, past, j, allowed_range):
    ref = (3.0 * cur - past) / 2.0
    dist = np.abs(cand[:, j] - ref)
    best = cand[int(np.argmin(dist)), j]           # argmin: the first band on a tie
    return 0.0 if abs(1.0 - best / ref) > allowed_range else best


def fix_f0(best, cand, frame_period, f0_floor, allowed_range):
    F = len(best)
    vrm = int(0.5 + 1000.0 / frame_period / f0_floor) * 2 + 1
    if F <= vrm:
        return np.zeros(F)
    f1 = np.zeros(F)
    for i in range(vrm, F - vrm):
        f1[i] = best[i] if abs((best[i] - best[i - 1]) / (EPS + best[i])) < allowed_range else 0.0
    c = (vrm - 1) // 2
    f = f1.copy()
    for i in range(c, F - c):
        if np.any(f1[i - c:i + c + 1] == 0):
            f[i] = 0.0
    sel = lambda cur, past, j: _select(cand, cur, past, j, allowed_range)
    # step 3
    ends = [n for n in range(F - 1) if f[n] != 0 and f[n + 1] == 0]
    for q, n in enumerate(ends):
        limit = ends[q + 1] if q + 1 < len(ends) else F - 1
        for j in range(n, limit):
            f[j + 1] = sel(f[j], f[j - 1] if j >= 1 else f[j], j + 1)
            if f[j + 1] == 0:
                break
    # step 4
    starts = [p for p in range(1, F) if f[p] != 0 and f[p - 1] == 0]
    for q in range(len(starts) - 1, -1, -1):
        p = starts[q]
        limit = starts[q - 1] if q > 0 else 1
        for j in range(p, limit, -1):
            f[j - 1] = sel(f[j], f[j + 1] if j + 1 < F else f[j], j - 1)
            if f[j - 1] == 0:
                break
    return f


def dio(x, fs, f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0, frame_period=5.0, allowed_range=0.1):
    """-> (f0 [F], t [F])."""
    cand, score = band_candidates(x, fs, frame_period, f0_floor, f0_ceil, channels_in_octave)
    nb, F = cand.shape
    bi = np.zeros(F, dtype=np.int64)
    for b in range(1, nb):
        bi = np.where(score[bi, np.arange(F)] > score[b], b, bi)
    best = cand[bi, np.arange(F)]
    f0 = fix_f0(best, cand, frame_period, f0_floor, allowed_range)
    return f0, np.arange(F) * frame_period / 1000.0


def _fix(Mf, Df, f, nh, fs, nfft):
    num = den = 0.0
    for k in range(1, nh + 1):
        j = mround(f * nfft / fs * k) % nfft
        m, d = Mf[j], Df[j]
        P = m.real * m.real + m.imag * m.imag
        ifr = 0.0 if P == 0 else j * fs / nfft + (m.real * d.imag - m.imag * d.real) / P * fs / (2.0 * math.pi)
        a = math.sqrt(P)
        num += a * ifr
        den += a * k
    return num / (den + EPS)


def stonemask(x, f0, t, fs):
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    out = np.zeros(len(f0))
    for i, (f, ti) in enumerate(zip(f0, t)):
        if not (40.0 < f <= fs / 12.0):
            continue
        hw = int(1.5 * fs / f + 1)
        n = 2 * hw + 1
        W = n / fs
        nfft = 2 ** (2 + int(math.log2(n)))
        r = np.array([mround((ti + (k - hw) / fs) * fs) for k in range(n)])
        seg = x[np.clip(r - 1, 0, L - 1)]
        tau = (r - 1) / fs - ti
        mw = 0.42 + 0.5 * np.cos(2 * math.pi * tau / W) + 0.08 * np.cos(4 * math.pi * tau / W)
        dw = np.empty(n)
        dw[0] = -mw[1] / 2.0
        dw[1:-1] = -(mw[2:] - mw[:-2]) / 2.0
        dw[-1] = mw[-2] / 2.0
        Mf = np.fft.fft(seg * mw, nfft)
        Df = np.fft.fft(seg * dw, nfft)
        f1 = _fix(Mf, Df, f, 2, fs, nfft)
        if f1 <= 0 or f1 > 2 * f:
            continue
        f2 = _fix(Mf, Df, f1, min(int(fs / 2 / f), 6), fs, nfft)
        out[i] = f if abs(f2 - f) > 0.2 * f else f2
    return out
