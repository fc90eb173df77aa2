"""Speaker similarity on the device: the number DEX-TTS is judged by (the reference's src/metric.py:69-95, 115-142, ``Evaluater.
calculate_accept`` / ``calculate_asv_score``): the cosine between the d-vector of a synthesised wav and that of its reference wav.
The d-vector is resemblyzer's ``VoiceEncoder``: 16 kHz, 25 ms window (n_fft 400), hop 160, 40 Slaney mels of the power spectrogram
(no logarithm), partials of 160 frames, ``LSTM(40, 256, 3)`` -> ``Linear(256, 256)`` -> ReLU -> L2 normalisation.

    normalize_volume(wav, target_dBFS=-30, increase_only=True, lengths=None)
    wav_to_mel_spectrogram(wav, lengths=None)             [.., n] -> [.., 1 + n // 160, 40]
    compute_partial_slices(n_samples, rate=1.3, min_coverage=0.75)      host integers
    preprocess_wav(wav, source_sr=None, lengths=None)     metric.py:115-142 without the VAD (see below)
    VoiceEncoder(device): load_state_dict, forward, embed_utterance, embed_utterances, embed_speaker
    speaker_similarity(syn, trg, ..., encoder=) -> cos [B];  asv_score(...) -> (mean, stderr);  score_synthesis(audio, ref_wavs, ...)

Everything runs in libdexamd.so (``csrc/speaker.hip``, C ABI ``dex_spk_*``); the network is fp32 throughout - a metric has no
reduced-precision mode.  Tensors must be CUDA tensors; a refused argument raises ``ValueError`` before anything is enqueued.

Two departures from the reference's number, both stated here so nobody compares unlike things:
  * ``trim_long_silences`` (metric.py:140) is webrtcvad, a host C library with no restatable definition: it is LEFT OUT.  Callers
    who want the reference's exact score trim on the host first and pass the trimmed wavs.
  * the resampling to 16 kHz is the library's ``wavprep.resample`` (resampy's kaiser_best); current librosa resamples with soxr.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from ._native import Handle, device_index, device_rows, i32_ptr, on_device, pad_wavs, per_device, resample_to_16k, stream, upload_weights

SAMPLING_RATE, N_FFT, HOP, N_MELS, PARTIALS_N_FRAMES, EMBED, HIDDEN, LAYERS = 16000, 400, 160, 40, 160, 256, 256, 3
AUDIO_NORM_TARGET_DBFS = -30.0


def state_dict_shapes() -> dict:
    """resemblyzer's checkpoint keys the encoder needs, with their shapes."""
    out = {}
    for l in range(LAYERS):
        out[f"lstm.weight_ih_l{l}"] = (4 * HIDDEN, N_MELS if l == 0 else HIDDEN)
        out[f"lstm.weight_hh_l{l}"] = (4 * HIDDEN, HIDDEN)
        out[f"lstm.bias_ih_l{l}"] = (4 * HIDDEN,)
        out[f"lstm.bias_hh_l{l}"] = (4 * HIDDEN,)
    out["linear.weight"] = (EMBED, HIDDEN)
    out["linear.bias"] = (EMBED,)
    return out


_IGNORED = ("similarity_weight", "similarity_bias")


def route_state_dict(sd) -> dict:
    """A resemblyzer checkpoint (``{"model_state": ...}`` or the state dict itself) -> {key: tensor} of exactly the keys of
    ``state_dict_shapes``.  ``similarity_weight`` / ``similarity_bias`` (the training loss's) are ignored; a missing key, an
    unexpected key or a wrong shape raises ``RuntimeError``, as ``tts.py`` does.  Needs no device."""
    if "model_state" in sd and not any(k.startswith("lstm.") for k in sd):
        sd = sd["model_state"]
    want = state_dict_shapes()
    missing = [k for k in want if k not in sd]
    if missing:
        raise RuntimeError(f"missing keys {missing[:4]}")
    extra = [k for k in sd if k not in want and k not in _IGNORED]
    if extra:
        raise RuntimeError(f"unexpected keys {sorted(extra)[:4]}")
    out = {}
    for k, shape in want.items():
        v = torch.as_tensor(sd[k])
        if tuple(v.shape) != shape:
            raise RuntimeError(f"{k}: expected shape {shape}, got {tuple(v.shape)}")
        out[k] = v
    return out


def compute_partial_slices(n_samples: int, rate: float = 1.3, min_coverage: float = 0.75):
    """resemblyzer's ``VoiceEncoder.compute_partial_slices``: (wav_slices, mel_slices), lists of ``slice`` objects, one pair per
    160-frame partial.  The last partial is dropped if it covers less than ``min_coverage`` of its 25600 samples and is not the only
    one.  Host integers only."""
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError(f"compute_partial_slices: n_samples must be >= 1, got {n_samples}")
    if not 0 < min_coverage <= 1:
        raise ValueError(f"compute_partial_slices: min_coverage must lie in (0, 1], got {min_coverage}")
    n_frames = int(math.ceil((n_samples + 1) / HOP))
    frame_step = int(round((SAMPLING_RATE / rate) / HOP))
    if not 0 < frame_step <= PARTIALS_N_FRAMES:
        raise ValueError(f"compute_partial_slices: the rate {rate} gives a frame step of {frame_step}, outside (0, {PARTIALS_N_FRAMES}]")
    wav_slices, mel_slices = [], []
    steps = max(1, n_frames - PARTIALS_N_FRAMES + frame_step + 1)
    for i in range(0, steps, frame_step):
        mel_slices.append(slice(i, i + PARTIALS_N_FRAMES))
        wav_slices.append(slice(i * HOP, (i + PARTIALS_N_FRAMES) * HOP))
    coverage = (n_samples - wav_slices[-1].start) / (wav_slices[-1].stop - wav_slices[-1].start)
    if coverage < min_coverage and len(mel_slices) > 1:
        mel_slices, wav_slices = mel_slices[:-1], wav_slices[:-1]
    return wav_slices, mel_slices


class _Spk(Handle):
    """One DexSpk handle (DFT twiddles, window, mel basis on the device; optionally the weights); its workspace is the network's."""

    def __init__(self, device):
        super().__init__("dex_spk", device)

    def workspace(self, P: int, T: int) -> torch.Tensor:
        need = int(self.lib.dex_spk_forward_workspace_bytes(P, T))
        if need == 0:
            raise ValueError(f"{P} rows of {T} frames are more than one call takes")
        return super().workspace(need)


_context = per_device(_Spk)


def normalize_volume(wav: torch.Tensor, target_dBFS: float = AUDIO_NORM_TARGET_DBFS, increase_only: bool = True, lengths=None) -> torch.Tensor:
    """resemblyzer's ``normalize_volume(wav, target_dBFS, increase_only=True)`` per row: dBFS = 10 log10(mean(wav^2)) with the mean in
    fp64; a row louder than the target is returned unchanged, a quieter one is multiplied by 10^((target - dBFS) / 20) (rounded to
    fp32, as numpy multiplies a float32 array by a scalar).  Only ``increase_only=True`` - what metric.py:139 calls - is built."""
    if not increase_only:
        raise ValueError("normalize_volume: only increase_only=True (the reference's call) is built")
    if not math.isfinite(float(target_dBFS)):
        raise ValueError(f"normalize_volume: target_dBFS must be finite, got {target_dBFS}")
    x, ln, one = device_rows(wav, lengths, "normalize_volume", refuse=ValueError)
    ctx = _context(x.device)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = ctx.lib.dex_spk_normalize_volume(ctx.h, x.data_ptr(), i32_ptr(ln), x.shape[0], x.shape[1], float(target_dBFS), out.data_ptr(),
                                              stream(x.device))
    ctx.check(rc, "dex_spk_normalize_volume")
    return out[0] if one else out


def wav_to_mel_spectrogram(wav: torch.Tensor, lengths=None) -> torch.Tensor:
    """resemblyzer's ``wav_to_mel_spectrogram``: ``librosa.feature.melspectrogram(y, sr=16000, n_fft=400, hop_length=160, n_mels=40).T``
    (center=True with zero padding, periodic Hann, POWER spectrogram, Slaney mels with area normalisation, no logarithm) for wav [n] or
    a ragged batch [B, n] -> float32 [1 + n // 160, 40] or [B, 1 + n // 160, 40]; row b fills 1 + lengths[b] // 160 frames, 0 past them."""
    x, ln, one = device_rows(wav, lengths, "wav_to_mel_spectrogram", refuse=ValueError)
    ctx = _context(x.device)
    B, n = x.shape
    mel = torch.empty(B, n // HOP + 1, N_MELS, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = ctx.lib.dex_spk_mel(ctx.h, x.data_ptr(), i32_ptr(ln), B, n, mel.data_ptr(), stream(x.device))
    ctx.check(rc, "dex_spk_mel")
    return mel[0] if one else mel


def preprocess_wav(wav: torch.Tensor, source_sr: Optional[int] = None, lengths=None):
    """metric.py:115-142 on the device for wav [n] or a ragged batch [B, n]: resample from ``source_sr`` to 16 kHz where it differs
    (``wavprep.resample``: resampy's kaiser_best in fp64, rounded to fp32 once; current librosa resamples with soxr), then
    ``normalize_volume(wav, -30, increase_only=True)``.  ``trim_long_silences`` (webrtcvad) is LEFT OUT: trim on the host first for
    the reference's exact number.  Returns (wav fp32 [n'] or [B, max n'], host int32 lengths)."""
    x, ln, one = device_rows(wav, lengths, "preprocess_wav", refuse=ValueError)
    if source_sr is not None and int(source_sr) <= 0:
        raise ValueError(f"preprocess_wav: source_sr must be positive, got {source_sr}")
    x, ln = resample_to_16k(x, ln, source_sr)
    out = normalize_volume(x, AUDIO_NORM_TARGET_DBFS, True, ln)
    return (out[0] if one else out), ln


class VoiceEncoder:
    """resemblyzer's ``VoiceEncoder`` on one MI355X.  ``load_state_dict`` takes resemblyzer's checkpoint (``pretrained.pt``)."""

    def __init__(self, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("VoiceEncoder runs on an MI355X only (no CPU path)")
        self.device = torch.device("cuda", device_index(device))
        self._ctx = _Spk(self.device)
        self._loaded = False

    def load_state_dict(self, sd, strict: bool = True):
        upload_weights(self._ctx, self._ctx.lib.dex_spk_load, route_state_dict(sd), self.device)
        self._loaded = True
        return self

    def _need_weights(self, what: str):
        if not self._loaded:
            raise ValueError(f"{what}: the encoder's weights are not loaded (load_state_dict)")

    def forward(self, mels: torch.Tensor) -> torch.Tensor:
        """mels [P, T, 40] (T >= 1) -> unit-norm embeddings [P, 256]."""
        self._need_weights("VoiceEncoder.forward")
        on_device(mels, "VoiceEncoder.forward", ValueError)
        if mels.dim() != 3 or mels.shape[2] != N_MELS or mels.shape[0] < 1 or mels.shape[1] < 1:
            raise ValueError(f"VoiceEncoder.forward: expected mels [P, T, {N_MELS}] with P, T >= 1, got {tuple(mels.shape)}")
        x = mels.to(device=self.device, dtype=torch.float32).contiguous()
        P, T, _ = x.shape
        ctx = self._ctx
        ws = ctx.workspace(P, T)
        out = torch.empty(P, EMBED, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = ctx.lib.dex_spk_forward(ctx.h, x.data_ptr(), P, T, out.data_ptr(), ws.data_ptr(), ws.numel(), stream(self.device))
        ctx.check(rc, "dex_spk_forward")
        return out

    __call__ = forward

    def _embed(self, x: torch.Tensor, ln: Sequence[int], rate: float, min_coverage: float, want_partials: bool):
        slices = [compute_partial_slices(n, rate, min_coverage) for n in ln]
        counts = np.array([len(m) for _, m in slices], dtype=np.int32)
        starts = np.array([m.start for _, ms in slices for m in ms], dtype=np.int32)
        B, n = x.shape
        P = len(starts)
        ctx = self._ctx
        ws = ctx.workspace(P, PARTIALS_N_FRAMES)
        out = torch.empty(B, EMBED, dtype=torch.float32, device=self.device)
        partials = torch.empty(P, EMBED, dtype=torch.float32, device=self.device) if want_partials else None
        with torch.cuda.device(self.device):
            rc = ctx.lib.dex_spk_embed(ctx.h, x.data_ptr(), i32_ptr(ln), B, n, i32_ptr(counts), i32_ptr(starts), P, out.data_ptr(),
                                       partials.data_ptr() if want_partials else None, ws.data_ptr(), ws.numel(), stream(self.device))
        ctx.check(rc, "dex_spk_embed")
        return out, partials, slices

    def embed_utterance(self, wav: torch.Tensor, return_partials: bool = False, rate: float = 1.3, min_coverage: float = 0.75):
        """wav [n] (a preprocessed 16 kHz wav) -> unit-norm embedding [256]; with ``return_partials`` also the partial embeddings
        [n_partials, 256] and the wav slices.  The wav counts as zero-padded to the last slice's end where it is shorter."""
        self._need_weights("VoiceEncoder.embed_utterance")
        if isinstance(wav, torch.Tensor) and wav.dim() != 1:
            raise ValueError(f"VoiceEncoder.embed_utterance: expected a wav [n], got {tuple(wav.shape)}")
        x, ln, _ = device_rows(wav, None, "VoiceEncoder.embed_utterance", refuse=ValueError)
        out, partials, slices = self._embed(x.to(self.device), ln, rate, min_coverage, return_partials)
        return (out[0], partials, slices[0][0]) if return_partials else out[0]

    def embed_utterances(self, wavs: torch.Tensor, lengths=None, rate: float = 1.3, min_coverage: float = 0.75) -> torch.Tensor:
        """A ragged padded batch wavs [B, n], row b ``lengths[b]`` samples -> [B, 256]: all utterances' partials in ONE network
        call.  Row b is bitwise ``embed_utterance(wavs[b, :lengths[b]])``."""
        self._need_weights("VoiceEncoder.embed_utterances")
        if isinstance(wavs, torch.Tensor) and wavs.dim() != 2:
            raise ValueError(f"VoiceEncoder.embed_utterances: expected wavs [B, n], got {tuple(wavs.shape)}")
        x, ln, _ = device_rows(wavs, lengths, "VoiceEncoder.embed_utterances", refuse=ValueError)
        return self._embed(x.to(self.device), ln, rate, min_coverage, False)[0]

    def embed_speaker(self, wavs, lengths=None, **kwargs) -> torch.Tensor:
        """resemblyzer's ``embed_speaker``: the L2-normalised mean of the utterance embeddings.  ``wavs`` is [B, n] with ``lengths``
        or a list of wavs [n_b]."""
        if not isinstance(wavs, torch.Tensor):
            wavs, lengths = pad_wavs(wavs, self.device)
        e = self.embed_utterances(wavs, lengths, **kwargs)
        m = e.mean(dim=0)
        return m / torch.linalg.vector_norm(m)


def cosine(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """calculate_accept (metric.py:69-79): <a, b> / (|a| |b|) per row of a, b [B, D] -> [B]."""
    for t in (a, b):
        on_device(t, "cosine", ValueError)
    if a.dim() != 2 or tuple(a.shape) != tuple(b.shape) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"cosine: expected two [B, D] tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
    a = a.to(torch.float32).contiguous()
    b = b.to(device=a.device, dtype=torch.float32).contiguous()
    ctx = _context(a.device)
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = ctx.lib.dex_spk_cosine(ctx.h, a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], out.data_ptr(), stream(a.device))
    ctx.check(rc, "dex_spk_cosine")
    return out


def _encoder(encoder, what: str) -> "VoiceEncoder":
    if not isinstance(encoder, VoiceEncoder):
        raise ValueError(f"{what}: pass encoder=VoiceEncoder(device) with resemblyzer's weights loaded (the library ships no checkpoint)")
    encoder._need_weights(what)
    return encoder


def paired_cosine(what, prepare, embed, syn, trg) -> torch.Tensor:
    """The similarity of B pairs, for this module's d-vectors and for ``wavlm``'s x-vectors: each side ``(wavs, lengths, sr)`` through
    ``prepare(wavs, lengths, sr)`` -> (rows [B, n] or [n] at 16 kHz, host lengths), both stacked as 2 B rows, embedded in ONE
    ``embed(rows, lengths)`` call -> cos [B]."""
    (s, sl), (t, tl) = prepare(*syn), prepare(*trg)
    s, t = (v[None] if v.dim() == 1 else v for v in (s, t))
    if s.shape[0] != t.shape[0]:
        raise ValueError(f"{what}: {s.shape[0]} synthesised rows against {t.shape[0]} reference rows")
    B, n = s.shape[0], max(s.shape[1], t.shape[1])
    both = torch.zeros(2 * B, n, dtype=torch.float32, device=s.device)
    both[:B, : s.shape[1]] = s
    both[B:, : t.shape[1]] = t
    e = embed(both, np.concatenate([sl, tl]))
    return cosine(e[:B], e[B:])


def _similarity(what, encoder, syn, syn_lengths, syn_sr, trg, trg_lengths, trg_sr) -> torch.Tensor:
    """Both sides through ``preprocess_wav``, embedded in ONE ``embed_utterances`` call -> cos [B]."""
    encoder = _encoder(encoder, what)
    return paired_cosine(what, lambda x, ln, sr: preprocess_wav(x, sr, ln), encoder.embed_utterances, (syn, syn_lengths, syn_sr),
                         (trg, trg_lengths, trg_sr))


def mean_stderr(cos):
    """(mean, std / sqrt(n)) of cosines (a tensor or an array) with numpy's population std: the error bar of ``asv_score``."""
    c = (cos.double().cpu().numpy() if torch.is_tensor(cos) else np.asarray(cos, np.float64)).reshape(-1)
    return float(np.mean(c)), float(np.std(c) / np.sqrt(len(c)))


def speaker_similarity(syn: torch.Tensor, trg: torch.Tensor, syn_lengths=None, trg_lengths=None, source_sr: Optional[int] = 22050,
                       encoder: Optional[VoiceEncoder] = None) -> torch.Tensor:
    """metric.py:69-79 for a batch: syn, trg [B, n] (or [n]) at ``source_sr`` Hz, rows of ``*_lengths`` samples -> cos [B] on the
    device.  Both sides go through ``preprocess_wav`` and are embedded in ONE ``embed_utterances`` call of 2 B utterances."""
    return _similarity("speaker_similarity", encoder, syn, syn_lengths, source_sr, trg, trg_lengths, source_sr)


def asv_score(syn, trg, syn_lengths=None, trg_lengths=None, source_sr: Optional[int] = 22050, encoder: Optional[VoiceEncoder] = None):
    """calculate_asv_score (metric.py:81-95): (mean, std / sqrt(n)) of the pairs' cosines, with numpy's population std."""
    return mean_stderr(speaker_similarity(syn, trg, syn_lengths, trg_lengths, source_sr, encoder))


def score_synthesis(audio: Sequence, ref_wavs: Sequence, sr: int = 22050, ref_sr: Optional[int] = None,
                    encoder: Optional[VoiceEncoder] = None):
    """The scores of ``synthesize.synthesize_tokens``' output: ``audio`` is its list of int16 waveforms (``sr`` Hz), ``ref_wavs`` the
    reference wavs in the same order (float arrays or tensors in [-1, 1], ``ref_sr`` Hz, default ``sr``) -> (cos [B] on the device,
    mean, stderr).  int16 waveforms are scaled by 1 / 32768; the score does not depend on that scale."""
    if len(audio) != len(ref_wavs) or len(audio) < 1:
        raise ValueError(f"score_synthesis: {len(audio)} waveforms against {len(ref_wavs)} reference wavs")
    encoder = _encoder(encoder, "score_synthesis")
    syn, sl = pad_wavs(audio, encoder.device, scale_int16=True)
    trg, tl = pad_wavs(ref_wavs, encoder.device, scale_int16=True)
    cos = _similarity("score_synthesis", encoder, syn, sl, sr, trg, tl, ref_sr or sr)
    return (cos,) + mean_stderr(cos)
