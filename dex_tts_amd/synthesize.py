"""Counterpart of the reference's synthesize flow around the decoder (GeDEX-TTS/synthesize.py:15-45 ->
GeDEXTTS.forward, model/tts.py:34-55; DEX-TTS/synthesize.py:88-110 -> DeXTTS.forward, model/tts.py:53-73), for the part
this library owns: everything from the aligned text-encoder output ``mu_y`` to the mel.

    seed_init(seed)                                   src/utils.py:94-103 (torch / numpy / random seeds)
    model = Diffusion(**cfg.model.decoder, dit_cfg=cfg.model.dit, n_feats, n_spks, spk_emb_dim)      tts.py:25 / :30
    model.load_state_dict(ckpt['ema' | 'state_dict'] entries under 'decoder.')                         synthesize.py:20-24
    y_max_length_ = fix_len_compatibility(y_max_length)                                              tts.py:40
    y_mask = sequence_mask(y_lengths, y_max_length_).unsqueeze(1)                                    tts.py:43
    dec_out = decoder(mu_y, y_mask, mu_y, [ref, ref_lengths, sty, sty_lengths,] n_timesteps, temperature, spk, infer=True)
    dec_out = dec_out[:, :, :y_max_length]                                                            tts.py:54

The text encoder / duration model / vocoder are not part of this library: ``mu_y`` comes in as an
array (e.g. dumped from the reference, or synthetic).  CLI:

    python -m dex_tts_amd.synthesize --config <reference base.yaml> --mu mu_y.npy [--lengths 210,180] [--ckpt model.pth]
           [--n_timesteps 50] [--temperature 1.5] [--seed 100] [--precision fp32|bf16|fp16] [--solver euler|heun|dpmpp_2m] --out mel.npy
           [--wav out.wav [--griffin_iters 60]]        (Griffin-Lim waveforms of the mels, dex_tts_amd.griffin_lim)
"""
from __future__ import annotations

import argparse
import random
from typing import Optional, Sequence

import numpy as np
import torch

from .config import ScoreNetConfig, fix_len_compatibility, from_reference_yaml
from .diffusion import Diffusion, from_config


def seed_init(seed: int = 100):
    """src/utils.py:94-103."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)


def sequence_mask(length: torch.Tensor, max_length: Optional[int] = None) -> torch.Tensor:
    """model/utils.py:6-10."""
    if max_length is None:
        max_length = int(length.max())
    x = torch.arange(int(max_length), dtype=length.dtype, device=length.device)
    return x.unsqueeze(0) < length.unsqueeze(1)


def config_from_model_section(model: dict, variant: str) -> ScoreNetConfig:
    """``cfg.model`` of a reference base.yaml -> ScoreNetConfig (tts.py:25: Diffusion(n_feats, **decoder, dit_cfg=dit,
    n_spks=..., spk_emb_dim=...)); DEX configs carry n_spks = 0, which Diffusion treats like 1 (no speaker plane)."""
    return from_reference_yaml(model["decoder"], model["dit"], variant, n_spks=max(int(model.get("n_spks") or 1), 1),
                               spk_emb_dim=int(model.get("spk_emb_dim", 64)), n_feats=int(model.get("n_feats", 80)))


def load_reference_config(path: str) -> ScoreNetConfig:
    import yaml
    with open(path) as f:
        model = yaml.safe_load(f)["model"]
    variant = "dex" if "tv_encoder" in model else "gedex"
    return config_from_model_section(model, variant)


def decoder_state_dict(ckpt: dict, ema: bool = True) -> dict:
    """The decoder's entries of a reference checkpoint (synthesize.py:20-24), without the 'decoder.' prefix."""
    sd = ckpt["ema"] if (ema and "ema" in ckpt) else ckpt.get("state_dict", ckpt)
    return {k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}


def prepare(mu_y: torch.Tensor, y_lengths: torch.Tensor, n_stages: int = 2):
    """tts.py:39-43,49: pad mu_y to the U-Net-compatible length and build y_mask.  Returns (mu_y_padded, y_mask [B,1,T'],
    y_max_length)."""
    y_max_length = int(y_lengths.max())
    t_pad = fix_len_compatibility(y_max_length, n_stages)
    B, F, T = mu_y.shape
    if T < t_pad:
        mu_y = torch.nn.functional.pad(mu_y, (0, t_pad - T))
    mu_y = mu_y[:, :, :t_pad]
    y_mask = sequence_mask(y_lengths, t_pad).unsqueeze(1).to(mu_y.dtype)
    return mu_y * y_mask, y_mask, y_max_length              # the aligned mu_y is zero past each utterance's length (attn path is masked)


@torch.no_grad()
def decode(model: Diffusion, mu_y: torch.Tensor, y_lengths: torch.Tensor, n_timesteps: int = 50, temperature: float = 1.5,
           spk: Optional[torch.Tensor] = None, ref: Optional[Sequence[torch.Tensor]] = None, ref_lengths=None,
           sty: Optional[torch.Tensor] = None, sty_lengths=None) -> torch.Tensor:
    """mu_y [B,80,T] (aligned encoder output) -> mel [B,80,y_max_length], exactly the decoder leg of GeDEXTTS.forward /
    DeXTTS.forward (tts.py:49-55 / :66-73)."""
    mu_p, y_mask, y_max = prepare(mu_y, y_lengths, len(model.cfg.dim_mults))
    if model.cfg.variant == "dex":
        out = model(mu_p, y_mask, mu_p, ref, ref_lengths, sty, sty_lengths, n_timesteps=n_timesteps, temperature=temperature,
                    spk=spk, infer=True)
    else:
        out = model(mu_p, y_mask, mu_p, n_timesteps=n_timesteps, temperature=temperature, spk=spk, infer=True)
    return out[:, :, :y_max]


MAX_VALUE = 32768.0          # synthesize.py:13-14


@torch.no_grad()
def synthesize_tokens(model, vocoder, x: torch.Tensor, x_lengths: torch.Tensor, n_timesteps: int = 50, temperature: float = 1.5,
                      spk: Optional[torch.Tensor] = None, length_scale: float = 1.0, style: Optional[dict] = None,
                      exact_lengths: bool = False, chunk_frames: Optional[int] = None):
    """synthesize.py:31-38 from the token sequence on (the text front-end - cleaners, CMU dictionary, ``intersperse`` - is the
    reference's and stays on the host): ``model`` a ``dex_tts_amd.tts.GeDEXTTS`` / ``DeXTTS``, ``vocoder`` a
    ``dex_tts_amd.vocoder.Generator``; DEX takes ``style = dict(ref, ref_lengths, sty, sty_lengths, lf0, lf0_lengths)``
    (DEX-TTS/synthesize.py:47-95).  Returns (list of int16 waveforms cut to each utterance's length, y_dec [B,80,Ty], attn).

    ``exact_lengths``: pass the encoder's ``y_len`` to the vocoder, so that every utterance of the batch is vocoded as if alone at its
    own length (``Generator.forward(y_dec, lengths)``).  Batched callers want True: past an utterance's last frame ``y_dec`` is 0, a
    log-mel of 0 is a loud broadband frame, and the generator's convolutions carry it 6 to 23 frames back into the valid tail, where the
    error against the utterance vocoded alone is as large as the signal (0.16 - 0.40 against a signal std of 0.15 - 0.27 in the
    project's four test geometries).  The reference synthesises at B = 1 and never meets this.  The default stays False, the padded
    call cut afterwards, so that existing results do not change; at B = 1 the two are the same.

    ``chunk_frames`` = N: vocode window by window of N mel frames (``Generator.forward(..., chunk_frames=N)``): the same waveforms, with
    a vocoder workspace that does not grow with the utterance.  Composes with ``exact_lengths``."""
    if style is not None:
        y_enc, y_dec, attn = model(x, x_lengths, style["ref"], style["ref_lengths"], style["sty"], style["sty_lengths"], style["lf0"],
                                   style["lf0_lengths"], n_timesteps=n_timesteps, temperature=temperature, spk=spk, length_scale=length_scale)
    else:
        y_enc, y_dec, attn = model(x, x_lengths, n_timesteps=n_timesteps, temperature=temperature, spk=spk, length_scale=length_scale)
    y_len = model.encoder._last["y_len"]
    chunk = {} if chunk_frames is None else {"chunk_frames": chunk_frames}
    wav = (vocoder(y_dec, y_len, **chunk) if exact_lengths else vocoder(y_dec, **chunk)).squeeze(1).clamp(-1, 1)      # [B, Ty * hop]
    hop = wav.shape[-1] // y_dec.shape[-1]
    y_len = y_len.to(torch.int64).cpu()
    audio = (wav.cpu().numpy() * MAX_VALUE).astype(np.int16)
    return [audio[b, : int(y_len[b]) * hop] for b in range(audio.shape[0])], y_dec, attn


def speaker_scores(encoder, audio, ref_wavs, sr: int = 22050, ref_sr: Optional[int] = None):
    """The reference's speaker-similarity score (src/metric.py:69-95) of ``synthesize_tokens``' list of int16 waveforms against the
    reference wavs, in the same order, on the device -> (cos [B], mean, stderr).  ``encoder`` is a ``speaker.VoiceEncoder`` with
    resemblyzer's weights loaded (speaker.py states what the score leaves out: the VAD trim)."""
    from . import speaker
    return speaker.score_synthesis(audio, ref_wavs, sr, ref_sr, encoder=encoder)


def sim_scores(model, audio, ref_wavs, sr: int = 22050, ref_sr: Optional[int] = None):
    """The WavLM x-vector speaker similarity (SIM) of ``synthesize_tokens``' list of int16 waveforms against the reference wavs, in
    the same order, on the device -> (cos [B], mean, stderr).  ``model`` is a ``wavlm.WavLMXVector`` with the checkpoint's weights
    loaded (wavlm.py states what the score is and its departures: the row-alone batching, the resampler, ``do_normalize``)."""
    from . import wavlm
    return wavlm.score_synthesis(model, audio, ref_wavs, sr, ref_sr)


def ecapa_sim_scores(model, audio, ref_wavs, sr: int = 22050, ref_sr: Optional[int] = None):
    """The WavLM-large + ECAPA-TDNN speaker similarity (the SIM-o of zero-shot TTS tables) of ``synthesize_tokens``' list of int16
    waveforms against the reference wavs, in the same order, on the device -> (cos [B], mean, stderr).  ``model`` is an
    ``ecapa.WavLMEcapa`` with the checkpoint's weights loaded (ecapa.py states what the score is and its departures: the row-alone
    batching, the resampler, and that it has not been checked against the real checkpoint)."""
    from . import ecapa
    return ecapa.score_synthesis(model, audio, ref_wavs, sr, ref_sr)


def mos_scores(model, audio, sr: int = 22050, domain: int = 0, judge: int = 288):
    """The UTMOS naturalness score (predicted MOS) of ``synthesize_tokens``' list of int16 waveforms (``sr`` Hz), on the device ->
    (mos [B], mean, stderr).  ``model`` is a ``mos.UTMOS`` with the checkpoint's weights loaded (mos.py states what the score is and
    its departures: the row-alone batching, the resampler, and that it has not been checked against the real checkpoint)."""
    from . import mos
    return mos.score_synthesis(model, audio, sr, domain, judge)


def asr_scores(model, audio, texts, sr: int = 22050):
    """The reference's ASR score (src/metric.py:21-67) of ``synthesize_tokens``' list of int16 waveforms (``sr`` Hz) against the
    input texts, in the same order -> (transcripts, cer_mean, cer_stderr, wer_mean, wer_stderr).  ``model`` is an
    ``asr.Wav2Vec2CTC`` with the checkpoint's weights loaded (asr.py states the one departure: the resampler)."""
    from . import asr
    if len(audio) != len(texts) or len(audio) < 1:
        raise ValueError(f"asr_scores: {len(audio)} waveforms against {len(texts)} texts")
    if not isinstance(model, asr.Wav2Vec2CTC):
        raise ValueError("asr_scores: pass an asr.Wav2Vec2CTC with the checkpoint's weights loaded (the library ships none)")
    preds = model.transcribe(list(audio), None, sr)
    return (preds, *asr.score_transcripts(texts, preds))


def align_scores(model, audio, texts, sr: int = 22050):
    """Word and character timings of ``synthesize_tokens``' list of int16 waveforms (``sr`` Hz) against the input texts, in the same
    order, and the recogniser's likelihood of each text -> (alignments, nll_per_char_mean, nll_per_char_stderr); an alignment is a
    row of ``asr.Wav2Vec2CTC.align`` (ctc_align.py holds the definitions).  ``model`` is an ``asr.Wav2Vec2CTC`` with the checkpoint's
    weights loaded.  The same departure as the other scores: the waveforms are resampled by ``wavprep.resample``."""
    from . import asr, ctc_align
    if len(audio) != len(texts) or len(audio) < 1:
        raise ValueError(f"align_scores: {len(audio)} waveforms against {len(texts)} texts")
    if not isinstance(model, asr.Wav2Vec2CTC):
        raise ValueError("align_scores: pass an asr.Wav2Vec2CTC with the checkpoint's weights loaded (the library ships none)")
    return ctc_align.alignment_score(texts, list(audio), sr=sr, model=model)


def whisper_scores(model, spec, vocab, audio, texts, sr: int = 22050, long_form: bool = False, num_beams: int = 1, length_penalty: float = 1.0,
                   policy=None):
    """The Whisper ASR score of ``synthesize_tokens``' list of int16 waveforms (``sr`` Hz) against the input texts, in the same order
    -> (transcripts, cer_mean, cer_stderr, wer_mean, wer_stderr).  ``model`` is a ``whisper.Whisper`` with the checkpoint's weights
    loaded, ``spec`` its ``GenerationSpec`` and ``vocab`` its token strings (whisper.py states the definitions and the two
    departures: the resampler, and the reference's ``normalize_sentence`` in place of Whisper's English normaliser).  ``long_form=True``
    scores waveforms of any length by timestamp-rule decoding over 30 s windows (``spec`` with the timestamp fields).  ``num_beams`` > 1
    decodes by beam search with ``length_penalty`` (not with the long form).  ``policy`` (a ``whisper.DecodingPolicy``): temperature
    fallback under the compression-ratio, log-prob and no-speech thresholds, short or long form (not with beams)."""
    from . import whisper
    if len(audio) != len(texts) or len(audio) < 1:
        raise ValueError(f"whisper_scores: {len(audio)} waveforms against {len(texts)} texts")
    if not isinstance(model, whisper.Whisper):
        raise ValueError("whisper_scores: pass a whisper.Whisper with the checkpoint's weights loaded (the library ships none)")
    return whisper.whisper_score(list(audio), texts, model=model, spec=spec, vocab=vocab, sr=sr, long_form=long_form, num_beams=num_beams,
                                 length_penalty=length_penalty, policy=policy)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="a reference base.yaml (GeDEX-TTS/config/*/base.yaml, DEX-TTS/config/*/base.yaml)")
    ap.add_argument("--mu", required=True, help=".npy with mu_y [B,80,T] (or [80,T])")
    ap.add_argument("--lengths", default=None, help="comma-separated valid frame counts (default: T for every utterance)")
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (model-train-best.pth); default: portable synthetic weights")
    ap.add_argument("--style", default=None, help="DEX: .npz with ref (6 x [B,mid,Tr]), ref_lengths, sty [B,mid,Ts], sty_lengths")
    ap.add_argument("--n_timesteps", type=int, default=50)
    ap.add_argument("--temperature", type=float, default=1.5)
    ap.add_argument("--seed", type=int, default=100)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--solver", default="euler", choices=["euler", "heun", "dpmpp_2m"],
                    help="euler: what the reference wires; heun: 2n - 1 network evaluations; dpmpp_2m: second order at n evaluations")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True)
    ap.add_argument("--wav", default=None, help="also write each mel as a Griffin-Lim waveform (no vocoder weights needed): OUT.wav for "
                                                "one utterance, OUT_<b>.wav for utterance b of a batch")
    ap.add_argument("--griffin_iters", type=int, default=60, help="Griffin-Lim iterations of --wav (audio/tools.py inv_mel_spec)")
    a = ap.parse_args(argv)

    seed_init(a.seed)
    cfg = load_reference_config(a.config)
    model = from_config(cfg)
    if a.ckpt:
        sd = decoder_state_dict(torch.load(a.ckpt, map_location="cpu"))
        if not sd:
            raise SystemExit(f"{a.ckpt}: no 'decoder.*' entries — not a DEX-TTS / GeDEX-TTS model checkpoint")
        model.load_state_dict(sd, strict=True)             # as the reference does (synthesize.py:20-24): a partial load must not pass silently
    else:
        from . import synth
        from .config import param_shapes
        w = synth.make_weights(param_shapes(cfg))
        sd = {}
        for k, v in w.items():
            sd[f"denoise_fn.{k}"] = torch.from_numpy(v)
            sd[f"precond_model.model.{k}"] = torch.from_numpy(v)
        model.load_state_dict(sd, strict=True)
    model = model.to(a.device).eval()
    model.precision = a.precision
    model.solver = a.solver
    mu = torch.from_numpy(np.load(a.mu).astype(np.float32))
    if mu.dim() == 2:
        mu = mu[None]
    lengths = torch.tensor([int(v) for v in a.lengths.split(",")] if a.lengths else [mu.shape[2]] * mu.shape[0])
    kw = {}
    if cfg.variant == "dex":
        if not a.style:
            raise SystemExit("DEX configs need --style (reference-wav encoder outputs)")
        s = np.load(a.style)
        kw = dict(ref=[torch.from_numpy(r).to(a.device) for r in s["ref"]], ref_lengths=torch.from_numpy(s["ref_lengths"]).to(a.device),
                  sty=torch.from_numpy(s["sty"]).to(a.device), sty_lengths=torch.from_numpy(s["sty_lengths"]).to(a.device))
    mel = decode(model, mu.to(a.device), lengths.to(a.device), a.n_timesteps, a.temperature, **kw)
    np.save(a.out, mel.cpu().numpy())
    print(f"{a.out}: mel {tuple(mel.shape)}")
    if a.wav:
        write_wavs(mel, lengths, a.wav, a.griffin_iters)


def write_wavs(mel: torch.Tensor, lengths: torch.Tensor, path: str, n_iters: int = 60):
    """--wav: each decoded mel [80, lengths[b]] through Griffin-Lim (dex_tts_amd.griffin_lim.mel_to_wav, the reference's
    inv_mel_spec) -> a float32 wav of 256 (lengths[b] - 2) samples at 22050 Hz; path for one utterance, <stem>_<b><ext> for a batch."""
    import os
    from scipy.io.wavfile import write
    from .griffin_lim import SAMPLING_RATE, mel_to_wav

    n = [int(v) for v in lengths.tolist()]
    wav = mel_to_wav(mel, n, n_iters=n_iters).cpu().numpy()
    stem, ext = os.path.splitext(path)
    for b in range(wav.shape[0]):
        out = path if wav.shape[0] == 1 else f"{stem}_{b}{ext or '.wav'}"
        write(out, SAMPLING_RATE, wav[b, : 256 * (n[b] - 2)])
        print(f"{out}: {256 * (n[b] - 2)} samples (Griffin-Lim, {n_iters} iterations)")


if __name__ == "__main__":
    main()
