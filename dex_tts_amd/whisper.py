"""The Whisper ASR score on the device: the recogniser zero-shot TTS work reports its WER with (``asr.py`` stays the reference's
wav2vec 2.0 CTC score; numbers from the two recognisers are not comparable).  HF's ``WhisperForConditionalGeneration`` in eval
mode, fp32 throughout: log-mel front end, encoder, decoder with a key/value cache, greedy decoding and beam search.

    WhisperConfig(...)                         HF's field names; defaults = openai/whisper-large-v3
    Whisper(config=None, device='cuda'):       load_state_dict (HF keys), log_mel, encode, forward, generate, generate_beam, transcribe;
                                               long form: log_mel_long, generate_segments, transcribe_long
    GenerationSpec(prompt_ids, suppress_tokens, begin_suppress_tokens, eos_token_id, no_timestamps_token_id=None,
                   max_initial_timestamp_index=None);  GenerationSpec.from_generation_config(..., timestamps=False)
    load_vocab(path), decode(ids, vocab)       host only
    whisper_score(wavs, texts, model=, spec=, vocab=, long_form=False, num_beams=1, length_penalty=1.0)
                                               -> (transcripts, cer_mean, cer_stderr, wer_mean, wer_stderr)

Everything runs in libdexamd.so (``csrc/whisper.hip``, C ABI ``dex_whisper_*``).  Nothing downloads and no checkpoint is shipped:
weights, the generation config and the vocabulary come from dicts or local files the caller names.  A row's features, logits and ids
are bitwise those of the row alone: every launch fixes its split and summation order from the config and the position.

Definitions (the contract)

Front end = ``WhisperFeatureExtractor``.  Input is 16 kHz; other rates go through ``wavprep.resample`` (kaiser_best), as in the other
two scores.  A row is zero-padded to ``n_samples = 2 * max_source_positions * 160`` (480 000 for the real models); a longer row
raises ``ValueError`` in ``log_mel``, ``generate`` and ``transcribe`` (a metric must not truncate silently; the long form below takes it).  Reflect-pad by 200, periodic
Hann(400), 400-point DFT at hop 160, power, the last frame dropped, mel (``num_mel_bins`` 80 or 128, Slaney scale and norm,
0 - 8000 Hz; the matrix is built on the host in float64, ``mel_filters``), ``log10(max(., 1e-10))``, floored at the row's own maximum
- 8, ``(x + 4) / 4``.  The device computes all of it in fp64 and rounds to fp32 once.

Encoder.  ``conv1`` (k 3, p 1) + erf GELU, ``conv2`` (k 3, s 2, p 1) + GELU, ``+ embed_positions`` (loaded, not recomputed), pre-LN
layers (``k_proj`` without bias, scale head_dim^-1/2 on q, GELU FFN), a final ``layer_norm``.  No attention mask: the padding is
attended to, as in HF, so a batch row is the row alone by construction.

Decoder step at position p.  Input ``embed_tokens[id] + embed_positions[p]``; per layer ``self_attn_layer_norm`` -> self-attention
over cache positions 0 .. p -> residual; ``encoder_attn_layer_norm`` -> cross-attention over all ``max_source_positions`` encoder
frames (its K and V are computed once per utterance) -> residual; ``final_layer_norm`` -> ``fc1`` -> GELU -> ``fc2`` -> residual;
then ``decoder.layer_norm`` and logits = h x ``embed_tokens``^T.  ``forward`` runs through this cached step one position at a time;
there is no other decoder path.

Greedy decoding is the library's own definition, a stated subset of HF ``generate``.  The prompt positions are fed first.  At
new-token step i ``suppress_tokens`` are set to -inf, at i = 0 ``begin_suppress_tokens`` as well, and the argmax takes the lowest
index on ties.  A row is finished once it emits ``eos_token_id``; from then on its output is eos.  The loop ends when every row has
finished, after ``max_new_tokens``, or when ``len(prompt) + i`` reaches ``max_target_positions``: it never writes past the cache.
Not built: language detection, ``condition_on_prev_tokens``, token-level timestamps.  Timestamps are built for the long form only
(below); temperature fallback and the three thresholds are the policy (further below).

Beam search (``generate_beam``; ``generate``, ``transcribe``, ``whisper_score`` with ``num_beams`` > 1) is HF ``generate(num_beams=K,
do_sample=False, early_stopping=False, num_return_sequences=1)``, one utterance at a time.  K = ``num_beams``, V = ``vocab_size``, P =
``len(prompt)``, ``lp`` = ``length_penalty`` (default 1.0).  ``num_beams=1`` is the greedy path above, untouched and bitwise.

  State per utterance.  K running hypotheses, each with an accumulated score, initially ``[0, -1e9, ...]`` (step 0 is decided by beam
  0 alone); a pool of at most K finished hypotheses with scores; a ``done`` flag.

  Step i = 0, 1, ..., for each running beam r: the fp32 logits of the cached step; ``log_softmax`` over the whole, unmasked row,
  computed in fp64 from the fp32 logits (a stated departure: HF computes it in fp32); ``suppress_tokens`` -> -inf, at i = 0
  ``begin_suppress_tokens`` as well (masked ids are not renormalised away - HF's order: softmax first, processors second); the beam's
  running score is added in fp64.

  Candidates.  The 2K largest of the K x V accumulated scores, in descending order; ties go to the lowest flat index ``r V + id``.
  Fewer than 2K unmasked ids raise ``ValueError``.  A candidate is finished if its id is eos; on the last step, ``i = n_new - 1`` with
  ``n_new = min(max_new_tokens, max_target_positions - P)``, every candidate is finished.  The next running beams are the first K
  unfinished candidates, in order: their scores, ids and parents become the running state (on the last step it stays as it is).

  Pool.  Only a finished candidate of rank < K enters, with the score ``score / (i + 1)^lp`` (the eos counts in the length).  The
  old pool comes first, then the new entries in rank order; the best K are kept, ties go to the earlier entry.

  Stop.  After the step the utterance is done if it was the last step, or if the pool holds K entries and ``best running score /
  (i + 1)^lp <= worst pool score``.  Done is sticky: a done utterance's state no longer changes, whatever the others do.

  Result.  The pool's best hypothesis -> ``ids`` (padded with eos), ``lengths`` (the tokens before the eos; the full count of a
  capped hypothesis) and ``scores`` (its pool score, float64).  The pool is never empty at the end.  An utterance's ids, lengths and
  scores are bitwise those of the utterance alone at the same K.

  On the device.  U utterances of K beams are U x K rows of the step.  The cross-attention K / V is computed and stored once per
  utterance, and one workgroup per (head, utterance) streams it once for the K queries.  The self-attention cache never moves: row
  r writes its new k / v into its own row at position p and reads position t from row ``anc[r][t]``; after the selection
  ``anc'[r'][0..p] = anc[parent(r')][0..p]`` and ``anc'[r'][p + 1] = r'``, an int copy.  The prompt is fed on all K rows.  The
  step's tail (three launches: the normaliser's chunk sums, the 2K best of every chunk of 2048 ids by the fp64 score, and the
  merge with the whole rule and the gather of the next step's embeddings) needs no host value; the host reads the done count every
  ``SYNC_EVERY`` steps.  Per query both attention forms keep the plain kernel's arithmetic bit for bit, so greedy and beam logits
  are comparable.

  Limits: ``2 <= K <= 8``; ``K x max_source_positions <= 13000`` (the K score rows of a cross-attention launch sit in LDS); ``U x K
  <= 32`` rows per network call, larger batches run ``32 // K`` utterances at a time.  Out of scope, each a ``ValueError`` naming the
  argument: ``timestamps=True`` or ``long_form=True`` with ``num_beams`` > 1 (the rule's per-row state would have to follow the
  parents), ``early_stopping`` other than ``False``, ``num_return_sequences`` > 1, sampling and temperature fallback.

Long form (``log_mel_long``, ``generate_segments``, ``transcribe_long``, ``whisper_score(long_form=True)``) mirrors HF
``generate(..., return_timestamps=True)`` at temperature 0 with ``condition_on_prev_tokens=False``: no no-speech, log-prob or
compression-ratio threshold, no fallback, no beams (beam search is built for the plain form only).  The spec carries ``no_timestamps_token_id`` (``timestamp_begin`` is that id + 1;
``from_generation_config(timestamps=True)`` fills it, leaves ``<|notimestamps|>`` out of the prompt and reads
``max_initial_timestamp_index``); a spec without it raises ``ValueError``, and so do fewer than ``max_source_positions + 1``
timestamp ids (``vocab_size - timestamp_begin``).

  Step rule.  At new-token step i of a window a row's logits pass, in HF's order, through ``begin_suppress_tokens`` (i = 0 only),
  ``suppress_tokens`` and the timestamp rule, in the order of operations of ``WhisperTimeStampLogitsProcessor.__call__``:
  ``no_timestamps_token_id`` -> -inf.  Pairing, with ``seq`` the new tokens so far: if the last token is a timestamp and the one
  before it is a timestamp too (or there is only one new token) every timestamp -> -inf; if the last is a timestamp and the one
  before it is not, ids [0, eos) -> -inf.  Monotonicity: if any timestamp was emitted, timestamps below ``last`` (in the "last is a
  timestamp, the one before is not" case) or below ``last + 1`` (otherwise) -> -inf.  At i = 0 every id below ``timestamp_begin``
  -> -inf, and with ``max_initial_timestamp_index`` every timestamp above ``timestamp_begin + max_initial_timestamp_index``.  Last,
  if ``logsumexp(timestamp logits) > max(text logits)`` over the masked row (text = every id below ``timestamp_begin``, eos
  included; both sides lack the same normaliser, so none is computed) every id below ``timestamp_begin`` -> -inf.  Then the argmax,
  lowest index on ties; finished and length bookkeeping as in the plain form.  The device keeps the rule's state (a row's last
  timestamp and its new-token count; its last two ids are in the ids buffer), so a step still needs no host value.  A masked id
  does not compete, and a row in which nothing competes (all NaN) yields id 0.

  Front end of a row of more than ``n_samples`` samples = ``WhisperFeatureExtractor(truncation=False)`` on that row alone: reflect-pad
  by 200 at the row's own ends, ``len // 160`` frames, the floor at the whole row's maximum - 8, fp64 rounded once.  A row of at most
  ``n_samples`` keeps ``log_mel``'s features (zero-padded, ``2 x max_source_positions`` frames).  ``F`` is the row's frame count.  A
  row above ``MAX_LONG_SAMPLES`` (30 minutes) raises ``ValueError``.  The fp64 log-spectrum of a call sits in a scratch buffer of
  rows x F_max x num_mel_bins doubles; rows are taken in groups that keep it under 1 GiB.

  Window loop.  ``seek = 0``; while ``seek < F``: ``n = min(F - seek, 2 x max_source_positions)``; the window's features are frames
  [seek, seek + n) followed by the feature value 0.0 up to the full window (HF's ``_get_input_segment``); encode, decode under the
  step rule from the prompt up to the cache's room; strip the trailing eos; cut the ids into segments and advance ``seek`` as
  ``_retrieve_segment`` does: consecutive timestamp pairs close segments; a single trailing timestamp means the whole window is
  consumed (``seek += n``); otherwise ``seek`` moves to the last pair's first timestamp index x 2 frames and the ids after that pair
  are discarded; with no pair at all the window is one segment and is consumed whole.  Times are ``seek x 0.01 + index x 0.02``
  seconds in float64.  A row's transcript is ``decode`` of its segments' ids joined (timestamp ids lie above eos and are skipped).

  The loop ends: ``seek`` grows by at least 2 frames per window (or reaches F).  A consumed window adds n >= 1, and n < 2 only for
  the last frame of the row.  Otherwise a pair exists and seek moves to its first timestamp's index x 2; that index is >= 1, because
  step 0 emits a timestamp (index >= 0), step 1 may not emit one (only one new token: all timestamps masked), and every later
  timestamp that follows text must exceed the last one emitted (``last + 1``), so the first member of any pair has index >= 1.

  Rows are independent: each window call gathers the rows still active (32 at most per network call); a row's features, segments
  and ids are bitwise those of the row alone.  One device-to-host copy of ids and lengths per window call is the only sync beyond
  the plain form's.

Fallback decoding (``DecodingPolicy``; ``policy=`` of ``generate``, ``transcribe``, ``generate_segments``, ``transcribe_long``,
``whisper_score``; ``None`` is the paths above, untouched) mirrors HF's ``generate_with_fallback``, ``_need_fallback``,
``_retrieve_avg_logprobs``, ``_retrieve_compression_ratio`` and ``WhisperNoSpeechDetection`` applied to ONE ROW ALONE: HF indexes its
skip and fallback flags by position in the shrinking fallback sub-batch; here a row's result is bitwise the row alone.

    DecodingPolicy(temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold=None, logprob_threshold=None,
                   no_speech_threshold=None, no_speech_token_id=None, seed=0);  DecodingPolicy.from_generation_config(config, ...)

  ``None`` switches a threshold off; ``no_speech_threshold`` requires ``logprob_threshold`` and ``no_speech_token_id``
  (``from_generation_config``: ``no_timestamps_token_id - 1``, as HF).  The first temperature is 0, temperatures rise, at most 8;
  anything else is a ``ValueError`` naming the field.  A policy with ``num_beams`` > 1 raises ``ValueError``.

  Per attempt and row the device keeps ``sum_logprob`` (fp64): over the new tokens, the emitted eos included, the sum of
  ``log_softmax(masked logits)[token]`` where the row is taken after ``begin_suppress_tokens``, ``suppress_tokens`` and, under
  timestamps, the timestamp rule, at temperature 1 (HF multiplies the temperature back in), normalised by an fp64 log-sum-exp over
  the surviving ids of the fp32 logits; ``n_scored``, the count of those tokens; ``avg_logprob = sum_logprob / n_scored``; and
  ``no_speech_prob``, the fp64 softmax of the UNPROCESSED logits at prompt position 0 (``<|startoftranscript|>``) at
  ``no_speech_token_id`` - the output projection at that one position, once per window, not per attempt (NaN without the id).
  The compression ratio stays on the host: HF's, on token bytes (``int(log2(V) / 8) + 1`` bytes per id, little endian,
  ``zlib.compress``) over the tokens HF passes (the eos included).

  Decision after an attempt, in HF's order: a retry is needed if the ratio exceeds its threshold or ``avg_logprob <
  logprob_threshold``; with ``no_speech_threshold``, ``avg_logprob < logprob_threshold and no_speech_prob > no_speech_threshold``
  skips the window instead (the long form adds the window's n frames to ``seek`` and emits no segment, the short form returns an
  empty row); otherwise the row is decoded again at the next temperature; after the last one its result stands.

  Sampling at T > 0 is the library's own (HF's ``torch.multinomial`` stream cannot be reproduced on a device): Gumbel-max.  The masked
  fp32 logits go to fp64, are divided by T, ``g = -log(-log(u))`` is added and the argmax is taken, lowest index on ties, through
  the greedy tail's finished / length / eos bookkeeping.  ``u = (w + 0.5) 2^-32`` with w a word of Philox4x32-10: key = ``seed`` (low,
  high 32 bits), counter = (id >> 2, new-token step i, attempt + 16 x seek, row key), word id & 3.  The row key defaults to the
  utterance's index in the call (``row_keys=``); ``seek`` is the window's first frame (0 in the short form).  The noise depends on
  nothing else: not the batch, not the rows decoded beside it.

  On the device.  One tail launch per step (``wsp_pick_policy_kernel``, plain and under the rule): sweep 1 is the greedy tail's own
  pass (the same ownership and fp32 reductions, so the rule's decision and at T = 0 the id are the existing tails' bit for bit);
  sweep 2 over the row, now in L2, sums exp(x - max) over the survivors in fp64 in an order fixed by V, perturbs, takes the argmax
  and adds the chosen id's log-probability to the row's sums.  A retry does NOT run the encoder again: the attempt decodes the rows
  that need one from the cross-attention K / V where the encoder left it (``wsp_attend_rows_kernel`` reads row ``rows[b]`` of the
  encoded batch).  Each attempt costs one device-to-host copy (ids, lengths and the statistics in one tensor).

  Departures from HF, stated plainly: the sampling stream is the library's; ``log_softmax`` and the no-speech softmax are fp64 (HF:
  fp32); a row is decided alone (HF: by sub-batch position); the ratio is on token bytes (HF's), not on decoded text
  (``openai-whisper``'s).

Host syncs.  Token ids, the finished flags and each row's length stay on the device; a step needs no host value.  The host reads
one finished-count every ``SYNC_EVERY`` = 8 steps to end early: a read drains the queue of launches the host has run ahead with
(tens of microseconds, against a step that streams the decoder's weights), so one per step would serialise host and device, while
at 8 an utterance decodes at most 7 steps past its end - a few percent of a sentence's 30 - 100 tokens.

``decode`` is GPT-2 byte-level decoding: the token strings joined, each character mapped back through the 256-entry byte table, the
bytes decoded as UTF-8 with replacement.  Ids >= ``eos_token_id`` are special and are skipped (in the ``.en`` and the multilingual
vocabularies alike the specials start at ``<|endoftext|>``).

WER normalisation is the reference's ``asr.normalize_sentence``, not Whisper's ``EnglishTextNormalizer``: numbers stay as written.

Family built: head_dim 64 (every released size), erf GELU, ``scale_embedding=False``, learned decoder positions,
``num_mel_bins`` <= 128; any other config raises ``NotImplementedError`` naming the field.  At most 32 rows run in one network call
(the step's linears carry the batch in registers); larger batches are run 32 rows at a time.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
import os
import zlib
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._native import device_rows, i32_ptr, on_device, stream
from ._wavnet import SAMPLING_RATE, NetHandle, WaveformNet
from .asr import score_transcripts

N_FFT, HOP = 400, 160
MAX_ROWS = 32                       # DEX_WHISPER_MAX_B
SYNC_EVERY = 8
MAX_LONG_SAMPLES = 28_800_000       # DEX_WHISPER_MAX_LONG_SAMPLES: 30 minutes at 16 kHz
_LONG_SCRATCH = 1 << 30             # bytes of fp64 log-spectrum one front-end call of the long form may hold
MIN_BEAMS, MAX_BEAMS = 2, 8         # DEX_WHISPER_MIN_BEAMS, DEX_WHISPER_MAX_BEAMS
BEAM_KEYS = 13000                   # DEX_WHISPER_BEAM_KEYS
MAX_TEMPERATURES = 8                # the attempts of a DecodingPolicy (the noise counter gives an attempt 4 bits)


@dataclasses.dataclass(frozen=True)
class WhisperConfig:
    """HF ``WhisperConfig`` fields the network reads, with the values of openai/whisper-large-v3."""
    vocab_size: int = 51866
    num_mel_bins: int = 128
    d_model: int = 1280
    encoder_layers: int = 32
    encoder_attention_heads: int = 20
    encoder_ffn_dim: int = 5120
    decoder_layers: int = 32
    decoder_attention_heads: int = 20
    decoder_ffn_dim: int = 5120
    max_source_positions: int = 1500
    max_target_positions: int = 448
    scale_embedding: bool = False
    activation_function: str = "gelu"


class DexWhisperConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab_size", "num_mel_bins", "d_model", "encoder_layers", "encoder_attention_heads", "encoder_ffn_dim",
                                         "decoder_layers", "decoder_attention_heads", "decoder_ffn_dim", "max_source_positions",
                                         "max_target_positions", "scale_embedding", "activation_gelu")]


def _c_config(cfg: WhisperConfig) -> DexWhisperConfig:
    c = DexWhisperConfig()
    for name, _ in DexWhisperConfig._fields_[:-2]:
        setattr(c, name, int(getattr(cfg, name)))
    c.scale_embedding = int(bool(cfg.scale_embedding))
    c.activation_gelu = int(cfg.activation_function == "gelu")
    return c


def mel_filters(n_mels: int) -> np.ndarray:
    """The front end's mel matrix, float64 [201, n_mels] (``transformers.audio_utils.mel_filter_bank(201, n_mels, 0, 8000, 16000,
    'slaney', 'slaney')``), as the library builds it.  Host only."""
    out = np.empty((N_FFT // 2 + 1, int(n_mels)), np.float64)
    if _lib.load().dex_whisper_mel_filters(int(n_mels), out.ctypes.data_as(C.POINTER(C.c_double))) != _lib.DEX_OK:
        raise ValueError(f"mel_filters: n_mels must lie in [1, 128], got {n_mels}")
    return out


@dataclasses.dataclass(frozen=True)
class GenerationSpec:
    """One decode run: the prompt fed before the first new token, the ids never emitted, the ids not emitted first, and eos; for the
    long form also ``<|notimestamps|>`` (the timestamps start behind it) and the cap of a window's first timestamp."""
    prompt_ids: Tuple[int, ...]
    suppress_tokens: Tuple[int, ...] = ()
    begin_suppress_tokens: Tuple[int, ...] = ()
    eos_token_id: int = 50257
    no_timestamps_token_id: Optional[int] = None
    max_initial_timestamp_index: Optional[int] = None

    @property
    def timestamp_begin(self) -> Optional[int]:
        return None if self.no_timestamps_token_id is None else self.no_timestamps_token_id + 1

    @classmethod
    def from_generation_config(cls, config, language: str = "en", task: str = "transcribe", timestamps: bool = False) -> "GenerationSpec":
        """From HF's ``generation_config.json`` (a dict, the file, or the directory that holds it): the prompt
        ``<|startoftranscript|> [<|lang|> <|task|>] <|notimestamps|>`` (the bracket for ``is_multilingual`` models) from the
        file's own ``decoder_start_token_id``, ``lang_to_id``, ``task_to_id`` and ``no_timestamps_token_id``, and its
        ``suppress_tokens``, ``begin_suppress_tokens`` and ``eos_token_id``.  An unknown language or task raises ``ValueError``.
        ``timestamps=True`` (the long form): the prompt ends before ``<|notimestamps|>``, and ``no_timestamps_token_id`` and
        ``max_initial_timestamp_index`` (where the file has one) are carried in the spec."""
        if not isinstance(config, dict):
            path = os.fspath(config)
            if os.path.isdir(path):
                path = os.path.join(path, "generation_config.json")
            with open(path, encoding="utf-8") as f:
                config = json.load(f)
        prompt = [int(config["decoder_start_token_id"])]
        if config.get("is_multilingual", False):
            lang = language if language.startswith("<|") else f"<|{language}|>"
            if lang not in config.get("lang_to_id", {}):
                raise ValueError(f"GenerationSpec: language {language!r} is not in the generation config's lang_to_id")
            if task not in config.get("task_to_id", {}):
                raise ValueError(f"GenerationSpec: task {task!r} is not in the generation config's task_to_id")
            prompt += [int(config["lang_to_id"][lang]), int(config["task_to_id"][task])]
        if not timestamps:
            prompt.append(int(config["no_timestamps_token_id"]))
        eos = config["eos_token_id"]
        eos = int(eos[0] if isinstance(eos, (list, tuple)) else eos)
        spec = cls(tuple(prompt), tuple(int(t) for t in config.get("suppress_tokens") or ()),
                   tuple(int(t) for t in config.get("begin_suppress_tokens") or ()), eos)
        if not timestamps:
            return spec
        if config.get("no_timestamps_token_id") is None:
            raise ValueError("GenerationSpec: timestamps=True needs the generation config's no_timestamps_token_id")
        cap = config.get("max_initial_timestamp_index")
        return dataclasses.replace(spec, no_timestamps_token_id=int(config["no_timestamps_token_id"]),
                                   max_initial_timestamp_index=None if cap is None else int(cap))


@dataclasses.dataclass(frozen=True)
class DecodingPolicy:
    """Fallback decoding (the module docstring's definition): the temperatures of the attempts in order, HF's three thresholds
    (``None`` switches a check off), ``<|nospeech|>`` and the key of the sampling noise."""
    temperatures: Tuple[float, ...] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
    compression_ratio_threshold: Optional[float] = None
    logprob_threshold: Optional[float] = None
    no_speech_threshold: Optional[float] = None
    no_speech_token_id: Optional[int] = None
    seed: int = 0

    def __post_init__(self):
        try:
            t = tuple(float(x) for x in self.temperatures)
        except TypeError:
            raise ValueError(f"DecodingPolicy: temperatures must be a sequence of numbers, got {self.temperatures!r}") from None
        object.__setattr__(self, "temperatures", t)
        if not 1 <= len(t) <= MAX_TEMPERATURES or t[0] != 0.0 or not all(np.isfinite(x) for x in t) or any(b <= a for a, b in zip(t, t[1:])):
            raise ValueError(f"DecodingPolicy: temperatures must start at 0, rise, and number 1 .. {MAX_TEMPERATURES}, got {t!r}")
        for name in ("compression_ratio_threshold", "logprob_threshold", "no_speech_threshold"):
            v = getattr(self, name)
            if v is not None and not np.isfinite(float(v)):
                raise ValueError(f"DecodingPolicy: {name} must be finite or None, got {v!r}")
        if self.no_speech_threshold is not None and self.logprob_threshold is None:
            raise ValueError("DecodingPolicy: no_speech_threshold requires logprob_threshold (a window is skipped only where both say so)")
        if self.no_speech_threshold is not None and self.no_speech_token_id is None:
            raise ValueError("DecodingPolicy: no_speech_threshold requires no_speech_token_id (DecodingPolicy.from_generation_config)")
        if self.no_speech_token_id is not None and int(self.no_speech_token_id) < 0:
            raise ValueError(f"DecodingPolicy: no_speech_token_id must be >= 0, got {self.no_speech_token_id!r}")
        if isinstance(self.seed, bool) or int(self.seed) != self.seed or not 0 <= int(self.seed) < 1 << 64:
            raise ValueError(f"DecodingPolicy: seed must be an integer in [0, 2^64), got {self.seed!r}")

    @classmethod
    def from_generation_config(cls, config, **fields) -> "DecodingPolicy":
        """From HF's ``generation_config.json`` (a dict, the file, or the directory that holds it): ``no_speech_token_id`` is
        ``no_timestamps_token_id - 1``, as in HF; ``fields`` are the other fields."""
        if not isinstance(config, dict):
            path = os.fspath(config)
            if os.path.isdir(path):
                path = os.path.join(path, "generation_config.json")
            with open(path, encoding="utf-8") as f:
                config = json.load(f)
        if config.get("no_timestamps_token_id") is None:
            raise ValueError("DecodingPolicy: the generation config has no no_timestamps_token_id (no_speech_token_id is that id - 1)")
        return cls(no_speech_token_id=int(config["no_timestamps_token_id"]) - 1, **fields)


def compression_ratio(tokens: Sequence[int], vocab_size: int) -> float:
    """HF's ``_retrieve_compression_ratio``: the ids as ``int(log2(V) / 8) + 1`` little-endian bytes each, their length over the
    length of their ``zlib.compress``.  Host only."""
    width = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(int(t).to_bytes(width, "little") for t in tokens)
    return len(raw) / len(zlib.compress(raw))


def fallback_decision(policy: DecodingPolicy, ratio: float, avg_logprob: float, no_speech_prob: float):
    """HF's ``_need_fallback`` for one row -> (needs a retry, is skipped as silence).  Host only."""
    need = skip = False
    if policy.compression_ratio_threshold is not None and ratio > policy.compression_ratio_threshold:
        need = True
    if policy.logprob_threshold is not None and avg_logprob < policy.logprob_threshold:
        need = True
    if policy.no_speech_threshold is not None and avg_logprob < policy.logprob_threshold and no_speech_prob > policy.no_speech_threshold:
        need, skip = False, True
    return need, skip


def check_beam_args(config: WhisperConfig, spec: GenerationSpec, num_beams: int, length_penalty: float = 1.0, timestamps: bool = False,
                    long_form: bool = False, early_stopping=False, num_return_sequences: int = 1, what: str = "Whisper.generate_beam") -> int:
    """The host-side refusals of beam search (the module docstring's limits and out-of-scope list), each a ``ValueError`` naming the
    argument.  Returns K.  Host only."""
    if isinstance(num_beams, bool) or int(num_beams) != num_beams or not MIN_BEAMS <= int(num_beams) <= MAX_BEAMS:
        raise ValueError(f"{what}: num_beams must be an integer in [{MIN_BEAMS}, {MAX_BEAMS}] (1 is greedy decoding, through generate), got {num_beams!r}")
    K = int(num_beams)
    if timestamps:
        raise ValueError(f"{what}: timestamps=True with num_beams > 1 is not built (the timestamp rule's state would have to follow the parents)")
    if long_form:
        raise ValueError(f"{what}: long_form=True with num_beams > 1 is not built (the long form decodes under the timestamp rule)")
    if early_stopping is not False:
        raise ValueError(f"{what}: early_stopping must be False, got {early_stopping!r}")
    if num_return_sequences != 1:
        raise ValueError(f"{what}: num_return_sequences must be 1, got {num_return_sequences!r}")
    lp = float(length_penalty)
    if not np.isfinite(lp):
        raise ValueError(f"{what}: length_penalty must be finite, got {length_penalty!r}")
    if K * config.max_source_positions > BEAM_KEYS:
        raise ValueError(f"{what}: num_beams x max_source_positions = {K * config.max_source_positions} is above {BEAM_KEYS} (the beams' scores of one "
                         "cross-attention launch sit in LDS)")
    masked = {int(t) for t in spec.suppress_tokens} | {int(t) for t in spec.begin_suppress_tokens}
    if config.vocab_size - len(masked) < 2 * K:
        raise ValueError(f"{what}: suppress_tokens and begin_suppress_tokens leave {config.vocab_size - len(masked)} ids, num_beams = {K} needs 2 x {K}")
    return K


def _byte_table():
    """GPT-2's printable stand-ins of the 256 byte values, inverted: character -> byte."""
    bs = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


_BYTE_OF = _byte_table()


def load_vocab(path) -> list:
    """HF's ``vocab.json`` ({token: id}; the file or the directory that holds it) -> the token strings by id (``''`` where an id has
    none).  Host only."""
    path = os.fspath(path)
    if os.path.isdir(path):
        path = os.path.join(path, "vocab.json")
    with open(path, encoding="utf-8") as f:
        table = json.load(f)
    out = [""] * (max(table.values()) + 1)
    for tok, i in table.items():
        out[int(i)] = tok
    return out


def decode(ids: Sequence[int], vocab: Sequence[str], eos_token_id: Optional[int] = None) -> str:
    """GPT-2 byte-level decoding of ``ids``; ids at or above ``eos_token_id`` (default: the id of ``<|endoftext|>`` in ``vocab``,
    else its length) are special and are skipped.  Host only."""
    if eos_token_id is None:
        eos_token_id = list(vocab).index("<|endoftext|>") if "<|endoftext|>" in vocab else len(vocab)
    text = "".join(vocab[int(i)] for i in ids if 0 <= int(i) < eos_token_id and int(i) < len(vocab))
    raw = bytearray()
    for ch in text:
        raw += bytes([_BYTE_OF[ch]]) if ch in _BYTE_OF else ch.encode("utf-8")
    return raw.decode("utf-8", errors="replace")


class _Handle(NetHandle):
    """The workspace of this network is a function of the row count alone."""

    def workspace(self, B: int) -> torch.Tensor:
        need = int(self._fn("workspace_bytes")(self.h, B))
        if need == 0:
            raise ValueError(f"{B} rows: {self.no_workspace}")
        return super(NetHandle, self).workspace(need)

    def beam_workspace(self, U: int, K: int) -> torch.Tensor:
        need = int(self._fn("beam_workspace_bytes")(self.h, U, K))
        if need == 0:
            raise ValueError(f"{U} utterances of {K} beams: {self.no_workspace}")
        return super(NetHandle, self).workspace(need)


class Whisper(WaveformNet):
    """HF's ``WhisperForConditionalGeneration`` in eval mode on one MI355X, fp32 (the module docstring states the definitions)."""
    _prefix, _config_name, _no_workspace = "dex_whisper", "WhisperConfig", f"one network call takes 1 .. {MAX_ROWS} rows"
    _c_config = staticmethod(_c_config)
    _ignored = staticmethod(lambda key: False)
    _handle = _Handle

    def __init__(self, config: Optional[WhisperConfig] = None, device="cuda"):
        super().__init__(config or WhisperConfig(), device)

    @property
    def n_samples(self) -> int:
        """Samples of one chunk: 2 x max_source_positions x 160."""
        return 2 * self.config.max_source_positions * HOP

    def load_state_dict(self, sd, strict: bool = True):
        """HF keys, with or without the ``model.`` prefix.  ``proj_out.weight`` is accepted and must equal
        ``decoder.embed_tokens.weight`` bitwise (``RuntimeError`` otherwise: an untied head is another network)."""
        out, proj = {}, None
        for k, v in sd.items():
            if k == "proj_out.weight":
                proj = v
            else:
                out[k if k.startswith("model.") else "model." + k] = v
        if proj is not None:
            emb = out.get("model.decoder.embed_tokens.weight")
            if emb is None or not torch.equal(torch.as_tensor(proj).cpu(), torch.as_tensor(emb).cpu()):
                raise RuntimeError("proj_out.weight differs from model.decoder.embed_tokens.weight: only the tied head is built")
        return super().load_state_dict(out, strict)

    # ---- front end
    def log_mel(self, wavs, lengths=None, sr: int = SAMPLING_RATE) -> torch.Tensor:
        """``wavs`` [B, n] (or [n]) with ``lengths``, or a list of wavs, at ``sr`` Hz -> features [B, num_mel_bins, 2 x
        max_source_positions] (``WhisperFeatureExtractor``).  What is stored past a row's length is not read.  A row longer than
        ``n_samples`` raises ``ValueError``.  Needs no weights."""
        what = "Whisper.log_mel"
        wavs, lengths = self._at_16k(wavs, lengths, sr, what)
        x, ln, one = device_rows(wavs, lengths, what, refuse=ValueError)
        if int(ln.max()) > self.n_samples:
            raise ValueError(f"{what}: a row of {int(ln.max())} samples is longer than one chunk of {self.n_samples} (long-form audio is not built)")
        x = x[:, : self.n_samples].contiguous().to(self.device)
        B, n = x.shape
        out = torch.empty(B, self.config.num_mel_bins, 2 * self.config.max_source_positions, dtype=torch.float32, device=self.device)
        ctx = self._ctx
        for r in range(0, B, MAX_ROWS):
            xb, ob, lb = x[r:r + MAX_ROWS], out[r:r + MAX_ROWS], np.ascontiguousarray(ln[r:r + MAX_ROWS])
            ws = ctx.workspace(xb.shape[0])
            with torch.cuda.device(self.device):
                rc = ctx.lib.dex_whisper_log_mel(ctx.h, xb.data_ptr(), i32_ptr(lb), xb.shape[0], n, ob.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 stream(self.device))
            ctx.check(rc, "dex_whisper_log_mel")
        return out[0] if one else out

    def _features(self, features, what: str) -> torch.Tensor:
        self._need_weights(what)
        on_device(features, what, ValueError)
        c = self.config
        if features.dim() != 3 or tuple(features.shape[1:]) != (c.num_mel_bins, 2 * c.max_source_positions) or features.shape[0] < 1:
            raise ValueError(f"{what}: expected features [B, {c.num_mel_bins}, {2 * c.max_source_positions}], got {tuple(features.shape)}")
        return features.to(device=self.device, dtype=torch.float32).contiguous()

    def _encode(self, f: torch.Tensor, out, ms=None) -> torch.Tensor:
        """The encoder of at most ``MAX_ROWS`` rows; its output and the cross-attention K / V stay in the workspace.  ``ms``: a
        ``c_float * 2`` that receives the milliseconds of the encoder and of the cross K / V (the call then waits)."""
        ctx = self._ctx
        ws = ctx.workspace(f.shape[0])
        with torch.cuda.device(self.device):
            rc = ctx.lib.dex_whisper_encode(ctx.h, f.data_ptr(), f.shape[0], out.data_ptr() if out is not None else None, ms, ws.data_ptr(),
                                            ws.numel(), stream(self.device))
        ctx.check(rc, "dex_whisper_encode")
        self.encoder_calls = getattr(self, "encoder_calls", 0) + 1          # what ``_trace`` reports under a policy
        return ws

    def encode(self, features: torch.Tensor) -> torch.Tensor:
        """features [B, num_mel_bins, 2 x max_source_positions] -> the encoder's last hidden state [B, max_source_positions, d_model]."""
        f = self._features(features, "Whisper.encode")
        out = torch.empty(f.shape[0], self.config.max_source_positions, self.config.d_model, dtype=torch.float32, device=self.device)
        for r in range(0, f.shape[0], MAX_ROWS):
            self._encode(f[r:r + MAX_ROWS], out[r:r + MAX_ROWS])
        return out

    def forward(self, features: torch.Tensor, decoder_input_ids: torch.Tensor) -> torch.Tensor:
        """features as for ``encode``, decoder_input_ids [B, L] (L <= max_target_positions) -> logits [B, L, vocab_size], through
        the cached step one position at a time."""
        what = "Whisper.forward"
        f = self._features(features, what)
        on_device(decoder_input_ids, what, ValueError)
        c = self.config
        if decoder_input_ids.dim() != 2 or decoder_input_ids.shape[0] != f.shape[0] or decoder_input_ids.shape[1] < 1:
            raise ValueError(f"{what}: expected decoder_input_ids [{f.shape[0]}, L], got {tuple(decoder_input_ids.shape)}")
        ids = decoder_input_ids.to(device=self.device, dtype=torch.int32).contiguous()
        B, L = ids.shape
        if L > c.max_target_positions:
            raise ValueError(f"{what}: {L} decoder positions, max_target_positions is {c.max_target_positions}")
        if int(ids.min()) < 0 or int(ids.max()) >= c.vocab_size:
            raise ValueError(f"{what}: decoder_input_ids must lie in [0, vocab_size = {c.vocab_size})")
        out = torch.empty(B, L, c.vocab_size, dtype=torch.float32, device=self.device)
        ctx = self._ctx
        for r in range(0, B, MAX_ROWS):
            fb, ib, ob = f[r:r + MAX_ROWS], ids[r:r + MAX_ROWS], out[r:r + MAX_ROWS]
            ws = self._encode(fb, None)
            with torch.cuda.device(self.device):
                rc = ctx.lib.dex_whisper_forward(ctx.h, ib.data_ptr(), fb.shape[0], L, ob.data_ptr(), ws.data_ptr(), ws.numel(), stream(self.device))
            ctx.check(rc, "dex_whisper_forward")
        return out

    __call__ = forward

    def _masks(self, spec: GenerationSpec):
        V = self.config.vocab_size
        for name in ("prompt_ids", "suppress_tokens", "begin_suppress_tokens"):
            bad = [t for t in getattr(spec, name) if not 0 <= int(t) < V]
            if bad:
                raise ValueError(f"Whisper.generate: {name} holds {bad[0]}, outside the vocabulary of {V}")
        sup = np.zeros(V, np.uint8)
        sup[list(spec.suppress_tokens)] = 1
        beg = sup.copy()
        beg[list(spec.begin_suppress_tokens)] = 1
        return torch.from_numpy(sup).to(self.device), torch.from_numpy(beg).to(self.device)

    def _decode_setup(self, spec: GenerationSpec, max_new_tokens: Optional[int], clamp: bool, refusal):
        """-> (max_new, the suppress and begin masks, the prompt as a host array).  ``max_new`` defaults to the room the prompt leaves
        in the cache; ``clamp`` cuts it to that room here (otherwise the library does).  ``refusal(max_new)``: the caller's message
        where no step could be taken."""
        room = self.config.max_target_positions - len(spec.prompt_ids)
        max_new = room if max_new_tokens is None else int(max_new_tokens)
        max_new = min(max_new, room) if clamp else max_new
        if not spec.prompt_ids or max_new < 1:
            raise ValueError(refusal(max_new))
        return (max_new, *self._masks(spec), np.ascontiguousarray(np.asarray(spec.prompt_ids, np.int32)))

    def _decode_inputs(self, what: str, features_or_wavs, spec: GenerationSpec, max_new_tokens, lengths, sr, clamp: bool):
        """What every decoder starts from -> (f, max_new, sup, beg, prompt): the features (given, or ``log_mel`` of the wavs) and
        ``_decode_setup``'s results."""
        c = self.config
        if not spec.prompt_ids or len(spec.prompt_ids) > c.max_target_positions:
            raise ValueError(f"{what}: a prompt of {len(spec.prompt_ids)} ids, max_target_positions is {c.max_target_positions}")
        if torch.is_tensor(features_or_wavs) and features_or_wavs.dim() == 3:
            f = self._features(features_or_wavs, what)
        else:
            f = self.log_mel(features_or_wavs, lengths, sr)
            f = f[None] if f.dim() == 2 else f
        return (f, *self._decode_setup(spec, max_new_tokens, clamp,
                                       lambda n: f"{what}: max_new_tokens must be >= 1 (and the prompt leave room in the cache), got {n}"))

    @staticmethod
    def _keys_and_seeks(what: str, B: int, row_keys, seeks, rule: str):
        """The words of the noise counter, one per row -> (keys, default the row's index; seeks, default 0); ``rule`` words the refusal."""
        keys = list(range(B)) if row_keys is None else [int(k) for k in row_keys]
        seeks = [0] * B if seeks is None else [int(s) for s in seeks]
        if len(keys) != B or len(seeks) != B or any(not 0 <= k < 1 << 32 for k in keys) or any(not 0 <= s < 1 << 27 for s in seeks):
            raise ValueError(f"{what}: {rule}")
        return keys, seeks

    def generate(self, features_or_wavs, spec: GenerationSpec, max_new_tokens: Optional[int] = None, lengths=None, sr: int = SAMPLING_RATE,
                 timestamps: bool = False, num_beams: int = 1, length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1,
                 policy: Optional[DecodingPolicy] = None, row_keys=None, seeks=None):
        """Greedy decoding (the module docstring's definition) of features [B, num_mel_bins, frames], or of wavs as ``log_mel`` takes
        them -> (ids [B, n] int32, a row padded with eos after its end; lengths [B] int32, the tokens before a row's eos), both on the
        device.  n is the number of steps decoded: at most ``max_new_tokens`` and ``max_target_positions - len(prompt)``.
        ``timestamps=True`` decodes one window under the long form's step rule (``spec`` with the timestamp fields).
        ``num_beams`` > 1: beam search, the first two results of ``generate_beam``.
        ``policy``: fallback decoding; a third result is a dict of per-row float64 / bool arrays on the host: ``temperature`` (of the
        attempt that stands), ``avg_logprob``, ``compression_ratio``, ``no_speech_prob`` (NaN without ``no_speech_token_id``),
        ``skipped`` (the row is silence: length 0) and ``attempts``.  ``row_keys`` [B] (default: the row's index) and ``seeks`` [B]
        (default 0) are the words of the noise counter."""
        what = "Whisper.generate"
        if policy is not None:
            if not isinstance(policy, DecodingPolicy):
                raise ValueError(f"{what}: policy must be a DecodingPolicy, got {type(policy).__name__}")
            if num_beams != 1:
                raise ValueError(f"{what}: num_beams > 1 with a policy is not built (sampling turns beams off; the greedy attempt has none either)")
        elif row_keys is not None or seeks is not None:
            raise ValueError(f"{what}: row_keys and seeks belong to a policy")
        if num_beams != 1:
            check_beam_args(self.config, spec, num_beams, length_penalty, timestamps, False, early_stopping, num_return_sequences, what)
            return self.generate_beam(features_or_wavs, spec, num_beams, length_penalty, max_new_tokens, lengths, sr)[:2]
        if early_stopping is not False or num_return_sequences != 1:
            raise ValueError(f"{what}: early_stopping and num_return_sequences belong to beam search (num_beams > 1)")
        self._need_weights(what)
        if timestamps:
            self._timestamp_spec(spec, what)
        f, max_new, sup, beg, prompt = self._decode_inputs(what, features_or_wavs, spec, max_new_tokens, lengths, sr, clamp=False)
        B = f.shape[0]
        if policy is not None:
            return self._generate_policy(f, spec, policy, max_new, timestamps, sup, beg, prompt, row_keys, seeks, what)
        ids = torch.empty(B, max_new, dtype=torch.int32, device=self.device)
        lens = torch.empty(B, dtype=torch.int32, device=self.device)
        ctx, steps, n = self._ctx, C.c_int(0), 0
        for r in range(0, B, MAX_ROWS):
            fb, ib, lb = f[r:r + MAX_ROWS], ids[r:r + MAX_ROWS], lens[r:r + MAX_ROWS]
            ws = self._encode(fb, None)
            tail = (fb.shape[0], max_new, SYNC_EVERY, ib.data_ptr(), lb.data_ptr(), C.byref(steps), ws.data_ptr(), ws.numel(), stream(self.device))
            with torch.cuda.device(self.device):
                if timestamps:
                    cap = -1 if spec.max_initial_timestamp_index is None else int(spec.max_initial_timestamp_index)
                    rc = ctx.lib.dex_whisper_generate_ts(ctx.h, i32_ptr(prompt), len(prompt), sup.data_ptr(), beg.data_ptr(), int(spec.eos_token_id),
                                                         int(spec.no_timestamps_token_id), cap, *tail)
                else:
                    rc = ctx.lib.dex_whisper_generate(ctx.h, i32_ptr(prompt), len(prompt), sup.data_ptr(), beg.data_ptr(), int(spec.eos_token_id), *tail)
            ctx.check(rc, "dex_whisper_generate_ts" if timestamps else "dex_whisper_generate")
            n = max(n, steps.value)
        return ids[:, :n], lens

    def _decode_policy(self, f: torch.Tensor, spec: GenerationSpec, policy: DecodingPolicy, max_new: int, timestamps: bool, sup, beg, prompt,
                       keys, seeks, attempts_out: Optional[list] = None) -> list:
        """Fallback decoding of at most ``MAX_ROWS`` rows of features: the encoder once, then per attempt one decode of the rows that
        still need one, from the cross K / V where the encoder left it -> per row a dict ``tokens`` (host ints, no eos), ``temperature``,
        ``avg_logprob``, ``compression_ratio``, ``no_speech_prob``, ``skipped``, ``attempts``.  ``attempts_out`` receives per attempt
        the list of its (row, temperature, tokens)."""
        ctx, dev, B, V = self._ctx, self.device, f.shape[0], self.config.vocab_size
        ws = self._encode(f, None)
        probe = policy.no_speech_token_id is not None
        if probe and not 0 <= int(policy.no_speech_token_id) < V:
            raise ValueError(f"DecodingPolicy: no_speech_token_id {policy.no_speech_token_id} is outside the vocabulary of {V}")
        cap = -1 if spec.max_initial_timestamp_index is None else int(spec.max_initial_timestamp_index)
        nots = int(spec.no_timestamps_token_id) if timestamps else -1
        u32, out, pending, steps = C.POINTER(C.c_uint32), [None] * B, list(range(B)), C.c_int(0)
        no_speech = np.full(B, np.nan)
        for attempt, T in enumerate(policy.temperatures):
            R = len(pending)
            rows = np.ascontiguousarray(np.asarray(pending, np.int32))
            kk = np.ascontiguousarray(np.asarray([keys[r] for r in pending], np.uint32))
            sk = np.ascontiguousarray(np.asarray([seeks[r] for r in pending], np.int32))
            ids = torch.empty(R, max_new, dtype=torch.int32, device=dev)
            lens = torch.empty(R, dtype=torch.int32, device=dev)
            slp, nsp = torch.zeros(R, dtype=torch.float64, device=dev), torch.zeros(R, dtype=torch.float64, device=dev)
            scored = torch.empty(R, dtype=torch.int32, device=dev)
            first = attempt == 0 and probe
            with torch.cuda.device(dev):
                rc = ctx.lib.dex_whisper_generate_policy(
                    ctx.h, i32_ptr(prompt), len(prompt), sup.data_ptr(), beg.data_ptr(), int(spec.eos_token_id), int(timestamps), nots, cap, float(T),
                    int(policy.seed), attempt, kk.ctypes.data_as(u32), i32_ptr(sk), B, i32_ptr(rows), R, max_new, SYNC_EVERY, ids.data_ptr(), lens.data_ptr(),
                    slp.data_ptr(), scored.data_ptr(), int(policy.no_speech_token_id) if probe else 0, nsp.data_ptr() if first else None, C.byref(steps),
                    ws.data_ptr(), ws.numel(), stream(dev))
            ctx.check(rc, "dex_whisper_generate_policy")
            n = steps.value
            # the attempt's one device-to-host copy: ids, lengths and the statistics, as float64 (every int32 is exact in it)
            host = torch.cat([ids[:, :n].double(), lens[:, None].double(), scored[:, None].double(), slp[:, None], nsp[:, None]], dim=1).cpu().numpy()
            retry, seen = [], []
            for a, r in enumerate(pending):
                length, n_scored, sum_lp = int(host[a, n]), int(host[a, n + 1]), float(host[a, n + 2])
                if first:
                    no_speech[r] = float(host[a, n + 3])
                tokens = host[a, :length].astype(np.int64).tolist()
                scored_tokens = tokens + [int(spec.eos_token_id)] * (n_scored - length)       # HF scores the emitted eos with the row
                avg, ratio = sum_lp / n_scored, compression_ratio(scored_tokens, V)
                need, skip = fallback_decision(policy, ratio, avg, no_speech[r])
                out[r] = dict(tokens=[] if skip else tokens, temperature=float(T), avg_logprob=avg, compression_ratio=ratio,
                              no_speech_prob=float(no_speech[r]), skipped=skip, attempts=attempt + 1)
                seen.append((r, float(T), tokens))
                if need:
                    retry.append(r)
            if attempts_out is not None:
                attempts_out.append(seen)
            pending = retry
            if not pending:
                break
        return out

    def _generate_policy(self, f, spec, policy, max_new, timestamps, sup, beg, prompt, row_keys, seeks, what):
        B = f.shape[0]
        keys, seeks = self._keys_and_seeks(what, B, row_keys, seeks, "row_keys and seeks must hold one value per row, keys in [0, 2^32), seeks in [0, 2^27)")
        rows = []
        for r in range(0, B, MAX_ROWS):
            rows += self._decode_policy(f[r:r + MAX_ROWS], spec, policy, max_new, timestamps, sup, beg, prompt, keys[r:r + MAX_ROWS], seeks[r:r + MAX_ROWS])
        n = max(1, max(len(x["tokens"]) + 1 for x in rows))
        n = min(n, max_new)
        ids = np.full((B, n), int(spec.eos_token_id), np.int32)
        for b, x in enumerate(rows):
            ids[b, : len(x["tokens"])] = x["tokens"]
        info = {k: np.asarray([x[k] for x in rows]) for k in ("temperature", "avg_logprob", "compression_ratio", "no_speech_prob", "skipped", "attempts")}
        return torch.from_numpy(ids).to(self.device), torch.tensor([len(x["tokens"]) for x in rows], dtype=torch.int32, device=self.device), info

    def generate_beam(self, features_or_wavs, spec: GenerationSpec, num_beams: int, length_penalty: float = 1.0, max_new_tokens: Optional[int] = None,
                      lengths=None, sr: int = SAMPLING_RATE, trace: bool = False):
        """Beam search (the module docstring's definition) of features or wavs as ``generate`` takes them -> (ids [U, n] int32, the
        best hypothesis padded with eos; lengths [U] int32; scores [U] float64, its pool score), on the device.  ``trace=True`` adds a
        dict: ``logits`` [n, U, K, V] fp32, ``tokens``, ``parents`` [n, U, K] int32 (-1 on an utterance's last step and once it is
        done), ``scores`` [n, U, K] float64 (the running scores after the step), and the pool at the end, best first: ``pool_ids``
        [U, K, n], ``pool_lengths``, ``pool_scores`` [U, K], ``pool_n`` [U]."""
        what = "Whisper.generate_beam"
        K = check_beam_args(self.config, spec, num_beams, length_penalty, what=what)
        self._need_weights(what)
        f, max_new, sup, beg, prompt = self._decode_inputs(what, features_or_wavs, spec, max_new_tokens, lengths, sr, clamp=True)
        U, V, dev = f.shape[0], self.config.vocab_size, self.device
        ids = torch.empty(U, max_new, dtype=torch.int32, device=dev)
        lens = torch.empty(U, dtype=torch.int32, device=dev)
        scores = torch.empty(U, dtype=torch.float64, device=dev)
        tr = None
        if trace:
            tr = dict(logits=torch.empty(max_new, U, K, V, dtype=torch.float32, device=dev), tokens=torch.empty(max_new, U, K, dtype=torch.int32, device=dev),
                      parents=torch.empty(max_new, U, K, dtype=torch.int32, device=dev), scores=torch.empty(max_new, U, K, dtype=torch.float64, device=dev),
                      pool_ids=torch.empty(U, K, max_new, dtype=torch.int32, device=dev), pool_lengths=torch.empty(U, K, dtype=torch.int32, device=dev),
                      pool_scores=torch.empty(U, K, dtype=torch.float64, device=dev), pool_n=torch.empty(U, dtype=torch.int32, device=dev))
        ctx, steps, n, group = self._ctx, C.c_int(0), 0, MAX_ROWS // K
        for r in range(0, U, group):
            fb = f[r:r + group]
            u = fb.shape[0]
            ws = ctx.beam_workspace(u, K)
            with torch.cuda.device(dev):
                ctx.check(ctx.lib.dex_whisper_encode(ctx.h, fb.data_ptr(), u, None, None, ws.data_ptr(), ws.numel(), stream(dev)), "dex_whisper_encode")
                t = [None] * 8
                if trace:                                       # per group: the group's utterances are contiguous only along dim 1
                    g = {k: (v[:, r:r + u].contiguous() if k in ("logits", "tokens", "parents", "scores") else v[r:r + u]) for k, v in tr.items()}
                    t = [g[k].data_ptr() for k in ("logits", "tokens", "parents", "scores", "pool_ids", "pool_lengths", "pool_scores", "pool_n")]
                rc = ctx.lib.dex_whisper_generate_beam(ctx.h, i32_ptr(prompt), len(prompt), sup.data_ptr(), beg.data_ptr(), int(spec.eos_token_id), u, K,
                                                       float(length_penalty), max_new, SYNC_EVERY, ids[r:r + u].data_ptr(), lens[r:r + u].data_ptr(),
                                                       scores[r:r + u].data_ptr(), C.byref(steps), *t, ws.data_ptr(), ws.numel(), stream(dev))
            ctx.check(rc, "dex_whisper_generate_beam")
            if trace:
                for k in ("logits", "tokens", "parents", "scores"):
                    tr[k][:, r:r + u] = g[k]
            n = max(n, steps.value)
        if trace:
            for k in ("logits", "tokens", "parents", "scores"):
                tr[k] = tr[k][:n]
            tr["pool_ids"] = tr["pool_ids"][:, :, :n]
            return ids[:, :n], lens, scores, tr
        return ids[:, :n], lens, scores

    def transcribe(self, wavs, spec: GenerationSpec, vocab: Sequence[str], lengths=None, sr: int = SAMPLING_RATE,
                   max_new_tokens: Optional[int] = None, num_beams: int = 1, length_penalty: float = 1.0, policy: Optional[DecodingPolicy] = None):
        """``wavs`` as ``log_mel`` takes them -> a list of transcripts (``decode`` of each row's tokens; one device-to-host copy).
        ``num_beams`` > 1 decodes by beam search; ``policy``: fallback decoding (a row skipped as silence is ``''``)."""
        ids, lens = self.generate(wavs, spec, max_new_tokens, lengths, sr, num_beams=num_beams, length_penalty=length_penalty, policy=policy)[:2]
        ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
        return [decode(ids[b, : int(lens[b])], vocab, spec.eos_token_id) for b in range(ids.shape[0])]


    # ---- long form (the module docstring's definition)
    def _timestamp_spec(self, spec: GenerationSpec, what: str):
        c = self.config
        if spec.no_timestamps_token_id is None:
            raise ValueError(f"{what}: the spec has no no_timestamps_token_id (GenerationSpec.from_generation_config(..., timestamps=True))")
        nots = int(spec.no_timestamps_token_id)
        if not 0 <= int(spec.eos_token_id) <= nots < c.vocab_size - 1:
            raise ValueError(f"{what}: no_timestamps_token_id {nots} must lie at or above eos_token_id {spec.eos_token_id} and inside the vocabulary of {c.vocab_size}")
        if c.vocab_size - (nots + 1) < c.max_source_positions + 1:
            raise ValueError(f"{what}: {c.vocab_size - (nots + 1)} timestamp ids behind no_timestamps_token_id, a window needs "
                             f"max_source_positions + 1 = {c.max_source_positions + 1}")
        if spec.max_initial_timestamp_index is not None and int(spec.max_initial_timestamp_index) < 0:
            raise ValueError(f"{what}: max_initial_timestamp_index must be >= 0, got {spec.max_initial_timestamp_index}")

    def log_mel_long(self, wavs, lengths=None, sr: int = SAMPLING_RATE):
        """``wavs`` as ``log_mel`` takes them, rows of any length up to ``MAX_LONG_SAMPLES`` -> (features [B, num_mel_bins, F_max],
        0.0 behind a row's frames; the rows' frame counts F, host int32 [B]).  A row of at most ``n_samples`` has ``log_mel``'s
        features, a longer one those of ``WhisperFeatureExtractor(truncation=False)`` on the row alone.  Needs no weights."""
        what = "Whisper.log_mel_long"
        wavs, lengths = self._at_16k(wavs, lengths, sr, what)
        x, ln, _ = device_rows(wavs, lengths, what, refuse=ValueError)
        if int(ln.max()) > MAX_LONG_SAMPLES:
            raise ValueError(f"{what}: a row of {int(ln.max())} samples is above the cap of {MAX_LONG_SAMPLES} (30 minutes)")
        x = x[:, : int(ln.max())].contiguous().to(self.device)
        B, n = x.shape
        M, chunk_frames = self.config.num_mel_bins, 2 * self.config.max_source_positions
        frames = np.where(ln <= self.n_samples, chunk_frames, ln // HOP).astype(np.int32)
        F = int(frames.max())
        out = torch.empty(B, M, F, dtype=torch.float32, device=self.device)
        group = max(1, min(MAX_ROWS, _LONG_SCRATCH // (F * M * 8)))
        scratch = torch.empty(min(group, B) * F * M, dtype=torch.float64, device=self.device)
        ctx = self._ctx
        for r in range(0, B, group):
            xb, ob, lb = x[r:r + group], out[r:r + group], np.ascontiguousarray(ln[r:r + group])
            fb = np.zeros(len(lb), np.int32)
            with torch.cuda.device(self.device):
                rc = ctx.lib.dex_whisper_log_mel_long(ctx.h, xb.data_ptr(), i32_ptr(lb), xb.shape[0], n, ob.data_ptr(), F, i32_ptr(fb),
                                                      scratch.data_ptr(), scratch.numel() * 8, stream(self.device))
            ctx.check(rc, "dex_whisper_log_mel_long")
            assert np.array_equal(fb, frames[r:r + group])
        return out, frames

    def _gather(self, feats: torch.Tensor, rows, seeks, ns) -> torch.Tensor:
        """The windows [seek, seek + n) of ``rows`` of ``feats`` [B, num_mel_bins, F_max] -> [len(rows), num_mel_bins, 2 x
        max_source_positions], 0.0 behind n (at most ``MAX_ROWS`` windows)."""
        ctx = self._ctx
        out = torch.empty(len(rows), self.config.num_mel_bins, 2 * self.config.max_source_positions, dtype=torch.float32, device=self.device)
        r, s, n = (np.ascontiguousarray(np.asarray(a, np.int32)) for a in (rows, seeks, ns))
        with torch.cuda.device(self.device):
            rc = ctx.lib.dex_whisper_gather_windows(ctx.h, feats.data_ptr(), feats.shape[0], feats.shape[2], i32_ptr(r), i32_ptr(s), i32_ptr(n), len(r),
                                                    out.data_ptr(), stream(self.device))
        ctx.check(rc, "dex_whisper_gather_windows")
        return out

    def generate_segments(self, wavs, spec: GenerationSpec, lengths=None, sr: int = SAMPLING_RATE, max_new_tokens: Optional[int] = None,
                          _trace: Optional[list] = None, policy: Optional[DecodingPolicy] = None, row_keys=None):
        """Long-form decoding (the module docstring's window loop) of ``wavs`` as ``log_mel_long`` takes them -> per row a list of
        segments ``{"start", "end", "tokens"}``: seconds in float64 and the segment's ids (its timestamps included) as host ints.
        ``_trace`` (a list, for tests and measurement) receives per network call the list of its (row, seek, n, new ids).
        ``policy``: fallback decoding of every window; a segment also carries its window's ``temperature``, ``avg_logprob``,
        ``compression_ratio`` and ``no_speech_prob``, a window skipped as silence emits none, and ``_trace`` receives per window group a
        dict: ``encoder_calls`` (1), ``windows`` [(row, seek, n)], ``attempts`` (per attempt its (row, temperature, ids)) and ``skipped``
        [(row, seek, n)].  ``row_keys`` [B] (default: the row's index): the rows' word of the noise counter."""
        what = "Whisper.generate_segments"
        self._need_weights(what)
        self._timestamp_spec(spec, what)
        if policy is not None and not isinstance(policy, DecodingPolicy):
            raise ValueError(f"{what}: policy must be a DecodingPolicy, got {type(policy).__name__}")
        if policy is None and row_keys is not None:
            raise ValueError(f"{what}: row_keys belong to a policy")
        feats, frames = self.log_mel_long(wavs, lengths, sr)
        B, W, tb = feats.shape[0], 2 * self.config.max_source_positions, int(spec.no_timestamps_token_id) + 1
        seek, out, keys, setup = [0] * B, [[] for _ in range(B)], None, None
        if policy is not None:
            keys, _ = self._keys_and_seeks(what, B, row_keys, None, "row_keys must hold one value in [0, 2^32) per row")
            setup = self._decode_setup(spec, max_new_tokens, False,
                                       lambda n: f"{what}: max_new_tokens must be >= 1 and the prompt of {len(spec.prompt_ids)} ids leave room in the cache")
        while True:
            active = [b for b in range(B) if seek[b] < int(frames[b])]
            if not active:
                return out
            for r in range(0, len(active), MAX_ROWS):
                rows = active[r:r + MAX_ROWS]
                ns = [min(int(frames[b]) - seek[b], W) for b in rows]
                res, entry = self._decode_window(feats, rows, [seek[b] for b in rows], ns, spec, max_new_tokens, policy, setup, keys)
                if _trace is not None:
                    _trace.append(entry)
                for (tokens, extra, skipped), b, n in zip(res, rows, ns):
                    if skipped:
                        seek[b] += n
                        continue
                    segments, advance = retrieve_segments(tokens, tb, seek[b], n)
                    out[b] += segments if extra is None else [dict(s, **extra) for s in segments]
                    seek[b] += advance

    def _decode_window(self, feats, rows, seeks, ns, spec, max_new_tokens, policy, setup, keys):
        """One network call of the window loop: the windows [seek, seek + n) of ``rows`` of ``feats``, decoded under the timestamp rule,
        plainly or (``setup`` from ``_decode_setup``, ``keys`` by row of ``feats``) under ``policy`` -> (per window its (new ids, the
        statistics a policy attaches to its segments or None, skipped as silence), the call's ``_trace`` entry)."""
        f, where = self._gather(feats, rows, seeks, ns), list(zip(rows, seeks, ns))
        if policy is None:
            ids, lens = self.generate(f, spec, max_new_tokens, timestamps=True)
            host = torch.cat([ids, lens[:, None]], dim=1).cpu().numpy()                     # the window's one device-to-host copy
            res = [(row[: int(row[-1])].tolist(), None, False) for row in host]
            return res, [(*w, x[0]) for w, x in zip(where, res)]                            # one entry per network call: (row, seek, n, ids)
        calls, attempts = getattr(self, "encoder_calls", 0), []
        got = self._decode_policy(f, spec, policy, setup[0], True, *setup[1:], [keys[b] for b in rows], seeks, attempts)
        res = [(x["tokens"], {k: x[k] for k in ("temperature", "avg_logprob", "compression_ratio", "no_speech_prob")}, x["skipped"]) for x in got]
        return res, dict(encoder_calls=self.encoder_calls - calls, windows=where, attempts=[[(rows[a], T, t) for a, T, t in att] for att in attempts],
                         skipped=[w for w, x in zip(where, got) if x["skipped"]])

    def transcribe_long(self, wavs, spec: GenerationSpec, vocab: Sequence[str], lengths=None, sr: int = SAMPLING_RATE,
                        max_new_tokens: Optional[int] = None, policy: Optional[DecodingPolicy] = None):
        """``wavs`` of any length -> a list of transcripts: ``decode`` of each row's segments' ids joined.  ``policy``: fallback
        decoding of every window."""
        rows = self.generate_segments(wavs, spec, lengths, sr, max_new_tokens, policy=policy)
        return [decode([t for seg in segments for t in seg["tokens"]], vocab, spec.eos_token_id) for segments in rows]


def retrieve_segments(tokens: Sequence[int], timestamp_begin: int, seek: int, n: int):
    """One window's new ids (the trailing eos stripped), decoded at frame ``seek`` over ``n`` frames -> (segments, the frames to
    advance ``seek`` by), as HF's ``_retrieve_segment`` cuts them.  Host only."""
    ts = [t >= timestamp_begin for t in tokens]
    single_ending = ts[-2:] == [False, True]
    cuts = [i + 1 for i in range(len(tokens) - 1) if ts[i] and ts[i + 1]]
    t0 = seek * 0.01
    if not cuts:
        stamps = [t for t in tokens if t >= timestamp_begin]
        # HF takes the window's end from a float32 tensor: int(n x 0.01 / 0.02) in that precision
        last = float(stamps[-1] - timestamp_begin) if stamps and stamps[-1] != timestamp_begin else int(np.float32(n) * np.float32(0.01) / np.float32(0.02))
        return [{"start": t0, "end": t0 + last * 0.02, "tokens": list(tokens)}], n
    if single_ending:
        cuts.append(len(tokens))
    else:
        cuts[-1] += 1                                 # the last pair's second timestamp stays with its segment's successor, as in HF
    segments, prev = [], 0
    for i, cut in enumerate(cuts):
        piece = list(tokens[prev:cut])
        end = piece[-1] if i < len(cuts) - 1 or single_ending else piece[-2]
        segments.append({"start": t0 + float(piece[0] - timestamp_begin) * 0.02, "end": t0 + float(end - timestamp_begin) * 0.02, "tokens": piece})
        prev = cut
    return segments, n if single_ending else (tokens[prev - 2] - timestamp_begin) * 2


def whisper_score(wavs, texts: Sequence[str], model: Optional[Whisper] = None, spec: Optional[GenerationSpec] = None,
                  vocab: Optional[Sequence[str]] = None, sr: int = SAMPLING_RATE, lengths=None, long_form: bool = False, num_beams: int = 1,
                  length_penalty: float = 1.0, policy: Optional[DecodingPolicy] = None):
    """Every wav transcribed by ``model``; CER and WER of ``asr.normalize_sentence(transcript)`` against
    ``asr.normalize_sentence(text)`` (the reference's normaliser, not Whisper's: numbers stay as written) ->
    (transcripts, cer_mean, cer_stderr, wer_mean, wer_stderr), the errors ``np.std / sqrt(n)``.  ``long_form=True``: rows of any
    length, through ``transcribe_long`` (``spec`` with the timestamp fields).  ``num_beams`` > 1: beam search (not with the long form).
    ``policy``: fallback decoding, short or long form (not with beams)."""
    if not isinstance(model, Whisper) or spec is None or vocab is None:
        raise ValueError("whisper_score: pass model=Whisper(...) with the checkpoint's weights loaded, spec= and vocab= (the library ships none)")
    if policy is not None:
        if num_beams != 1:
            raise ValueError("whisper_score: num_beams > 1 with a policy is not built")
        preds = (model.transcribe_long if long_form else model.transcribe)(wavs, spec, vocab, lengths, sr, policy=policy)
    elif num_beams != 1:
        check_beam_args(model.config, spec, num_beams, length_penalty, long_form=long_form, what="whisper_score")
        preds = model.transcribe(wavs, spec, vocab, lengths, sr, num_beams=num_beams, length_penalty=length_penalty)
    else:
        preds = (model.transcribe_long if long_form else model.transcribe)(wavs, spec, vocab, lengths, sr)
    if len(preds) != len(texts) or not preds:
        raise ValueError(f"whisper_score: {len(texts)} texts against {len(preds)} wavs")
    return (preds, *score_transcripts(texts, preds))
