"""Host-side mirror of the reference's HiFi-GAN ``Generator`` (GeDEX-TTS/hifigan/models.py:112-173, built by
``get_vocoder`` src/utils.py:251-281 from hifigan/config.json): same constructor (``Generator(h)`` with the config
attributes), same state-dict keys — with or without weight norm (``*.weight_g`` / ``*.weight_v`` pairs of a training
checkpoint, or plain ``*.weight`` after ``remove_weight_norm()``) — same ``forward(mel [B,80,T]) -> wav [B,1,T*256]``.
The arithmetic runs in libdexamd.so (``dex_vocode``: implicit-GEMM convolutions on the exact-fp32 MFMA path); PyTorch owns
tensors and the stream.  No CPU path."""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, Optional

import torch

from . import _lib
from ._native import NativeModule, stream

HIFIGAN_V1 = dict(num_mels=80, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
                  resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]])


# BigVGAN-base, 22 kHz / 80 bands: the configuration src/utils.py:267 reads from bigvgan/bigvgan_base_22khz_80band/config.json (not in
# the reference tree; these are the published values of that file).
BIGVGAN_BASE = dict(num_mels=80, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
                    resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
                    activation="snakebeta", snake_logscale=True)
# BigVGAN, 22 kHz / 80 bands (112 M parameters): the reference's ``vocoder: 'bigvgan'`` choice, bigvgan/bigvgan_22khz_80band/config.json
# (published values; not in the reference tree either).  Six up-sampling stages 768/384/192/96/48/24 wide: the first four run on the
# implicit GEMM, the 48- and 24-channel stages on the narrow kernels (vocoder_narrow.hip).
BIGVGAN_22KHZ = dict(num_mels=80, upsample_rates=[4, 4, 2, 2, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4, 4, 4], upsample_initial_channel=1536,
                     resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
                     activation="snakebeta", snake_logscale=True)
ACTIVATION = {None: 0, "snake": 1, "snakebeta": 2}


class AttrDict(dict):
    """hifigan/__init__.py's AttrDict: config.json keys as attributes."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.__dict__ = self


def _get(h, name, default=None):
    if isinstance(h, dict):
        return h.get(name, default)
    return getattr(h, name, default)


def param_shapes(h) -> Dict[str, tuple]:
    """Generator.state_dict() after remove_weight_norm(): key -> shape (hifigan/models.py:116-148; with ``activation`` =
    'snake' / 'snakebeta' in the config: BigVGAN, bigvgan/models.py:141-184 — nested ``ups.<i>.0``, an Activation1d per ResBlock conv
    with its alpha [, beta] and the two resampling-filter buffers, ``activation_post``)."""
    c0 = int(_get(h, "upsample_initial_channel"))
    rates, ksz = list(_get(h, "upsample_rates")), list(_get(h, "upsample_kernel_sizes"))
    rk = list(_get(h, "resblock_kernel_sizes"))
    act = _get(h, "activation")
    if act not in ACTIVATION:
        raise ValueError(f"activation {act!r}: expected 'snake' or 'snakebeta' (BigVGAN) or none (HiFi-GAN)")
    ups = ".0" if act else ""
    out = {"conv_pre.weight": (c0, int(_get(h, "num_mels", 80)), 7), "conv_pre.bias": (c0,)}
    for i, k in enumerate(ksz):
        out[f"ups.{i}{ups}.weight"] = (c0 >> i, c0 >> (i + 1), k)
        out[f"ups.{i}{ups}.bias"] = (c0 >> (i + 1),)

    def activation(p, ch):
        out[f"{p}.act.alpha"] = (ch,)
        if act == "snakebeta":
            out[f"{p}.act.beta"] = (ch,)
        out[f"{p}.upsample.filter"] = (1, 1, 12); out[f"{p}.downsample.lowpass.filter"] = (1, 1, 12)
    for i in range(len(rates)):
        ch = c0 >> (i + 1)
        for j, k in enumerate(rk):
            for cs in ("convs1", "convs2"):
                for m in range(3):
                    out[f"resblocks.{i * len(rk) + j}.{cs}.{m}.weight"] = (ch, ch, k)
                    out[f"resblocks.{i * len(rk) + j}.{cs}.{m}.bias"] = (ch,)
            if act:
                for l in range(6):
                    activation(f"resblocks.{i * len(rk) + j}.activations.{l}", ch)
    if act:
        activation("activation_post", c0 >> len(rates))
    out["conv_post.weight"] = (1, c0 >> len(rates), 7)
    out["conv_post.bias"] = (1,)
    return out


def make_config(h) -> _lib.DexVocoderConfig:
    """The library's DexVocoderConfig of a HiFi-GAN / BigVGAN config (config.json keys, attribute or dict access)."""
    c = _lib.DexVocoderConfig()
    rates, ksz, rk, rd = (list(_get(h, n)) for n in ("upsample_rates", "upsample_kernel_sizes", "resblock_kernel_sizes", "resblock_dilation_sizes"))
    c.num_mels, c.upsample_initial_channel, c.n_upsamples = int(_get(h, "num_mels", 80)), int(_get(h, "upsample_initial_channel")), len(rates)
    for i, (u, k) in enumerate(zip(rates, ksz)):
        c.upsample_rates[i], c.upsample_kernel_sizes[i] = int(u), int(k)
    c.activation, c.snake_logscale = ACTIVATION[_get(h, "activation")], int(bool(_get(h, "snake_logscale", False)))
    c.n_resblock_kernels = len(rk)
    for j, k in enumerate(rk[:3]):
        c.resblock_kernel_sizes[j] = int(k)
        for m in range(3):
            c.resblock_dilation_sizes[j][m] = int(rd[j][m])
    return c


def fold_weight_norm(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``weight = g * v / ||v||`` with the norm over every dim but 0 (torch.nn.utils.weight_norm, dim=0 — also for the
    ConvTranspose1d layers, whose dim 0 is the INPUT channel): what remove_weight_norm() leaves (models.py:169-173)."""
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_g"):
            base = k[: -len("_g")]
            wv = sd[base + "_v"].float()
            norm = wv.flatten(1).norm(dim=1).reshape(-1, *([1] * (wv.dim() - 1)))
            out[base] = v.float() * wv / norm
        elif k.endswith(".weight_v"):
            continue
        else:
            out[k] = v
    return out


class Generator(NativeModule):
    prefix, noun = "dex_voc", "vocoder"

    def __init__(self, h=None):
        super().__init__()
        h = AttrDict(HIFIGAN_V1) if h is None else h
        if str(_get(h, "resblock", "1")) != "1":
            raise ValueError("only ResBlock / AMPBlock type '1' (hifigan/config.json V1, bigvgan base) is built")
        self.h = h
        self._register(param_shapes(h))

    # ---- checkpoint surface ---------------------------------------------------------------------------------------
    def _fold_checkpoint(self, sd):
        return fold_weight_norm(sd)

    def remove_weight_norm(self):
        """No-op: weight norm is folded at load time (the reference calls this right after loading, utils.py:278)."""
        return self

    # ---- engine -----------------------------------------------------------------------------------------------------
    def _config(self):
        return make_config(self.h)

    def _library_weights(self):
        # BigVGAN: the library takes ONE copy of the resampling filter (all 73 buffers are the same Kaiser-sinc constant) and lists only
        # activation_post's pair
        sd = self.state_dict()
        f0 = sd.get("activation_post.upsample.filter")
        for k in self.shapes:
            if k.endswith(".filter") and not torch.equal(sd[k], f0):
                raise RuntimeError(f"{k} differs from activation_post.upsample.filter: per-layer resampling filters are not supported")
        return sd

    @property
    def halo_frames(self) -> int:
        """Mel frames of context a window needs on each side (``dex_voc_halo_frames``): every sample of the frames [t0, t0 + n) depends on
        nothing outside [t0 - H, t0 + n + H).  A function of the configuration alone; needs no device."""
        self._create()
        return int(self._lib.dex_voc_halo_frames(self._ctx))

    def _inputs(self, x, lengths):
        """(mel fp32 contiguous, lengths as device int32 or None) of a call, checked; the engine is up and the precision mode set."""
        dev = x.device
        if lengths is not None:
            lengths = torch.as_tensor(lengths)
            if lengths.numel() != x.shape[0] or lengths.is_floating_point():
                raise ValueError(f"lengths must hold B = {x.shape[0]} integer frame counts, got {tuple(lengths.shape)} {lengths.dtype}")
        self._engine(dev)
        with torch.cuda.device(dev):
            # operand precision of the convolutions: 'fp32' (default, the parity mode), 'bf16' or 'fp16' (attribute ``precision``)
            self._check(self._lib.dex_voc_set_precision(self._ctx, _lib.PRECISION[getattr(self, "precision", "fp32")]))
            mel = x.to(dtype=torch.float32).contiguous()
            if mel.shape[1] != int(_get(self.h, "num_mels", 80)):
                raise ValueError(f"mel has {mel.shape[1]} channels, the generator expects {_get(self.h, 'num_mels', 80)}")
            ln = None if lengths is None else lengths.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        return mel, ln

    @staticmethod
    def _chunk(chunk_frames, T):
        n = int(chunk_frames)
        if n != chunk_frames or n < 1:
            raise ValueError(f"chunk_frames must be a positive integer, got {chunk_frames!r}")
        return min(n, T)

    def _window(self, mel, ln, t0, n, out_ptr, out_bstride, N):
        """Enqueue ``dex_vocode_window`` for the frames [t0, t0 + n) on the current stream (workspace: that of N-frame windows)."""
        dev = mel.device
        B, _, T = mel.shape
        need = int(self._lib.dex_voc_window_workspace_bytes(self._ctx, B, N))
        base, nbytes = self._workspace(need, dev)
        self._check(self._lib.dex_vocode_window(self._ctx, C.c_void_p(mel.data_ptr()), C.c_void_p(ln.data_ptr() if ln is not None else None), B, T,
                                                t0, n, C.c_void_p(out_ptr), out_bstride, C.c_void_p(base), nbytes, stream(dev)))

    @torch.no_grad()
    def forward(self, x: torch.Tensor, lengths=None, chunk_frames=None) -> torch.Tensor:
        """mel [B, num_mels, T] -> wav [B, 1, T * prod(upsample_rates)] (models.py:150-167).

        ``lengths`` (a sequence or an integer tensor of B frame counts, on any device): a ragged batch.  Utterance b is vocoded exactly
        as if it had been passed alone as ``x[b:b+1, :, :lengths[b]]`` (``dex_vocode_ragged``): its waveform ends at ``lengths[b] * hop``
        and is exactly zero behind that, and whatever ``x`` holds past ``lengths[b]`` is ignored.  Without it the padded batch is
        vocoded as one [B, T] tensor, and the padding (a log-mel of 0 is a loud frame) reaches the last frames of every shorter
        utterance.  The lengths stay on the device: no host synchronisation.

        ``chunk_frames`` = N: the same tensor (in fp32 bit for bit), computed window by window of N frames into the output
        (``dex_vocode_window``): the workspace is that of one window of min(N, T) frames plus ``halo_frames`` on each side, whatever T
        is, at the price of recomputing the halo per window.  ``stream()`` hands the windows out one by one."""
        mel, ln = self._inputs(x, lengths)
        dev = mel.device
        B, M, T = mel.shape
        with torch.cuda.device(dev):
            n = int(self._lib.dex_voc_samples(self._ctx, T))
            wav = torch.empty(B, 1, n, dtype=torch.float32, device=dev)
            if chunk_frames is not None:
                N, hop = self._chunk(chunk_frames, T), n // T
                for t0 in range(0, T, N):
                    self._window(mel, ln, t0, min(N, T - t0), wav.data_ptr() + 4 * t0 * hop, n, N)
                self._keep = (mel, ln)
            elif ln is None:
                need = int(self._lib.dex_voc_workspace_bytes(self._ctx, B, T))
                base, nbytes = self._workspace(need, dev)
                self._check(self._lib.dex_vocode(self._ctx, C.c_void_p(mel.data_ptr()), B, T, C.c_void_p(wav.data_ptr()), C.c_void_p(base),
                                                 nbytes, stream(dev)))
                self._keep = mel
            else:
                need = int(self._lib.dex_voc_ragged_workspace_bytes(self._ctx, B, T))
                base, nbytes = self._workspace(need, dev)
                self._check(self._lib.dex_vocode_ragged(self._ctx, C.c_void_p(mel.data_ptr()), C.c_void_p(ln.data_ptr()), B, T,
                                                        C.c_void_p(wav.data_ptr()), C.c_void_p(base), nbytes, stream(dev)))
                self._keep = (mel, ln)
            return wav

    def stream(self, x: torch.Tensor, lengths=None, chunk_frames: int = 64):
        """``forward(x, lengths)`` handed out as it is computed: yields ``(t0, wav_chunk [B, 1, n * hop], event)`` per window of
        ``chunk_frames`` mel frames, in order (the last one may be shorter); the chunks' concatenation is ``forward``'s tensor.  Each
        chunk is enqueued on the current stream when the generator is advanced, and ``event`` (a ``torch.cuda.Event``) is recorded
        behind it: a consumer waits for the event - ``event.synchronize()``, or ``other_stream.wait_event(event)`` in front of its copy -
        and takes chunk i while chunk i + 1 computes.  Nothing here synchronises."""
        mel, ln = self._inputs(x, lengths)
        dev = mel.device
        B, M, T = mel.shape
        N = self._chunk(chunk_frames, T)
        hop = int(self._lib.dex_voc_samples(self._ctx, 1))
        for t0 in range(0, T, N):
            n = min(N, T - t0)
            with torch.cuda.device(dev):
                chunk = torch.empty(B, 1, n * hop, dtype=torch.float32, device=dev)
                self._window(mel, ln, t0, n, chunk.data_ptr(), n * hop, N)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
            yield t0, chunk, ev


def get_vocoder(config_path: Optional[str] = None, ckpt: Optional[dict] = None, device="cuda") -> Generator:
    """src/utils.py:251-281: config.json -> Generator -> load ckpt['generator'] -> eval -> remove_weight_norm -> device.  The
    'hifigan' choice's config.json builds HiFi-GAN; a BigVGAN config.json ('bigvgan_base' or 'bigvgan': ``activation`` set) BigVGAN."""
    h = AttrDict(json.load(open(config_path))) if config_path else AttrDict(HIFIGAN_V1)      # a BigVGAN config.json selects BigVGAN
    g = Generator(h)
    if ckpt is not None:
        g.load_state_dict(ckpt["generator"] if "generator" in ckpt else ckpt)
    return g.eval().to(device)


BigVGAN = Generator      # bigvgan/__init__.py: ``from .models import BigVGAN as Generator`` — Generator(AttrDict(BIGVGAN_BASE / BIGVGAN_22KHZ))
