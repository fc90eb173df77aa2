"""Host-side mirror of the DEX style encoders and the pre-decoder lines of ``DeXTTS.forward`` (DEX-TTS/model/tts.py:26-31,
55-67; model/ref_encoder.py TVEncoder / LF0Encoder / TIVEncoder): one module holding ``tv_encoder.* / lf0_encoder.* /
tiv_encoder.* / conv_sty.*`` under the reference's state-dict names, so the matching entries of a DeXTTS checkpoint load
unchanged.  ``forward(ref, ref_lengths, sty, sty_lengths, lf0, lf0_lengths)`` returns what the reference feeds on:

    ref_skips  list of [B, c_h, Tr]      -> Diffusion.forward(ref=...)            (tts.py:67,84)
    sty_dec    [B, 2*dim, Ts]            -> Diffusion.forward(sty=...)            (tts.py:65-66)
    sty_enc    [B, c_out]                -> TextEncoder(x, x_lengths, sty_enc)    (tts.py:62-63,68)

Eval mode only (dropout off, BatchNorm on running statistics — folded into the preceding convolution here —, frozen VQ
codebook).  The arithmetic runs in libdexamd.so (``dex_style_encode``); no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from . import _lib
from ._native import NativeModule, stream

VCTK = dict(tv_encoder=dict(c_in=80, num_layer=6, c_h=128, c_out=192, c_out_g=192, commit_w=0.25, n_emb=512),
            lf0_encoder=dict(c_in=1, c_h=192, c_out=192, c_out_g=192, num_layer=2),
            tiv_encoder=dict(c_in=80, num_layer=6, c_h=128, c_out=64), dim=64)


def _basic(out, p, cin, cout, norm):
    out[f"{p}.conv.weight"] = (cout, cin, 3)
    if norm == "ln":
        out[f"{p}.ln.weight"] = (cout,); out[f"{p}.ln.bias"] = (cout,)
    elif norm == "bn":
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{p}.bn.{k}"] = (cout,)
        out[f"{p}.bn.num_batches_tracked"] = ()


def _projection(out, p, cin, ch):
    out[f"{p}.conv_1.weight"] = (ch, cin, 3); out[f"{p}.conv_1.bias"] = (ch,)
    out[f"{p}.norm_1.gamma"] = (ch,); out[f"{p}.norm_1.beta"] = (ch,)
    out[f"{p}.conv_2.weight"] = (ch, ch, 3); out[f"{p}.conv_2.bias"] = (ch,)
    out[f"{p}.norm_2.gamma"] = (ch,); out[f"{p}.norm_2.beta"] = (ch,)
    out[f"{p}.proj.weight"] = (ch, ch, 1); out[f"{p}.proj.bias"] = (ch,)


def param_shapes(cfg) -> Dict[str, tuple]:
    """The reference state dict of (tv_encoder, lf0_encoder, tiv_encoder, conv_sty), in registration order."""
    tv, lf, ti = cfg["tv_encoder"], cfg["lf0_encoder"], cfg["tiv_encoder"]
    o: Dict[str, tuple] = {}
    p = "tv_encoder"
    _basic(o, f"{p}.in_conv", tv["c_in"], tv["c_h"], "ln")
    for i in range(tv["num_layer"]):
        _basic(o, f"{p}.conv_blocks.{i}.conv_block.0", tv["c_h"], tv["c_h"], "ln")
        _basic(o, f"{p}.conv_blocks.{i}.conv_block.1", tv["c_h"], tv["c_h"], "")
    _basic(o, f"{p}.out_conv", tv["c_h"], tv["c_out"], "")
    o[f"{p}.vq.embedding"] = (tv["n_emb"], tv["c_out"]); o[f"{p}.vq.ema_count"] = (tv["n_emb"],); o[f"{p}.vq.ema_weight"] = (tv["n_emb"], tv["c_out"])
    _projection(o, f"{p}.proj_0", tv["c_out"], tv["c_out_g"])
    _basic(o, f"{p}.proj_1", tv["c_out_g"], tv["c_out_g"], "bn")
    p = "lf0_encoder"
    _basic(o, f"{p}.in_conv", lf["c_in"], lf["c_h"], "ln")
    H = lf["c_h"] // 2
    for l in range(lf["num_layer"]):
        for sfx in ("", "_reverse"):
            o[f"{p}.rnn_layer.weight_ih_l{l}{sfx}"] = (3 * H, lf["c_h"]); o[f"{p}.rnn_layer.weight_hh_l{l}{sfx}"] = (3 * H, H)
            o[f"{p}.rnn_layer.bias_ih_l{l}{sfx}"] = (3 * H,); o[f"{p}.rnn_layer.bias_hh_l{l}{sfx}"] = (3 * H,)
    _basic(o, f"{p}.out_conv", lf["c_h"], lf["c_out"], "ln")
    _projection(o, f"{p}.proj", lf["c_out"], lf["c_out_g"])
    p = "tiv_encoder"
    _basic(o, f"{p}.in_conv", ti["c_in"], ti["c_h"], "bn")
    for i in range(ti["num_layer"]):
        _basic(o, f"{p}.conv_blocks.{i}.conv_block.0", ti["c_h"], ti["c_h"], "bn")
        _basic(o, f"{p}.conv_blocks.{i}.conv_block.1", ti["c_h"], ti["c_h"], "")
    _basic(o, f"{p}.out_conv", ti["c_h"], ti["c_out"], "bn")
    o["conv_sty.weight"] = (cfg["dim"] * 2, tv["c_out_g"], 1); o["conv_sty.bias"] = (cfg["dim"] * 2,)
    return o


def fold_batchnorm(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """BasicConv with norm_type 'bn' in eval mode (base.py:54-58: conv without bias -> BatchNorm1d(eps 1e-5) on running
    statistics) == conv with weight * s[co] and bias beta - mean * s, s = gamma / sqrt(var + eps).  Returns the library's
    view of the state dict: '<p>.conv.weight' + '<p>.conv.bias' replace '<p>.bn.*'."""
    out = {}
    for k, v in sd.items():
        if ".bn." in k:
            continue
        out[k] = v
    for k in sd:
        if k.endswith(".bn.weight"):
            p = k[: -len(".bn.weight")]
            s = sd[f"{p}.bn.weight"].double() / torch.sqrt(sd[f"{p}.bn.running_var"].double() + 1e-5)
            out[f"{p}.conv.weight"] = (sd[f"{p}.conv.weight"].double() * s.view(-1, 1, 1)).float()
            out[f"{p}.conv.bias"] = (sd[f"{p}.bn.bias"].double() - sd[f"{p}.bn.running_mean"].double() * s).float()
    return out


class StyleEncoders(NativeModule):
    """``load_state_dict`` accepts the four sub-dicts of a DeXTTS checkpoint (keys tv_encoder.* / lf0_encoder.* / tiv_encoder.* /
    conv_sty.*; other keys are ignored unless ``strict``)."""
    prefix, noun = "dex_style", "style"

    def __init__(self, cfg=None):
        super().__init__()
        self.cfg = dict(VCTK) if cfg is None else cfg
        self._register(param_shapes(self.cfg), dtype=lambda key: torch.int64 if key.endswith("num_batches_tracked") else torch.float32)

    def _config(self):
        tv, lf, ti = self.cfg["tv_encoder"], self.cfg["lf0_encoder"], self.cfg["tiv_encoder"]
        return _lib.DexStyleConfig(tv["c_in"], ti["num_layer"], ti["c_h"], tv["num_layer"], tv["c_h"], tv["c_out"], tv["c_out_g"], tv["n_emb"],
                                   lf["c_h"], lf["c_out"], lf["c_out_g"], lf["num_layer"], self.cfg["dim"] * 2)

    def _library_weights(self):
        return fold_batchnorm({k: v.float() if v.is_floating_point() else v for k, v in self.state_dict().items()})

    @torch.no_grad()
    def forward(self, ref: torch.Tensor, ref_lengths: torch.Tensor, sty: torch.Tensor, sty_lengths: torch.Tensor,
                lf0: torch.Tensor, lf0_lengths: torch.Tensor, return_indices: bool = False, return_vq_loss: bool = False):
        """tts.py:55-67: ref [B,80,Tr] (or [B,1,80,Tr]), sty [B,80,Ts], lf0 [B,Tl] + lengths -> (ref_skips, sty_dec, sty_enc).
        return_indices appends the VQ codes [B,Ts] int32; return_vq_loss appends, last, the eval-mode VQ commitment loss of
        compute_loss (ref_encoder.py:226, commit_w of the tv_encoder config) as a 0-d device tensor (dex_style_encode_loss: the
        other outputs are bitwise those of dex_style_encode)."""
        dev = ref.device
        self._engine(dev)
        with torch.cuda.device(dev):
            f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
            i = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
            ref, sty, lf0 = f(ref.squeeze(1) if ref.dim() == 4 else ref), f(sty.squeeze(1) if sty.dim() == 4 else sty), f(lf0)
            rl, sl, ll = i(ref_lengths), i(sty_lengths), i(lf0_lengths)
            B, M, Tr = ref.shape
            Ts, Tl = sty.shape[2], lf0.shape[1]
            tv, ti = self.cfg["tv_encoder"], self.cfg["tiv_encoder"]
            if sty.shape[:2] != (B, M) or lf0.shape[0] != B or M != tv["c_in"]:
                raise ValueError("ref / sty must be [B, n_mels, T] and lf0 [B, T] with one batch size")
            skips = [torch.empty(B, ti["c_h"], Tr, dtype=torch.float32, device=dev) for _ in range(ti["num_layer"])]
            sty_dec = torch.empty(B, self.cfg["dim"] * 2, Ts, dtype=torch.float32, device=dev)
            sty_enc = torch.empty(B, tv["c_out"], dtype=torch.float32, device=dev)
            idx = torch.empty(B, Ts, dtype=torch.int32, device=dev)
            wsq = self._lib.dex_style_loss_workspace_bytes if return_vq_loss else self._lib.dex_style_workspace_bytes
            need = int(wsq(self._ctx, B, Tr, Ts, Tl))
            base, nbytes = self._workspace(need, dev)
            arr = (C.c_void_p * len(skips))(*[s.data_ptr() for s in skips])
            a = _lib.DexStyleArgs(B, Tr, Ts, Tl, ref.data_ptr(), rl.data_ptr(), sty.data_ptr(), sl.data_ptr(), lf0.data_ptr(), ll.data_ptr(),
                                  C.cast(arr, C.POINTER(C.c_void_p)), sty_dec.data_ptr(), sty_enc.data_ptr(), idx.data_ptr(), base, nbytes)
            st = stream(dev)
            if return_vq_loss:
                vq_loss = torch.empty((), dtype=torch.float32, device=dev)
                self._check(self._lib.dex_style_encode_loss(self._ctx, C.byref(a), float(tv.get("commit_w", 0.25)), vq_loss.data_ptr(), st))
            else:
                self._check(self._lib.dex_style_encode(self._ctx, C.byref(a), st))
            self._keep = (ref, sty, lf0, rl, sl, ll, arr)
            out = (skips, sty_dec, sty_enc) + ((idx,) if return_indices else ())
            return out + (vq_loss,) if return_vq_loss else out
