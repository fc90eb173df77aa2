"""Host plumbing the wrappers of libdexamd.so share: the ctypes helpers of the stateless entry points (align, audio, f0, wavprep, engine)
and ``NativeModule``, the ``nn.Module`` base of the modules that own one weight-holding context (text encoder, style encoders,
vocoder): the flat buffer registry under the reference's dotted names, the checkpoint surface, and the context's create / upload /
finalize / destroy cycle."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from . import _lib


def stream(dev) -> C.c_void_p:
    """The current torch stream of ``dev`` as a dex_stream_t."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def check(rc, what):
    if rc != _lib.DEX_OK:
        raise (ValueError if rc == -1 else RuntimeError)(f"{what} failed ({rc})")


def i32_ptr(a):
    """A contiguous host int32 array as an ``int32_t*`` argument."""
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def device_rows(x, lengths):
    """x [L] or [B, L] (device) -> (fp32 [B, L] on the device, host int32 lengths, one-row flag)."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("the f0 tracker runs on an MI355X only (no CPU path): pass a CUDA tensor")
    one = x.dim() == 1
    x = x.reshape(1, -1) if one else x
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be [L] or [B, L]")
    B, L = x.shape
    ln = np.full(B, L, dtype=np.int32) if lengths is None else np.asarray(torch.as_tensor(lengths).cpu(), dtype=np.int32).reshape(-1)
    if ln.shape != (B,) or (ln < 1).any() or (ln > L).any():
        raise ValueError(f"lengths must hold B = {B} values in [1, {L}]")
    return x.to(torch.float32).contiguous(), np.ascontiguousarray(ln), one


class NativeModule(nn.Module):
    """Subclasses call ``_register(shapes)`` in their constructor and supply ``_config()`` (the context's config struct) and
    ``_library_weights()`` (key -> tensor, a superset of the library's inventory).  ``prefix`` names the context's symbols
    (``<prefix>_create`` ... ``<prefix>_last_error``), ``noun`` the module in error messages."""
    prefix = ""
    noun = ""

    def _register(self, shapes: Dict[str, tuple], dtype=lambda key: torch.float32):
        self.shapes = shapes
        for key, shape in shapes.items():           # flat parameter registry under the reference's dotted names
            self.register_buffer(key.replace(".", "__"), torch.zeros(shape, dtype=dtype(key)), persistent=False)
        self._ctx = None
        self._lib = None
        self._loaded_key = None
        self._ws = None

    # ---- checkpoint surface
    def state_dict(self, *a, **k):
        return {key: getattr(self, key.replace(".", "__")) for key in self.shapes}

    def _fold_checkpoint(self, sd):
        """The checkpoint as the registry holds it (the vocoder folds weight norm here)."""
        return sd

    def load_state_dict(self, sd, strict: bool = True):
        sd = self._fold_checkpoint(dict(sd))
        missing = [k for k in self.shapes if k not in sd]
        extra = [k for k in sd if k not in self.shapes]
        if strict and (missing or extra):
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: missing {missing[:4]}, unexpected {extra[:4]}")
        for k, v in sd.items():
            if k in self.shapes:
                buf = getattr(self, k.replace(".", "__"))
                if tuple(v.shape) != tuple(buf.shape):
                    raise RuntimeError(f"{k}: shape {tuple(v.shape)} != {tuple(buf.shape)}")
                buf.copy_(v.detach().to(buf.dtype))
        self._loaded_key = None
        return self

    # ---- engine
    def _fn(self, name):
        return getattr(self._lib, f"{self.prefix}_{name}")

    def _check(self, rc):
        if rc != 0:
            msg = self._fn("last_error")(self._ctx)
            raise RuntimeError(f"libdexamd {self.noun} error {rc}: {msg.decode() if msg else '?'}")

    def _create(self):
        """The context itself (host only: the configuration is checked, the weight inventory laid out; nothing touches a device)."""
        if self._ctx is None:
            self._lib = _lib.load()
            c = self._config()
            ctx = C.c_void_p()
            rc = self._fn("create")(C.byref(c), C.byref(ctx))
            self._ctx = ctx
            self._check(rc)

    def _engine(self, device):
        """Create the context once; upload the weights the library lists and finalize whenever a buffer changed since the last upload."""
        if device.type != "cuda":
            raise RuntimeError("dex_tts_amd runs on an AMD GPU (torch device 'cuda' on ROCm); no CPU path exists")
        self._create()
        bufs = [getattr(self, k.replace(".", "__")) for k in self.shapes]
        key = (str(device),) + tuple((b._version, b.data_ptr()) for b in bufs)
        if key != self._loaded_key:
            sd = self._library_weights()
            with torch.cuda.device(device):
                st = stream(device)
                keep = []
                for i in range(self._fn("num_weights")(self._ctx)):
                    name = C.c_char_p(); shp = (C.c_int64 * 4)(); nd = C.c_int()
                    self._check(self._fn("weight_info")(self._ctx, i, C.byref(name), shp, C.byref(nd)))
                    k = name.value.decode()
                    w = sd[k].to(device=device, dtype=torch.float32).contiguous()
                    shape = (C.c_int64 * 4)(*([int(s) for s in w.shape] + [0] * (4 - w.dim())))
                    self._check(self._fn("load_weight_async")(self._ctx, k.encode(), C.c_void_p(w.data_ptr()), shape, w.dim(), st))
                    keep.append(w)
                self._check(self._fn("finalize")(self._ctx, st))
            self._loaded_key = key

    def __del__(self):
        try:
            if self._ctx is not None and self._ctx.value:
                self._fn("destroy")(self._ctx)
        except Exception:
            pass

    def _workspace(self, need, dev):
        """A 256-byte-aligned device workspace of at least ``need`` bytes, kept between calls: (address, usable bytes)."""
        if self._ws is None or self._ws.numel() < need + 256 or self._ws.device != dev:
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = (self._ws.data_ptr() + 255) // 256 * 256
        return base, self._ws.numel() - (base - self._ws.data_ptr())
