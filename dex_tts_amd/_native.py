"""Host plumbing the wrappers of libdexamd.so share.  The waveform-side wrappers (speaker, asr, griffin_lim, wavprep, f0, audio,
align) take from here: the argument marshalling (``stream``, ``i32_ptr``, ``host_lengths``, ``on_device``, ``device_rows``,
``pad_wavs``, ``resample_to_16k``), ``Handle`` (the owner of one C handle: create, ``check``, growing workspace, destroy) with
``per_device`` and ``upload_weights``, and the stateless ``check``.  ``NativeModule`` is the ``nn.Module`` base of the modules that
own one weight-holding context (text encoder, style encoders, vocoder): the flat buffer registry under the reference's dotted names,
the checkpoint surface, and the context's create / upload / finalize / destroy cycle."""
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
        raise (ValueError if rc == _lib.DEX_ERR_ARG else RuntimeError)(f"{what} failed ({rc})")


def i32_ptr(a):
    """A contiguous host int32 array as an ``int32_t*`` argument (the pointer keeps the array alive)."""
    assert a.dtype == np.int32 and a.flags.c_contiguous, "the C ABI reads B packed int32 values"
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def host_lengths(lengths, B, hi, lo=1, what="lengths"):
    """``lengths`` (None = ``hi`` for every row, a tensor on any device, an ndarray or a sequence) -> contiguous host int32 [B];
    ``ValueError`` for a wrong count or a value outside [lo, hi].  Host only."""
    if lengths is None:
        lengths = np.full(B, hi)
    ln = np.asarray(lengths.detach().cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
    if ln.shape != (B,):
        raise ValueError(f"{what}: {ln.size} lengths for {B} rows")
    if (ln < lo).any() or (ln > hi).any():
        raise ValueError(f"{what}: every length must lie in [{lo}, {hi}], got {ln.tolist()}")
    return np.ascontiguousarray(ln.astype(np.int32))


def on_device(x, what, refuse=RuntimeError):
    """``x`` if it is a CUDA tensor; else ``refuse`` naming the entry point ``what``."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise refuse(f"{what} runs on an MI355X only (no CPU path): pass CUDA tensors")
    return x


def device_rows(x, lengths, what, dtype=torch.float32, refuse=RuntimeError):
    """x [n] or [B, n] (a CUDA tensor, else ``refuse``), lengths as for ``host_lengths`` -> (contiguous [B, n] in ``dtype`` on the
    device, host int32 lengths in [1, n], one-row flag).  Needs no library."""
    on_device(x, what, refuse)
    if x.dim() not in (1, 2) or x.shape[0] < 1 or x.shape[-1] < 1:
        raise ValueError(f"{what}: expected [n] or [B, n] with at least one sample, got {tuple(x.shape)}")
    one = x.dim() == 1
    x = (x[None] if one else x).to(dtype).contiguous()
    return x, host_lengths(lengths, x.shape[0], x.shape[1], what=what), one


def pad_wavs(wavs, device, scale_int16=False):
    """A list of 1-D wavs (tensors or arrays of any integer or float type) -> (fp32 [B, max n] on ``device``, 0 past a row's end,
    host int32 lengths).  ``scale_int16``: int16 rows are scaled by 1 / 32768."""
    rows = []
    for w in wavs:
        a = np.asarray(w.cpu() if torch.is_tensor(w) else w).reshape(-1)
        rows.append(a.astype(np.float32) / 32768.0 if scale_int16 and a.dtype == np.int16 else a.astype(np.float32))
    if not rows or min(len(r) for r in rows) < 1:
        raise ValueError("every wav needs at least one sample")
    out = torch.zeros(len(rows), max(len(r) for r in rows), dtype=torch.float32)
    for b, r in enumerate(rows):
        out[b, : len(r)] = torch.from_numpy(r)
    return out.to(device), np.array([len(r) for r in rows], dtype=np.int32)


def resample_to_16k(x, ln, sr):
    """Rows x fp32 [B, n] of host lengths ``ln`` at ``sr`` Hz -> (rows, lengths) at 16 kHz: ``wavprep.resample`` (kaiser_best in
    fp64) rounded to fp32 once; as they are where ``sr`` is None or 16000."""
    if sr is None or int(sr) == 16000:
        return x, ln
    from . import wavprep
    y, lo = wavprep.resample(x, int(sr), 16000, lengths=ln)
    return y.to(torch.float32), lo


def device_index(device) -> int:
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def per_device(make):
    """``make(device)`` memoised by the device's index: the one-per-device objects (handles, tables) of the stateless entry points."""
    cache = {}

    def get(device):
        key = device_index(device)
        if key not in cache:
            cache[key] = make(torch.device("cuda", key))
        return cache[key]
    return get


class Handle:
    """Owner of one C handle of the symbols ``<prefix>_create`` / ``_destroy`` / ``_last_error`` (``dex_spk``, ``dex_asr``,
    ``dex_gl``, ``dex_mel``), created under ``device`` with ``create_args`` before the out pointer, and of one growing byte
    workspace.  ``arg_errors``: the return codes ``check`` raises as ``ValueError`` (a refused argument, weights not loaded)."""

    def __init__(self, prefix, device="cuda", *create_args, arg_errors=(_lib.DEX_ERR_ARG, _lib.DEX_ERR_STATE)):
        self.prefix, self.arg_errors = prefix, arg_errors
        self.device = torch.device("cuda", device_index(device))
        self.lib = _lib.load()
        self.h = self._ws = None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._fn("create")(*create_args, C.byref(h))
        if rc != _lib.DEX_OK:
            raise self.create_failed(rc)
        self.h = h

    def _fn(self, name):
        return getattr(self.lib, f"{self.prefix}_{name}")

    def create_failed(self, rc):
        return RuntimeError(f"{self.prefix}_create failed ({rc})")

    def __del__(self):
        try:
            if self.h:
                self._fn("destroy")(self.h)
                self.h = None
        except Exception:
            pass

    def check(self, rc, what):
        if rc != _lib.DEX_OK:
            msg = self._fn("last_error")(self.h)
            raise (ValueError if rc in self.arg_errors else RuntimeError)(f"{what}: {msg.decode() if msg else '?'} ({rc})")

    def workspace(self, need) -> torch.Tensor:
        """A uint8 tensor of at least ``need`` bytes, kept between calls; the old buffer is released before a larger one is made."""
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws


def upload_weights(handle, load_fn, tensors, device):
    """Every ``{key: tensor}`` through ``load_fn(h, key, fp32 data, shape, ndim, stream)`` (``dex_spk_load`` / ``dex_asr_load``) on the
    current stream of ``device``, which is synchronised before the device copies the uploads read are dropped."""
    keep = []
    with torch.cuda.device(device):
        for k, v in tensors.items():
            t = v.detach().to(device=device, dtype=torch.float32).contiguous()
            keep.append(t)
            shape = (C.c_int64 * t.dim())(*t.shape)
            handle.check(load_fn(handle.h, k.encode(), t.data_ptr(), shape, t.dim(), stream(device)), f"{load_fn.__name__}({k})")
        torch.cuda.current_stream(device).synchronize()


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
