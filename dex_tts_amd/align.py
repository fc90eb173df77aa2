"""Monotonic alignment search on the device: the Glow-TTS ``maximum_path`` that DEX-TTS / GeDEX-TTS call in ``compute_loss``
(model/monotonic_align, tts.py:99-109 / GeDEX :70-80), the log-prior it searches, forced alignment from ``mu_x`` / ``y``, and the
duration and prior loss reductions of the validation pass.  The arithmetic runs in libdexamd.so (csrc/mas.hip); the contract is the
docstring of tests/mas_restatement.py, and the path is bitwise the reference's Cython core's for the same fp32 input.  There is no CPU
path: CPU tensors and tensors that require grad are refused with RuntimeError.

    from dex_tts_amd.align import maximum_path        # drop-in for model.monotonic_align.maximum_path
    attn = maximum_path(log_prior, attn_mask.squeeze(1))
    dur = mas_durations(mu_x, x_lengths, y, y_lengths)  # [B, Tx] int32 frames per token (forced alignment)
    y_cut, mu_y_cut, y_cut_mask, cut_lengths = segment(mu_x, dur, y, y_lengths, out_size=172)   # the random out_size cut
"""
from __future__ import annotations

import random

import numpy as np
import torch

from . import _lib
from ._native import check, i32_ptr, stream

MAX_TX, MAX_TY = 2048, 8192          # include/dex_amd.h DEX_MAS_MAX_TX / DEX_MAS_MAX_TY


def _dev(*ts):
    for t in ts:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("the alignment search runs on an MI355X only (no CPU path): pass CUDA tensors")
        if t.requires_grad:
            raise RuntimeError("the alignment search is forward-only (no backward): detach the inputs or call it under torch.no_grad()")
    return ts[0].device


def _lens(v, B):
    ln = np.ascontiguousarray(np.asarray(torch.as_tensor(v).detach().cpu(), dtype=np.int64).reshape(-1))
    if ln.shape != (B,) or (ln < 0).any() or (ln > np.iinfo(np.int32).max).any():
        raise ValueError(f"lengths must hold B = {B} non-negative values")
    return np.ascontiguousarray(ln.astype(np.int32))


def log_prior(mu_x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """tts.py:100-106: mu_x [B, F, Tx], y [B, F, Ty] -> log_prior [B, Tx, Ty] fp32 (a transposed view of the frame-major [B, Ty, Tx]
    tensor the search reads)."""
    return _log_prior_yx(mu_x, y).transpose(1, 2)


def _log_prior_yx(mu_x, y):
    dev = _dev(mu_x, y)
    lib = _lib.load()
    if mu_x.dim() != 3 or y.dim() != 3 or mu_x.shape[:2] != y.shape[:2]:
        raise ValueError("mu_x must be [B, F, Tx] and y [B, F, Ty]")
    B, F, Tx = mu_x.shape
    Ty = y.shape[2]
    with torch.cuda.device(dev):
        m, yy = mu_x.to(torch.float32).contiguous(), y.to(torch.float32).contiguous()
        out = torch.empty(B, Ty, Tx, dtype=torch.float32, device=dev)
        check(lib.dex_mas_log_prior(m.data_ptr(), yy.data_ptr(), B, F, Tx, Ty, out.data_ptr(), stream(dev)), "dex_mas_log_prior")
    return out


def _search(value, mask, tx, ty, want_path):
    """value: fp32 [B, Tx, Ty] view (any strides) -> (dur [B, Tx] int32, path [B, Tx, Ty] fp32 or None)."""
    lib = _lib.load()
    dev = value.device
    B, Tx, Ty = value.shape
    if mask is not None and mask.stride() != value.stride():
        mask = mask.contiguous()
        value = value.contiguous()
    need = int(lib.dex_mas_workspace_bytes(B, Tx, Ty))
    if need == 0:
        raise ValueError(f"[B, Tx, Ty] = {[B, Tx, Ty]}: need B >= 1, 1 <= Tx <= {MAX_TX}, 1 <= Ty <= {MAX_TY}")
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        dur = torch.empty(B, Tx, dtype=torch.int32, device=dev)
        path = torch.empty(B, Tx, Ty, dtype=torch.float32, device=dev) if want_path else None
        sb, sx, sy = value.stride()
        check(lib.dex_mas_durations(value.data_ptr(), mask.data_ptr() if mask is not None else None, B, Tx, Ty, sb, sx, sy,
                                    i32_ptr(tx), i32_ptr(ty), dur.data_ptr(), path.data_ptr() if path is not None else None,
                                    ws.data_ptr(), need, stream(dev)), "dex_mas_durations")
    return dur, path


@torch.no_grad()
def maximum_path(value: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """model.monotonic_align.maximum_path: value, mask [b, t_x, t_y] -> the 0/1 path [b, t_x, t_y] in value's dtype on value's
    device.  As the reference: the search runs on value * mask in fp32 and the lengths are mask.sum(1)[:, 0], mask.sum(2)[:, 0]."""
    dev = _dev(value, mask)
    if value.dim() != 3 or tuple(mask.shape) != tuple(value.shape):
        raise ValueError("value and mask must both be [b, t_x, t_y]")
    B = value.shape[0]
    tx = _lens(mask.sum(1)[:, 0], B)              # the reference reads these on the host as well
    ty = _lens(mask.sum(2)[:, 0], B)
    v = value if value.dtype == torch.float32 else value.to(torch.float32)
    m = mask if mask.dtype == torch.float32 else mask.to(torch.float32)
    with torch.cuda.device(dev):
        _, path = _search(v, m, tx, ty, True)
    return path if value.dtype == torch.float32 else path.to(value.dtype)


@torch.no_grad()
def mas_durations(mu_x: torch.Tensor, x_lengths, y: torch.Tensor, y_lengths, return_log_prior: bool = False):
    """Forced alignment as compute_loss finds it: mu_x [B, F, Tx], y [B, F, Ty] + lengths -> per-token durations [B, Tx] int32
    (frames of each token; 0 past x_lengths).  return_log_prior: also the [B, Tx, Ty] log-prior the search ran on."""
    _dev(mu_x, y)
    B = mu_x.shape[0]
    tx, ty = _lens(x_lengths, B), _lens(y_lengths, B)
    lp = _log_prior_yx(mu_x, y)                                # [B, Ty, Tx]
    dur, _ = _search(lp.transpose(1, 2), None, tx, ty, False)
    return (dur, lp.transpose(1, 2)) if return_log_prior else dur


@torch.no_grad()
def dur_prior_losses(logw: torch.Tensor, dur: torch.Tensor, x_lengths, y: torch.Tensor, mu_y: torch.Tensor, y_lengths):
    """The duration and prior losses of compute_loss (tts.py:112-113 with utils.py:42-44, and :148-149) as two 0-d device tensors:

        dur_loss   = sum (logw - log(1e-8 + dur) x_mask)^2 / sum x_lengths            logw [B, 1, Tx] or [B, Tx], dur [B, Tx]
        prior_loss = sum 0.5 ((y - mu_y)^2 + log 2 pi) y_mask / (sum y_mask n_feats)  y, mu_y [B, n_feats, Ty]

    Per-utterance partial sums in a fixed order and one combine, all on the device."""
    dev = _dev(logw, dur, y, mu_y)
    lib = _lib.load()
    B = y.shape[0]
    lw = logw.reshape(B, -1).to(torch.float32).contiguous()
    Tx = lw.shape[1]
    d = dur.to(torch.int32).contiguous()
    if tuple(d.shape) != (B, Tx) or y.shape != mu_y.shape or y.dim() != 3:
        raise ValueError("logw [B, (1,) Tx], dur [B, Tx], y / mu_y [B, n_feats, Ty]")
    F, Ty = y.shape[1], y.shape[2]
    tx, ty = _lens(x_lengths, B), _lens(y_lengths, B)
    need = int(lib.dex_mas_loss_workspace_bytes(B))
    with torch.cuda.device(dev):
        yy, mm = y.to(torch.float32).contiguous(), mu_y.to(torch.float32).contiguous()
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        check(lib.dex_mas_losses(lw.data_ptr(), d.data_ptr(), i32_ptr(tx), B, Tx, yy.data_ptr(), mm.data_ptr(), i32_ptr(ty), F, Ty,
                                 out.data_ptr(), ws.data_ptr(), need, stream(dev)), "dex_mas_losses")
    return out[0], out[1]


def segment_offsets(y_lengths, out_size: int) -> np.ndarray:
    """The per-row cut offsets of compute_loss (tts.py:119-124), drawn from Python's ``random`` exactly as the reference draws them:
    ``random.choice(range(0, max_offset))`` for a row with max_offset = y_len - out_size > 0, else 0 without a draw.  After
    ``random.seed(s)`` this returns the reference's offsets and leaves ``random`` in the reference's state.  -> int64 [B]."""
    yl = np.asarray(torch.as_tensor(y_lengths).detach().cpu(), dtype=np.int64).reshape(-1)
    return np.array([random.choice(range(0, m)) if m > 0 else 0 for m in (max(int(l) - int(out_size), 0) for l in yl)], dtype=np.int64)


@torch.no_grad()
def segment(mu_x: torch.Tensor, dur: torch.Tensor, y: torch.Tensor, y_lengths, out_size=None, offsets=None):
    """The out_size cut of compute_loss and mu_y = attn^T mu_x on it (tts.py:115-144), without the [B, Tx, Ty] path:

        mu_x [B, F, Tx], dur [B, Tx] int32 (mas_durations), y [B, F, Ty] + lengths
        -> y_cut [B, F, S], mu_y_cut [B, F, S], y_cut_mask [B, 1, S] fp32 on the device, cut_lengths int64 [B] on the host

    S = out_size when out_size < Ty (a cut), else Ty.  Row b keeps frames [off_b, off_b + cut_b), cut_b = min(S, y_len_b); past
    cut_b every output is 0.  ``offsets`` (host, [B]) default to ``segment_offsets(y_lengths, out_size)`` for a cut and to 0
    otherwise.  mu_y_cut is bitwise the reference's 0/1 matmul."""
    dev = _dev(mu_x, dur, y)
    lib = _lib.load()
    if mu_x.dim() != 3 or y.dim() != 3 or mu_x.shape[:2] != y.shape[:2] or tuple(dur.shape) != (mu_x.shape[0], mu_x.shape[2]):
        raise ValueError("mu_x must be [B, F, Tx], dur [B, Tx] and y [B, F, Ty]")
    B, F, Tx = mu_x.shape
    Ty = y.shape[2]
    yl = _lens(y_lengths, B)
    cut = out_size is not None and int(out_size) < Ty
    S = int(out_size) if cut else Ty
    if S < 1:
        raise ValueError(f"out_size must be >= 1, got {out_size}")
    if offsets is None:
        offsets = segment_offsets(yl, S) if cut else np.zeros(B, np.int64)
    off = np.asarray(torch.as_tensor(offsets).detach().cpu(), dtype=np.int64).reshape(-1)
    cl = np.minimum(yl.astype(np.int64), S)
    if off.shape != (B,) or (off < 0).any() or (off > yl - cl).any():
        raise ValueError(f"offsets must hold B = {B} values with 0 <= offset <= y_length - min(S, y_length)")
    off32 = np.ascontiguousarray(off.astype(np.int32))
    with torch.cuda.device(dev):
        m, yy, d = mu_x.to(torch.float32).contiguous(), y.to(torch.float32).contiguous(), dur.to(torch.int32).contiguous()
        y_cut = torch.empty(B, F, S, dtype=torch.float32, device=dev)
        mu_cut = torch.empty(B, F, S, dtype=torch.float32, device=dev)
        mask = torch.empty(B, 1, S, dtype=torch.float32, device=dev)
        check(lib.dex_loss_segment(m.data_ptr(), d.data_ptr(), yy.data_ptr(), B, F, Tx, Ty, i32_ptr(yl), i32_ptr(off32), S, y_cut.data_ptr(),
                                   mu_cut.data_ptr(), mask.data_ptr(), stream(dev)), "dex_loss_segment")
    return y_cut, mu_cut, mask, torch.from_numpy(cl)
