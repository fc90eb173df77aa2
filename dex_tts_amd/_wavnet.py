"""What the wrappers of the waveform networks share (asr.py: wav2vec 2.0 CTC; wavlm.py: WavLM x-vector; mos.py: UTMOS; whisper.py),
the Python side of ``csrc/wav_trunk.h``: the trunk's half of the config struct (``fill_trunk_config``), the weight inventory of a
handle (``weight_shapes``), the host-only entry points of a network (``HostEntry``: frame counts, the inventory of a config, the
lengths one call refuses), the routing of an HF state dict (``route_hf_state_dict``), the handle (``NetHandle``) and the base class
of the networks (``WaveformNet``: device, weights, the front end that brings wavs to 16 kHz rows, the checked inputs and the body of
every network call).  ``_native.py`` stays what every wrapper of the library shares."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._native import Handle, device_index, device_rows, i32_ptr, pad_wavs, resample_to_16k, stream, upload_weights

SAMPLING_RATE = 16000
MAX_CONV = 8                        # DEX_ASR_MAX_CONV, DEX_WAVLM_MAX_CONV


def fill_trunk_config(c, cfg):
    """The trunk's fields of the C struct ``c`` from the config dataclass ``cfg`` (the names agree between the two networks);
    ``NotImplementedError`` for what the struct cannot even express.  Returns ``c``."""
    for name in ("hidden_act", "feat_extract_activation"):
        if getattr(cfg, name) != "gelu":
            raise NotImplementedError(f"{name}={getattr(cfg, name)!r}: only 'gelu' (erf) is built")
    n = len(cfg.conv_dim)
    if not (1 <= n <= MAX_CONV) or len(cfg.conv_kernel) != n or len(cfg.conv_stride) != n:
        raise NotImplementedError(f"conv_dim / conv_kernel / conv_stride: 1 .. {MAX_CONV} layers of equal count, got "
                                  f"{n} / {len(cfg.conv_kernel)} / {len(cfg.conv_stride)}")
    c.n_conv = n
    for i in range(n):
        c.conv_dim[i], c.conv_kernel[i], c.conv_stride[i] = int(cfg.conv_dim[i]), int(cfg.conv_kernel[i]), int(cfg.conv_stride[i])
    c.conv_bias = int(bool(cfg.conv_bias))
    c.hidden, c.n_layers, c.n_heads, c.intermediate = int(cfg.hidden_size), int(cfg.num_hidden_layers), int(cfg.num_attention_heads), int(cfg.intermediate_size)
    c.do_stable_layer_norm = int(bool(cfg.do_stable_layer_norm))
    c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups = int(cfg.num_conv_pos_embeddings), int(cfg.num_conv_pos_embedding_groups)
    c.layer_norm_eps = float(cfg.layer_norm_eps)
    return c


def weight_shapes(lib, prefix: str, handle) -> dict:
    """{key: shape} of ``<prefix>_weight_info``, in the library's registration order."""
    out = {}
    key, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
    for i in range(getattr(lib, prefix + "_num_weights")(handle)):
        getattr(lib, prefix + "_weight_info")(handle, i, C.byref(key), shape, C.byref(nd))
        out[key.value.decode()] = tuple(int(shape[k]) for k in range(nd.value))
    return out


class HostEntry:
    """The host-only entry points of the network whose C symbols start with ``prefix``: ``c_config`` makes the C struct of a config,
    ``default`` is the config class, ``config_name`` heads the refusal of a config outside the family.  No device is touched."""

    def __init__(self, prefix: str, c_config, default, config_name: str):
        self.prefix, self.c_config, self.default, self.config_name = prefix, c_config, default, config_name

    def _c(self, config):
        return self.c_config(config or self.default())

    def num_frames(self, n_samples: int, config=None) -> int:
        n = int(getattr(_lib.load(), self.prefix + "_num_frames")(C.byref(self._c(config)), int(n_samples)))
        if n < 0:
            raise ValueError(f"num_frames: bad arguments ({n_samples} samples)")
        return n

    def min_samples(self, config=None) -> int:
        n = int(getattr(_lib.load(), self.prefix + "_min_samples")(C.byref(self._c(config))))
        if n < 0:
            raise ValueError("min_samples: bad geometry")
        return n

    def state_dict_shapes(self, config=None) -> dict:
        """The inventory of a handle that lives for this call only."""
        lib, h = _lib.load(), C.c_void_p()
        if getattr(lib, self.prefix + "_create")(C.byref(self._c(config)), C.byref(h)) != _lib.DEX_OK:
            raise NotImplementedError(f"{self.config_name}.{getattr(lib, self.prefix + '_last_error')(None).decode()}")
        try:
            return weight_shapes(lib, self.prefix, h)
        finally:
            getattr(lib, self.prefix + "_destroy")(h)

    def check_lengths(self, lengths, n_samples: int, config, what: str, too_short: str, max_frames: int) -> int:
        """``ValueError`` for a row below ``min_samples`` (``too_short`` says what needs them) and for a padded length of more than
        ``max_frames`` encoder frames.  Returns the frames of ``n_samples``."""
        need = self.min_samples(config)
        short = [int(v) for v in lengths if v < need]
        if short:
            raise ValueError(f"{what}: {short[0]} samples are too short: {too_short.format(need=need)}")
        T = self.num_frames(n_samples, config)
        if T > max_frames:
            raise ValueError(f"{what}: {n_samples} samples are {T} encoder frames; one call takes at most {max_frames}")
        return T


_HF_PARAM = {"parametrizations.weight.original0": "weight_g", "parametrizations.weight.original1": "weight_v"}


def route_hf_state_dict(sd, want: dict, strict: bool, ignored):
    """An HF state dict against the inventory ``want`` -> ({key: tensor} of what arrived, missing keys).  The positional
    convolution is taken in either weight-norm spelling; keys for which ``ignored(key)`` holds are dropped.  A wrong shape or
    (``strict``) a missing or unexpected key raises ``RuntimeError``.  Host only."""
    routed = {}
    for k, v in sd.items():
        for old, new in _HF_PARAM.items():
            if k.endswith(old):
                k = k[: -len(old)] + new
        routed[k] = v
    missing = [k for k in want if k not in routed]
    extra = [k for k in routed if k not in want and not ignored(k)]
    if strict and missing:
        raise RuntimeError(f"missing keys {missing[:4]}")
    if strict and extra:
        raise RuntimeError(f"unexpected keys {sorted(extra)[:4]}")
    tensors = {}
    for k, shape in want.items():
        if k in routed:
            v = torch.as_tensor(routed[k])
            if tuple(v.shape) != shape:
                raise RuntimeError(f"{k}: expected shape {shape}, got {tuple(v.shape)}")
            tensors[k] = v
    return tensors, missing


class NetHandle(Handle):
    """One handle of a network (the config, and once loaded the packed weights); its workspace is the network's.  ``config_name``
    heads the refusal of a config outside the family, ``no_workspace`` ends the refusal of a batch one call does not take."""

    def __init__(self, prefix: str, c_struct, device, config_name: str, no_workspace: str):
        self.config_name, self.no_workspace = config_name, no_workspace
        super().__init__(prefix, device, C.byref(c_struct))

    def create_failed(self, rc):
        return NotImplementedError(f"{self.config_name}.{self._fn('last_error')(None).decode()}")

    def shapes(self) -> dict:
        return weight_shapes(self.lib, self.prefix, self.h)

    def workspace(self, B: int, n: int) -> torch.Tensor:
        need = int(self._fn("workspace_bytes")(self.h, B, n))
        if need == 0:
            raise ValueError(f"{B} rows of {n} samples: {self.no_workspace}")
        return super().workspace(need)


class WaveformNet:
    """Base of ``Wav2Vec2CTC``, ``WavLMXVector``, ``UTMOS`` and ``Whisper``: one network in eval mode on one MI355X, fp32.  A subclass
    names its symbols (``_prefix``), its config (``_config_name``, ``_c_config``), what its workspace refuses (``_no_workspace``),
    the checkpoint keys it never reads (``_ignored``) and, where its calls take wavs, the module's ``check_lengths``
    (``_check_lengths``); ``_handle`` is its handle class where its workspace takes other arguments."""
    _prefix = _config_name = _no_workspace = ""
    _handle = NetHandle

    def __init__(self, config, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"{type(self).__name__} runs on an MI355X only (no CPU path)")
        self.config = config
        self.device = torch.device("cuda", device_index(device))
        self._ctx = self._handle(self._prefix, self._c_config(config), self.device, self._config_name, self._no_workspace)
        self._loaded = False

    def state_dict_shapes(self) -> dict:
        """The HF state-dict keys the network needs, with their shapes (weight norm in its ``weight_g`` / ``weight_v`` spelling)."""
        return self._ctx.shapes()

    def load_state_dict(self, sd, strict: bool = True):
        """HF keys.  The positional convolution is taken as ``...conv.weight_g`` / ``weight_v`` or as ``...conv.parametrizations.
        weight.original0`` / ``original1``; the training-side keys the class names are ignored.  A wrong shape or (``strict``) a
        missing or unexpected key raises ``RuntimeError`` before anything is uploaded; with ``strict=False`` the network stays
        unusable until every key has arrived."""
        tensors, missing = route_hf_state_dict(sd, self.state_dict_shapes(), strict, self._ignored)
        self._loaded = False
        upload_weights(self._ctx, self._ctx._fn("load"), tensors, self.device)
        if not missing:
            self.finalize()
            torch.cuda.current_stream(self.device).synchronize()        # the operands are packed when this returns
        return self

    def finalize(self):
        """Pack the operands (``<prefix>_finalize``); ``ValueError`` naming the first key that was never loaded."""
        ctx = self._ctx
        with torch.cuda.device(self.device):
            ctx.check(ctx._fn("finalize")(ctx.h, stream(self.device)), f"{self._prefix}_finalize")
        self._loaded = True
        return self

    def _need_weights(self, what: str):
        if not self._loaded:
            raise ValueError(f"{what}: the network's weights are not loaded (load_state_dict)")

    def _rows(self, wav, lengths, what: str):
        """The inputs of a network call: (fp32 rows [B, n] on the device, host lengths, one-row flag)."""
        self._need_weights(what)
        x, ln, one = device_rows(wav, lengths, what, refuse=ValueError)
        return x.to(self.device), ln, one

    def _inputs(self, wav, lengths, what: str):
        """``_rows`` and the frames of the padded batch, once the module's ``check_lengths`` has passed the lengths."""
        x, ln, one = self._rows(wav, lengths, what)
        return x, ln, one, self._check_lengths(ln, x.shape[1], self.config, what)

    def _hidden(self, wav, lengths) -> torch.Tensor:
        """The body of a subclass's ``hidden_states``: [B, n] (or [n]) -> ``<prefix>_hidden``'s [B, T, hidden] (or [T, hidden])."""
        x, ln, one, T = self._inputs(wav, lengths, f"{type(self).__name__}.hidden_states")
        out = torch.empty(x.shape[0], T, self.config.hidden_size, dtype=torch.float32, device=self.device)
        return self._run("hidden", x, ln, out, int(self.do_normalize), out.data_ptr(), one=one)

    @classmethod
    def _model(cls, model, what: str):
        if not isinstance(model, cls):
            raise ValueError(f"{what}: pass model={cls.__name__}(...) with the checkpoint's weights loaded (the library ships none)")
        return model

    def _utterances(self, wavs, lengths, sr, what: str):
        """``wavs`` [B, n] with ``lengths``, or a list of wavs, at ``sr`` Hz -> (wavs, lengths) at 16 kHz."""
        if isinstance(wavs, torch.Tensor) and wavs.dim() != 2:
            raise ValueError(f"{what}: expected wavs [B, n] or a list, got {tuple(wavs.shape)}")
        return self._at_16k(wavs, lengths, sr, what)

    def _run(self, name: str, x, ln, out, *args, one: bool = False):
        """The body of a network call ``<prefix>_<name>(h, x, lengths, B, n, *args, workspace, bytes, stream)`` -> ``out``."""
        B, n = x.shape
        ctx = self._ctx
        ws = ctx.workspace(B, n)
        with torch.cuda.device(self.device):
            rc = ctx._fn(name)(ctx.h, x.data_ptr(), i32_ptr(ln), B, n, *args, ws.data_ptr(), ws.numel(), stream(self.device))
        ctx.check(rc, f"{self._prefix}_{name}")
        return out[0] if one else out

    def _at_16k(self, wavs, lengths, sr, what: str):
        """``wavs`` [B, n] (or [n]) with ``lengths``, or a list of wavs (float, or int16 scaled by 1 / 32768), at ``sr`` Hz -> (wavs,
        lengths) at 16 kHz, resampled by ``wavprep.resample`` where ``sr`` differs."""
        if int(sr) <= 0:
            raise ValueError(f"{what}: sr must be positive, got {sr}")
        if not isinstance(wavs, torch.Tensor):
            wavs, lengths = pad_wavs(wavs, self.device, scale_int16=True)
        if int(sr) != SAMPLING_RATE:
            x, ln, _ = device_rows(wavs, lengths, what, refuse=ValueError)
            wavs, lengths = resample_to_16k(x, ln, sr)
        return wavs, lengths
