"""CPU: the weight plumbing every native context shares (csrc/weight_store.h) keeps the C ABI it had: for the score network, the text
encoder, the style encoders and the vocoder, the library's inventory (*_num_weights / *_weight_info) is the set of tensors the Python
module uploads, and the argument and state errors of *_load_weight*, *_finalize and *_last_error return the same codes and text.
Every case fails before any device allocation, so no GPU is needed."""
import ctypes as C
import json
import os

import pytest

from dex_tts_amd import _lib, config as Cfg, style as S, text as T, vocoder as V

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEX_ERR_ARG, DEX_ERR_STATE = -1, -2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dex_tts_amd import build
        build.build(verbose=False)
    return _lib.load()


def text_module():
    kw = dict(json.load(open(os.path.join(GOLD, "manifest_text_gedex_lj.json")))["config"])
    return T.TextEncoder(**kw, variant="gedex")


def _uploaded_text():
    return {k: tuple(v.shape) for k, v in text_module().state_dict().items()}


def _uploaded_style():
    m = S.StyleEncoders()
    return {k: tuple(v.shape) for k, v in S.fold_batchnorm(m.state_dict()).items()}


def _uploaded_vocoder(h):
    return {k: tuple(s) for k, s in V.param_shapes(h).items() if not (k.endswith(".filter") and not k.startswith("activation_post."))}


# (symbol prefix, last-error symbol, null-context text, message noun, config factory, uploaded key -> shape, keys the module has and the
# library does not take)
CONTEXTS = {
    "score_gedex_lj": ("dex_ctx", "dex_last_error", "null context", "",
                       lambda: _lib.make_config(Cfg.gedex_lj()), lambda: {k: tuple(v) for k, v in Cfg.param_shapes(Cfg.gedex_lj()).items()}, ()),
    # the RetNet decay buffer: use_decay is off in every config the library builds
    "text_gedex_lj": ("dex_text", "dex_text_last_error", "null text context", "text-encoder ",
                      lambda: text_module()._config(), _uploaded_text, ("encoder.retnet_rel_pos.decay",)),
    # the VQ's EMA statistics (training only) and TIVEncoder.out_conv, whose output nothing downstream reads (tts.py:67)
    "style_vctk": ("dex_style", "dex_style_last_error", "null style context", "style ",
                   lambda: S.StyleEncoders()._config(), _uploaded_style,
                   ("tv_encoder.vq.ema_count", "tv_encoder.vq.ema_weight", "tiv_encoder.out_conv.conv.weight", "tiv_encoder.out_conv.conv.bias")),
    "hifigan_v1": ("dex_voc", "dex_voc_last_error", "null vocoder context", "vocoder ",
                   lambda: V.make_config(V.HIFIGAN_V1), lambda: _uploaded_vocoder(V.HIFIGAN_V1), ()),
    "bigvgan_base": ("dex_voc", "dex_voc_last_error", "null vocoder context", "vocoder ",
                     lambda: V.make_config(V.BIGVGAN_BASE), lambda: _uploaded_vocoder(V.BIGVGAN_BASE), ()),
}


class Ctx:
    def __init__(self, lib, name):
        self.lib = lib
        self.prefix, last_error, self.null_text, self.noun, config, self.uploaded, self.unused = CONTEXTS[name]
        self.cfg = config()
        self.h = C.c_void_p()
        self.fn = lambda s: getattr(lib, f"{self.prefix}_{s}")
        self.last_error = getattr(lib, last_error)
        assert self.fn("create")(C.byref(self.cfg), C.byref(self.h)) == 0, self.error()

    def error(self):
        return self.last_error(self.h).decode()

    def inventory(self):
        out = {}
        for i in range(self.fn("num_weights")(self.h)):
            key = C.c_char_p(); shp = (C.c_int64 * 4)(); nd = C.c_int()
            assert self.fn("weight_info")(self.h, i, C.byref(key), shp, C.byref(nd)) == 0
            out[key.value.decode()] = tuple(shp[k] for k in range(nd.value))
        return out

    def load(self, key, shape):
        shp = (C.c_int64 * 4)(*(list(shape) + [0] * (4 - len(shape))))
        fake = C.c_void_p(256)             # never dereferenced: every case below is refused before the copy
        return self.fn("load_weight_async")(self.h, key.encode(), fake, shp, len(shape), None)

    def close(self):
        self.fn("destroy")(self.h)


@pytest.fixture(params=list(CONTEXTS))
def ctx(lib, request):
    x = Ctx(lib, request.param)
    yield x
    x.close()


def test_inventory_is_what_the_module_uploads(ctx):
    got, want = ctx.inventory(), ctx.uploaded()
    assert all(k in want for k in ctx.unused)
    assert got == {k: s for k, s in want.items() if k not in ctx.unused}


def test_weight_info_out_of_range(ctx):
    n = ctx.fn("num_weights")(ctx.h)
    key = C.c_char_p(); shp = (C.c_int64 * 4)(); nd = C.c_int()
    assert ctx.fn("weight_info")(ctx.h, n, C.byref(key), shp, C.byref(nd)) == DEX_ERR_ARG
    assert ctx.fn("weight_info")(ctx.h, -1, C.byref(key), shp, C.byref(nd)) == DEX_ERR_ARG
    assert ctx.fn("weight_info")(None, 0, C.byref(key), shp, C.byref(nd)) == DEX_ERR_ARG
    assert ctx.fn("num_weights")(None) == 0


def test_load_refuses_unknown_key(ctx):
    assert ctx.load("no.such.weight", (4,)) == DEX_ERR_ARG
    assert ctx.error() == f"unknown {ctx.noun}weight key 'no.such.weight'"


def test_load_refuses_wrong_ndim(ctx):
    key, shape = next(iter(ctx.inventory().items()))
    assert ctx.load(key, shape + (1,)) == DEX_ERR_ARG
    assert ctx.error() == f"weight '{key}': expected {len(shape)} dims, got {len(shape) + 1}"


def test_load_refuses_wrong_dim(ctx):
    key, shape = next((k, s) for k, s in ctx.inventory().items() if len(s) >= 2)
    bad = shape[:1] + (shape[1] + 1,) + shape[2:]
    assert ctx.load(key, bad) == DEX_ERR_ARG
    assert ctx.error() == f"weight '{key}': dim 1 is {shape[1] + 1}, expected {shape[1]}"


def test_load_refuses_null_arguments(ctx):
    key, shape = next(iter(ctx.inventory().items()))
    shp = (C.c_int64 * 4)(*(list(shape) + [0] * (4 - len(shape))))
    load = ctx.fn("load_weight_async")
    assert load(ctx.h, None, C.c_void_p(256), shp, len(shape), None) == DEX_ERR_ARG
    assert load(ctx.h, key.encode(), None, shp, len(shape), None) == DEX_ERR_ARG
    assert load(None, key.encode(), C.c_void_p(256), shp, len(shape), None) == DEX_ERR_ARG


def test_finalize_before_load(ctx):
    first = next(iter(ctx.inventory()))
    assert ctx.fn("finalize")(ctx.h, None) == DEX_ERR_STATE
    assert ctx.error() == f"{ctx.noun}weight '{first}' was never loaded"
    assert ctx.fn("finalize")(None, None) == DEX_ERR_ARG


def test_last_error_of_null_context(ctx):
    assert ctx.last_error(None).decode() == ctx.null_text


def test_blocking_load_of_score_network(lib):
    """dex_ctx_load_weight (the blocking form) refuses what the asynchronous one refuses, with the same text."""
    x = Ctx(lib, "score_gedex_lj")
    try:
        key, shape = next(iter(x.inventory().items()))
        for k, s, msg in (("no.such.weight", shape, "unknown weight key 'no.such.weight'"),
                          (key, shape + (1,), f"weight '{key}': expected {len(shape)} dims, got {len(shape) + 1}")):
            shp = (C.c_int64 * 4)(*(list(s) + [0] * (4 - len(s))))
            assert lib.dex_ctx_load_weight(x.h, k.encode(), C.c_void_p(256), shp, len(s)) == DEX_ERR_ARG
            assert x.error() == msg
        assert lib.dex_ctx_load_weight(None, key.encode(), C.c_void_p(256), shp, len(shape)) == DEX_ERR_ARG
    finally:
        x.close()
