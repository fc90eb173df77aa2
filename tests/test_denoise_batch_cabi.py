"""CPU: the batched EDMPrecond call with a noise level per utterance exists at every layer - declared in include/dex_amd.h, exported by
the built library, bound in _lib.py with the header's struct layout - and the loss entry points take ``batched``."""
import ctypes as C
import inspect
import os
import re

import pytest

from dex_tts_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dex_tts_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "dex_amd.h")).read()
    assert re.search(r"int\s+dex_denoise_batch\(DexCtx\* ctx, const DexDenoiseBatchArgs\* args, dex_stream_t stream\);", hdr)
    assert hasattr(lib, "dex_denoise_batch")
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    assert bound["dex_denoise_batch"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.DexDenoiseBatchArgs), C.c_void_p])


def test_struct_layout_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "dex_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} DexDenoiseBatchArgs;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["DexSampleArgs s", "const float* x_dev", "const float* sigma_dev"]
    S = _lib.DexDenoiseBatchArgs
    assert [(n, t) for n, t in S._fields_] == [("s", _lib.DexSampleArgs), ("x_dev", C.c_void_p), ("sigma_dev", C.c_void_p)]
    # the first two members sit where DexDenoiseArgs has them; sigma_dev follows x_dev
    assert S.s.offset == _lib.DexDenoiseArgs.s.offset == 0 and S.x_dev.offset == _lib.DexDenoiseArgs.x_dev.offset
    assert S.sigma_dev.offset == S.x_dev.offset + C.sizeof(C.c_void_p) and C.sizeof(S) == S.sigma_dev.offset + C.sizeof(C.c_void_p)


def test_null_arguments_are_refused_without_a_gpu(lib):
    assert lib.dex_denoise_batch(None, None, None) == -1


def test_loss_entry_points_take_batched_and_default_to_the_loop():
    from dex_tts_amd import diffusion, edm, engine, tts
    for fn in (edm.EDMLoss.forward, diffusion.Diffusion.forward, tts.GeDEXTTS.loss_value, tts.DeXTTS.loss_value):
        par = inspect.signature(fn).parameters
        assert "batched" in par and par["batched"].default is False, fn
    assert list(inspect.signature(engine.ScoreNetEngine.denoise_batch).parameters)[:5] == ["self", "x", "sigma", "mask", "mu"]
    par = list(inspect.signature(diffusion._Precond.forward).parameters)
    assert par[:5] == ["self", "x", "sigma", "mask", "mu"] and par[-2:] == ["spk", "mask_ratio"]
