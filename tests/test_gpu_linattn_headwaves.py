"""The head-parallel form of the linear-attention context pass (linattn_kvctx_hw_kernel: 16 waves, one head each, the prologue shared
through LDS) computes every (sub-tile, head) state with the same instructions as the 4-wave form and merges in the same wave order, so
the sampler's output must be the same BITS under DEX_LINATTN_HEADWAVES=1 and =0 - at the B = 1 shapes, small batches, ragged widths
(npix % 128 != 0, npix % 32 != 0) and every sub-tile count, in each reduced-precision mode (the exact-fp32 mode never reaches the fused
linear attention).  DEX_H_BF16=0 takes the run-time-flag instantiations (FL = -1) of both forms.  The forms without the ResnetBlock
prologue (PRO = false) are not covered: every call of the fused modes passes the prologue, so nothing reaches them."""
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U

pytestmark = pytest.mark.gpu


def _run(eng, case, n, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        mu, mask, z = (torch.from_numpy(case[k]).cuda() for k in ("mu", "mask", "z"))
        y = eng.sample(z, mask, mu, n, **U.engine_kwargs(case)).cpu().numpy()
        rows = [r["name"] for r in eng.profile_rows()]
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return y, any("linattn_kvctx_hw_kernel" in r for r in rows), any(r == "linattn_kvctx_kernel" for r in rows)


@pytest.mark.parametrize("kw", [
    dict(B=1, T=512),                                 # the headline: 80x512 (C = 64) and 40x256 (C = 128, C = 64)
    dict(B=2, T=512, lengths=[512, 301]),
    dict(B=3, T=500, lengths=[500, 333, 77]),         # npix % 128 != 0
    dict(B=1, T=804, lengths=[803]),                  # npix % 128 != 0, and npix % 32 != 0 at half resolution
])
@pytest.mark.parametrize("nsub", [None, "1", "2", "4"])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16x2"])
def test_headwaves_form_is_bitwise_the_four_wave_form(kw, nsub, prec):
    cfg, eng, w = U.engine_for("gedex_lj")
    case = U.make_case(cfg, **kw)
    eng.set_precision(prec)
    eng.profile(True)
    extra = {} if nsub is None else {"DEX_LINATTN_NSUB": nsub}
    try:
        y0, hw0, old0 = _run(eng, case, 2, {"DEX_LINATTN_HEADWAVES": "0", **extra})
        y1, hw1, old1 = _run(eng, case, 2, {"DEX_LINATTN_HEADWAVES": "1", **extra})
    finally:
        eng.profile(False)
        eng.set_precision("fp32")
    assert (hw0, old0) == (False, True)
    # the forms did run (their results agree to the bit); the split-weight build keeps the 4-wave form at C = 128 (LDS)
    assert hw1 and old1 == (prec == "fp16x2"), (hw1, old1)
    assert np.isfinite(y1).all()
    assert np.array_equal(y0, y1), float(np.abs(y0 - y1).max())


@pytest.mark.parametrize("kw", [dict(B=1, T=512), dict(B=3, T=500, lengths=[500, 333, 77])])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16x2"])
def test_headwaves_form_is_bitwise_the_four_wave_form_with_runtime_flags(kw, prec):
    cfg, eng, w = U.engine_for("gedex_lj")
    case = U.make_case(cfg, **kw)
    eng.set_precision(prec)
    eng.profile(True)
    try:
        y0, hw0, old0 = _run(eng, case, 2, {"DEX_LINATTN_HEADWAVES": "0", "DEX_H_BF16": "0"})
        y1, hw1, old1 = _run(eng, case, 2, {"DEX_LINATTN_HEADWAVES": "1", "DEX_H_BF16": "0"})
    finally:
        eng.profile(False)
        eng.set_precision("fp32")
    assert (hw0, old0) == (False, True)
    assert hw1 and old1 == (prec == "fp16x2"), (hw1, old1)
    assert np.isfinite(y1).all()
    assert np.array_equal(y0, y1), float(np.abs(y0 - y1).max())
