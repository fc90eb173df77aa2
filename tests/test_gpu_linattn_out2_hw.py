"""The wave-split form of the linear-attention tail (linattn_out2_hw_kernel: one 32-pixel slot over four waves, he tiles of q^T then co
tiles of y^T split by wave, the x and q fragments shared through LDS) runs every MFMA chain of the direct form in the same K order on
the same operands and adds the residual and bias in the same order, so the sampler's output must be the same BITS under
DEX_LINATTN_OUT2_HW=1 and =0 - at the B = 1 shapes, small batches, ragged widths (npix % 128 != 0, npix % 32 != 0 at half resolution),
in each reduced-precision mode (fp16x2: the split-weight hi + lo chain) and with the run-time-flag context pass (DEX_H_BF16=0).  The
80x512 launch of B = 1 keeps the throughput form under both settings (its x and y are 16-bit there), so the forms meet at 40x256."""
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
    return y, any("linattn_out2_hw_kernel" in r for r in rows)


@pytest.mark.parametrize("kw", [
    dict(B=1, T=512),                                 # the headline: 40x256 at C = 128 and C = 64
    dict(B=2, T=512, lengths=[512, 301]),
    dict(B=3, T=500, lengths=[500, 333, 77]),         # npix % 128 != 0
    dict(B=1, T=804, lengths=[803]),                  # npix % 128 != 0, and npix % 32 != 0 at half resolution
])
@pytest.mark.parametrize("hbf", [None, "0"])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16x2"])
def test_wave_split_tail_is_bitwise_the_direct_form(kw, hbf, prec):
    cfg, eng, w = U.engine_for("gedex_lj")
    case = U.make_case(cfg, **kw)
    eng.set_precision(prec)
    eng.profile(True)
    extra = {} if hbf is None else {"DEX_H_BF16": hbf}
    try:
        y0, hw0 = _run(eng, case, 2, {"DEX_LINATTN_OUT2_HW": "0", **extra})
        y1, hw1 = _run(eng, case, 2, {"DEX_LINATTN_OUT2_HW": "1", **extra})
        yd, hwd = _run(eng, case, 2, dict(extra))
    finally:
        eng.profile(False)
        eng.set_precision("fp32")
    assert not hw0 and hw1 and hwd        # the forms did run, and the default takes the wave-split one at these shapes
    assert np.isfinite(y1).all()
    assert np.array_equal(y0, y1), float(np.abs(y0 - y1).max())
    assert np.array_equal(yd, y1)
