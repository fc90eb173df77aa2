"""The row deals of the small-grid linear-attention kernels.  With DEX_KVCTX_ROWS=1 the head-parallel context pass
(linattn_kvctx_hw_kernel) deals the 8-channel items of its prologue - h2, the residual, the mask value, the Xout store, the write into the
LDS x image - to the slot's 256 lanes in memory order instead of lane = pixel; with DEX_OUT2_ROWS=1 the wave-split tail
(linattn_out2_hw_kernel) loads x and stores y as whole pixel rows, eight per wave.  Both only change which lane moves which element: every
element sees the same operations in the same order, so the sampler's output must be the same BITS with each knob at 1 and at 0, each part
alone and both together.

Shapes (GeDEX-LJ, 80 mel bins: 80 x T at C = 64, 40 x T/2 at C = 128 and C = 64):
  B = 1, T = 64                    full sub-tiles; every launch takes the hw forms, the 80-row C = 64 tail included (40 workgroups)
  B = 1, T = 100                   npix % 128 != 0 at full resolution, npix % 32 != 0 at half resolution (40 x 50): a slot past the end
                                   and a ragged last sub-tile whose items straddle npix
  B = 2, T = 96, lengths [96, 37]  masked pixels inside a sub-tile: the mask value is the item's own pixel's
  B = 3, T = 68, lengths [68, 50, 9]
each with DEX_LINATTN_NSUB unset, 1, 2 and 4, in bf16, fp16 and fp16x2 (the split-weight build has the head-parallel form at C = 64 only);
one pass with DEX_H_BF16=0 (the run-time-flag instantiations, fp32 h2), and T = 512 for the workload's own shapes.

Strides: the tail of the middle stage (40 x T/2, C = 128) writes the skip half of the up path's concatenation buffer, ldy = 256 and
y_coff = 128 - in every case here.  x, Xout and the residual of these jobs are dense (ldx = ldres = C, x_coff = 0): no job of the sampler
reaches the fused linear attention with another stride."""
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U

pytestmark = pytest.mark.gpu

CASES = [
    dict(B=1, T=64),
    dict(B=1, T=100),
    dict(B=2, T=96, lengths=[96, 37]),
    dict(B=3, T=68, lengths=[68, 50, 9]),
]
KNOBS = [("0", "0"), ("1", "0"), ("0", "1"), ("1", "1")]          # (DEX_KVCTX_ROWS, DEX_OUT2_ROWS); the first is the reference


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
    return y, any("linattn_kvctx_hw_kernel" in r for r in rows), any("linattn_out2_hw_kernel" in r for r in rows)


def _check(kw, prec, extra):
    cfg, eng, w = U.engine_for("gedex_lj")
    case = U.make_case(cfg, **kw)
    eng.set_precision(prec)
    eng.profile(True)
    try:
        out = [_run(eng, case, 2, {"DEX_KVCTX_ROWS": kv, "DEX_OUT2_ROWS": o2, **extra}) for kv, o2 in KNOBS]
    finally:
        eng.profile(False)
        eng.set_precision("fp32")
    y0 = out[0][0]
    assert np.isfinite(y0).all()
    for (kv, o2), (y, kv_hw, o2_hw) in zip(KNOBS, out):
        assert kv_hw and o2_hw, (kv, o2, kv_hw, o2_hw)              # the small-grid forms did run
        assert np.array_equal(y0, y), (kv, o2, float(np.abs(y0 - y).max()))


@pytest.mark.parametrize("kw", CASES)
@pytest.mark.parametrize("nsub", [None, "1", "2", "4"])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16x2"])
def test_row_deals_are_bitwise_the_lane_per_pixel_deals(kw, nsub, prec):
    _check(kw, prec, {} if nsub is None else {"DEX_LINATTN_NSUB": nsub})


@pytest.mark.parametrize("kw", CASES)
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16x2"])
def test_row_deals_are_bitwise_with_runtime_flags(kw, prec):
    _check(kw, prec, {"DEX_H_BF16": "0"})


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16x2"])
def test_row_deals_are_bitwise_at_the_workload_shapes(prec):
    _check(dict(B=1, T=512), prec, {})
