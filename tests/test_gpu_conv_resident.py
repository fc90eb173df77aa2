"""The resident-weights schedule of the U-Net's 3x3 patch convolution (conv3x3_lp_kernel<..., resident>): all nine taps of a workgroup's
weight slice sit in LDS behind ONE barrier, and every output element still runs the chain of the streamed forms - taps 0..8, then the four
16-wide K steps, on the same MFMA, the 1x1 shortcut on the centre tap - so the sampler's output must be the same BITS under
DEX_CONV_RESIDENT=1 and =0.  The launcher takes it for Cin = 64 in one chunk where the grid is at most one round of the CUs: the 5-row
one-round forms (64 -> 64 at 80 x 512, 64 -> 128 with the shortcut at 40 x 256) and the 2-row 64 -> 64 form at 40 x 256, i.e. B = 1 at
T <= 512 in the bf16 and fp16 modes; never in the split-weight mode (18 taps), and not at T = 800 or B = 2 (more than one round).  The
ten-wave fused-tail form (PRO2 at 80 x 512) keeps its streamed schedule: resident it was no faster inside the sampler's step."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gpu_util as U

pytestmark = pytest.mark.gpu

RESIDENT = re.compile(r"conv3x3_lp_kernel<[\d,]+,resident>")
ONE_ROUND_64 = re.compile(r"conv3x3_lp_kernel<64,(64,64|128,32),5,0,")    # the one-round forms with Cin = 64, fused tail excepted
SMALL_64 = re.compile(r"conv3x3_lp_kernel<64,64,64,2,")                   # the 2-row 64 -> 64 form


def _run(eng, case, n, env, use_graph=False):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        mu, mask, z = (torch.from_numpy(case[k]).cuda() for k in ("mu", "mask", "z"))
        y = eng.sample(z, mask, mu, n, use_graph=use_graph, **U.engine_kwargs(case)).cpu().numpy()
        rows = [] if use_graph else [r["name"] for r in eng.profile_rows()]
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return y, rows


def _resident(rows):
    return [r for r in rows if RESIDENT.search(r)]


@pytest.mark.parametrize("name,kw,taken", [
    ("gedex_lj", dict(B=1, T=512), True),                              # the headline's shapes
    ("gedex_lj", dict(B=1, T=500, lengths=[467]), True),               # a partial strip and a ragged mask: clamped loads, unfull epilogue
    ("dex_vctk", dict(B=1, T=512, Tr=100, Ts=100), True),              # dex_b1
    ("gedex_lj", dict(B=2, T=512, lengths=[512, 301]), False),         # gedex_b2: 512 / 320 workgroups
    ("gedex_lj", dict(B=1, T=800), False),                             # 400 / 260 / 416 workgroups: more than one round of 256 CUs
])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16x2"])
def test_resident_forms_are_bitwise_the_streamed_forms(name, kw, taken, prec):
    cfg, eng, w = U.engine_for(name)
    case = U.make_case(cfg, **kw)
    eng.set_precision(prec)
    eng.profile(True)
    try:
        y0, r0 = _run(eng, case, 2, {"DEX_CONV_RESIDENT": "0"})
        y1, r1 = _run(eng, case, 2, {"DEX_CONV_RESIDENT": "1"})
        yd, rd = _run(eng, case, 2, {})
    finally:
        eng.profile(False)
        eng.set_precision("fp32")
    assert _resident(r0) == []
    assert rd == r1                                    # the default is the knob's on position, launch for launch
    assert len(r0) == len(r1)                          # a form changes, never the number of launches
    if prec == "fp16x2" or not taken:
        assert _resident(r1) == []
    else:
        # exactly where the rule says: every one-round launch with Cin = 64 but the fused tail, and every 2-row 64 -> 64 launch, and nothing else
        eligible = [r for r in r1 if ONE_ROUND_64.search(r) or SMALL_64.search(r)]
        assert eligible and eligible == _resident(r1)
        assert {re.sub(r",resident>", ">", r) for r in eligible} == {r for r in r0 if ONE_ROUND_64.search(r) or SMALL_64.search(r)}
    assert np.isfinite(y1).all()
    assert np.array_equal(y0, y1), float(np.abs(y0 - y1).max())
    assert np.array_equal(yd, y1)


@pytest.mark.parametrize("use_graph", [False, True])
def test_headline_sampler_is_bitwise_under_both_schedules(use_graph):
    """A whole 50-step gedex_b1 call in the headline's mode, eager and as a captured graph."""
    cfg, eng, w = U.engine_for("gedex_lj")
    case = U.make_case(cfg, B=1, T=512)
    eng.set_precision("bf16")
    try:
        y0, _ = _run(eng, case, 50, {"DEX_CONV_RESIDENT": "0"}, use_graph)
        y1, _ = _run(eng, case, 50, {"DEX_CONV_RESIDENT": "1"}, use_graph)
    finally:
        eng.set_precision("fp32")
    assert np.isfinite(y1).all()
    assert np.array_equal(y0, y1), float(np.abs(y0 - y1).max())
