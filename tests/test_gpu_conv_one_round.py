"""The one-round forms of the U-Net's 3x3 patch convolution (conv3x3_lp_kernel with 5-row tiles: ten waves of one row x 32 channels at
64 -> 64, 32-channel output slices of five row-waves at 64 -> 128) run every output element's chain of the 2- / 4-row forms - the same
channel chunks, then taps, then 16-wide K steps on the same MFMA - and the GroupNorm partials are fixed-point sums, so the sampler's
output must be the same BITS under DEX_CONV_ROUND1=1 and =0.  The launcher takes them where their grid fits one round of the CUs and
the current form's does not, filling at least three quarters of them: the 64 -> 64 and 64 -> 128 launches of B = 1 at T <= 512 (GeDEX and
DEX; in the split-weight mode not the 64 -> 64 fused tail); T = 800 and B = 2 keep the current forms."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gpu_util as U

pytestmark = pytest.mark.gpu

ONE_ROUND = re.compile(r"conv3x3_lp_kernel<\d+,\d+,\d+,5,")


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
    return y, sum(1 for r in rows if ONE_ROUND.search(r))


@pytest.mark.parametrize("name,kw,taken", [
    ("gedex_lj", dict(B=1, T=512), True),                              # the headline's shapes
    ("gedex_lj", dict(B=1, T=500, lengths=[467]), True),               # a partial strip and a ragged mask
    ("dex_vctk", dict(B=1, T=512, Tr=100, Ts=100), True),              # dex_b1
    ("gedex_lj", dict(B=1, T=800), False),                             # gedex_b1_t800: 400 / 416 workgroups, the current forms
    ("gedex_lj", dict(B=2, T=512, lengths=[512, 301]), False),         # gedex_b2
])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp16x2"])
def test_one_round_forms_are_bitwise_the_current_forms(name, kw, taken, prec):
    cfg, eng, w = U.engine_for(name)
    case = U.make_case(cfg, **kw)
    eng.set_precision(prec)
    eng.profile(True)
    try:
        y0, n0 = _run(eng, case, 2, {"DEX_CONV_ROUND1": "0"})
        y1, n1 = _run(eng, case, 2, {"DEX_CONV_ROUND1": "1"})
        yd, nd = _run(eng, case, 2, {})
    finally:
        eng.profile(False)
        eng.set_precision("fp32")
    assert n0 == 0
    assert (n1 > 0) == taken and nd == n1     # the default takes the one-round forms exactly where the rule says
    assert np.isfinite(y1).all()
    assert np.array_equal(y0, y1), float(np.abs(y0 - y1).max())
    assert np.array_equal(yd, y1)


@pytest.mark.parametrize("use_graph", [False, True])
def test_headline_sampler_is_bitwise_under_both_forms(use_graph):
    """A whole 50-step gedex_b1 call in the headline's mode, eager and as a captured graph."""
    cfg, eng, w = U.engine_for("gedex_lj")
    case = U.make_case(cfg, B=1, T=512)
    eng.set_precision("bf16")
    try:
        y0, _ = _run(eng, case, 50, {"DEX_CONV_ROUND1": "0"}, use_graph)
        y1, _ = _run(eng, case, 50, {"DEX_CONV_ROUND1": "1"}, use_graph)
    finally:
        eng.set_precision("fp32")
    assert np.isfinite(y1).all()
    assert np.array_equal(y0, y1), float(np.abs(y0 - y1).max())
