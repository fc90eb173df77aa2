"""The small-grid forms of the two launches at the ends of the DiT bottleneck.

patch_embed_fused_kernel<KS, C, TOK>: 4 (or 2) tokens per workgroup instead of 8, the mask fetched once per tap column, the depthwise
weights staged once per workgroup - the same fmaf chain per output, one rounding, the same MFMAs.  igemm_lp_nwalk_kernel_small: 32-row
workgroups of four 64-column tiles with the weight fragments straight from the fragment-ordered twin - the walker's LayerNorm staging,
K order and scatter.  Neither changes an operation or its order, so the sampler's output must be the same BITS under every setting of
DEX_PE_TOK and DEX_NWALK_SMALL, against the two-kernel patch embedding (DEX_PATCH_FUSED=0) and against the single-shot GEMM
(DEX_GEMM_NWALK=0), with the fp32 and - at batch size, the small form forced - the 16-bit concatenation buffer.  The launchers take
the new forms where the current grid misses one round of the CUs and the new one fits it (the B = 1 shapes), not at batch size."""
import os
import re

import numpy as np
import pytest
import torch

from dex_tts_amd import _lib
from tests import gpu_util as U

pytestmark = pytest.mark.gpu

SHAPES = [
    # 260 tokens per utterance (not a multiple of 4 or 8: a workgroup straddles the utterances), masked columns inside patches, right
    # zero padding and a crop in the scatter, 9 row tiles of 32 with a partial last one
    ("gedex_lj", dict(B=2, T=100, lengths=[100, 61])),
    # 3 x 3 / stride-2 patches, the TIV affine folded into the load, no input mask
    ("dex_vctk", dict(B=1, T=64, lengths=[57], Tr=40, Ts=40, sty_lengths=[33])),
]
HEADLINE = ("gedex_lj", dict(B=1, T=512))             # 650 tokens (650 % 4 = 2), 21 row tiles: the shape the launchers' rules switch


def _run(eng, case, n, env, use_graph=False, rows=False):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        mu, mask, z = (torch.from_numpy(case[k]).cuda() for k in ("mu", "mask", "z"))
        y = eng.sample(z, mask, mu, n, use_graph=use_graph, **U.engine_kwargs(case)).cpu().numpy()
        names = [r["name"] for r in eng.profile_rows()] if rows else []
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return (y, names) if rows else y


def _same(a, b):
    assert np.isfinite(a).all()
    assert np.array_equal(a, b), float(np.abs(a - b).max())


@pytest.mark.parametrize("name,kw", SHAPES)
@pytest.mark.parametrize("prec", [p for p in ("bf16", "fp16", "fp16x2") if p in _lib.PRECISION])
def test_patch_embed_tiles_are_bitwise_the_eight_token_form(name, kw, prec):
    cfg, eng, w = U.engine_for(name)
    case = U.make_case(cfg, **kw)
    eng.set_precision(prec)
    eng.profile(True)
    pe = lambda rows: sorted({r for r in rows if "patch_embed_fused_kernel" in r})
    try:
        ref, rows = _run(eng, case, 3, {"DEX_PE_TOK": "8"}, rows=True)
        assert pe(rows) == ["patch_embed_fused_kernel"], pe(rows)            # the fused launch ran, in the 8-token form
        for tok in ("4", "2"):
            y, rows = _run(eng, case, 3, {"DEX_PE_TOK": tok}, rows=True)
            assert pe(rows) == [f"patch_embed_fused_kernel<{tok}>"], pe(rows)
            _same(ref, y)
        y, rows = _run(eng, case, 3, {"DEX_PATCH_FUSED": "0"}, rows=True)
        assert pe(rows) == [], pe(rows)
        _same(ref, y)
    finally:
        eng.profile(False)
        eng.set_precision("fp32")


# the up path's first conv reading the 16-bit concatenation buffer: conv3x3_lp_kernel<CC, 64, NSL, TH, PRO2, RES = 1, XB = 1, ...>
CAT16_CONV = re.compile(r"conv3x3_lp_kernel<\d+,64,\d+,\d+,\d,1,1,")


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_unpatchify_small_form_writes_the_16_bit_concatenation_buffer_bitwise(prec):
    """The 16-bit twin of the concatenation buffer exists at batch size only (>= 256 tail workgroups), where the launcher's rule keeps the
    walker: gedex_lj B = 4, T = 512 (ragged, 21 row tiles of 32 per utterance with a partial last one, a cropped last token column) with the
    small form forced runs its 16-bit scatter; DEX_CAT_LP=0 at the same shape its fp32 scatter."""
    cfg, eng, w = U.engine_for("gedex_lj")
    case = U.make_case(cfg, B=4, T=512, lengths=[512, 301, 77, 500])
    small = lambda rows: any("igemm_lp_nwalk_kernel_small" in r for r in rows)
    cat16 = lambda rows: any(CAT16_CONV.search(r) for r in rows)
    eng.set_precision(prec)
    eng.profile(True)
    try:
        y1, r1 = _run(eng, case, 2, {"DEX_NWALK_SMALL": "1"}, rows=True)
        y0, r0 = _run(eng, case, 2, {"DEX_NWALK_SMALL": "0"}, rows=True)
        yd, rd = _run(eng, case, 2, {}, rows=True)
        y32, r32 = _run(eng, case, 2, {"DEX_NWALK_SMALL": "1", "DEX_CAT_LP": "0"}, rows=True)
        ys, rs = _run(eng, case, 2, {"DEX_GEMM_NWALK": "0"}, rows=True)
    finally:
        eng.profile(False)
        eng.set_precision("fp32")
    assert cat16(r1) and cat16(r0) and cat16(rd), sorted({r for r in r1 if "conv3x3_lp_kernel" in r})   # the 16-bit buffer is on ...
    assert not cat16(r32) and not cat16(rs)                                                           # ... and off where it is switched off
    assert small(r1) and small(r32) and not small(r0) and not small(rd) and not small(rs)              # (the rule keeps the walker at B = 4)
    _same(y1, y0)
    _same(y1, yd)
    _same(y32, ys)


@pytest.mark.parametrize("name,kw", SHAPES)
@pytest.mark.parametrize("cat_lp", [{}, {"DEX_CAT_LP": "0"}], ids=["catdefault", "cat32"])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_unpatchify_small_form_is_bitwise_the_walker_and_the_single_shot_kernel(name, kw, cat_lp, prec):
    """At these small shapes the concatenation buffer is fp32 with or without DEX_CAT_LP (its 16-bit twin is a batch-size form: the test
    above); both settings run the fp32 scatter."""
    cfg, eng, w = U.engine_for(name)
    case = U.make_case(cfg, **kw)
    eng.set_precision(prec)
    eng.profile(True)
    try:
        y1, r1 = _run(eng, case, 3, {"DEX_NWALK_SMALL": "1", **cat_lp}, rows=True)
        y0, r0 = _run(eng, case, 3, {"DEX_NWALK_SMALL": "0", **cat_lp}, rows=True)
        ys = _run(eng, case, 3, {"DEX_GEMM_NWALK": "0", **cat_lp})
    finally:
        eng.profile(False)
        eng.set_precision("fp32")
    assert any("igemm_lp_nwalk_kernel_small" in r for r in r1) and not any("igemm_lp_nwalk_kernel_small" in r for r in r0)
    assert any(r == "igemm_lp_nwalk_kernel<256>" for r in r0)
    _same(y1, y0)
    _same(y1, ys)


@pytest.mark.parametrize("prec", [p for p in ("bf16", "fp16", "fp16x2") if p in _lib.PRECISION])
def test_headline_shape_is_bitwise_under_every_form(prec):
    name, kw = HEADLINE
    cfg, eng, w = U.engine_for(name)
    case = U.make_case(cfg, **kw)
    eng.set_precision(prec)
    try:
        ref = _run(eng, case, 3, {"DEX_PE_TOK": "8", "DEX_NWALK_SMALL": "0"})
        _same(ref, _run(eng, case, 3, {}))
        _same(ref, _run(eng, case, 3, {"DEX_PE_TOK": "4", "DEX_NWALK_SMALL": "1"}))
        _same(ref, _run(eng, case, 3, {"DEX_PE_TOK": "2"}))
        _same(ref, _run(eng, case, 3, {"DEX_PATCH_FUSED": "0", "DEX_GEMM_NWALK": "0"}))
    finally:
        eng.set_precision("fp32")


def test_headline_eager_equals_graph_replay_with_both_forms_on():
    name, kw = HEADLINE
    cfg, eng, w = U.engine_for(name)
    case = U.make_case(cfg, **kw)
    eng.set_precision("bf16")
    env = {"DEX_PE_TOK": "4", "DEX_NWALK_SMALL": "1"}
    try:
        eager = _run(eng, case, 3, env)
        for _ in range(2):
            _same(eager, _run(eng, case, 3, env, use_graph=True))
    finally:
        eng.set_precision("fp32")


def test_rules_take_the_small_forms_at_the_headline_shape_and_not_at_batch_size():
    cfg, eng, w = U.engine_for("gedex_lj")
    eng.set_precision("bf16")
    eng.profile(True)
    try:
        _, head = _run(eng, U.make_case(cfg, **HEADLINE[1]), 2, {}, rows=True)
        _, batch = _run(eng, U.make_case(cfg, B=4, T=64), 2, {}, rows=True)
    finally:
        eng.profile(False)
        eng.set_precision("fp32")
    pe = lambda rows: sorted({r for r in rows if "patch_embed_fused_kernel" in r})
    fl = lambda rows: sorted({r for r in rows if "igemm_lp_nwalk_kernel" in r})
    assert pe(head) == ["patch_embed_fused_kernel<4>"], pe(head)
    assert fl(head) == ["igemm_lp_nwalk_kernel_small<256>"], fl(head)
    assert pe(batch) == ["patch_embed_fused_kernel"], pe(batch)
    assert fl(batch) == ["igemm_lp_nwalk_kernel<256>"], fl(batch)
