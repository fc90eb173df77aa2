"""The reduced-precision convolution kernels ONE LAUNCH AT A TIME against a plain fp64 reference of the same operation.

conv3x3_bf16.hip / conv3x3_stream.hip / conv3x3_regw.hip (every branch of launch_conv3x3_lp), conv_down.hip and convt_up.hip are
reached through the test-only shim (tests/kshim), which fills Conv3P / ConvDownP / ConvTUpP and calls the library's own launchers;
weights are packed by the library's own packers.  Each case (tests/conv_cases.py) asserts the instantiation it meant to run - a
launcher that silently re-routes fails the case instead of shrinking coverage - and holds every output element to the bound
tests/conv_reference.py derives for it: Y as stored (fp32 or 16-bit), the fused shortcut, the block output x' of the fused tail, and
the GroupNorm statistics decoded from their fixed-point slots.  Every comparison records max(err / tol)
(profiles/conv_kernel_parity_measured.jsonl holds a run's lines).

Large-batch cases (8-row tiles: 512 tiles, no knob; 16-bit plain input: 256 tiles; padding-only tiles: 1024 workgroups) run the launch
at full batch and evaluate the reference on conv_cases' `subset`: the first and the last utterance and every ragged one.

In fp16x2 a case skips only where the shim says the build has no split-weight form of it; in bf16 / fp16 nothing skips."""
import os
import re

import pytest
import torch

from tests import conv_cases as K
from tests import conv_reference as R

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture
def knobs():
    """The case's DEX_* knobs for one launch (the launchers read the environment outside a C-ABI call), restored afterwards."""
    saved = {k: os.environ.get(k) for k in K.KNOBS}

    def set_(env):
        for k in K.KNOBS:
            os.environ.pop(k, None)
        for k, v in env.items():
            assert k in K.KNOBS, k
            os.environ[k] = str(v)
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _dev():
    return torch.device("cuda", 0)


def _nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype).to(_dev())


def _nchw64(t):
    return t.detach().cpu().to(torch.float64).permute(0, 3, 1, 2)


def _record(case, prec, **ratios):
    from tests import gpu_util
    gpu_util.record(f"convk:{case['name']}:{prec}", **ratios)


def _check(case, prec, ratios):
    _record(case, prec, **ratios)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}          # (NaN - an element the kernel never wrote - fails too)
    assert not bad, (case["name"], prec, ratios)


def run_conv3(case, prec, ks):
    d = K.make_inputs(case, prec)
    lp = ks.LP_DTYPE[prec]
    H, W, B, cin, cout = case["H"], case["W"], case["B"], case["Cin"], case["Cout"]
    dev = _dev()
    f32 = lambda t: t.to(torch.float32).contiguous().to(dev)
    wbf, w_lo = ks.pack("nk", f32(d["w"].permute(2, 3, 1, 0).reshape(9 * cin, cout)), prec)
    T = d["mask"].shape[1]
    t = dict(X=_nhwc(d["X"], lp if case["xb"] else torch.float32), Wbf=wbf, bias=f32(d["bias"]), mask=f32(d["mask"]),
             Y=torch.full((B, H, W, cout), NAN, dtype=lp if case["yb"] else torch.float32, device=dev),
             gn_stats=torch.zeros(B, 8, R.GN_SLOTS, 2, dtype=torch.int64, device=dev))
    kw = dict(H=H, W=W, Cin=cin, Cout=cout, B=B, ldx=cin, mask_ws=d["mask_ws"], mask_bstride=T, step=case["step"], row_bstride=case["rbs"],
              x_bf16=case["xb"], y_bf16=case["yb"], xout_lp=case["xol"], w_lo_off=w_lo)
    if case["frag"]:
        t["Wfrag"], _ = ks.pack("frag", f32(d["w"].permute(2, 3, 1, 0).reshape(9 * cin, cout)), prec)
    if case["res"]:
        rkn = f32(d["res_w"][:, :, 0, 0].t())
        t["res_w"], kw["res_lo_off"] = ks.pack("nk", rkn, prec)
        if case["frag"]:
            t["res_wfrag"], _ = ks.pack("frag", rkn, prec)
        t["res_b"] = f32(d["res_b"])
        t["res_y"] = torch.full((B, H, W, cout), NAN, dtype=torch.float32, device=dev)
    pro = d.get("pro")
    if pro is not None:
        t.update(pro_stats=d["pro_fix"].to(dev), pro_gamma=f32(pro["gamma"]), pro_beta=f32(pro["beta"]))
        if pro.get("tadd") is not None:
            t["pro_tadd"] = f32(pro["tadd"])
        if pro.get("res") is not None:
            t["pro_res"] = _nhwc(pro["res"], torch.float32)
        r2 = pro.get("res2")
        if r2 is not None:
            t.update(res2_w=f32(r2["w"]), res2_b=f32(r2["b"]), res2_mu=f32(r2["mu"]), res2_x=f32(r2["x"]), res2_scal=f32(r2["scal"]))
            if r2["spk"] is not None:
                t["res2_spk"] = f32(r2["spk"])
            kw.update(res2_scal_stride=r2["scal"].shape[1], res2_planes=case["planes"])
        if pro.get("res") is not None or r2 is not None:
            t["pro_xout"] = torch.full((B, H, W, cin), NAN, dtype=lp if case["xol"] else torch.float32, device=dev)
    if prec == "fp16x2" and case["strip"]:
        try:
            strip = ks.conv3x3(prec, t, dry=True, **kw)
        except ks.ShimError as e:
            assert "no such form" in str(e), e
            strip = False
        if not strip:
            pytest.skip("the shim's predicates: the split-weight build has no strip-walking form of this launch")
    sym = ks.conv3x3(prec, t, **kw)
    torch.cuda.synchronize()
    want = case["sym_x2"] if prec == "fp16x2" else case["sym"]
    assert re.match(want, sym), (case["name"], prec, "ran", sym, "meant", want)

    idx = case["subset"] or list(range(B))
    ref = K.reference_of(case, K.take(d, idx) if case["subset"] else d, prec)
    assert ref["amb_share"] <= R.AMB_SHARE_MAX, ref["amb_share"]
    ti = torch.as_tensor(idx, device=dev)
    ratios = {"Y": R.ratio(_nchw64(t["Y"][ti]), ref["Y"], ref["tol_Y"])}
    mean, meansq = R.decode_stats(t["gn_stats"][ti].cpu())
    ratios["mean"] = R.ratio(mean, ref["mean"], ref["tol_mean"])
    ratios["meansq"] = R.ratio(meansq, ref["meansq"], ref["tol_meansq"])
    if case["res"]:
        ratios["res_y"] = R.ratio(_nchw64(t["res_y"][ti]), ref["res_y"], ref["tol_res"])
    if "xout" in ref:
        ratios["xout"] = R.ratio(_nchw64(t["pro_xout"][ti]), ref["xout"], ref["tol_xout"])
    ratios["amb_share"] = ref["amb_share"]
    _check(case, prec, ratios)


def _convt_parity_matrices(w):
    """ConvTranspose2d(4, 2, 1) as four 2x2-tap sub-convolutions, one per output parity (kernels.h, ConvTUpP):
    Wfrag[ph*2 + pw] = [K = (th*2 + tw)*64 + ci][co] = w[ci][co][kh][kw], kh = (ph ? 0 : 1) + 2 th, kw likewise."""
    mats = []
    for ph in range(2):
        for pw in range(2):
            taps = [w[:, :, (0 if ph else 1) + 2 * th, (0 if pw else 1) + 2 * tw] for th in range(2) for tw in range(2)]
            mats.append(torch.cat(taps, 0).contiguous())
    return mats


def run_strip(case, prec, ks):
    d = K.make_inputs(case, prec)
    lp = ks.LP_DTYPE[prec]
    up = case["kind"] == "up"
    H, W, B = case["H"], case["W"], case["B"]
    ldx, xc, ldy, yc = case["ldx"], case["x_coff"], case["ldy"], case["y_coff"]
    if not ks.predicate("convt_up_supported" if up else "conv_down_supported", prec, 64, H, W, ldx, ldy, *(() if up else (xc,))):
        assert prec == "fp16x2", "only the split-weight build may lack the form"
        pytest.skip("the shim's predicate: no split-weight form")
    dev = _dev()
    f32 = lambda t: t.to(torch.float32).contiguous().to(dev)
    g = torch.Generator().manual_seed(7)
    xdt = lp if case["a_lp"] else torch.float32
    X = (torch.randn(B, H, W, ldx, generator=g) * 3).to(xdt)         # the other channels of the buffer: finite values nobody may read
    X[..., xc:xc + 64] = d["X"].permute(0, 2, 3, 1).to(xdt)
    Ho, Wo = (2 * H, 2 * W) if up else (H // 2, W // 2)
    ydt = lp if case["c_lp"] else torch.float32
    Y0 = torch.randn(B, Ho, Wo, ldy, generator=g).to(ydt)           # what lies in the buffer before the launch
    Y = Y0.clone().to(dev)
    t = dict(X=X.contiguous().to(dev), bias=f32(d["bias"]), inmask=f32(d["mask"]), Y=Y)
    if up:
        for par, m in enumerate(_convt_parity_matrices(d["w"])):
            t[f"Wfrag{par}"], _ = ks.pack("frag", f32(m), prec)
    else:
        t["Wfrag"], _ = ks.pack("frag", f32(d["w"].permute(2, 3, 1, 0).reshape(9 * 64, 64)), prec)
    fn = ks.convt_up if up else ks.conv_down
    sym = fn(prec, t, H=H, W=W, B=B, ldx=ldx, x_coff=xc, ldy=ldy, y_coff=yc, a_lp=case["a_lp"], c_lp=case["c_lp"], inmask_ws=d["mask_ws"],
             mask_bstride=d["mask"].shape[1])
    torch.cuda.synchronize()
    assert re.match(case["sym"], sym), (case["name"], sym)
    ref = K.reference_of(case, d, prec)
    got = Y.cpu()
    ratios = {"Y": R.ratio(got[..., yc:yc + 64].to(torch.float64).permute(0, 3, 1, 2), ref["Y"], ref["tol_Y"])}
    # the rest of the buffer (the other half of a concatenation buffer): untouched, bit for bit
    keep = torch.ones(ldy, dtype=torch.bool)
    keep[yc:yc + 64] = False
    ibits = torch.int16 if case["c_lp"] else torch.int32
    assert torch.equal(got[..., keep].contiguous().view(ibits), Y0[..., keep].contiguous().view(ibits)), "wrote outside its channels"
    _check(case, prec, ratios)


@pytest.fixture(scope="module")
def ks():
    from tests import kshim
    kshim.load()
    return kshim


@pytest.mark.parametrize("prec", K.PRECS)
@pytest.mark.parametrize("name", [c["name"] for c in K.CONV3])
def test_conv3x3_launch(name, prec, ks, knobs):
    case = K.BY_NAME[name]
    knobs(case["env"])
    run_conv3(case, prec, ks)


@pytest.mark.parametrize("prec", K.PRECS)
@pytest.mark.parametrize("name", [c["name"] for c in K.STRIPS])
def test_strip_launch(name, prec, ks, knobs):
    case = K.BY_NAME[name]
    knobs(case["env"])
    run_strip(case, prec, ks)


def test_shim_rejects_what_the_launchers_cannot_run(ks):
    """A mistyped case is an error code, never a launch: nothing below reaches the device."""
    dev = _dev()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    H, W, B, C = 40, 36, 1, 64
    base = dict(X=z(B, H, W, C), Wbf=z(9 * C * C, dt=torch.int16), bias=z(C), mask=z(B, 2 * W), Y=z(B, H, W, C))
    kw = dict(H=H, W=W, Cin=C, Cout=C, B=B, ldx=C, mask_ws=2, mask_bstride=2 * W)
    with pytest.raises(ks.ShimError, match="null"):                  # a required pointer
        ks.conv3x3("bf16", {k: v for k, v in base.items() if k != "bias"}, **kw)
    with pytest.raises(ks.ShimError, match="unsupported"):           # channel counts no kernel is built for
        ks.conv3x3("bf16", dict(base, Wbf=z(9 * 96 * C, dt=torch.int16), X=z(B, H, W, 96)), **dict(kw, Cin=96, ldx=96))
    with pytest.raises(ks.ShimError, match="no such form"):          # 16-bit plain input off the forms that read it
        ks.conv3x3("bf16", dict(base, X=z(B, H, W, C, dt=torch.bfloat16)), x_bf16=True, **kw)
    with pytest.raises(ks.ShimError, match="no such form"):          # a fused tail without its GroupNorm statistics
        ks.conv3x3("bf16", dict(base, pro_res=z(B, H, W, C), pro_xout=z(B, H, W, C)), **kw)
    with pytest.raises(ks.ShimError, match="bytes"):                 # a buffer smaller than the descriptor implies
        ks.conv3x3("bf16", dict(base, Y=z(B, H, W, C // 2)), **kw)
    with pytest.raises(ks.ShimError, match="unsupported"):           # Downsample of an odd width
        ks.conv_down("bf16", dict(X=z(B, 80, 35, C), Wfrag=z(9 * C * C, dt=torch.int16), bias=z(C), inmask=z(B, 35), Y=z(B, 40, 17, C)),
                     H=80, W=35, B=B, ldx=C, ldy=C, mask_bstride=35)
