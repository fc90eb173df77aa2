"""CPU tests of the per-launch convolution reference (tests/conv_reference.py) that tests/test_gpu_conv_kernels.py holds the HIP
kernels to:

  * the restatement IS the model's operation: with rounding off it reproduces oracle/dex_oracle.py's block / resnet_block and the
    Downsample / Upsample expressions of denoiser_forward in fp64;
  * a torch fp32 evaluation of every form with the same rounding points passes the derived bound (and sits far below it);
  * every case keeps its ambiguity set under the cap and its fp32 prologue error 4x inside what the bound allows for;
  * planted faults of the kind a kernel can have each FAIL the per-launch bound while the same outputs stay inside today's
    whole-network bound LOWP[prec]["call"] scaled to the tensor - what the suite let through before;
  * the Python mirror of the fixed-point statistics round-trips.

The planted faults are built small on purpose.  LOWP is 2x the rounding noise of a whole network evaluation, relative to a mel of
range 11.5: (max, mean) * max|y| / 11.5 here.  A fault has to be above the per-launch bound - K u sum|a w|, 7e-5 of y where the sum
is coherent - and below that, down to 3.5e-4 (max) / 4.3e-5 (mean) of max|y| in fp16x2.  So the inputs are non-negative (coherent
sums), loud in a band of eight columns and quiet (8e-4, with a bias of 1e-3) elsewhere - at every utterance's end and in the padding, where the
positional faults sit - and the value faults differ by 2.5e-4."""
import pytest
import torch
import torch.nn.functional as F

from dex_tts_amd.tolerances import LOWP
from oracle import dex_oracle as O
from tests import conv_cases as K
from tests import conv_reference as R

MEL_RANGE = 11.5


# ---- the fixed-point statistics -----------------------------------------------------------------------------------------------
def test_gn_fix_mirror_round_trips():
    g = torch.Generator().manual_seed(3)
    mean = torch.randn(3, 8, generator=g, dtype=torch.float64) * 4
    meansq = mean * mean + torch.rand(3, 8, generator=g, dtype=torch.float64) * 9
    fix = R.encode_stats(mean, meansq, seed=5)
    assert fix.shape == (3, 8, R.GN_SLOTS, 2) and fix.dtype == torch.int64
    m2, q2 = R.decode_stats(fix)
    assert (m2 - mean).abs().max() <= 0.5 / R.GN_FIX_ONE and (q2 - meansq).abs().max() <= 0.5 / R.GN_FIX_ONE
    assert torch.equal(R.encode_stats(m2, q2, seed=9).sum(-2), fix.sum(-2))          # any split over the slots, the same totals
    # gn_fix itself: partial sums of n values, entered one by one, decode to their mean within one rounding each
    vals = torch.randn(40, 16, generator=g)
    parts = [R.gn_fix(float(v.sum()), 1.0 / vals.numel()) for v in vals]
    assert all(isinstance(p, int) for p in parts)
    exact = sum(float(v.sum()) for v in vals) / vals.numel()
    assert abs(sum(parts) / R.GN_FIX_ONE - exact) <= len(parts) * 0.5 / R.GN_FIX_ONE
    assert R.gn_fix(1e30, 1.0) == int(9.0e18) and R.gn_fix(-1e30, 1.0) == -int(9.0e18)       # saturates instead of wrapping
    assert R.gn_fix(0.5, 2.0 ** -36) == 0 and R.gn_fix(1.5, 2.0 ** -36) == 2                   # round half to even


# ---- the restatement is the model's operation ---------------------------------------------------------------------------------

def test_reference_is_the_models_resnet_block():
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B, ci, co, H, Wd = 3, 64, 128, 6, 10
    p = "downs.1.0"
    Wt = {f"{p}.block1.block.0.weight": rn(co, ci, 3, 3) * 0.05, f"{p}.block1.block.0.bias": rn(co) * 0.1,
          f"{p}.block1.block.1.weight": 1 + 0.2 * rn(co), f"{p}.block1.block.1.bias": 0.2 * rn(co),
          f"{p}.block2.block.0.weight": rn(co, co, 3, 3) * 0.05, f"{p}.block2.block.0.bias": rn(co) * 0.1,
          f"{p}.block2.block.1.weight": 1 + 0.2 * rn(co), f"{p}.block2.block.1.bias": 0.2 * rn(co),
          f"{p}.mlp.1.weight": rn(co, 32) * 0.1, f"{p}.mlp.1.bias": rn(co) * 0.1,
          f"{p}.res_conv.weight": rn(co, ci, 1, 1) * 0.1, f"{p}.res_conv.bias": rn(co) * 0.1}
    x, temb = rn(B, ci, H, Wd), rn(B, 32)
    mask = (torch.arange(Wd)[None] < torch.tensor([10, 4, 7])[:, None]).double()
    m4 = mask[:, None, None, :]
    want = O.resnet_block(Wt, p, x, m4, temb, 8)
    want_b1 = O.block(Wt, f"{p}.block1", x, m4, 8)

    # launch 1: the first conv with the fused 1x1 shortcut;  launch 2: block1's tail + time bias in front of the second conv
    # (one table row per utterance);  the block's output is x' of the fused tail in front of whatever conv comes next
    l1 = R.reference("conv3", None, x, Wt[f"{p}.block1.block.0.weight"], Wt[f"{p}.block1.block.0.bias"], mask,
                     res_w=Wt[f"{p}.res_conv.weight"], res_b=Wt[f"{p}.res_conv.bias"])
    tadd = O.linear(Wt, f"{p}.mlp.1", O.mish(temb))
    pro1 = dict(mean=l1["mean"], meansq=l1["meansq"], gamma=Wt[f"{p}.block1.block.1.weight"], beta=Wt[f"{p}.block1.block.1.bias"])
    got_b1, _, _ = R.transform(l1["Y"], mask, 1, pro1)
    assert (got_b1 - want_b1).abs().max() < 1e-12
    l2 = R.reference("conv3", None, l1["Y"], Wt[f"{p}.block2.block.0.weight"], Wt[f"{p}.block2.block.0.bias"], mask,
                     pro=dict(pro1, tadd=tadd, rows=torch.arange(B)))
    pro2 = dict(mean=l2["mean"], meansq=l2["meansq"], gamma=Wt[f"{p}.block2.block.1.weight"], beta=Wt[f"{p}.block2.block.1.bias"],
                res=l1["res_y"])
    l3 = R.reference("conv3", None, l2["Y"], rn(co, co, 3, 3) * 0.05, rn(co), mask, pro=pro2)
    assert (l3["xout"] - want).abs().max() < 1e-11
    assert (l3["a"] - want * m4).abs().max() < 1e-11                  # ... and the next conv sees x * mask (diffusion.py:44)


def test_reference_is_the_models_first_shortcut_and_resamplers():
    g = torch.Generator().manual_seed(12)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B, H, Wd = 2, 6, 10
    mask = (torch.arange(Wd)[None] < torch.tensor([10, 5])[:, None]).double()
    m4 = mask[:, None, None, :]
    # the first ResnetBlock's shortcut: res_conv(stack(mu, c_in * x, spk) * mask)  (denoiser_forward / resnet_block)
    mu, xx, spk, w1, b1 = rn(B, H, Wd), rn(B, H, Wd), rn(B, H), rn(3, 64), rn(64)
    scal = torch.rand(4, 4, generator=g, dtype=torch.float64)
    rows = torch.tensor([1, 3])
    planes = torch.stack([mu, xx * scal[rows, 2][:, None, None], spk[:, :, None].expand(-1, -1, Wd)], 1)
    want = F.conv2d(planes * m4, w1.t()[:, :, None, None], b1)
    got, _ = R.res2_shortcut(dict(w=w1, b=b1, mu=mu, x=xx, spk=spk, scal=scal, rows=rows), m4, torch.float64)
    assert (got - want).abs().max() < 1e-12
    # Downsample (dex_oracle.py: h = h * md; F.conv2d(h, ..., stride=2, padding=1)) and Upsample (F.conv_transpose2d(h * mu_, ...))
    x = rn(B, 64, H, Wd)
    wd, bd, wu, bu = rn(64, 64, 3, 3) * 0.05, rn(64), rn(64, 64, 4, 4) * 0.05, rn(64)
    d = R.reference("down", None, x, wd, bd, mask)
    assert (d["Y"] - F.conv2d(x * m4, wd, bd, stride=2, padding=1)).abs().max() < 1e-12 and d["Y"].shape[-2:] == (H // 2, Wd // 2)
    u = R.reference("up", None, x, wu, bu, mask)
    assert (u["Y"] - F.conv_transpose2d(x * m4, wu, bu, stride=2, padding=1)).abs().max() < 1e-12 and u["Y"].shape[-2:] == (2 * H, 2 * Wd)
    # the half-resolution stage reads every second frame of the mask
    full = (torch.arange(2 * Wd)[None] < torch.tensor([20, 9])[:, None]).double()
    assert torch.equal(R.col_mask(full, 2, Wd, torch.float64)[:, 0, 0], full[:, ::2])


# ---- every case: the ambiguity cap and the measured delta -----------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in K.CONV3 if c["form"] != "plain"])
def test_case_keeps_the_ambiguity_cap_and_delta(name):
    case = K.BY_NAME[name]
    for prec in ("bf16", "fp16"):                                    # (fp16x2 rounds its activations like fp16)
        d = K.make_inputs(case, prec)
        if case["subset"]:
            d = K.take(d, case["subset"])
        q = R.prologue_fp32_error_ulps(d["X"], d["mask"], d["mask_ws"], d["pro"])
        assert 4 * q <= R.DELTA_ULPS, (name, prec, q)
        t, _, scale = R.transform(d["X"], d["mask"], d["mask_ws"], d["pro"])
        share = float((R.ambiguity(t, prec, R.DELTA_ULPS * (R.U32 / 2) * scale) > 0).double().mean())
        assert share <= R.AMB_SHARE_MAX, (name, prec, share)


def test_ambiguity_set_is_what_it_says():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 - 1e-7, 1.0 - 2.0 ** -9 + 1e-7, 0.0, 3.0], dtype=torch.float64)
    amb = R.ambiguity(t, "bf16", torch.full_like(t, 1e-6))
    # bf16 spacing is 2^-7 above 1 and 2^-8 below: the two values next to a midpoint are ambiguous, by the spacing on their side
    assert amb.tolist() == [0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 0.0, 0.0]
    assert float(R.half_ulp_out(torch.tensor([1.5], dtype=torch.float64), "fp16")) == 2.0 ** -11


# ---- a torch fp32 evaluation with the same rounding points passes the bound ---------------------------------------------------------
EMULATED = ["c64_2row_plain_res", "c64_2row_pro_xb_res", "c64_4row_pro2_xb", "c64_round1_pro2", "c128res_round1_res", "c128res_4row_w8",
            "c128_2row_pro_xb", "c128_4row_pro2", "c64res_2row_256", "walk_pro2_xb", "pp_res2_xb", "pp_res2", "regw_pro2_xol",
            "down_f32_lp_cat", "down_lp_f32", "up_lp_lp", "up_f32_f32_cat"]


@pytest.mark.parametrize("prec", K.PRECS)
@pytest.mark.parametrize("name", EMULATED)
def test_fp32_emulation_passes_the_bound(name, prec):
    case = K.BY_NAME[name]
    d = K.make_inputs(case, prec)
    ref = K.reference_of(case, d, prec)
    emu = K.reference_of(case, d, prec, dtype=torch.float32)
    lp_out = case.get("yb") or case.get("c_lp")
    y = R.round_lp(emu["Y"], prec) if lp_out else emu["Y"]           # stored as the kernel stores it
    ratios = {"Y": R.ratio(y, ref["Y"], ref["tol_Y"])}
    if "res_y" in ref:
        ratios["res_y"] = R.ratio(emu["res_y"], ref["res_y"], ref["tol_res"])
    if "xout" in ref:
        xo = R.round_lp(emu["xout"], prec) if case["xol"] else emu["xout"]
        ratios["xout"] = R.ratio(xo, ref["xout"], ref["tol_xout"])
    if "mean" in ref:
        ratios["mean"] = R.ratio(emu["mean"], ref["mean"], ref["tol_mean"])
        ratios["meansq"] = R.ratio(emu["meansq"], ref["meansq"], ref["tol_meansq"])
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if case["kind"] == "conv3" and case["form"] == "plain" and not lp_out:
        assert ratios["Y"] < 0.01, ratios                            # an fp32 accumulation sits far below the any-order bound


# ---- planted faults -------------------------------------------------------------------------------------------------------------
QUIET, EPS = 8e-4, 2.5e-4
FH, FW, FB = 8, 100, 4
FLENS = [100, 20, 87, 60]


def _fault_inputs(cin, cout, prec, seed=21):
    """Non-negative inputs, loud in columns 6..13 and QUIET elsewhere (every utterance's end, the padding, the image's last strip);
    positive weights of sum ~ 1 per output channel; channel 9's weights are channel 8's times 1 + EPS; the rows of one column differ by
    a ripple of relative size EPS."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: 0.5 + torch.rand(*s, generator=g)
    amp = torch.full((FW,), QUIET)
    amp[6:14] = 1.0
    ripple = 1.0 + EPS * torch.linspace(-1, 1, FH)[None, None, :, None]
    X = (u(FB, cin, 1, FW) * amp[None, None, None, :] * ripple).float()
    w = u(cout, cin, 3, 3) / (9 * cin)
    bias = 1e-3 * u(cout)
    w[9], bias[9] = w[8] * (1 + EPS), bias[8]
    if prec == "fp16x2":                 # every weight 0.4 of an fp16 spacing above its fp16 rounding: the lo halves add up coherently
        hi = w.half().float()
        w = (hi.double() + 0.4 * R.lp_spacing(hi.double(), "fp16")[0]).float()
    mask = (torch.arange(FW)[None] < torch.tensor(FLENS)[:, None]).float()
    return dict(X=X, w=w, bias=bias, mask=mask, res_w=u(cout, cin, 1, 1) / cin, res_b=0.1 * u(cout))


def _lowp_ok(prec, got, truth):
    """Today's whole-network criterion scaled to this tensor: max|d| and mean|d| against the unrounded fp64 operation."""
    mx, mn = LOWP[prec]["call"]
    s = float(truth.abs().max()) / MEL_RANGE
    e = (got.double() - truth).abs()
    return float(e.max()) <= mx * s and float(e.mean()) <= mn * s, (float(e.max()) / s, float(e.mean()) / s, mx, mn)


def _both(prec, what, got, ref, tol, truth, healthy):
    """The fault fails the per-launch bound (the healthy evaluation passes it), and stays inside the whole-network bound."""
    assert R.ratio(healthy, ref, tol) <= 1.0, (what, "healthy", R.ratio(healthy, ref, tol))
    r = R.ratio(got, ref, tol)
    assert r > 1.0, (what, prec, "not caught by the per-launch bound", r)
    ok, figs = _lowp_ok(prec, got, truth)
    assert ok, (what, prec, "outside LOWP - the fault is too large to show the gap", figs)


@pytest.mark.parametrize("prec", K.PRECS)
def test_planted_faults_fail_the_launch_bound_inside_the_network_bound(prec):
    d = _fault_inputs(64, 64, prec)
    args = ("conv3", prec, d["X"], d["w"], d["bias"], d["mask"])
    ref = R.reference(*args)
    emu = R.reference(*args, dtype=torch.float32)
    truth = R.reference("conv3", None, d["X"], d["w"], d["bias"], d["mask"])
    a, wq = emu["a"], R.split_weights(d["w"], prec)

    # 1. one tap dropped in the edge column of the last, partial strip (columns 96..99 of utterance 0): tap (kh, kw) = (1, 0) of column 99
    w_tap = torch.zeros_like(wq)
    w_tap[:, :, 1, 0] = wq[:, :, 1, 0]
    y = emu["Y"].clone()
    y[0, :, :, FW - 1] -= F.conv2d(a, w_tap, padding=1)[0, :, :, FW - 1]
    _both(prec, "tap dropped", y, ref["Y"], ref["tol_Y"], truth["Y"], emu["Y"])

    # 2. the mask ignored in one ragged column: the first padded column of utterance 1 (shorter than a strip) is read as valid
    m2 = d["mask"].clone()
    m2[1, FLENS[1]] = 1.0
    y = R.reference("conv3", prec, d["X"], d["w"], d["bias"], m2, dtype=torch.float32)["Y"]
    _both(prec, "mask ignored", y, ref["Y"], ref["tol_Y"], truth["Y"], emu["Y"])

    # 3. two output channels of one 32-wide slice swapped
    y = emu["Y"].clone()
    y[:, [8, 9]] = y[:, [9, 8]]
    _both(prec, "channels swapped", y, ref["Y"], ref["tol_Y"], truth["Y"], emu["Y"])

    # 4. the lo half of the split weights omitted
    if prec == "fp16x2":
        y = R.reference(*args, dtype=torch.float32, drop_lo=True)["Y"]
        _both(prec, "lo half omitted", y, ref["Y"], ref["tol_Y"], truth["Y"], emu["Y"])

    # 5. statistics missing one tile's contribution (rows 0..1, columns 64..95 of utterance 0, group 2): decoded mean / mean of squares
    B, C, H, Wd = emu["Y"].shape
    n = H * Wd * (C // 8)
    tile = emu["Y"][0, 16:24, 0:2, 64:96].double()
    mean_f, msq_f = emu["mean"].clone().double(), emu["meansq"].clone().double()
    mean_f[0, 2] -= tile.sum() / n
    msq_f[0, 2] -= (tile * tile).sum() / n
    assert R.ratio(emu["mean"], ref["mean"], ref["tol_mean"]) <= 1.0 and R.ratio(emu["meansq"], ref["meansq"], ref["tol_meansq"]) <= 1.0
    # (a quiet tile carries next to none of the squares: it is the mean that gives the missing contribution away)
    assert R.ratio(mean_f, ref["mean"], ref["tol_mean"]) > 1.0 and R.ratio(msq_f, ref["meansq"], ref["tol_meansq"]) <= 1.0
    # ... seen by the whole-network bound through their consumer, the next conv's GroupNorm
    ga, be = torch.ones(C), torch.zeros(C)
    z_true = R.group_norm_from_stats(truth["Y"], truth["mean"], truth["meansq"], ga, be)
    z_f = R.group_norm_from_stats(emu["Y"].double(), mean_f, msq_f, ga, be)
    ok, figs = _lowp_ok(prec, z_f, z_true)
    assert ok, ("statistics", prec, figs)

    # 6. the time-bias row of utterance 0 used for utterance 1 (rows EPS apart, as at two neighbouring noise levels)
    g = torch.Generator().manual_seed(5)
    row0 = 0.2 + 0.2 * torch.rand(64, generator=g)
    pro = dict(mean=torch.zeros(FB, 8, dtype=torch.float64), meansq=torch.ones(FB, 8, dtype=torch.float64) - R.GN_EPS,
               gamma=torch.ones(64), beta=torch.zeros(64), tadd=torch.stack([row0 + k * EPS for k in range(FB)]), rows=torch.arange(FB))
    Xp = (d["X"] / d["X"].amax() * 1.5).float()
    pargs = ("conv3", prec, Xp, d["w"], d["bias"], d["mask"])
    pref = R.reference(*pargs, pro=pro)
    assert pref["amb_share"] <= R.AMB_SHARE_MAX
    pemu = R.reference(*pargs, pro=pro, dtype=torch.float32)
    ptruth = R.reference("conv3", None, Xp, d["w"], d["bias"], d["mask"], pro=pro)
    y = R.reference(*pargs, pro=dict(pro, rows=torch.tensor([0, 0, 2, 3])), dtype=torch.float32)["Y"]
    _both(prec, "time-bias row", y, pref["Y"], pref["tol_Y"], ptruth["Y"], pemu["Y"])

    # 7. the fused 1x1 shortcut taken from a non-centre tap (the row below: tap (2, 1)).  The last image row then reads the zero
    # halo, so the input as a whole is quiet here (3e-5 under a shortcut bias of 0.1): the whole-network bound cannot see it
    d2 = _fault_inputs(64, 128, prec, seed=22)
    X7 = (d2["X"] / d2["X"].amax() * 3e-5).float()
    rargs = ("conv3", prec, X7, d2["w"], d2["bias"], d2["mask"])
    rref = R.reference(*rargs, res_w=d2["res_w"], res_b=d2["res_b"])
    remu = R.reference(*rargs, res_w=d2["res_w"], res_b=d2["res_b"], dtype=torch.float32)
    rtruth = R.reference("conv3", None, X7, d2["w"], d2["bias"], d2["mask"], res_w=d2["res_w"], res_b=d2["res_b"])
    below = torch.cat([remu["a"][:, :, 1:], torch.zeros_like(remu["a"][:, :, :1])], 2)
    y = F.conv2d(below, R.split_weights(d2["res_w"], prec), d2["res_b"])
    _both(prec, "shortcut tap", y, rref["res_y"], rref["tol_res"], rtruth["res_y"], remu["res_y"])
