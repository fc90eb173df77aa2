"""The launches tests/test_gpu_conv_kernels.py runs one at a time, and their inputs (shared with tests/test_conv_reference_cpu.py,
which checks on the CPU that every case keeps its share of ambiguous input elements under the cap and its fp32 prologue inside DELTA).

Shapes are the smallest at which each form of the launchers can go wrong: H in {80, 40} (the model's only heights), W in
{4, 36, 68, 100, 128} (narrower than a 32-column strip, strips with 4 pixels in the last one, full strips), ragged masks with one
utterance shorter than a strip and one ending mid-strip, and the smallest B at which the launcher picks the form - with the DEX_*
knobs where a threshold would otherwise need a large grid.  The 8-row forms (512 tiles, no knob) and the cases that need real
batch-regime grids run at B = 52 / 13 and evaluate the reference on `subset`: the first and the last utterance and every ragged one."""
import re

import torch

from tests import conv_reference as R

PRECS = ("bf16", "fp16", "fp16x2")
S2, PP0, PP2 = {"DEX_CONV_STREAM": 2}, {"DEX_CONV_PP": 0}, {"DEX_CONV_PP": 2}
NOSMALL, NOW8, NORES, NOR1 = {"DEX_CONV_SMALL_MAX": 1}, {"DEX_CONV_W8": 0}, {"DEX_CONV_RESIDENT": 0}, {"DEX_CONV_ROUND1": 0}
REGW = {"DEX_REGW_MIN_TILES": 1}
KNOBS = ("DEX_CONV_STREAM", "DEX_CONV_PP", "DEX_CONV_SMALL_MAX", "DEX_REGW_MIN_TILES", "DEX_CONV_ROUND1", "DEX_CONV_RESIDENT", "DEX_CONV_W8",
         "DEX_CONV_TH8", "DEX_CONV_SKIP_DEAD", "DEX_CONV_REGW", "DEX_CONV_REGW_RES", "DEX_REGW_WGS", "DEX_CONV_DOWN_WGS", "DEX_CONVT_WGS",
         "DEX_CONVT_MT")


def _lp(s):
    return f"conv3x3_lp_kernel<{s}>"


def c3(name, H, W, B, cin, cout, form, sym, env=(), res=False, xb=False, yb=False, xol=False, rbs=0, step=0, x2=None, frag=False,
       planes=0, subset=None, strip=False):
    """form: plain | pro | pro2 | res2.  sym: the instantiation the case means to run (regex, bf16 / fp16); x2: in the split-weight
    build (default: the same form without resident weights).  strip: a strip-walking form (none exists in the split-weight build)."""
    e = {}
    for d in env if isinstance(env, (list, tuple)) else (env,):
        e.update(d)
    if x2 is None:
        x2 = sym.replace(",resident", "")
    return dict(kind="conv3", name=name, H=H, W=W, B=B, Cin=cin, Cout=cout, form=form, sym="^" + re.escape(sym) + "$",
                sym_x2="^" + re.escape(x2) + "$", env=e, res=res, xb=xb, yb=yb, xol=xol, rbs=rbs, step=step, frag=frag, planes=planes,
                subset=subset, strip=strip)


B52 = [0, 1, 2, 3, 51]
B13 = [0, 1, 2, 3, 12]

CONV3 = [
    # ---- 64 -> 64 patch forms: 2-row (resident / streamed weights), 4-row, the 5-row one-round forms
    c3("c64_2row_plain_res", 40, 100, 1, 64, 64, "plain", _lp("64,64,64,2,0,0,0,4,resident")),
    c3("c64_2row_pro_xb_res", 40, 36, 2, 64, 64, "pro", _lp("64,64,64,2,0,0,1,4,resident"), xb=True, yb=True, rbs=1),
    c3("c64_2row_pro2_xb_res", 40, 68, 1, 64, 64, "pro2", _lp("64,64,64,2,1,0,1,4,resident"), xb=True, yb=True),
    c3("c64_2row_pro2_res", 40, 128, 1, 64, 64, "pro2", _lp("64,64,64,2,1,0,0,4,resident")),
    c3("c64_2row_pro2", 40, 4, 1, 64, 64, "pro2", _lp("64,64,64,2,1,0,0,4"), NORES),
    c3("c64_2row_pro", 80, 36, 1, 64, 64, "pro", _lp("64,64,64,2,0,0,0,4"), NORES, step=1),
    c3("c64_2row_pro_xb", 40, 100, 1, 64, 64, "pro", _lp("64,64,64,2,0,0,1,4"), NORES, xb=True, yb=True),
    c3("c64_2row_pro2_xb", 40, 36, 2, 64, 64, "pro2", _lp("64,64,64,2,1,0,1,4"), NORES, xb=True),
    c3("c64_4row_plain", 80, 68, 2, 64, 64, "plain", _lp("64,64,64,4,0,0,0,4"), NOSMALL),
    c3("c64_4row_pro_xb", 80, 100, 1, 64, 64, "pro", _lp("64,64,64,4,0,0,1,4"), NOSMALL, xb=True, yb=True),
    c3("c64_4row_pro2", 40, 36, 2, 64, 64, "pro2", _lp("64,64,64,4,1,0,0,4"), NOSMALL),
    c3("c64_4row_pro2_xb", 40, 4, 2, 64, 64, "pro2", _lp("64,64,64,4,1,0,1,4"), NOSMALL, xb=True, yb=True),
    c3("c64_round1_plain_res", 80, 100, 4, 64, 64, "plain", _lp("64,64,64,5,0,0,0,10,resident")),
    c3("c64_round1_pro_xb_res", 80, 128, 4, 64, 64, "pro", _lp("64,64,64,5,0,0,1,10,resident"), xb=True, yb=True, rbs=1),
    c3("c64_round1_plain", 80, 128, 4, 64, 64, "plain", _lp("64,64,64,5,0,0,0,10"), NORES),
    c3("c64_round1_pro_xb", 80, 100, 4, 64, 64, "pro", _lp("64,64,64,5,0,0,1,10"), NORES, xb=True, yb=True, step=2),
    c3("c64_round1_pro2_xb", 80, 128, 4, 64, 64, "pro2", _lp("64,64,64,5,1,0,1,10"), xb=True, yb=True, x2=_lp("64,64,64,4,1,0,1,4")),
    c3("c64_round1_pro2", 80, 100, 4, 64, 64, "pro2", _lp("64,64,64,5,1,0,0,10"), x2=_lp("64,64,64,4,1,0,0,4")),
    # ---- padding-only tiles (skip_dead): B >= 4 and >= 1024 workgroups; utterance 1 is shorter than a strip
    c3("c64_skip_dead", 80, 128, 13, 64, 64, "plain", _lp("64,64,64,4,0,0,0,4"), {"DEX_CONV_STREAM": 0}, subset=B13),
    c3("c64_skip_dead_off", 80, 128, 13, 64, 64, "plain", _lp("64,64,64,4,0,0,0,4"), {"DEX_CONV_STREAM": 0, "DEX_CONV_SKIP_DEAD": 0}, subset=B13),
    # ---- 64 -> 128 with the fused 1x1 shortcut
    c3("c128res_round1_res", 40, 128, 2, 64, 128, "plain", _lp("64,128,32,5,0,1,0,5,resident"), res=True),
    c3("c128res_round1", 40, 100, 2, 64, 128, "plain", _lp("64,128,32,5,0,1,0,5"), NORES, res=True),
    c3("c128res_2row", 40, 36, 1, 64, 128, "plain", _lp("64,128,64,2,0,1,0,4"), NOR1, res=True),
    c3("c128res_4row", 40, 68, 1, 64, 128, "plain", _lp("64,128,128,4,0,1,0,4"), [NOSMALL, NOW8], res=True),
    c3("c128res_4row_w8", 40, 68, 2, 64, 128, "plain", _lp("64,128,128,4,0,1,0,8"), NOSMALL, res=True, yb=True),
    c3("c128res_4row_w8_xb", 40, 36, 13, 64, 128, "plain", _lp("64,128,128,4,0,1,1,8"), res=True, xb=True, yb=True, subset=B13),
    # ---- 128 -> 128
    c3("c128_2row_pro", 40, 36, 1, 128, 128, "pro", _lp("128,128,64,2,0,0,0,4")),
    c3("c128_2row_plain", 40, 4, 2, 128, 128, "plain", _lp("128,128,64,2,0,0,0,4")),
    c3("c128_2row_pro_xb", 40, 68, 1, 128, 128, "pro", _lp("128,128,64,2,0,0,1,4"), xb=True, yb=True, rbs=1),
    c3("c128_2row_pro2", 40, 36, 2, 128, 128, "pro2", _lp("128,128,64,2,1,0,0,4")),
    c3("c128_2row_pro2_xb", 40, 100, 1, 128, 128, "pro2", _lp("128,128,64,2,1,0,1,4"), xb=True, yb=True),
    c3("c128_4row_w8_pro_xb", 40, 36, 2, 128, 128, "pro", _lp("128,128,128,4,0,0,1,8"), NOSMALL, xb=True, yb=True),
    c3("c128_4row_w8_pro2_xb", 40, 68, 1, 128, 128, "pro2", _lp("128,128,128,4,1,0,1,8"), NOSMALL, xb=True, yb=True),
    c3("c128_4row_w8_plain", 40, 100, 1, 128, 128, "plain", _lp("128,128,128,4,0,0,0,8"), NOSMALL),
    c3("c128_4row_w8_pro2", 40, 36, 1, 128, 128, "pro2", _lp("128,128,128,4,1,0,0,8"), NOSMALL),
    c3("c128_4row_pro", 40, 68, 1, 128, 128, "pro", _lp("128,128,128,4,0,0,0,4"), [NOSMALL, NOW8], step=1),
    c3("c128_4row_pro_xb", 40, 36, 1, 128, 128, "pro", _lp("128,128,128,4,0,0,1,4"), [NOSMALL, NOW8], xb=True, yb=True),
    c3("c128_4row_pro2", 40, 36, 2, 128, 128, "pro2", _lp("128,128,128,4,1,0,0,4"), [NOSMALL, NOW8]),
    c3("c128_4row_pro2_xb", 40, 4, 1, 128, 128, "pro2", _lp("128,128,128,4,1,0,1,4"), [NOSMALL, NOW8], xb=True),
    c3("c128_8row_pro_xb", 40, 36, 52, 128, 128, "pro", _lp("128,128,128,8,0,0,1,8"), xb=True, yb=True, rbs=1, subset=B52),
    c3("c128_8row_pro", 40, 36, 52, 128, 128, "pro", _lp("128,128,128,8,0,0,0,8"), subset=B52),
    c3("c128_8row_off_pro_xb", 40, 36, 52, 128, 128, "pro", _lp("128,128,128,4,0,0,1,8"), {"DEX_CONV_TH8": 0}, xb=True, yb=True, subset=B52),
    # ---- 128 / 256 -> 64 with the fused 1x1 shortcut (the up path's first conv; xb: the 16-bit concatenation buffer)
    c3("c64res_2row_128", 40, 36, 1, 128, 64, "plain", _lp("128,64,64,2,0,1,0,4"), res=True),
    c3("c64res_2row_256", 40, 68, 1, 256, 64, "plain", _lp("128,64,64,2,0,1,0,4"), res=True),
    c3("c64res_4row_256", 40, 36, 2, 256, 64, "plain", _lp("128,64,64,4,0,1,0,4"), [NOSMALL, NOW8], res=True),
    c3("c64res_4row_w8_128", 40, 100, 1, 128, 64, "plain", _lp("128,64,64,4,0,1,0,8"), NOSMALL, res=True),
    c3("c64res_4row_w8_256_xb", 40, 36, 2, 256, 64, "plain", _lp("128,64,64,4,0,1,1,8"), NOSMALL, res=True, xb=True),
    c3("c64res_8row_128", 40, 36, 52, 128, 64, "plain", _lp("128,64,64,8,0,1,0,8"), res=True, subset=B52),
    c3("c64res_8row_256_xb", 40, 36, 52, 256, 64, "plain", _lp("128,64,64,8,0,1,1,8"), res=True, xb=True, subset=B52),
    # ---- the strip walker (conv3x3_stream64_kernel<PRO, PRO2, XB>)
    c3("walk_plain", 80, 100, 2, 64, 64, "plain", "conv3x3_stream64_kernel<0,0,0>", [S2, PP0], strip=True),
    c3("walk_pro_xb", 40, 36, 2, 64, 64, "pro", "conv3x3_stream64_kernel<1,0,1>", [S2, PP0], xb=True, yb=True, rbs=1, strip=True),
    c3("walk_pro", 80, 68, 1, 64, 64, "pro", "conv3x3_stream64_kernel<1,0,0>", [S2, PP0], step=1, strip=True),
    c3("walk_pro2_xb", 80, 128, 2, 64, 64, "pro2", "conv3x3_stream64_kernel<1,1,1>", [S2, PP0], xb=True, yb=True, xol=True, strip=True),
    c3("walk_pro2", 40, 4, 2, 64, 64, "pro2", "conv3x3_stream64_kernel<1,1,0>", [S2, PP0], strip=True),
    # ---- its ping-pong form (conv3x3_pp64_kernel<PRO, TAIL, XB>; TAIL 2 = the recomputed shortcut res2_*)
    c3("pp_plain", 80, 100, 2, 64, 64, "plain", "conv3x3_pp64_kernel<0,0,0>", [S2, PP2], strip=True),
    c3("pp_plain_xb", 40, 68, 2, 64, 64, "plain", "conv3x3_pp64_kernel<0,0,1>", [S2, PP2], xb=True, yb=True, strip=True),
    c3("pp_pro_xb", 80, 36, 2, 64, 64, "pro", "conv3x3_pp64_kernel<1,0,1>", [S2, PP2], xb=True, yb=True, rbs=1, strip=True),
    c3("pp_pro", 40, 100, 1, 64, 64, "pro", "conv3x3_pp64_kernel<1,0,0>", [S2, PP2], step=2, strip=True),
    c3("pp_pro2_xb", 80, 68, 2, 64, 64, "pro2", "conv3x3_pp64_kernel<1,1,1>", [S2, PP2], xb=True, yb=True, xol=True, strip=True),
    c3("pp_pro2", 40, 36, 2, 64, 64, "pro2", "conv3x3_pp64_kernel<1,1,0>", [S2, PP2], strip=True),
    c3("pp_res2_xb", 80, 100, 2, 64, 64, "res2", "conv3x3_pp64_kernel<1,2,1>", [S2, PP2], xb=True, yb=True, xol=True, planes=3, strip=True),
    c3("pp_res2", 80, 36, 2, 64, 64, "res2", "conv3x3_pp64_kernel<1,2,0>", [S2, PP2], planes=2, rbs=1, strip=True),
    # ---- the register-weight forms (conv3x3_regw.hip: fragment-order weights, 16-bit output)
    c3("regw_pro", 40, 100, 2, 128, 128, "pro", "conv3x3_rw_kernel", REGW, xb=True, yb=True, rbs=1, frag=True, strip=True),
    c3("regw_pro2", 40, 36, 2, 128, 128, "pro2", "conv3x3_rw_kernel", REGW, xb=True, yb=True, frag=True, strip=True),
    c3("regw_pro2_xol", 40, 68, 1, 128, 128, "pro2", "conv3x3_rw_kernel", REGW, xb=True, yb=True, xol=True, frag=True, strip=True),
    c3("regw_res128", 40, 100, 2, 64, 128, "plain", "conv3x3_rw_res128_kernel", REGW, res=True, yb=True, frag=True, strip=True),
    c3("regw_res128_xb", 40, 36, 2, 64, 128, "plain", "conv3x3_rw_res128_kernel", REGW, res=True, xb=True, yb=True, frag=True, strip=True),
]


def strip_case(kind, name, H, W, B, a_lp, c_lp, ldx=64, x_coff=0, ldy=64, y_coff=0):
    return dict(kind=kind, name=name, H=H, W=W, B=B, a_lp=a_lp, c_lp=c_lp, ldx=ldx, x_coff=x_coff, ldy=ldy, y_coff=y_coff,
                sym="^conv_down_kernel$" if kind == "down" else "^convt_up_kernel$", env={}, subset=None)


# Downsample reads the stage's attention output where it lies (the skip half of a concatenation buffer: ldx = 128, x_coff = 64);
# Upsample writes half of the next stage's concatenation buffer (ldy = 128): the other half must stay untouched, bit for bit
STRIPS = [
    strip_case("down", "down_f32_f32", 80, 100, 2, False, False),
    strip_case("down", "down_f32_lp_cat", 80, 36, 2, False, True, ldx=128, x_coff=64),
    strip_case("down", "down_lp_f32", 40, 68, 2, True, False),
    strip_case("down", "down_lp_lp_cat", 80, 128, 4, True, True, ldx=128, x_coff=64),
    strip_case("down", "down_narrow", 80, 4, 2, True, True),
    strip_case("up", "up_f32_f32", 40, 36, 2, False, False),
    strip_case("up", "up_f32_f32_cat", 40, 68, 2, False, False, ldy=128),
    strip_case("up", "up_lp_f32_cat", 40, 100, 2, True, False, ldy=128),
    strip_case("up", "up_f32_lp_cat_hi", 40, 36, 2, False, True, ldy=128, y_coff=64),
    strip_case("up", "up_lp_lp", 40, 128, 4, True, True),
    strip_case("up", "up_narrow", 40, 4, 2, True, True, ldy=128),
]

ALL = CONV3 + STRIPS
BY_NAME = {c["name"]: c for c in ALL}


def lengths(W, B, mask_ws):
    """Utterance lengths in frames: the first full, the second shorter than a 32-column strip, the third ending mid-strip
    (13 columns short), the fourth 40 columns short; the rest - and the last utterance of every batch above four - full."""
    if B == 1:
        return [(W - 5 if W > 8 else W) * mask_ws]
    cols = [W, min(20, W - 1), max(W - 13, 1), max(W - 40, 2)] + [W] * max(B - 4, 0)
    return [c * mask_ws for c in cols[:B]]


def make_inputs(case, prec, seed=None):
    """CPU tensors of one case (NCHW fp32 unless noted) - the same numbers go to the device and to the reference."""
    g = torch.Generator().manual_seed(seed if seed is not None else sum(map(ord, case["name"])))
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    H, W, B = case["H"], case["W"], case["B"]
    ws = 1 if H == 80 else 2                          # the half-resolution stage reads every second frame of the mask
    T = W * ws
    lens = lengths(W, B, ws)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()
    d = dict(mask=mask, mask_ws=ws, lens=lens)
    if case["kind"] != "conv3":
        X = rn(B, 64, H, W)
        if case["a_lp"]:
            X = R.round_lp(X, prec)
        d.update(X=X, bias=rn(64, scale=0.1))
        d["w"] = rn(64, 64, 3, 3, scale=0.05) if case["kind"] == "down" else rn(64, 64, 4, 4, scale=0.07)
        return d
    cin, cout = case["Cin"], case["Cout"]
    X = rn(B, cin, H, W) * (1.0 + 0.5 * torch.rand(1, cin, 1, 1, generator=g)) + 0.3 * rn(1, cin, 1, 1)
    if case["xb"]:
        X = R.round_lp(X, prec)
    d.update(X=X, w=rn(cout, cin, 3, 3, scale=1.5 / (9 * cin) ** 0.5), bias=rn(cout, scale=0.1))
    if case["res"]:
        d.update(res_w=rn(cout, cin, 1, 1, scale=1.0 / cin ** 0.5), res_b=rn(cout, scale=0.1))
    if case["form"] != "plain":
        xg = X.double().reshape(B, R.GROUPS, -1)
        fix = R.encode_stats(xg.mean(-1), (xg * xg).mean(-1), seed=1)
        mean, meansq = R.decode_stats(fix)
        rows = case["step"] + torch.arange(B) * case["rbs"]
        nrows = int(rows.max()) + 1
        # Where Mish's argument is negative, or large against its value's 16-bit spacing, the value is small against the magnitudes
        # the prologue adds up, and such elements fill the ambiguity set (conv_reference.AMB_SHARE_MAX): seven channels of eight
        # get a narrow, positive pre-activation (gamma ~ 0.4, beta ~ 1.5), every eighth the wide one (gamma ~ 1, beta ~ 0) that
        # walks Mish's negative side; the shortcut and its planes sit on the positive side too.
        wide = (torch.arange(cin) % 8) == 3
        gamma = torch.where(wide, 1.0 + rn(cin, scale=0.2), 0.4 + rn(cin, scale=0.08))
        beta = torch.where(wide, rn(cin, scale=0.2), 1.5 + rn(cin, scale=0.2))
        pro = dict(mean=mean, meansq=meansq, gamma=gamma, beta=beta, rows=rows)
        if case["form"] == "pro":
            pro["tadd"] = rn(nrows, cin, scale=0.3)
        elif case["form"] == "pro2":
            pro["res"] = 0.5 + rn(B, cin, H, W, scale=0.5)
        else:
            scal = torch.rand(nrows, 4, generator=g) + 0.25
            pro["res2"] = dict(w=rn(case["planes"], 64, scale=0.3).abs(), b=rn(64, scale=0.1), mu=0.5 + rn(B, H, W, scale=0.5),
                               x=0.5 + rn(B, H, W, scale=0.5), spk=rn(B, H) if case["planes"] == 3 else None, scal=scal, rows=rows)
        d.update(pro=pro, pro_fix=fix)
    return d


def take(d, idx):
    """The inputs of the utterances idx (what the reference of a large-batch case is evaluated on)."""
    idx = torch.as_tensor(idx)
    out = dict(d)
    for k in ("X", "mask"):
        out[k] = d[k][idx]
    if "pro" in d:
        p = dict(d["pro"])
        for k in ("mean", "meansq", "rows", "res"):
            if p.get(k) is not None:
                p[k] = p[k][idx]
        if p.get("res2") is not None:
            r2 = dict(p["res2"])
            for k in ("mu", "x", "spk", "rows"):
                if r2.get(k) is not None:
                    r2[k] = r2[k][idx]
            p["res2"] = r2
        out["pro"] = p
    return out


def reference_of(case, d, prec, **kw):
    """The reference (tests/conv_reference.py) of a case on inputs d (already cut to the subset)."""
    if case["kind"] == "conv3":
        return R.reference("conv3", prec, d["X"], d["w"], d["bias"], d["mask"], d["mask_ws"], pro=d.get("pro"), res_w=d.get("res_w"),
                           res_b=d.get("res_b"), y_lp=case["yb"], xout_lp=case["xol"], **kw)
    return R.reference(case["kind"], prec, d["X"], d["w"], d["bias"], d["mask"], d["mask_ws"], y_lp=case["c_lp"], **kw)


def measure_prologue_fp32_error():
    """The measurement behind conv_reference.DELTA_ULPS: the fp32 prologue against the fp64 one over every prologue case and mode."""
    worst = 0.0
    for case in CONV3:
        if case["form"] == "plain":
            continue
        for prec in PRECS:
            d = make_inputs(case, prec)
            if case["subset"]:
                d = take(d, case["subset"])
            worst = max(worst, R.prologue_fp32_error_ulps(d["X"], d["mask"], d["mask_ws"], d["pro"]))
    return worst
