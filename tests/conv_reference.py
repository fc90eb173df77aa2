"""Plain references of ONE launch of the reduced-precision convolution kernels, with a derived per-element bound.

torch, fp64, CPU.  Each operation is restated from the comments of the parameter structs (csrc/kernels.h: Conv3P, ConvDownP,
ConvTUpP) and from the model (oracle/dex_oracle.py: block, resnet_block, Downsample, Upsample), not from the kernels:

    input transform   plain  a = X * mask
                      PRO    a = mask * (Mish(GN(X; pro_stats, gamma, beta)) + tadd[step + b * row_bstride])
                      PRO2   x' = mask * Mish(GN(X)) + res   (also expected in pro_xout),  a = mask * x'
                             res given (pro_res) or recomputed:  res = b1 + sum_q w1[q] * (plane_q * mask),
                             planes (mu, c_in * x[, spk])
    operand rounding  a and the weights to the mode's 16-bit type; fp16x2: weights as hi + lo, lo = fp16(w - fp16(w))
    contraction       3x3/s1/p1, 3x3/s2/p1, ConvTranspose(4,2,1), accumulated in fp64, + bias
    shortcut          res_y = 1x1 conv of the same rounded a (the centre tap) + res_b
    statistics        per (utterance, group of Cout/8 channels): mean and mean of squares of the unrounded output

Tensors are NCHW here, as in the model; masks are [B, T] with the image's column w at mask[b, w * mask_ws].

The bound of an output element is derived, not measured on the kernel:

    tol = K * u * (|a| (*) |w| + |bias|) + (amb (*) |w|) [+ half an output ulp where the output is stored in 16 bits]

K = the number of products of an output element (taps x Cin; twice that with split weights) + 1 for the bias, u = 2^-23: the
forward bound of ANY fp32 summation order of K terms (products of two 16-bit operands are exact in fp32), which also covers an
accumulator that truncates.  `amb` is the 16-bit spacing of every input element whose fp64 transformed value lies within delta of
a rounding boundary: the device evaluates the prologue in fp32 with fast exp / rcp, so such an element may legitimately round to
the other neighbour.  Plain forms have amb = 0 (fp32 x 0/1 mask is exact).

The prologue's fp32 error is proportional to the magnitudes it adds up (GroupNorm's scaled value and shift, the activation, the time
bias, the shortcut): `scale`, per element.  How many unit roundoffs of that scale it amounts to is the one number that cannot be
derived - the device's exp2 / rcp are not specified to the ulp.  It was measured on this reference ALONE (the prologue in torch
fp32 against fp64, on every prologue case of tests/conv_cases.py, every mode) and given 8x:

    python -c "from tests import conv_cases as K; print(K.measure_prologue_fp32_error())"      ->  2.3857   (x 8 = DELTA_ULPS)

so delta = DELTA_ULPS * 2^-24 * scale.  tests/test_conv_reference_cpu.py re-measures it on every case (another host's libm may
differ in the last place: it must leave 4x), and both test files cap the share of ambiguous input elements of a case at
AMB_SHARE_MAX, so the ambiguity set cannot hide a failure.
"""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -23
GN_SLOTS = 32                                  # csrc/kernels.h
GN_FIX_ONE = float(2 ** 36)                    # csrc/bf16_util.h: gn_fix
GN_EPS = 1e-5
GROUPS = 8
PROLOGUE_FP32_ULPS_MEASURED = 2.39             # max |fp32 - fp64| / (2^-24 * scale) over the prologue cases (see above)
DELTA_ULPS = 8 * PROLOGUE_FP32_ULPS_MEASURED   # 8x the measurement: fast device intrinsics are a few ulp worse than libm
AMB_SHARE_MAX = 0.02

LP_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp16x2": torch.float16}
_MANT = {"bf16": 7, "fp16": 10, "fp16x2": 10}          # stored significand bits
_EMIN = {"bf16": -126, "fp16": -14, "fp16x2": -14}     # exponent of the smallest normal


# ---- 16-bit grids ------------------------------------------------------------------------------------------------------------
def round_lp(x, prec):
    """Round to nearest even on the mode's 16-bit grid, through fp32 as the device does; returns x's dtype.  prec None: no rounding
    (the restated operation itself, tests/test_conv_reference_cpu.py)."""
    if prec is None:
        return x
    return x.to(torch.float32).to(LP_DTYPE[prec]).to(x.dtype)


def lp_spacing(r, prec):
    """Spacing of the 16-bit grid around the grid point(s) r: (away from zero, towards zero)."""
    m, e = torch.frexp(r.abs().to(torch.float64))             # |r| = m * 2^e, m in [0.5, 1)
    e = (e - 1).clamp(min=_EMIN[prec])
    e = torch.where(r == 0, torch.full_like(e, _EMIN[prec]), e)
    up = torch.ldexp(torch.ones_like(m), e - _MANT[prec])
    down = torch.where((m == 0.5) & (e > _EMIN[prec]), up / 2, up)
    return up, down


def ambiguity(t, prec, delta):
    """For fp64 values t: the grid spacing towards the OTHER neighbour where t lies within delta of a rounding boundary, else 0."""
    r = round_lp(t, prec)
    up, down = lp_spacing(r, prec)
    d = t.abs() - r.abs()                                     # > 0: t lies on the far side of r
    gap = torch.where(d >= 0, up, down)
    dist = gap / 2 - d.abs()
    return torch.where((dist <= delta) & (t != 0), gap, torch.zeros_like(gap))


def half_ulp_out(y, prec):
    up, _ = lp_spacing(round_lp(y, prec), prec)
    return up / 2


def split_weights(w, prec, drop_lo=False):
    """The weights as the MFMAs see them (fp64): rounded once, or hi + lo in the split-weight mode."""
    hi = round_lp(w, prec)
    if prec != "fp16x2" or drop_lo:
        return hi
    return hi + round_lp(w.to(torch.float32).to(w.dtype) - hi, prec)


# ---- fixed-point statistics --------------------------------------------------------------------------------------------------
def gn_fix(partial, inv_n):
    """Python mirror of gn_fix (csrc/bf16_util.h): round(fp32 partial * inv_n * 2^36) as a saturating 64-bit integer."""
    d = float(torch.tensor(partial, dtype=torch.float32)) * inv_n * GN_FIX_ONE
    d = min(max(d, -9.0e18), 9.0e18)
    return int(round(d))                                       # Python rounds half to even, like __double2ll_rn


def encode_stats(mean, meansq, seed=0):
    """[B, 8] means / means of squares -> int64 [B, 8, GN_SLOTS, 2] whose slots sum to round(value * 2^36): a producer's partials
    arrive spread over the slots, in any split."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(*mean.shape, GN_SLOTS, 2, dtype=torch.int64)
    for k, v in enumerate((mean, meansq)):
        total = torch.round(v.to(torch.float64) * GN_FIX_ONE).to(torch.int64)
        parts = torch.randint(-(1 << 30), 1 << 30, (*mean.shape, GN_SLOTS), generator=g, dtype=torch.int64)
        parts[..., 0] += total - parts.sum(-1)
        out[..., k] = parts
    return out


def decode_stats(fix):
    """int64 [B, 8, GN_SLOTS, 2] -> (mean, meansq) fp64 [B, 8]."""
    s = fix.to(torch.int64).sum(-2).to(torch.float64) / GN_FIX_ONE
    return s[..., 0], s[..., 1]


# ---- the operation -----------------------------------------------------------------------------------------------------------
def mish(x):
    """x * tanh(softplus(x)) - diffusion.py:8-10."""
    return x * torch.tanh(F.softplus(x))


def col_mask(mask, mask_ws, W, dtype):
    return mask[:, ::mask_ws][:, :W].to(dtype)[:, None, None, :]


def group_norm_from_stats(X, mean, meansq, gamma, beta):
    """GroupNorm_8 with the producer's statistics: (x - mean) / sqrt(meansq - mean^2 + eps) * gamma + beta."""
    B, C = X.shape[:2]
    var = (meansq - mean * mean).clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    mu_c = mean.repeat_interleave(C // GROUPS, dim=1)[:, :, None, None].to(X.dtype)
    rs_c = rstd.repeat_interleave(C // GROUPS, dim=1)[:, :, None, None].to(X.dtype)
    return (X - mu_c) * rs_c * gamma.to(X.dtype)[None, :, None, None] + beta.to(X.dtype)[None, :, None, None]


def res2_shortcut(r2, m, dtype):
    """The first ResnetBlock's shortcut: res_conv((mu, c_in * x[, spk]) * mask), a 1x1 conv of 2 - 3 planes (diffusion.py:70,171-175).
    Returns it and the sum of the magnitudes of its terms."""
    c_in = r2["scal"][r2["rows"], 2].to(dtype)[:, None, None]
    planes = [r2["mu"].to(dtype), r2["x"].to(dtype) * c_in]
    if r2.get("spk") is not None:
        planes.append(r2["spk"].to(dtype)[:, :, None].expand_as(planes[0]))
    P = torch.stack(planes, 1) * m                            # [B, planes, H, W]
    w = r2["w"].to(dtype)                                     # [planes, 64]
    b = r2["b"].to(dtype)[None, :, None, None]
    return torch.einsum("bqhw,qc->bchw", P, w) + b, torch.einsum("bqhw,qc->bchw", P.abs(), w.abs()) + b.abs()


def transform(X, mask, mask_ws, pro, dtype=torch.float64):
    """The convolution's input before operand rounding, x' of the PRO2 form (or None), and per element the sum of the magnitudes
    the prologue adds up on the way (GroupNorm's scaled value and shift, the activation, time bias, shortcut): the scale its fp32
    rounding errors are proportional to (None for the plain form, which is exact)."""
    X = X.to(dtype)
    m = col_mask(mask, mask_ws, X.shape[-1], dtype)
    if pro is None:
        return X * m, None, None
    C = X.shape[1]
    var = (pro["meansq"] - pro["mean"] * pro["mean"]).clamp(min=0)
    rstd = (1.0 / torch.sqrt(var + GN_EPS)).repeat_interleave(C // GROUPS, dim=1)[:, :, None, None].to(dtype)
    mu_c = pro["mean"].repeat_interleave(C // GROUPS, dim=1)[:, :, None, None].to(dtype)
    ga, be = pro["gamma"].to(dtype)[None, :, None, None], pro["beta"].to(dtype)[None, :, None, None]
    h = mish(group_norm_from_stats(X, pro["mean"], pro["meansq"], pro["gamma"], pro["beta"]))
    scale = (X.abs() + mu_c.abs()) * rstd * ga.abs() + be.abs() + h.abs()
    res = pro.get("res")
    if res is not None:
        res = res.to(dtype)
        res_mag = res.abs()
    elif pro.get("res2") is not None:
        res, res_mag = res2_shortcut(pro["res2"], m, dtype)
    if res is not None:
        xo = m * h + res
        return m * xo, xo, scale + res_mag
    if pro.get("tadd") is not None:
        ta = pro["tadd"].to(dtype)[pro["rows"]][:, :, None, None]          # row of utterance b: step + b * row_bstride
        h, scale = h + ta, scale + ta.abs()
    return m * h, None, scale


def prologue_fp32_error_ulps(X, mask, mask_ws, pro):
    """max |fp32 - fp64| of the prologue's outputs on this reference alone, in fp32 unit roundoffs (2^-24) of `scale`."""
    t64, x64, sc = transform(X, mask, mask_ws, pro, torch.float64)
    t32, x32, _ = transform(X, mask, mask_ws, pro, torch.float32)
    q = ((t32.double() - t64).abs() / (sc * (U32 / 2))).max()
    if x64 is not None:
        q = torch.maximum(q, ((x32.double() - x64).abs() / (sc * (U32 / 2))).max())
    return float(q)


def _contract(kind, a, w, bias):
    if kind == "conv3":
        return F.conv2d(a, w, bias, padding=1)
    if kind == "down":
        return F.conv2d(a, w, bias, stride=2, padding=1)
    if kind == "up":
        return F.conv_transpose2d(a, w, bias, stride=2, padding=1)
    raise ValueError(kind)


def _terms(kind, w):
    """Products per output element."""
    if kind == "up":
        return 4 * w.shape[0]                                 # [Cin, Cout, 4, 4]: 2 x 2 taps reach an output pixel
    return w.shape[1] * w.shape[2] * w.shape[3]


def reference(kind, prec, X, w, bias, mask, mask_ws=1, pro=None, res_w=None, res_b=None, y_lp=False, xout_lp=False,
              delta_ulps=None, drop_lo=False, dtype=torch.float64, stats=True):
    """One launch.  dtype = float64: the reference and its bounds.  dtype = float32: the same operation with the same rounding
    points evaluated in fp32 (tests/test_conv_reference_cpu.py holds it to the bound); no bounds are returned then.

    kind "conv3" | "down" | "up";  X [B, Cin, H, W];  w the model's weight tensor (conv: [Cout, Cin, kh, kw], up: [Cin, Cout, 4, 4]).
    Returns a dict: Y, tol_Y, a (the rounded input), amb_share, and where asked res_y / tol_res, xout / tol_xout, mean / meansq /
    tol_mean / tol_meansq ([B, 8])."""
    f64 = dtype == torch.float64
    t, xo, scale = transform(X, mask, mask_ws, pro, dtype)
    a = round_lp(t, prec)
    wq = split_weights(w.to(dtype), prec, drop_lo)
    y = _contract(kind, a, wq, bias.to(dtype))
    out = {"Y": y, "a": a}
    if res_w is not None:
        rq = split_weights(res_w.to(dtype), prec, drop_lo)
        out["res_y"] = F.conv2d(a, rq, res_b.to(dtype))
    if xo is not None:
        out["xout"] = xo
    if stats and kind == "conv3":
        B, C = y.shape[:2]
        yg = y.reshape(B, GROUPS, -1)
        out["mean"], out["meansq"] = yg.mean(-1), (yg * yg).mean(-1)
    if not f64 or prec is None:
        return out
    split = 2 if prec == "fp16x2" else 1
    delta = (DELTA_ULPS if delta_ulps is None else delta_ulps) * (U32 / 2) * scale if pro is not None else None
    amb = ambiguity(t, prec, delta) if pro is not None else torch.zeros_like(t)
    out["amb_share"] = float((amb > 0).double().mean())
    K = split * _terms(kind, w) + 1
    mag = _contract(kind, a.abs(), wq.abs(), bias.to(dtype).abs())
    tol = K * U32 * mag + _contract(kind, amb, wq.abs(), None)
    out["tol_fp32"] = tol                                     # of the fp32 value the device holds before it stores
    out["tol_Y"] = tol + half_ulp_out(y.abs() + tol, prec) if y_lp else tol
    if res_w is not None:
        Kr = split * res_w.shape[1] + 1
        out["tol_res"] = Kr * U32 * F.conv2d(a.abs(), rq.abs(), res_b.to(dtype).abs()) + F.conv2d(amb, rq.abs(), None)
    if xo is not None:
        # x' = mask * Mish(GN(X)) + res on the device: the fp32 prologue (delta), one fused multiply-add
        tx = delta + 2 * U32 * xo.abs()
        out["tol_xout"] = tx + half_ulp_out(xo.abs() + tx, prec) if xout_lp else tx
    if stats and kind == "conv3":
        # every contribution is an fp32 sum of at most 16 values per image row and lane, rows walked in sequence, then a shuffle
        # tree (depth <= 16 H + 8 additions; + 1 for the square), entered as round(partial / n * 2^36): one integer rounding each,
        # at most one contribution per 8 output values
        B, C, H, W = y.shape
        depth = 16 * H + 9
        count = H * W * (C // GROUPS) / 8
        t1 = tol.reshape(B, GROUPS, -1)
        ya = y.abs().reshape(B, GROUPS, -1)
        out["tol_mean"] = t1.mean(-1) + depth * (U32 / 2) * ya.mean(-1) + count / GN_FIX_ONE
        out["tol_meansq"] = (2 * ya * t1 + t1 * t1).mean(-1) + depth * (U32 / 2) * (ya * ya).mean(-1) + count / GN_FIX_ONE
    return out


def ratio(got, ref, tol):
    """max(err / tol) of a comparison (the figure every GPU case records)."""
    err = (got.to(torch.float64) - ref).abs()
    return float((err / tol.clamp(min=1e-300)).max())
