"""Plain fp64 reference of ONE launch of the linear-attention kernels of the U-Net stages - csrc/linattn_fused.hip (linattn_kvctx_kernel,
linattn_kvctx_hw_kernel, linattn_merge_kernel, linattn_out2_direct_kernel, linattn_out2_hw_kernel, linattn_out2_kernel) and, in the fp32
mode, csrc/linattn.hip (linattn_ctx_kernel, linattn_combine_kernel) - the packers of their operand layouts, and the derived bounds.
torch, fp64, no device code: every function runs wherever its inputs live.

THE OPERATION (diffusion.py:74-92, Residual(Rezero(LinearAttention)), four heads of 32).  x is [B, N, C], channels last:

    q | k | v = Wqkv x                              1x1 projection, rows q (128) then k then v
    p[d, n]   = softmax over the positions n of k[d, n], per head channel d
    ctx[d, e] = sum_n p[d, n] v[e, n]               per head
    out[e, n] = sum_d ctx[d, e] q[d, n]
    y         = x + g (Wout out + b)

q enters linearly, so the kernels use the collapsed form  y = x + W2 (Wq x) + g b,  W2 = g Wout blockdiag_h(ctx_h^T)  (C x 128 per
utterance); tests/test_linattn_reference_cpu.py holds the two forms equal in fp64.

PER LAUNCH.  The context pass writes, per block of 128 * nsub pixels, head and channel d, a partial (m, s, ctx[d, :]) with
s = sum_n exp(k_n - m), ctx[d, e] = sum_n exp(k_n - m) v[e, n] over the block's pixels.  Here a partial is (M, S, Cx) relative to the
TRUE maximum M of its range, and a kernel's (m, s, c) is compared after the exact change of reference  s e^(m - M),  c e^(m - M).  The
merge kernel folds the partials flash-style, normalises, multiplies by Wout and g and stores W2 in the tail's A-fragment order:

    W2[b][co][he = 32 h + d]  at 16-bit offset  ((((b C/32 + co/32) 8 + ks) 64 + 32 hh + co%32) 8 + j
    hh = (d >> 2) & 1,   j = (d & 3) + 4 ((d >> 3) & 1),   ks = 2 h + (d >> 4)          (the comment in linattn_merge_kernel)

- the he index in the accumulator row order of the tail's q^T tiles.  Wq is in plain A-fragment order (launch_pack_lp_frag_nk):
element (he, c) at ((he/32 C/16 + c/16) 64 + 32 ((c >> 3) & 1) + he%32) 8 + (c & 7); Wkv is the row-major 16-bit cast; the split mode's lo
half sits lo_off elements behind the hi half in the same layout.

OPERANDS ON GRIDS (tests/linattn_cases.py; the CPU test asserts every property).  x = x^ (1 +- 2^-13) with x^ on the 2^-3 grid, |x^| <= 1:
its rounding to either 16-bit type is x^, with no tie (half an fp16 ulp is at least 2^-12 relative).  Weights: multiples of 2^-6 below 1/4 (bf16, fp16), plus in
fp16x2 a lo half of +-1..3 * 2^-16 under a hi half of at least 1/8 (hi ulp 2^-13: the fp16 rounding of the weight is the hi half and
hi + lo is the weight, exactly); the k-stress rows hold +-1/2 only.  Every product x^ w is then a multiple of 2^-19 and every partial sum
of a row is below sum |x^| |w| < 32 = 2^24 * 2^-19 (stress rows: multiples of 2^-4 below 64): fp32 accumulates k, v and q EXACTLY in any
order, with any rounding of the accumulator.  The extra fp32 term a split weight would add (2 C products instead of C) is therefore zero
on these operands - the lo products only have to be read from the right place; a lo image from another place moves k by 2^-16 per
weight, which the m check (below) sees at 2^-23.  What remains is what the kernels add by construction:

CONTEXT PASS.  u = 2^-8 (bf16) / 2^-11 (fp16, fp16x2).  Per partial, with P_n = e^(k_n - M), N pixels in the range, m* = M - KSHIFT
(KSHIFT = 14 ln 2 in the fp16 modes, 0 in bf16), F = nsub + 1 rescales:

    e_p(n)     = 2^-24 (2 |k_n| + 3 |m*| + 4)     p_n = exp2(fma(k_n, L, -m L)), L = fl(log2 e): L's rounding times |k_n|, the product
                 m L and L's rounding times 2 |m|, the fma's rounding times |k_n - m| <= |k_n| + |m|, all times ln 2 log2 e = 1, and v_exp_f32
                 (1 ulp = 2^-23, counted as 4 * 2^-24 with the reciprocal-free remainder)
    e_chain(n) = 2^-23 (1.5 (M - k_n) + 1.5 F)    every later rescale multiplies s and ctx by __expf(m_old - m_new) = exp2((..) L): per factor
                 2^-23 |arg| (the product with L, L itself) + 2^-24 |arg| (the subtraction) + 2^-23 (exp2) + 2^-24 (the multiply); the
                 arguments telescope to m_final - m(n) <= M - k_n, and there are at most nsub in the wave and one in the LDS merge
    e_sum      = (N + 16) 2^-23                  any order of N exact products (two 16-bit values: 22 bits) in an fp32 accumulator, also
                 one that truncates; 16 for the 4-wave merge
    tol_c[d,e] = sum_n P_n |v_n[e]| (2 u + u^2 + e_p + e_chain + e_sum + dk_n[d]) + sum_n P_n dv_n[e] + 2^-39 sum_n |v_n[e]|
                 2 u + u^2: p and v are rounded to 16 bits for the second MFMA.  The last term exists in the fp16 modes only: a p below
                 2^-14 is subnormal and rounds with absolute error 2^-25, and the change of reference multiplies by e^(m* - M) = 2^-14 -
                 this is what the 14 octaves of KSHIFT leave (without them it would be 2^-25, on weights up to 1).
    tol_s[d]   = sum_n P_n (e_p + e_chain + dk_n[d]) + S (N + 16) 2^-23          (s adds the UNROUNDED p)
    tol_m[d]   = max_n dk_n[d] + 2^-23 (|M| + KSHIFT)      m is fl(M - KSHIFT) in fp16 and M itself in bf16 when k is exact

dk, dv are zero on the grid operands.  In the PRO launches x = mask (Mish(GN(h2)) + r) or mask Mish(GN(h2)) + r is computed in fp32 with
fast exp / rcp: tests/conv_reference.py's machinery applies unchanged - delta = DELTA_ULPS 2^-24 scale, `ambiguity` gives the 16-bit
spacing amb of every x within delta of a rounding boundary - and dk_n = split C 2^-23 sum_c |x^_c| |w_c| + sum_c amb_c |w_c| (dv alike,
+ 2^-25 in the fp16 modes for a subnormal v).  Xout: delta + 2 * 2^-23 |x| (one fused multiply-add), plus for a 16-bit store one rounding
to nearest of the fp32 value: half a 16-bit ulp of |x| + tol, the conv test's rule.

MERGED.  The fp64 merge of a kernel's partials against the full-range reference: the same merge applied to the partial bounds (after
the change of reference to the global maximum), for S and Cx alike.

MERGE KERNEL (synthetic fp32 partials, exact inputs).  Each lane folds ceil(nblk / 8) partials with a running maximum, eight lanes merge:
a partial's weight e^(m_c - M) is a chain of at most F = ceil(nblk / 8) + 1 __expf factors whose arguments telescope to M - m_c, so its
relative error is D_c = 2^-23 (1.5 (M - m_c) + 1.5 F) as in e_chain.  With A[d, e] = sum_c w_c |c_c[d, e]| / sum_c w_c s_c:

    tol_ctx[d,e] = sum_c w_c |c_c| D_c / S + |ctx| sum_c w_c s_c D_c / S + (nblk + 10) 2^-23 (A + |ctx|)
                   (numerator and denominator sums of nblk terms in any order, the division)
    tol_W2[co,he] = |g| sum_e |Wout[co,e]| tol_ctx[d,e] + 34 * 2^-24 |g| sum_e |Wout ctx| + half a 16-bit ulp of |W2| + tol
                   (32 fmas and the product with g; one rounding to nearest of the fp32 value)

A partial with m = -inf has weight zero and contributes nothing.

TAIL.  x^ = the 16-bit rounding of x (exact, above), q = Wq x^ exact in fp32, q^ = ONE rounding of q to 16 bits - no ambiguity - and
y = x + sum_he W2[co, he] q^[he] + g b: 128 exact products in an fp32 accumulator in any order, then two additions:

    tol_y = 130 * 2^-23 (sum_he |W2| |q^| + |x| + |g b|)   (+ sum_he dW2 |q^| where W2 carries its own bound: the chained launches)
            + for a 16-bit Y or Y2 half a 16-bit ulp of |y| + tol

The residual is the fp32 x of the launch (x_lp: the 16-bit x that was stored), NOT x^: eps is there to tell them apart.

FP32 MODE (linattn.hip).  k, v are read as fp32, nothing is rounded to 16 bits: tol_c = sum_n P_n |v_n| (e_p32 + e_chain + (N + 16) 2^-23)
with e_p32(n) = 2^-23 (1.5 |k_n - M| + 1.5) (one __expf of k_n - m), F = ceil(chunk / 128) + 1; the combine as the merge kernel with
F = nchunks (one weighted sum, no chain: D_c = 2^-23 (1.5 (M - m_c) + 1.5)) and no final rounding: tol_Weff = |g| sum_e |Wout| tol_ctx +
34 * 2^-24 |g| sum_e |Wout ctx|.

No output element is excluded anywhere.  No constant was enlarged after the first run on the device.
"""
import numpy as np
import torch

from tests import conv_reference as CR

HEADS, DH, HID = 4, 32, 128
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp16x2": 2.0 ** -11}
U32 = 2.0 ** -23
KSHIFT32 = float(np.float32(14.0) * np.float32(0.69314718056))
KSHIFT = {"bf16": 0.0, "fp16": KSHIFT32, "fp16x2": KSHIFT32, None: 0.0}
LP_DTYPE = CR.LP_DTYPE
X_GRID, W_GRID, LO_GRID = 2.0 ** -3, 2.0 ** -6, 2.0 ** -16
# Share of a PRO case's x the operand bound may call ambiguous.  The conv test caps its cases at 2 %; here fp16's grid is finer than the
# prologue's delta allows at small |x| (delta follows the magnitudes the prologue adds up, about 4e-6, the fp16 spacing at |x| = 1/16 is
# 6e-5), and the cases measure 2.7 % on the reference alone.  An ambiguous element is still held to ONE 16-bit spacing.
AMB_SHARE_MAX = 0.05
TINY = 2.0 ** -126


# ---- layouts ------------------------------------------------------------------------------------------------------------------
def w2_offset(co, he, C):
    """16-bit offset of W2[co][he] inside one utterance's C * 128 block (the formula in linattn_merge_kernel's comment)."""
    h, d = he >> 5, he & 31
    hh, j, ks = (d >> 2) & 1, (d & 3) + 4 * ((d >> 3) & 1), 2 * h + (d >> 4)
    return ((((co >> 5) * 8 + ks) * 64) + hh * 32 + (co & 31)) * 8 + j


def w2_offset_plain(co, he, C):
    """The mutant: plain A-fragment order of the he index (no accumulator-row permutation)."""
    return ((((co >> 5) * 8 + (he >> 4)) * 64) + ((he >> 3) & 1) * 32 + (co & 31)) * 8 + (he & 7)


def wq_offset(he, c, C):
    """16-bit offset of Wq[he][c] (launch_pack_lp_frag_nk, K = C, N = 128)."""
    return ((((he >> 5) * (C // 16) + (c >> 4)) * 64) + ((c >> 3) & 1) * 32 + (he & 31)) * 8 + (c & 7)


def _index(fn, rows, cols, C):
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    off = fn(r, c, C).ravel()
    assert np.array_equal(np.sort(off), np.arange(rows * cols))
    return torch.from_numpy(off)


def pack_w2(W2, permute=True):
    """[B, C, 128] -> [B, C * 128] in the tail's layout."""
    B, C, _ = W2.shape
    out = torch.empty(B, C * HID, dtype=W2.dtype, device=W2.device)
    out[:, _index(w2_offset if permute else w2_offset_plain, C, HID, C).to(W2.device)] = W2.reshape(B, C * HID)
    return out


def unpack_w2(f, C):
    return f[:, _index(w2_offset, C, HID, C).to(f.device)].reshape(f.shape[0], C, HID)


def pack_wq(Wq):
    """[128, C] -> [128 * C] in A-fragment order."""
    C = Wq.shape[1]
    out = torch.empty(HID * C, dtype=Wq.dtype, device=Wq.device)
    out[_index(wq_offset, HID, C, C).to(Wq.device)] = Wq.reshape(-1)
    return out


def unpack_wq(f, C):
    return f[_index(wq_offset, HID, C, C).to(f.device)].reshape(HID, C)


def mfma_32x32x16(a_frag, b_frag):
    """The contraction of v_mfma_f32_32x32x16 on lane-held fragments [64 lanes, 8]: lane (i = lane & 31, hh = lane >> 5) holds
    A[i][8 hh + j] and B[8 hh + j][i]; returns D [32, 32] with D[row][col] = sum_k A[row][k] B[k][col] (fp64)."""
    A = torch.zeros(32, 16, dtype=torch.float64)
    Bm = torch.zeros(16, 32, dtype=torch.float64)
    for lane in range(64):
        i, hh = lane & 31, lane >> 5
        A[i, 8 * hh:8 * hh + 8] = a_frag[lane].to(torch.float64)
        Bm[8 * hh:8 * hh + 8, i] = b_frag[lane].to(torch.float64)
    return A @ Bm


def acc_row(r, hh):
    """Row of accumulator register r in lane half hh (the C / D layout of the 32x32 MFMAs)."""
    return (r & 3) + 8 * (r >> 2) + 4 * hh


# ---- the operation ------------------------------------------------------------------------------------------------------------
def project(x, Wqkv, prec):
    """q, k, v [B, N, 128] fp64 from x [B, N, C] and Wqkv [384, C], operands as the MFMAs see them (prec None: unrounded)."""
    xh = CR.round_lp(x.to(torch.float64), prec)
    wh = CR.split_weights(Wqkv.to(torch.float64), prec)
    y = xh @ wh.T
    return y[..., :HID], y[..., HID:2 * HID], y[..., 2 * HID:]


def textbook(x, Wqkv, Wout, bout, g):
    """Residual(Rezero(LinearAttention)) as the model states it, fp64."""
    x = x.to(torch.float64)
    B, N, C = x.shape
    q, k, v = (t.reshape(B, N, HEADS, DH) for t in project(x, Wqkv, None))
    p = torch.softmax(k, dim=1)
    ctx = torch.einsum("bnhd,bnhe->bhde", p, v)
    out = torch.einsum("bhde,bnhd->bnhe", ctx, q).reshape(B, N, HID)
    return x + float(g) * (out @ Wout.to(torch.float64).T + bout.to(torch.float64))


def partial(k, v, lo=0, hi=None):
    """(M, S, Cx, A) of the pixels lo <= n < hi: M [B, 4, 32] the true maximum, S = sum_n e^(k_n - M), Cx[d, e] = sum_n e^(k_n - M)
    v_n[e], A the same sum of magnitudes.  k, v: [B, N, 128] fp64."""
    B = k.shape[0]
    kk = k[:, lo:hi].reshape(B, -1, HEADS, DH)
    vv = v[:, lo:hi].reshape(B, -1, HEADS, DH)
    M = kk.max(dim=1).values
    P = torch.exp(kk - M[:, None])
    return M, P.sum(dim=1), torch.einsum("bnhd,bnhe->bhde", P, vv), torch.einsum("bnhd,bnhe->bhde", P, vv.abs())


def merge(parts):
    """fp64 flash merge of partials [(m, s, c), ...] (m may hold -inf: weight zero) -> (M, S, Cx) relative to M = max m."""
    M = torch.stack([p[0] for p in parts]).max(dim=0).values
    w = [torch.where(torch.isinf(p[0]), torch.zeros_like(M), torch.exp(p[0] - M)) for p in parts]
    return M, sum(wi * p[1] for wi, p in zip(w, parts)), sum(wi[..., None] * p[2] for wi, p in zip(w, parts))


def blocks(npix, nsub):
    """Pixel ranges of the context pass's workgroups."""
    step = 128 * nsub
    return [(lo, min(npix, lo + step)) for lo in range(0, npix, step)]


def w2_of(ctxn, Wout, g):
    """W2[b][co][32 h + d] = g sum_e Wout[co][32 h + e] ctxn[b][h][d][e] (fp64), and the same sum of magnitudes without g."""
    Wo = Wout.to(torch.float64).reshape(-1, HEADS, DH)
    W2 = float(g) * torch.einsum("che,bhde->bchd", Wo, ctxn)
    mag = torch.einsum("che,bhde->bchd", Wo.abs(), ctxn.abs())
    B, C = W2.shape[:2]
    return W2.reshape(B, C, HID), mag.reshape(B, C, HID)


def collapsed(x, Wqkv, Wout, bout, g):
    """The same operation through W2: y = x + W2 (Wq x) + g b (fp64, unrounded)."""
    x = x.to(torch.float64)
    q, k, v = project(x, Wqkv, None)
    M, S, Cx, _ = partial(k, v)
    W2, _ = w2_of(Cx / S[..., None], Wout, g)
    return x + torch.einsum("bnk,bck->bnc", q, W2) + float(g) * bout.to(torch.float64)


# ---- the PRO prologue -----------------------------------------------------------------------------------------------------------
def prologue(h2, mean, meansq, gamma, beta, res, mask, mask_ws, W, under):
    """x [B, N, C] fp64 of a PRO launch and the scale its fp32 error is proportional to.  h2 [B, N, C] (pixel n = row * W + column),
    mean / meansq [B, 8], res [B, N, C] or None, mask [B, T] with column w at mask[b, w * mask_ws]."""
    B, N, C = h2.shape
    H = N // W
    X = h2.to(torch.float64).reshape(B, H, W, C).permute(0, 3, 1, 2)
    m = CR.col_mask(mask, mask_ws, W, torch.float64)
    gn = CR.group_norm_from_stats(X, mean, meansq, gamma, beta)
    act = CR.mish(gn)
    var = (meansq - mean * mean).clamp(min=0)
    rstd = (1.0 / torch.sqrt(var + CR.GN_EPS)).repeat_interleave(C // CR.GROUPS, dim=1)[:, :, None, None]
    mu_c = mean.repeat_interleave(C // CR.GROUPS, dim=1)[:, :, None, None]
    scale = (X.abs() + mu_c.abs()) * rstd * gamma.to(torch.float64).abs()[None, :, None, None] + beta.to(torch.float64).abs()[None, :, None, None] + act.abs()
    if res is not None:
        r = res.to(torch.float64).reshape(B, H, W, C).permute(0, 3, 1, 2)
        x = m * (act + r) if under else m * act + r
        scale = scale + r.abs()
    else:
        x = m * act
    back = lambda t: t.permute(0, 2, 3, 1).reshape(B, N, C)
    return back(x), back(scale.expand_as(x))


def xout_tolerance(x, scale, prec, xout_lp):
    delta = CR.DELTA_ULPS * (U32 / 2) * scale
    tol = delta + 2 * U32 * x.abs()
    return (tol + CR.half_ulp_out(x.abs() + tol, prec) if xout_lp else tol), delta


def operand_error(x, delta, W, prec):
    """dk / dv-style bound [B, N, rows] of W x^ where x^ is the device's 16-bit rounding of an fp32 x known to delta."""
    split = 2 if prec == "fp16x2" else 1
    xh = CR.round_lp(x, prec)
    wa = CR.split_weights(W.to(torch.float64), prec).abs()
    amb = CR.ambiguity(x, prec, delta)
    return split * W.shape[1] * U32 * (xh.abs() @ wa.T) + amb @ wa.T, float((amb > 0).double().mean())


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def partial_tolerance(k, v, lo, hi, prec, nsub, dk=None, dv=None, fp32_mode=False, chunk_subtiles=None):
    """(tol_m, tol_s, tol_c) of the partial over lo <= n < hi (module docstring)."""
    B = k.shape[0]
    kk = k[:, lo:hi].reshape(B, -1, HEADS, DH)
    vv = v[:, lo:hi].reshape(B, -1, HEADS, DH).abs()
    N = kk.shape[1]
    M = kk.max(dim=1).values
    P = torch.exp(kk - M[:, None])
    S = P.sum(dim=1)
    ks = KSHIFT[prec]
    zero = torch.zeros_like(kk)
    dkk = zero if dk is None else dk[:, lo:hi].reshape(B, -1, HEADS, DH)
    dvv = zero if dv is None else dv[:, lo:hi].reshape(B, -1, HEADS, DH)
    if fp32_mode:
        F = chunk_subtiles + 1
        e_p = U32 * (1.5 * (kk - M[:, None]).abs() + 1.5)
        u2 = 0.0
    else:
        F = nsub + 1
        e_p = (U32 / 2) * (2 * kk.abs() + 3 * (M[:, None] - ks).abs() + 4)
        u2 = 2 * U[prec] + U[prec] ** 2
        if prec != "bf16":
            dvv = dvv + 2.0 ** -25
    e_chain = U32 * (1.5 * (M[:, None] - kk) + 1.5 * F)
    e_sum = (N + 16) * U32
    per_n = e_p + e_chain + dkk                                               # [B, N, 4, 32 d]
    tol_s = (P * per_n).sum(dim=1) + S * e_sum
    tol_c = torch.einsum("bnhd,bnhe->bhde", P * (per_n + u2 + e_sum), vv) + torch.einsum("bnhd,bnhe->bhde", P, dvv)
    if prec not in ("bf16", None) and not fp32_mode:
        tol_c = tol_c + 2.0 ** -39 * vv.sum(dim=1)[:, :, None, :]
    tol_m = dkk.max(dim=1).values + U32 * (M.abs() + ks) + TINY
    return tol_m, tol_s, tol_c


def partial_ratios(got, ref, tol, prec):
    """max(err / tol) of a kernel's (m, s, c) against the reference's (M, S, Cx), after the change of reference to M."""
    m, s, c = (t.to(torch.float64) for t in got)
    M, S, Cx = ref[:3]
    tm, ts, tc = tol
    f = torch.exp(m - M)
    r_m = ((m - (M - KSHIFT[prec])).abs() / tm).max().item()
    r_s = ((s * f - S).abs() / ts).max().item()
    r_c = ((c * f[..., None] - Cx).abs() / tc.clamp(min=TINY)).max().item()
    return r_m, r_s, r_c


def merged_ratios(got_parts, ref_parts, tols):
    """The fp64 merge of a kernel's partials against the merge of the reference's (== the full-range reference), with the merged bound."""
    _, Sg, Cg = merge([tuple(t.to(torch.float64) for t in p) for p in got_parts])
    Mg = torch.stack([p[0].to(torch.float64) for p in got_parts]).max(dim=0).values
    Mr, Sr, Cr_ = merge([p[:3] for p in ref_parts])
    w = [torch.exp(p[0] - Mr) for p in ref_parts]
    ts = sum(wi * t[1] for wi, t in zip(w, tols))
    tc = sum(wi[..., None] * t[2] for wi, t in zip(w, tols))
    f = torch.exp(Mg - Mr)
    return ((Sg * f - Sr).abs() / ts).max().item(), ((Cg * f[..., None] - Cr_).abs() / tc.clamp(min=TINY)).max().item()


def merge_reference(pm, ps, pc, Wout, g, prec, combine=False):
    """The merge kernel on partials pm / ps [B, 4, nblk, 32], pc [B, 4, nblk, 32, 32] (fp32 values): W2 [B, C, 128] fp64 (unrounded) and
    its bound (module docstring; combine=True: the fp32 mode's linattn_combine_kernel, no 16-bit store)."""
    pm, ps, pc = (t.to(torch.float64) for t in (pm, ps, pc))
    nblk = pm.shape[2]
    M = pm.max(dim=2).values
    w = torch.where(torch.isinf(pm), torch.zeros_like(pm), torch.exp(pm - M[:, :, None]))
    S = (w * ps).sum(dim=2)
    ctx = (w[..., None] * pc).sum(dim=2) / S[..., None]
    F = 1 if combine else (nblk + 7) // 8 + 1
    D = U32 * (1.5 * torch.where(torch.isinf(pm), torch.zeros_like(pm), M[:, :, None] - pm) + 1.5 * F)
    A = (w[..., None] * pc.abs()).sum(dim=2) / S[..., None]
    tol_ctx = ((w * D)[..., None] * pc.abs()).sum(dim=2) / S[..., None] + ctx.abs() * ((w * ps * D).sum(dim=2) / S)[..., None] \
        + (nblk + 10) * U32 * (A + ctx.abs())
    W2, mag = w2_of(ctx, Wout, g)
    t2, _ = w2_of(tol_ctx, Wout.abs(), abs(float(g)))
    tol = t2 + 34 * (U32 / 2) * abs(float(g)) * mag
    if not combine:
        tol = tol + CR.half_ulp_out(W2.abs() + tol, prec)
    return W2, tol, ctx


def tail_reference(x, Wq, W2h, bias_eff, prec, dW2=None):
    """(y [B, N, C] fp64, its bound as fp32, its bound as a 16-bit Y / Y2) of one tail launch.  x: the launch's X (fp32 values, or the 16-bit values of an x_lp launch);
    Wq [128, C] fp32; W2h [B, C, 128] the 16-bit VALUES of W2; bias_eff = g b; dW2: a bound W2h carries itself (chained launches)."""
    x = x.to(torch.float64)
    xh = CR.round_lp(x, prec)
    q = xh @ CR.split_weights(Wq.to(torch.float64), prec).T
    qh = CR.round_lp(q, prec)
    W2h = W2h.to(torch.float64)
    b = bias_eff.to(torch.float64)
    y = x + torch.einsum("bnk,bck->bnc", qh, W2h) + b
    tol = 130 * U32 * (torch.einsum("bnk,bck->bnc", qh.abs(), W2h.abs()) + x.abs() + b.abs())
    if dW2 is not None:
        tol = tol + torch.einsum("bnk,bck->bnc", qh.abs(), dW2)
    return y, tol, (tol + CR.half_ulp_out(y.abs() + tol, prec))


ratio = CR.ratio


# ---- emulations of the kernels' arithmetic (fp32 and 16-bit, in the kernels' order; tests/test_linattn_reference_cpu.py) ------------
def _f32(t):
    return t.to(torch.float32)


def emulate_kvctx(x, Wkv, npix, nsub, prec, mutant=None):
    """The context pass on x [B, npix, C]: per block four waves of nsub 32-pixel sub-tiles, the online softmax of kv_head_step in fp32,
    p and v rounded to 16 bits for the second product, the LDS merge of the waves.  Returns [(m, s, c)] per block, fp32.
    mutant: None | "s_no_rescale" | "no_inf" | "no_kshift"."""
    lp = LP_DTYPE[prec]
    B = x.shape[0]
    xh = CR.round_lp(x.to(torch.float64), prec)
    kv = _f32(xh @ CR.split_weights(Wkv.to(torch.float64), prec).T)              # exact on the cases' grids
    L = torch.tensor(1.4426950408889634, dtype=torch.float32)
    ksh = torch.tensor(0.0 if mutant == "no_kshift" else KSHIFT[prec], dtype=torch.float32)
    ninf = -float("inf")
    out = []
    for lo, hi in blocks(npix, nsub):
        wm, wsum, wc = [], [], []
        for wave in range(4):
            m = torch.full((B, HID), ninf)
            s = torch.zeros(B, HID)
            c = torch.zeros(B, HEADS, DH, DH)
            for sub in range(nsub):
                p0 = lo + (wave * nsub + sub) * 32
                if p0 >= npix:
                    break
                idx = torch.arange(p0, p0 + 32).clamp(max=npix - 1)
                k, v = kv[:, idx, :HID].clone(), kv[:, idx, HID:]
                if mutant != "no_inf":
                    k[:, torch.arange(p0, p0 + 32) >= npix] = ninf
                mx = k.max(dim=1).values
                mn = torch.maximum(m, mx - ksh)
                alpha = torch.exp(m - mn)
                p = torch.exp2(k * L - (mn * L)[:, None])
                s = (s if mutant == "s_no_rescale" else s * alpha) + p.sum(dim=1)
                ph, vh = _f32(p.to(lp)).reshape(B, 32, HEADS, DH), _f32(v.to(lp)).reshape(B, 32, HEADS, DH)
                c = c * alpha.reshape(B, HEADS, DH, 1) + torch.einsum("bnhd,bnhe->bhde", ph, vh)
                m = mn
            wm.append(m), wsum.append(s), wc.append(c)
        Mx = torch.stack(wm).max(dim=0).values
        f = [torch.where(torch.isinf(mw), torch.zeros_like(Mx), torch.exp(mw - Mx)) for mw in wm]
        out.append((Mx.reshape(B, HEADS, DH), sum(fi * si for fi, si in zip(f, wsum)).reshape(B, HEADS, DH),
                    sum(fi.reshape(B, HEADS, DH, 1) * ci for fi, ci in zip(f, wc))))
    return out


def emulate_merge(pm, ps, pc, Wout, g, prec, mutant=None):
    """linattn_merge_kernel in fp32: eight lanes fold the partials pl, pl + 8, .. with a running maximum, merge, divide, 32 fmas with
    Wout, times g, one rounding to 16 bits.  Returns the 16-bit VALUES W2 [B, C, 128].  mutant: None | "unweighted"."""
    pm, ps, pc = _f32(pm), _f32(ps), _f32(pc)
    B, _, nblk, _ = pm.shape
    ninf = -float("inf")
    lanes = []
    for pl in range(8):
        m = torch.full((B, HEADS, DH), ninf)
        acc, s = torch.zeros(B, HEADS, DH, DH), torch.zeros(B, HEADS, DH)
        for c in range(pl, nblk, 8):
            mn = torch.maximum(m, pm[:, :, c])
            a = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - mn))
            w = torch.where(torch.isinf(pm[:, :, c]), torch.zeros_like(m), torch.exp(pm[:, :, c] - mn))
            if mutant == "unweighted":
                a, w = torch.ones_like(a), torch.ones_like(w)
            acc = acc * a[..., None] + w[..., None] * pc[:, :, c]
            s = s * a + w * ps[:, :, c]
            m = mn
        lanes.append((m, s, acc))
    M = torch.stack([l[0] for l in lanes]).max(dim=0).values
    w = [torch.where(torch.isinf(l[0]), torch.zeros_like(M), torch.exp(l[0] - M)) for l in lanes]
    if mutant == "unweighted":
        w = [torch.ones_like(M) for _ in lanes]
    ctx = sum(wi[..., None] * l[2] for wi, l in zip(w, lanes)) / sum(wi * l[1] for wi, l in zip(w, lanes))[..., None]
    W2 = torch.einsum("che,bhde->bchd", _f32(Wout).reshape(-1, HEADS, DH), ctx) * torch.tensor(float(g), dtype=torch.float32)
    return _f32(W2.reshape(B, -1, HID).to(LP_DTYPE[prec]))


def emulate_tail(x, Wq, W2h, bias_eff, prec, y_lp=False, mutant=None):
    """The tail in fp32: x^ and q^ rounded to 16 bits, y = (W2 q^ + x) + bias.  mutant: None | "res_rounded"."""
    lp = LP_DTYPE[prec]
    x = _f32(x)
    xh = _f32(x.to(lp))
    q = _f32(xh.to(torch.float64) @ CR.split_weights(Wq.to(torch.float64), prec).T)
    qh = _f32(q.to(lp))
    y = torch.einsum("bnk,bck->bnc", qh, _f32(W2h)) + (xh if mutant == "res_rounded" else x) + _f32(bias_eff)
    return _f32(y.to(lp)) if y_lp else y
