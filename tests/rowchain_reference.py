"""Plain fp64 reference of ONE launch of the fused DiT row chain (csrc/dit_rowchain.hip: dit_rowchain_kernel<ATTN>,
dit_rowchain64_kernel, dit_rowchain64a_kernel, dit_rowchain_cluster_kernel<QKV_ONLY, LOCAL>), an evaluation of the same operation with
the kernels' rounding points, and the derived bounds.  torch, CPU, no device code.

THE OPERATION (DitChainP in csrc/kernels.h; model/dit.py's DiTBlock).  Per token row, hidden 256, mlp 512, two heads of 128:

    O    = the attention output: given (fp32 rows, or 16-bit rows: o_lp), the merge of key-split partials
           O = sum_s w_s O_s / sum_s w_s,  w_s = l_s 2^(m_s - max m)  (attn_reference.merge; rows from tail_row0 on merge the tail
           partials instead), or the softmax attention of Qin / Kin / Vin itself (attn_inline)
    x1   = x + gate_msa (O Wproj + b_proj)
    a1   = LN(x1) (1 + scale_mlp) + shift_mlp                 LayerNorm without affine, eps 1e-6
    h    = GELU(a1 W1 + b1)                                    exact erf
    x2   = x1 + gate_mlp (h W2 + b2)                           -> X
    a2   = LN(x2) (1 + next scale_msa) + next shift_msa
    qkv  = a2 Wqkv + b_qkv;  q qscale, k, v                    -> Qh / Kh / Vt in the attention kernels' fragment layouts

ada row of element b: step + b row_bstride, its six 256-vectors are shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp.
qkv_only: x2 = X (the first block's launch).  A null next_shift: no qkv stage (the last block).  Weights are what the pack holds: the
16-bit rounding of the fp32 matrix, or hi + lo in fp16x2 (conv_reference.split_weights).

reference() evaluates this in fp64 with NO internal rounding.  evaluate() evaluates it in fp64 or fp32 WITH the kernels' rounding
points: O, a1, h, a2 to the mode's 16-bit type (round to nearest even, pack2_lp) and q / k / v after bias and scale.  (The cluster
form rounds the two key halves of O before it merges them; evaluate rounds the merged O - the hard bound below covers both.)

HARD BOUND OF x2 (every element, none excluded): a first-order forward bound of the plain reference through the three rounding points
in front of x2.  u = 2^-8 (bf16) / 2^-11 (fp16, fp16x2), e = 2^-23, |W| = |hi| + |lo|, K' = K (x 2 with split weights) + 8 (bias,
gate, residual, the cluster form's four-way fp32 sums):

    dO    = u Omag + 16 e Omag                                 given O; Omag = sum_s w_s |O_s| / sum_s w_s (the merge in fp32)
          = attn_reference.tolerance / merged_tolerance        attn_inline (the cluster form: of its two key halves, merged)
    dx1   = |g_msa| (dO |Wp| + K' e (Omag |Wp| + |b_p|)) + 2 e (|x| + |g_msa| |O Wp + b_p|)
    dy    = (d + mean d + (|y| + dy0) mean((|y| + dy0) d)) / (sigma - rms d)      LayerNorm: |J| d with J = (I - 11'/n - yy'/n) / sigma,
            y = (x1 - mean) / sigma, sigma reduced by what d can take from it and |y| widened by the first pass dy0 (the mean-value point)
    da1   = |1 + scale| dy + 16 e (|y| |1 + scale| + |shift|)  then  + u (|a1| + da1) + sub        (fp32 LN: 8-level sums, rsqrt, 3 products)
    dpre  = da1 |W1| + K' e (|a1| |W1| + |b1|)
    dh    = 1.13 dpre + 0.5 |pre| (1.5e-7 + 8 e) + 4 e |h|     then  + u (|h| + dh) + sub          (|GELU'| <= 1.13; gelu_erf_rc's erf: A&S 7.1.26)
    dx2   = dx1 + |g_mlp| (dh |W2| + K' e (|h| |W2| + |b2|)) + 2 e (|x1| + |g_mlp| |h W2 + b2|) + e |x2|

Carried through |W| three times in a row this is wide (every one of the 256 / 512 terms of a product at its worst sign).  The same
first-order chain holds with the MLP branch carried per row in the 2-norm, and the bound used is the elementwise MINIMUM of the two:

    ||dx1||  = max|g_msa| (||dO|| ||Wp||_2 + ...) + ...              (spectral norm of the packed weights)
    ||da1||  = max|1 + scale| ||dx1|| / (sigma - rms d) + ...        the LayerNorm's Lipschitz bound: ||J||_2 <= 1 / sigma (two projections)
    ||dpre|| = ||da1|| ||W1||_2 + ...,   ||dh|| = 1.13 ||dpre|| + ... + u (||h|| + ||dh||)
    dx2_j    = dx1_j + |g_mlp_j| (||dh|| ||W2[:, j]||_2 + K' e (|h| |W2| + |b2|)_j) + ...          (Cauchy-Schwarz per output column)

with the rounding and fp32 terms of the elementwise chain as row norms.  dx1 itself stays elementwise (one product).

sub = 2^-25 in the fp16 modes (a value below 2^-14 rounds with that absolute error), 0 in bf16.

SHARP BOUND OF q / k / v, anchored on the launch's own x2 (an exact fp32 input of the last stage; X itself in a qkv_only launch):
a2 is recomputed in fp64 from the x2 the device wrote, rounded, and

    tol = K' e (|a2| |Wq| + |b_q|) sc + (amb |Wq|) sc + half an output ulp,      sc = qscale for q, 1 for k and v

amb is the 16-bit spacing of every a2 whose fp64 value lies within delta of a rounding boundary (conv_reference.ambiguity): the
device computes the LayerNorm in fp32 with v_rsq_f32, so such an element may legitimately round to the other neighbour.
delta = DELTA_ULPS 2^-24 scale with scale = (|x2| + |mean x2| + mean |x2|) / sigma |1 + scale_msa| + |a2| (the shift is exact); the fp32-vs-fp64 LayerNorm error of this reference ALONE
was measured over every case of tests/rowchain_cases.py and every mode and given 8x:

    python -c "from tests import rowchain_cases as K; print(K.measure_ln_fp32_error())"      ->  2.51   (x 8 = DELTA_ULPS)

tests/test_rowchain_reference_cpu.py re-measures it (it must leave 4x) and both test files cap the share of ambiguous a2 elements of
a case at conv_reference.AMB_SHARE_MAX.

RMS-ERROR RATIO.  A worst-case bound cannot see a fault of the size of one rounding inside O -> x2 (two of the roundings sit behind
GEMMs), so x2 is also held to  rms(got - reference) / rms(evaluate(fp32) - reference) <= RATIO_MAX = 1.10  over the whole output, per
32-column tile and per row tile (32 or 64 rows by form; a row tile with fewer than 8 live rows is folded into its neighbour, and a
launch of fewer than 8 rows in all has the whole-output statistic only: a tile statistic is never over fewer than 256 elements).  A
second faithful fp32 evaluation in another summation order stays within [0.998, 1.004]; truncating one internal rounding gives >= 1.49
(M = 640 rows, CPU probe), so 1.10 is 25 x the faithful spread and well under the mildest mutant.
"""
import torch

from tests import attn_reference as AR
from tests.conv_reference import AMB_SHARE_MAX, ambiguity, half_ulp_out, lp_spacing, round_lp, split_weights  # noqa: F401

H, MLP = 256, 512
U = AR.U
E32 = 2.0 ** -23
LN_EPS = 1e-6
GELU_SLOPE = 1.13
ERF_ERR = 1.5e-7 + 8 * E32
LN_FP32_ULPS_MEASURED = 2.51
DELTA_ULPS = 8 * LN_FP32_ULPS_MEASURED
RATIO_MAX = 1.10
MUTANTS = ("trunc_a1", "trunc_h", "drop_lo", "gate_swap", "merge_unweighted", "ln_affine_prev_step")
FORM_ROWS = {"dit_rowchain_kernel<false>": 32, "dit_rowchain_kernel<true> xcd_map=0": 32, "dit_rowchain_kernel<true> xcd_map=1": 32,
             "dit_rowchain64_kernel": 64, "dit_rowchain64a_kernel": 64, "dit_rowchain_cluster_kernel<true,false>": 32,
             "dit_rowchain_cluster_kernel<false,false>": 32, "dit_rowchain_cluster_kernel<false,true>": 32}


def owned_rows(form, N, Npad):
    """Rows of the q / k / v^T operand buffers (per element and head) a form writes, read from its store code: the 32-row forms
    store whole 32-row tiles of the ceil(N / 32) they grid for (store_qkv_tile_d); the 64-row forms two 32-row halves per 64-row tile,
    a half that starts at or past Npad is skipped (the `break` of dit_rowchain64_kernel, the buffer descriptors' range in the
    generated streams)."""
    rows = FORM_ROWS[form]
    end = (N + rows - 1) // rows * rows
    return range(0, min(end, Npad))


def trunc_lp(x, prec):
    """x on the mode's 16-bit grid, rounded TOWARDS ZERO (a mutant's rounding)."""
    r = round_lp(x, prec)
    _, down = lp_spacing(r, prec)
    return torch.where(r.abs() > x.abs(), r - torch.sign(r) * down.to(r.dtype), r)


def weights(inp, prec, dtype=torch.float64, drop_lo=False):
    return {k: split_weights(inp[k], prec, drop_lo).to(dtype) for k in ("Wp", "W1", "W2", "Wq")}


def abs_weights(inp, prec):
    out = {}
    for k in ("Wp", "W1", "W2", "Wq"):
        hi = round_lp(inp[k], prec)
        out[k] = hi.abs() + (round_lp(inp[k] - hi, prec).abs() if prec == "fp16x2" else 0.0)
    return out


def layer_norm(x):
    """(y, sigma): y = (x - mean) / sqrt(var + eps) over the last axis."""
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    sigma = torch.sqrt((xc * xc).mean(-1, keepdim=True) + LN_EPS)
    return xc / sigma, sigma


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _per_head(w, B, N):
    """[B, 2, N] per (element, head, row) -> [B, N, 256] (head h owns columns 128 h .. + 127)."""
    return w.permute(0, 2, 1).repeat_interleave(128, dim=2)


def merge_parts(parts, dtype=torch.float64, unweighted=False):
    """attn_reference.merge of [(m_s, l_s, O_s)] with m, l [B, 2, N] and O_s [B, N, 256]; returns (O, sum_s w_s |O_s| / sum_s w_s)."""
    B, _, N = parts[0][0].shape
    ps = []
    for m, l, O in parts:
        m, l = (torch.zeros_like(m), torch.ones_like(l)) if unweighted else (m, l)
        ps.append((_per_head(m.to(dtype), B, N), _per_head(l.to(dtype), B, N), O.to(dtype)))
    M = torch.stack([p[0] for p in ps]).max(dim=0).values
    w = [p[1] * torch.exp2(p[0] - M) for p in ps]
    W = sum(w)
    return sum(wi * p[2] for wi, p in zip(w, ps)) / W, sum(wi * p[2].abs() for wi, p in zip(w, ps)) / W


def _gh_to_rows(o, B, N):
    """[2 B, N, 128] (element, head) pairs -> [B, N, 256]."""
    return o.reshape(B, 2, N, 128).permute(0, 2, 1, 3).reshape(B, N, 256)


def _given_O(case, inp, dtype, unweighted=False):
    """(O, Omag) of a launch whose attention ran separately."""
    B, N = case["B"], case["N"]
    if case["ksplit"] > 1:
        return merge_parts(inp["parts"], dtype, unweighted)
    O = inp["O"].to(dtype)
    Omag = O.abs()
    if case["tail_ks"] > 1:
        t0 = case["tail_row0"]
        To, Tm = merge_parts(inp["tail_parts"], dtype, unweighted)
        O, Omag = torch.cat([O[:, :t0], To[:, t0:]], 1), torch.cat([Omag[:, :t0], Tm[:, t0:]], 1)
    return O, Omag


def _inline_reference(case, inp, prec):
    """fp64 attention of Qin / Kin / Vin and its tolerance as dO ([B, N, 256] each)."""
    B, N = case["B"], case["N"]
    q, k, v = inp["q"], inp["k"], inp["v"]
    O, A, _, _ = AR.attention_qkv(q, k, v, N)
    vmax = v[:, :N].abs().max(dim=1).values
    if "cluster" in case["form"]:
        # the cluster form's members take the key tiles [0, ceil(nt / 2)) and [ceil(nt / 2), nt) of a head, round their own normalised
        # O_c, and the projections are merged with the flash weights: the merged bound of the two partial bounds
        nt = (N + 31) // 32
        mid = min(N, (nt + 1) // 2 * 32)
        halves = [(0, mid)] + ([(mid, N)] if mid < N else [])
        refs, tols = [], []
        for lo, hi in halves:
            Oc, Ac, Mc, Lc = AR.attention_qkv(q, k, v, N, lo, hi)
            refs.append((Mc, Lc, Oc))
            tols.append(AR.tolerance(Oc, Ac, v[:, lo:hi].abs().max(dim=1).values, N, prec, True))
        dO = AR.merged_tolerance(refs, tols, N) if len(halves) > 1 else tols[0]
    else:
        dO = AR.tolerance(O, A, vmax, N, prec, True)
    return _gh_to_rows(O, B, N), _gh_to_rows(dO, B, N)


def _ada(case, inp, dtype, prev=False):
    """The six adaLN vectors of every element [B, 1, 256] each and the next block's (shift, scale)."""
    rows = [case["step"] + b * case["row_bstride"] - (1 if prev else 0) for b in range(case["B"])]
    a = inp["ada"].to(dtype)[rows]                                    # [B, 6, 256]
    six = [a[:, i][:, None, :] for i in range(6)]
    if case["last"]:
        return six, None, None
    rows = [case["step"] + b * case["row_bstride"] for b in range(case["B"])]
    return six, inp["next_shift"].to(dtype)[rows][:, None, :], inp["next_scale"].to(dtype)[rows][:, None, :]


def _mm(a, w, reorder):
    """a @ w; reorder: the same sum in another order (K reversed, in four chunks)."""
    if not reorder:
        return a @ w
    K = w.shape[0]
    idx = torch.arange(K - 1, -1, -1)
    a, w = a[..., idx], w[idx]
    q = K // 4
    return ((a[..., :q] @ w[:q] + a[..., q:2 * q] @ w[q:2 * q]) + a[..., 2 * q:3 * q] @ w[2 * q:3 * q]) + a[..., 3 * q:] @ w[3 * q:]


def _chain(case, inp, prec, dtype, rounded, mutant=None, reorder=False, x2=None):
    """The operation.  rounded: with the kernels' rounding points.  x2 given: only the last stage, from that x2."""
    assert mutant is None or mutant in MUTANTS
    B, N = case["B"], case["N"]
    rnd = (lambda t, name=None: (trunc_lp if mutant == name and name else round_lp)(t, prec)) if rounded else (lambda t, name=None: t)
    W = weights(inp, prec, dtype, drop_lo=mutant == "drop_lo")
    six, nsh, nsc = _ada(case, inp, dtype)
    sh_msa, sc_msa, g_msa, sh_mlp, sc_mlp, g_mlp = six
    if mutant == "gate_swap":
        g_msa, g_mlp = g_mlp, g_msa
    if mutant == "ln_affine_prev_step":
        prev = _ada(case, inp, dtype, prev=True)[0]
        sh_mlp, sc_mlp = prev[3], prev[4]
    out = {}
    if x2 is not None:
        x2 = x2.to(dtype)
    elif case["qkv_only"]:
        x2 = inp["X"].to(dtype)
    else:
        x = inp["X"].to(dtype)
        if case["attn_inline"]:
            if rounded:
                Qf, Kf, Vf = (f(t).to(torch.float32) for f, t in ((AR.pack_qk, inp["q"]), (AR.pack_qk, inp["k"]), (AR.pack_vt, inp["v"])))
                O = _gh_to_rows(AR.emulate(Qf, Kf, Vf, N, prec, out_lp=True)[0], B, N).to(dtype)
            else:
                O = inp["_O_inline"].to(dtype)
        else:
            O = rnd(_given_O(case, inp, dtype, unweighted=mutant == "merge_unweighted")[0])
        x1 = x + g_msa * (_mm(O, W["Wp"], reorder) + inp["bp"].to(dtype))
        y1, _ = layer_norm(x1)
        a1 = rnd(y1 * (1.0 + sc_mlp) + sh_mlp, "trunc_a1")
        pre = _mm(a1, W["W1"], reorder) + inp["b1"].to(dtype)
        h = rnd(gelu(pre), "trunc_h")
        x2 = x1 + g_mlp * (_mm(h, W["W2"], reorder) + inp["b2"].to(dtype))
        out.update(O=O, x1=x1, a1=a1, pre=pre, h=h)
    out["x2"] = x2
    if not case["last"]:
        y2, s2 = layer_norm(x2)
        a2 = y2 * (1.0 + nsc) + nsh
        # the magnitudes the fp32 LayerNorm + modulate adds up: the row's values and mean over sigma, scaled, the shift, the result
        out["a2_exact"] = a2
        # (the row's mean |x| too: the errors of the row sums reach every element of the row, however small its own terms)
        out["ln_scale"] = ((x2.abs() + x2.mean(-1, keepdim=True).abs() + x2.abs().mean(-1, keepdim=True)) / s2 * (1.0 + nsc).abs()
                           + a2.abs())
        a2 = rnd(a2)
        qkv = _mm(a2, W["Wq"], reorder) + inp["bq"].to(dtype)
        sc = torch.ones(3 * H, dtype=dtype)
        sc[:H] = case["qscale"]
        out.update(a2=a2, qkv=rnd(qkv * sc), sc=sc)
    return out


def evaluate(case, inp, prec, dtype=torch.float32, mutant=None, reorder=False):
    """The operation with the kernels' rounding points, in dtype.  Returns dict(x2 [B, N, 256], qkv [B, N, 768] or absent)."""
    return _chain(case, inp, prec, dtype, True, mutant, reorder)


def reference(case, inp, prec):
    """The plain fp64 operation and the hard bound of x2: dict(x2, tol_x2, qkv (unrounded, q scaled), ...)."""
    B, N = case["B"], case["N"]
    dt = torch.float64
    if case["attn_inline"] and not case["qkv_only"]:
        inp["_O_inline"], dO_inline = _inline_reference(case, inp, prec)
    r = _chain(case, inp, prec, dt, False)
    if case["qkv_only"]:
        r["tol_x2"] = torch.zeros_like(r["x2"])                        # X is not written: bitwise unchanged
        return r
    u, sub = U[prec], (2.0 ** -25 if prec != "bf16" else 0.0)
    Wa = abs_weights(inp, prec)
    split = 2 if prec == "fp16x2" else 1
    six, _, _ = _ada(case, inp, dt)
    _, _, g_msa, sh_mlp, sc_mlp, g_mlp = six
    x, O, x1, a1, pre, h, x2 = inp["X"].to(dt), r["O"], r["x1"], r["a1"], r["pre"], r["h"], r["x2"]
    if case["attn_inline"]:
        Omag, dO = O.abs() + dO_inline, dO_inline
    else:
        Omag = _given_O(case, inp, dt)[1]
        dO = (u + 16 * E32) * Omag
    kp = lambda K: (K * split + 8) * E32
    bp, b1, b2 = (inp[k].to(dt).abs() for k in ("bp", "b1", "b2"))
    dx1 = g_msa.abs() * (dO @ Wa["Wp"] + kp(H) * (Omag @ Wa["Wp"] + bp)) + 2 * E32 * (x.abs() + (x1 - x).abs())
    y, sigma = layer_norm(x1)
    s_lo = sigma - torch.sqrt((dx1 * dx1).mean(-1, keepdim=True))
    assert bool((s_lo > 0.5 * sigma).all()), "the LayerNorm step of the bound needs d << sigma"
    ya = y.abs()
    lnb = lambda yy: (dx1 + dx1.mean(-1, keepdim=True) + yy * (yy * dx1).mean(-1, keepdim=True)) / s_lo
    dy = lnb(ya + lnb(ya))
    da1 = (1.0 + sc_mlp).abs() * dy + 16 * E32 * (ya * (1.0 + sc_mlp).abs() + sh_mlp.abs())
    da1 = da1 + u * (a1.abs() + da1) + sub
    dpre = da1 @ Wa["W1"] + kp(H) * (a1.abs() @ Wa["W1"] + b1)
    dh = GELU_SLOPE * dpre + 0.5 * pre.abs() * ERF_ERR + 4 * E32 * h.abs()
    dh = dh + u * (h.abs() + dh) + sub
    tail = 2 * E32 * (x1.abs() + (x2 - x1).abs()) + E32 * x2.abs()
    fc2_sum = kp(MLP) * (h.abs() @ Wa["W2"] + b2)
    dx2 = dx1 + g_mlp.abs() * (dh @ Wa["W2"] + fc2_sum) + tail
    # the same chain with the MLP branch carried in the rows' 2-norms (module docstring): never wider, both hold
    n2 = lambda t: torch.sqrt((t * t).sum(-1, keepdim=True))
    W = weights(inp, prec, dt)
    spec = lambda w: float(torch.linalg.matrix_norm(w, ord=2))
    ndx1 = g_msa.abs().amax(-1, keepdim=True) * (n2(dO) * spec(W["Wp"]) + n2(kp(H) * (Omag @ Wa["Wp"] + bp))) + n2(2 * E32 * (x.abs() + (x1 - x).abs()))
    ndx1 = torch.minimum(ndx1, n2(dx1))
    nda1 = (1.0 + sc_mlp).abs().amax(-1, keepdim=True) * ndx1 / s_lo + n2(16 * E32 * (ya * (1.0 + sc_mlp).abs() + sh_mlp.abs()))
    nda1 = nda1 + u * (n2(a1) + nda1) + sub * H ** 0.5
    ndpre = nda1 * spec(W["W1"]) + n2(kp(H) * (a1.abs() @ Wa["W1"] + b1))
    ndh = GELU_SLOPE * ndpre + n2(0.5 * pre.abs() * ERF_ERR + 4 * E32 * h.abs())
    ndh = ndh + u * (n2(h) + ndh) + sub * MLP ** 0.5
    col2 = torch.sqrt((W["W2"] * W["W2"]).sum(0))                       # |dh W2|_j <= ||dh|| ||W2[:, j]||
    dx2_n = dx1 + g_mlp.abs() * (ndh * col2 + fc2_sum) + tail
    r["tol_x2"] = torch.minimum(dx2, dx2_n)
    return r


def qkv_reference(case, inp, prec, x2, delta_ulps=None):
    """The last stage recomputed from the x2 the launch wrote (fp32 values): dict(qkv [B, N, 768], tol, amb_share)."""
    dt = torch.float64
    r = _chain(case, inp, prec, dt, True, x2=x2.to(dt))
    Wa = abs_weights(inp, prec)["Wq"]
    split = 2 if prec == "fp16x2" else 1
    delta = (DELTA_ULPS if delta_ulps is None else delta_ulps) * (E32 / 2) * r["ln_scale"]
    amb = ambiguity(r["a2_exact"], prec, delta)
    W = weights(inp, prec, dt)["Wq"]
    exact = (r["a2"] @ W + inp["bq"].to(dt)) * r["sc"]
    tol = ((H * split + 8) * E32 * (r["a2"].abs() @ Wa + inp["bq"].to(dt).abs()) + amb @ Wa) * r["sc"]
    tol = tol + half_ulp_out(exact.abs() + tol, prec)
    return dict(qkv=exact, tol=tol, amb_share=float((amb > 0).double().mean()))


def ln_fp32_error_ulps(case, inp, prec, x2):
    """max |fp32 - fp64| of LN + modulate of x2 on this reference alone, in fp32 unit roundoffs (2^-24) of its scale."""
    a64 = _chain(case, inp, prec, torch.float64, False, x2=x2)
    a32 = _chain(case, inp, prec, torch.float32, False, x2=x2.to(torch.float32))
    return float(((a32["a2_exact"].double() - a64["a2_exact"]).abs() / (a64["ln_scale"] * (E32 / 2))).max())


# ---- the rms-error ratio ---------------------------------------------------------------------------------------------------------
def _rms(e):
    return float(torch.sqrt((e * e).mean()))


def row_groups(B, N, rows):
    """Row tiles [(b, r0, r1)] grouped for the statistic: a tile with fewer than 8 live rows joins the group of the tile before it."""
    groups = []
    for b in range(B):
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            if r1 - r0 < 8 and groups:
                groups[-1].append((b, r0, r1))
            else:
                groups.append([(b, r0, r1)])
    return groups


def rms_ratios(got, ref, ev, rows):
    """rms(got - ref) / rms(ev - ref): (whole output, worst 32-column tile, worst row tile).  [B, N, 256] each."""
    B, N, _ = ref.shape
    ed, er = got.to(torch.float64) - ref, ev.to(torch.float64) - ref
    whole = _rms(ed) / _rms(er)
    if B * N < 8:                                   # (every statistic is over at least 8 rows: 256 elements of a column tile)
        return whole, whole, whole
    col = max(_rms(ed[..., c:c + 32]) / _rms(er[..., c:c + 32]) for c in range(0, H, 32))
    row = 0.0
    for g in row_groups(B, N, rows):
        d = torch.cat([ed[b, r0:r1] for b, r0, r1 in g])
        r = torch.cat([er[b, r0:r1] for b, r0, r1 in g])
        row = max(row, _rms(d) / _rms(r))
    return whole, col, row


def ratio(got, ref, tol):
    """max(err / tol) of a comparison; an element with tol == 0 must be exact."""
    err = (got.to(torch.float64) - ref).abs()
    return float((err / tol.clamp(min=1e-300)).max())
