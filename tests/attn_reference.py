"""Plain fp64 reference of ONE launch of the fragment-operand softmax attention kernels (csrc/attention_direct.hip:
attn_direct_kernel, attn_direct_ring_kernel; csrc/attention_q64.hip: attn_q64_kernel), the packers of their operand format, and
the derived per-element bound.  torch / numpy, fp64, no device code: attention() runs wherever its inputs live.

OPERAND FORMAT (AttnDirectP in csrc/kernels.h; read from the layout comment of attention_direct.hip and from the producer's stores,
store_qkv_tile in dit_rowchain.hip).  Per (element, head) an operand is Npad * 128 16-bit elements, 32-row tiles of 4096 elements:

    q / k   row r, feature d      tile r >> 5, inside it  (((d >> 4) * 64 + ((d >> 3) & 1) * 32 + (r & 31)) << 3) + (d & 7)
    v^T     position p of a tile holds key row swz(p) = p with bits 2 and 3 swapped; feature d at position p is at
            ((((d >> 5) * 2 + (p >> 4)) * 64 + ((p >> 3) & 1) * 32 + (d & 31)) << 3) + (p & 7)

THE OPERATION.  The producer folds log2(e) / sqrt(d) into q, so scores s_j = q . k_j are in the log2 domain:

    O_d = sum_j 2^(s_j - M) v_jd / sum_j 2^(s_j - M)      over the keys j < N of a key range, M = max_j s_j
    A_d = sum_j softmax_j |v_jd|                          (the magnitude the bound scales with)

A key split writes, per split s, the normalised O_s and (m_s, l_s) with l_s = sum_j 2^(s_j - m_s); the consumer merges
O = sum_s w_s O_s / sum_s w_s,  w_s = l_s 2^(m_s - max m).

THE BOUND.  What the kernels do: scores and everything else in fp32, the reference maximum m lags the true maximum by at most LAG
(the move test `mx > m + 8`), P = 2^(s - m) is rounded to the mode's 16-bit type by round-to-nearest-even (pack2_lp) for the P V
product while l sums the UNROUNDED fp32 P.  Per output element

    tol = (u + C (N + 16) 2^-23) A_d + u_out |O_d| + sub

    u      2^-8 (bf16) / 2^-11 (fp16, fp16x2): the unit roundoff of the 16-bit type (8 / 11 significant bits).  A rounded P_j is
           P_j (1 + r_j) with |r_j| <= u, l keeps the unrounded P_j, so the rounding moves O_d by sum_j w_j r_j v_jd <= u A_d.
    scores tests/attn_cases.py draws q on the 2^-6 grid, k on the 2^-5 grid (spikes and sentinels too): every product is a multiple
           of 2^-11 and every partial sum is below 2^13, so fp32 accumulates the 128 products EXACTLY in any order, also when the
           accumulator is seeded with -m (a maximum of exact scores is on the same grid).  s_j - m carries no error; the CPU test
           asserts the grid property of every case's operands.
    C = 2  the fp32 remainder, in units of (N + 16) 2^-23 A_d = 2 (N + 16) 2^-24 A_d:
             * the P V accumulation: products of two 16-bit values are exact in fp32 (at most 22 significant bits), any summation
               order of N terms is within N 2^-24 sum |terms|, and each lazy rescale (at most N / 32 of them, counted inside the
               16 + N) multiplies by a factor that ALSO multiplies l, so only its rounding counts;  <= (N + 16) 2^-24 A_d
             * l: a sum of N positive fp32 terms;  <= (N + 16) 2^-24 relative, which moves O by that times |O_d| <= A_d
           Together 2 (N + 16) 2^-24 A_d = half of the C term.  The other half, (N + 16) 2^-23 A_d >= 17 * 2^-23 A_d, holds the terms
           that do not grow with N: v_exp_f32 is good to 1 ulp (2^-23 relative on P_j, in numerator and denominator: <= 2 * 2^-23
           A_d), the reciprocal and the final multiply (<= 3.5 ulp), and the 8-wave LDS merge of attn_direct_kernel (exp2f, 8 fmas,
           in numerator and denominator: <= 10 ulp) - 2^-24 * (4 + 3.5 + 10) < 17 * 2^-23.
    u_out  u for 16-bit output rows (one rounding to nearest), else 2^-23.
    sub    N 2^-25 max_j |v_jd| in the fp16 modes, 0 in bf16: a P_j below 2^-14 is subnormal in fp16 and rounds with ABSOLUTE error
           <= 2^-25; l >= 1 because m <= true maximum (the maximal key contributes >= 1), so the division does not amplify it.  bf16 has
           fp32's exponent range: no such term (a P below 2^-126 contributes < N 2^-126).
No output element is excluded anywhere.

(m, l).  m must lie in [M - LAG, M] for the true maximum M of the partial's key range, and l 2^m must match the fp64 sum_j 2^s_j
within (N + 16) 2^-23 relative (N fp32 additions and the rescales at 2^-24 each, 1 ulp per exp2).

MERGED.  For the fp64 merge of a kernel's partials the bound is the same merge applied to the partial bounds, plus the error of the
weights: w_s carries l_s's relative error e_l = (N + 16) 2^-23, which moves the merged value by at most 2 e_l sum_s w_s |O_s| / sum_s w_s.
"""
import numpy as np
import torch

HD = 128
TILE = 32 * HD
LAG = 8.0                                       # the kernels' move test: mx > m_run + 8.f (log2 domain)
C_FP32 = 2.0
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp16x2": 2.0 ** -11}
U32 = 2.0 ** -23
LP_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp16x2": torch.float16}
Q_GRID, K_GRID = 2.0 ** -6, 2.0 ** -5           # see "scores" above


# ---- fragment packers ---------------------------------------------------------------------------------------------------------
def swz(p):
    """p with bits 2 and 3 swapped."""
    return (p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1)


def qk_offset(r, d):
    return (r >> 5) * TILE + ((((d >> 4) * 64 + ((d >> 3) & 1) * 32 + (r & 31)) << 3) + (d & 7))


def vt_offset(pos, d):
    """Offset of feature d at position pos (tile pos >> 5, position pos & 31 inside it)."""
    p = pos & 31
    return (pos >> 5) * TILE + (((((d >> 5) * 2 + (p >> 4)) * 64 + ((p >> 3) & 1) * 32 + (d & 31)) << 3) + (p & 7))


_PERM = {}


def _perm(kind, npad, swap=True):
    """gather[i] = the row-major index (row * 128 + d) of the element stored at packed offset i."""
    key = (kind, npad, swap)
    if key not in _PERM:
        r, d = np.meshgrid(np.arange(npad), np.arange(HD), indexing="ij")
        if kind == "qk":
            off, src = qk_offset(r, d), r * HD + d
        else:                                   # r is the POSITION; it holds key row (tile, swz(position))
            row = (r & ~31) | swz(r & 31) if swap else r
            off, src = vt_offset(r, d), row * HD + d
        g = np.empty(npad * HD, dtype=np.int64)
        g[off.ravel()] = src.ravel()
        assert np.array_equal(np.sort(off.ravel()), np.arange(npad * HD))
        _PERM[key] = torch.from_numpy(g)
    return _PERM[key]


def _pack(x, kind, swap=True):
    npad = x.shape[-2]
    assert x.shape[-1] == HD and npad % 32 == 0
    return x.reshape(*x.shape[:-2], npad * HD)[..., _perm(kind, npad, swap).to(x.device)]


def _unpack(f, kind, swap=True):
    npad = f.shape[-1] // HD
    g = _perm(kind, npad, swap).to(f.device)
    out = torch.empty_like(f)
    out[..., g] = f
    return out.reshape(*f.shape[:-1], npad, HD)


def pack_qk(x):
    """[..., Npad, 128] rows -> [..., Npad * 128] in q / k fragment order."""
    return _pack(x, "qk")


def unpack_qk(f):
    return _unpack(f, "qk")


def pack_vt(v, swap=True):
    """[..., Npad, 128] value rows -> [..., Npad * 128] in v^T fragment order (swap=False: a mutant without the bit-2/3 swap)."""
    return _pack(v, "vt", swap)


def unpack_vt(f, swap=True):
    return _unpack(f, "vt", swap)


# ---- the operation ------------------------------------------------------------------------------------------------------------
def scores(q, k, N):
    """fp64 [G, N, N] log2-domain scores of the live rows."""
    return q[:, :N].to(torch.float64) @ k[:, :N].to(torch.float64).transpose(1, 2)


def attention(s, v, lo=0, hi=None, rows=None):
    """Softmax attention over the keys lo <= j < hi of scores s [G, N, N] (fp64) and values v [G, >= N, 128], for the query rows
    `rows` (a slice; default all).  Returns O [G, R, 128], A (sum_j softmax_j |v_jd|), M [G, R] (the true maximum) and L
    (sum_j 2^(s_j - M)), all fp64."""
    hi = s.shape[2] if hi is None else hi
    rows = slice(None) if rows is None else rows
    sr = s[:, rows, lo:hi]
    vv = v[:, lo:hi].to(torch.float64)
    M = sr.max(dim=-1).values
    p = torch.exp2(sr - M[..., None])
    L = p.sum(dim=-1)
    w = p / L[..., None]
    return w @ vv, w @ vv.abs(), M, L


def attention_qkv(q, k, v, N, lo=0, hi=None, rows=None, chunk=1 << 22):
    """attention() from the operands, a few (element, head) pairs at a time (the score matrix of a large case is never held whole)."""
    hi = N if hi is None else hi
    rows = slice(0, N) if rows is None else rows
    R_ = max(rows.stop - rows.start, 1)
    step = max(1, chunk // (R_ * max(hi - lo, 1)))
    outs = []
    for g0 in range(0, q.shape[0], step):
        s = q[g0:g0 + step, rows].to(torch.float64) @ k[g0:g0 + step, lo:hi].to(torch.float64).transpose(1, 2)
        outs.append(attention(s, v[g0:g0 + step, lo:hi]))
    return tuple(torch.cat([o[i] for o in outs]) for i in range(4))


def merge(parts):
    """fp64 merge of key-split partials [(m_s, l_s, O_s), ...]: O = sum_s w_s O_s / sum_s w_s, w_s = l_s 2^(m_s - max m).
    Returns (O, M, L) with L relative to M = max m."""
    M = torch.stack([p[0] for p in parts]).max(dim=0).values
    w = [p[1] * torch.exp2(p[0] - M) for p in parts]
    L = sum(w)
    return sum(wi[..., None] * p[2] for wi, p in zip(w, parts)) / L[..., None], M, L


def tolerance(O, A, vabs_max, N, prec, out_lp):
    """Per-element bound (module docstring).  vabs_max: [G, 128] max_j |v_jd| over the partial's keys."""
    u = U[prec]
    sub = N * 2.0 ** -25 * vabs_max[:, None, :] if prec != "bf16" else 0.0
    return (u + C_FP32 * (N + 16) * U32) * A + (u if out_lp else U32) * O.abs() + sub


def l_tolerance(N):
    return (N + 16) * U32


def merged_tolerance(ref_parts, tols, N):
    """Bound of the fp64 merge of a kernel's partials (module docstring, MERGED).  ref_parts: [(M_s, L_s, O_s)] of the reference."""
    M = torch.stack([p[0] for p in ref_parts]).max(dim=0).values
    w = [p[1] * torch.exp2(p[0] - M) for p in ref_parts]
    W = sum(w)
    t = sum(wi[..., None] * ti for wi, ti in zip(w, tols)) / W[..., None]
    absO = sum(wi[..., None] * p[2].abs() for wi, p in zip(w, ref_parts)) / W[..., None]
    return t + 2 * l_tolerance(N) * absO


def ml_ratios(m, l, M, L, N):
    """(m, l) of a partial against the reference's true maximum M and L = sum_j 2^(s_j - M): the two ratios that must be <= 1."""
    m, l = m.to(torch.float64), l.to(torch.float64)
    r_m = ((m - (M - LAG / 2)).abs() / (LAG / 2)).max().item()                       # m in [M - LAG, M]
    r_l = ((l * torch.exp2(m - M) - L).abs() / L / l_tolerance(N)).max().item()
    return r_m, r_l


# ---- an emulation of the kernels' arithmetic (tests/test_attn_reference_cpu.py: the bound holds for it, its mutants break it) --
def emulate(Qf, Kf, Vf, N, prec, lo_tile=0, hi_tile=None, out_lp=False, mutant=None):
    """One partial the way the kernels compute it, from PACKED fp32-valued operands [G, Npad * 128]: 32-key tiles lo_tile <= t <
    hi_tile, fp32 scores, a reference maximum per 32-query block that moves when some row of the block exceeds it by more than LAG,
    P rounded to the mode's 16-bit type for the product, fp32 row sums of the unrounded P, fp32 or 16-bit output.
    Returns (O [G, N, 128] fp32, m [G, N], l [G, N]).
    mutant: None | "drop_last" | "admit_pad" | "no_swap" | ("skip_tile", t) | "row_off" (the rest act on the caller's side)."""
    lp = LP_DTYPE[prec]
    q = unpack_qk(Qf).to(torch.float32)
    k = unpack_qk(Kf).to(torch.float32)
    v = unpack_vt(Vf, swap=mutant != "no_swap").to(torch.float32)
    G, npad = q.shape[0], q.shape[1]
    nt = npad // 32
    hi_tile = nt if hi_tile is None else hi_tile
    n_keys = N - 1 if mutant == "drop_last" else N + 1 if mutant == "admit_pad" else N
    o = torch.zeros(G, npad, HD, dtype=torch.float32)
    m = torch.full((G, npad), -float("inf"), dtype=torch.float32)
    l = torch.zeros(G, npad, dtype=torch.float32)
    for t in range(lo_tile, hi_tile):
        if isinstance(mutant, tuple) and mutant[0] == "skip_tile" and mutant[1] == t:
            continue
        k0 = t * 32
        s = q @ k[:, k0:k0 + 32].transpose(1, 2)                                    # [G, npad, 32] fp32 (exact on the cases' grids)
        dead = torch.arange(k0, k0 + 32) >= min(n_keys, npad)
        s[:, :, dead] = -float("inf")
        mx = s.max(dim=-1).values
        move = (mx > m + LAG).reshape(G, nt, 32).any(dim=-1, keepdim=True).expand(G, nt, 32).reshape(G, npad)
        m_new = torch.where(move, torch.maximum(m, mx), m)
        alpha = torch.where(move, torch.exp2(m - m_new), torch.ones_like(m))
        alpha = torch.where(torch.isnan(alpha), torch.zeros_like(alpha), alpha)      # (-inf) - (-inf): nothing accumulated yet
        l, o, m = l * alpha, o * alpha[..., None], m_new
        p = torch.exp2(s - m[..., None])
        p = torch.where(torch.isnan(p), torch.zeros_like(p), p)
        l = l + p.sum(dim=-1)
        o = o + p.to(lp).to(torch.float32) @ v[:, k0:k0 + 32]
    out = o / l[..., None]
    if out_lp:
        out = out.to(lp).to(torch.float32)
    if mutant == "row_off":
        out = torch.roll(out, 1, dims=1)
    return out[:, :N], m[:, :N], l[:, :N]
