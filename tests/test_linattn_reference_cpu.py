"""CPU checks of the linear-attention per-launch reference (tests/linattn_reference.py) and cases (tests/linattn_cases.py): the layouts
against an emulated MFMA contraction, the grid properties the bounds rest on, the collapsed algebra against the textbook form, an fp32 /
16-bit emulation of every kernel inside the bound at every case shape and mode - and mutants of that emulation OUTSIDE it: the bound's
sharpness is part of what is tested."""
import os
import re

import pytest
import torch

from tests import conv_reference as CR
from tests import linattn_cases as K
from tests import linattn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- layouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", K.CS)
def test_packers_round_trip(C):
    W2 = torch.arange(2 * C * 128, dtype=torch.float64).reshape(2, C, 128)
    assert torch.equal(R.unpack_w2(R.pack_w2(W2), C), W2)
    assert not torch.equal(R.unpack_w2(R.pack_w2(W2, permute=False), C), W2)
    Wq = torch.arange(128 * C, dtype=torch.float64).reshape(128, C)
    assert torch.equal(R.unpack_wq(R.pack_wq(Wq), C), Wq)


@pytest.mark.parametrize("C", K.CS)
def test_packers_against_the_mfma_contraction(C):
    """The tail's two chained GEMMs on lane-held fragments read from the packed Wq and W2 exactly as the kernels index them:
    q^T tile t = sum_ks mfma(Wq fragment (t, ks), x fragment ks); its accumulator registers, eight at a time, ARE the B fragments of
    K-steps 2 t and 2 t + 1 of the second GEMM, whose A fragments are W2's (ct, ks).  The result must be W2 (Wq x)."""
    g = torch.Generator().manual_seed(C)
    Wq = torch.randn(128, C, generator=g, dtype=torch.float64)
    W2 = torch.randn(1, C, 128, generator=g, dtype=torch.float64)
    x = torch.randn(32, C, generator=g, dtype=torch.float64)                        # 32 pixels of one wave
    wqf = R.pack_wq(Wq).reshape(4, C // 16, 64, 8)
    w2f = R.pack_w2(W2)[0].reshape(C // 32, 8, 64, 8)
    lane = torch.arange(64)
    i, hh = lane & 31, lane >> 5
    xf = [torch.stack([x[i[l], ks * 16 + 8 * hh[l]:ks * 16 + 8 * hh[l] + 8] for l in range(64)]) for ks in range(C // 16)]
    qf = []
    for t in range(4):
        q = sum(R.mfma_32x32x16(wqf[t, ks], xf[ks]) for ks in range(C // 16))       # q^T[he = 32 t + row][px = col]
        for k2 in range(2):                                                          # registers 8 k2 .. 8 k2 + 7 of every lane
            qf.append(torch.stack([torch.stack([q[R.acc_row(8 * k2 + j, int(hh[l])), int(i[l])] for j in range(8)]) for l in range(64)]))
    y = torch.cat([sum(R.mfma_32x32x16(w2f[ct, ks], qf[ks]) for ks in range(8)) for ct in range(C // 32)])    # y^T [co][px]
    want = W2[0] @ (Wq @ x.T)
    assert (y - want).abs().max() <= 1e-9 * want.abs().max()


def test_context_fragments_are_the_accumulators():
    """kv_head_step's second MFMA takes the k and v accumulator registers as its B and A fragments: register r of lane (i, hh) holds
    pixel acc_row(r, hh) of channel i in both, so ctx^T[e][d] = sum_px v[px][e] p[px][d] with no shuffle."""
    g = torch.Generator().manual_seed(1)
    p, v = torch.randn(32, 32, generator=g, dtype=torch.float64), torch.randn(32, 32, generator=g, dtype=torch.float64)     # [px][channel]
    ctxT = torch.zeros(32, 32, dtype=torch.float64)
    for k2 in range(2):
        va = torch.stack([torch.stack([v[R.acc_row(8 * k2 + j, l >> 5), l & 31] for j in range(8)]) for l in range(64)])
        pb = torch.stack([torch.stack([p[R.acc_row(8 * k2 + j, l >> 5), l & 31] for j in range(8)]) for l in range(64)])
        ctxT += R.mfma_32x32x16(va, pb)
    assert (ctxT - v.T @ p).abs().max() <= 1e-12


# ---- the operation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", K.CS)
def test_collapsed_form_is_the_textbook_form(C):
    Wqkv, Wout, bout = K.make_weights(C, "fp16x2")
    x = K.make_x(C, 2, 77)
    a, b = R.textbook(x, Wqkv, Wout, bout, K.G), R.collapsed(x, Wqkv, Wout, bout, K.G)
    assert (a - b).abs().max() <= 1e-12 * a.abs().max()


def _row_grid(w):
    """Per row the power-of-two grid its non-zero weights lie on."""
    out = torch.ones(w.shape[0], dtype=torch.float64)
    w = w.double()
    for e in range(1, 25):
        off = ((w * 2.0 ** (e - 1)).round() != w * 2.0 ** (e - 1)).any(dim=1)
        out = torch.where(off, torch.full_like(out, 2.0 ** -e), out)
    assert bool(((w / out[:, None]).round() == w / out[:, None]).all())
    return out


@pytest.mark.parametrize("C", K.CS)
@pytest.mark.parametrize("prec", K.PRECS)
def test_operands_lie_on_the_grids_the_bounds_assume(C, prec):
    Wqkv, _, _ = K.make_weights(C, prec)
    wh = CR.split_weights(Wqkv.double(), prec)
    assert torch.equal(wh, Wqkv.double())                                           # the MFMAs see the weight itself (hi, or hi + lo)
    if prec == "fp16x2":
        lo = Wqkv.double() - CR.round_lp(Wqkv.double(), prec)
        plain = (Wqkv.abs() != 0.5) & (Wqkv != 0)
        assert bool((lo[plain] != 0).all())                                         # non-zero lo halves: a mis-indexed lo image is an error
    gw = _row_grid(Wqkv)
    for npix, nsub, B in K.CTX_SHAPES:
        x = K.make_x(C, B, npix)
        xh = CR.round_lp(x.double(), prec)
        assert bool(((xh / R.X_GRID).round() == xh / R.X_GRID).all() and (xh.abs() <= 1).all())
        assert bool(((x.double() - xh).abs() <= xh.abs() * 2.0 ** -13).all())
        assert bool((x.double() != xh)[xh != 0].all())                              # the fp32 x and its rounding differ wherever x^ != 0
        mag = xh.abs() @ Wqkv.double().abs().T                                      # every partial sum of a row is below this
        assert bool((mag < 2.0 ** 24 * R.X_GRID * gw).all()), (C, prec, npix)      # 24 bits hold it: fp32 accumulates exactly
        q, k, v = R.project(x, Wqkv, prec)
        for t in (q, k, v):
            assert torch.equal(t.float().double(), t)
        if prec != "bf16":                                                          # no v is subnormal in fp16 unless it is exact there
            assert torch.equal(CR.round_lp(v, prec)[v.abs() < 2.0 ** -14], v[v.abs() < 2.0 ** -14])


@pytest.mark.parametrize("npix,nsub,B", K.CTX_SHAPES)
def test_blocks_cover_every_pixel_once_and_merge_to_the_full_reference(npix, nsub, B):
    bl = R.blocks(npix, nsub)
    assert len(bl) == K.nblk_of(npix, nsub)
    seen = torch.zeros(npix, dtype=torch.int32)
    for lo, hi in bl:
        seen[lo:hi] += 1
    assert bool((seen == 1).all())
    Wqkv, _, _ = K.make_weights(64, "bf16")
    _, k, v = R.project(K.make_x(64, B, npix), Wqkv, "bf16")
    M, S, Cx = R.merge([R.partial(k, v, lo, hi)[:3] for lo, hi in bl])
    Mf, Sf, Cf, _ = R.partial(k, v)
    assert torch.equal(M, Mf)
    assert ((S - Sf).abs() / Sf).max() <= 1e-12 and ((Cx - Cf).abs().max() / Cf.abs().max()) <= 1e-12


# ---- emulation inside the bound, mutants outside --------------------------------------------------------------------------------
def _ctx_ratios(C, prec, npix, nsub, B, mutant=None):
    Wqkv, _, _ = K.make_weights(C, prec)
    x = K.make_x(C, B, npix)
    _, k, v = R.project(x, Wqkv, prec)
    got = R.emulate_kvctx(x, Wqkv[128:], npix, nsub, prec, mutant)
    worst = [0.0, 0.0, 0.0]
    refs, tols = [], []
    for (lo, hi), g in zip(R.blocks(npix, nsub), got):
        ref, tol = R.partial(k, v, lo, hi), R.partial_tolerance(k, v, lo, hi, prec, nsub)
        refs.append(ref), tols.append(tol)
        worst = [max(a, b) for a, b in zip(worst, R.partial_ratios(g, ref, tol, prec))]
    return dict(m=worst[0], s=worst[1], c=worst[2], merged=max(R.merged_ratios(got, refs, tols)))


@pytest.mark.parametrize("npix,nsub,B", K.CTX_SHAPES)
@pytest.mark.parametrize("C", K.CS)
@pytest.mark.parametrize("prec", K.PRECS)
def test_context_pass_emulation_is_inside_the_bound(npix, nsub, B, C, prec):
    r = _ctx_ratios(C, prec, npix, nsub, B)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("mutant,prec,key", [("s_no_rescale", "bf16", "s"), ("s_no_rescale", "fp16", "s"), ("no_inf", "bf16", "c"),
                                             ("no_inf", "fp16x2", "s"), ("no_kshift", "fp16", "c"), ("no_kshift", "fp16x2", "c")])
def test_context_pass_mutants_break_the_bound(mutant, prec, key):
    """Rescaling ctx but not s; admitting the clamped rows past npix (no -inf); no KSHIFT in fp16 on the spike channel, whose other
    pixels sit 16 below the maximum and are subnormal as fp16 without the shift."""
    r = _ctx_ratios(64, prec, 1000, 3, 1, mutant)
    assert r[key] > 1.0, r
    if mutant == "no_kshift":
        assert r["m"] > 1.0, r                                                      # m itself leaves its window


@pytest.mark.parametrize("nblk", K.MERGE_NBLK)
@pytest.mark.parametrize("prec", K.PRECS)
def test_merge_emulation_is_inside_the_bound_and_unweighted_is_not(nblk, prec):
    _, Wout, _ = K.make_weights(64, prec)
    pm, ps, pc = K.make_partials(nblk, 2)
    W2, tol, _ = R.merge_reference(pm, ps, pc, Wout, K.G, prec)
    assert R.ratio(R.emulate_merge(pm, ps, pc, Wout, K.G, prec), W2, tol) <= 1.0
    if nblk > 1:
        assert R.ratio(R.emulate_merge(pm, ps, pc, Wout, K.G, prec, "unweighted"), W2, tol) > 1.0


@pytest.mark.parametrize("prec", K.PRECS)
def test_w2_without_the_permutation_breaks_the_bound(prec):
    _, Wout, _ = K.make_weights(64, prec)
    pm, ps, pc = K.make_partials(9, 2)
    W2, tol, _ = R.merge_reference(pm, ps, pc, Wout, K.G, prec)
    got = R.emulate_merge(pm, ps, pc, Wout, K.G, prec)
    assert R.ratio(R.unpack_w2(R.pack_w2(got, permute=False), 64), W2, tol) > 10.0


@pytest.mark.parametrize("npix,B", [(n, b) for n in K.TAIL_NPIX for b in K.TAIL_B])
@pytest.mark.parametrize("C", K.CS)
@pytest.mark.parametrize("prec", K.PRECS)
def test_tail_emulation_is_inside_the_bound_and_its_mutants_are_not(npix, B, C, prec):
    Wqkv, _, bout = K.make_weights(C, prec)
    x, W2h = K.make_x(C, B, npix), K.make_w2(C, B, prec)
    y, tol, tol_lp = R.tail_reference(x, Wqkv[:128], W2h, K.G * bout, prec)
    assert R.ratio(R.emulate_tail(x, Wqkv[:128], W2h, K.G * bout, prec), y, tol) <= 1.0
    assert R.ratio(R.emulate_tail(x, Wqkv[:128], W2h, K.G * bout, prec, y_lp=True), y, tol_lp) <= 1.0
    assert R.ratio(R.emulate_tail(x, Wqkv[:128], W2h, K.G * bout, prec, mutant="res_rounded"), y, tol) > 1.0     # residual from x^
    assert R.ratio(R.emulate_tail(x, Wqkv[:128], W2h, K.G * K.G * bout, prec), y, tol) > 1.0                     # bias scaled twice by g
    if prec == "fp16x2" and npix >= 33:                                                                          # lo image dropped
        hi = CR.round_lp(Wqkv[:128].double(), prec).float()
        assert R.ratio(R.emulate_tail(x, hi, W2h, K.G * bout, prec), y, tol) > 1.0


@pytest.mark.parametrize("C", K.CS)
@pytest.mark.parametrize("prec", K.PRECS)
def test_prologue_ambiguity_share_is_small(C, prec):
    """The PRO launches' operand bound may call an x ambiguous (within delta of a 16-bit rounding boundary); the share is capped as in the
    conv test, so the ambiguity set cannot hide a failure."""
    Wqkv, _, _ = K.make_weights(C, prec)
    for fl in (1, 14):
        P = K.make_pro(C, prec, fl, True)
        x, scale = R.prologue(P["h2"], P["mean"], P["meansq"], P["gamma"], P["beta"], P["res"], K.mask_of(P["cols"], 2), 2, K.PRO_W, bool(fl & 8))
        _, delta = R.xout_tolerance(x, scale, prec, False)
        _, share = R.operand_error(x, delta, Wqkv[128:], prec)
        assert share <= R.AMB_SHARE_MAX, share
        x32, _ = R.prologue(P["h2"].float(), P["mean"].float(), P["meansq"].float(), P["gamma"], P["beta"], P["res"], K.mask_of(P["cols"], 2), 2, K.PRO_W, bool(fl & 8))
        assert bool(torch.isfinite(x32).all())


# ---- every instantiation has a case ---------------------------------------------------------------------------------------------
def test_every_instantiation_of_the_launchers_is_named_by_a_case():
    """The launchers' switch statements, read from the source: the FL values they instantiate and every form string they report must be
    the set the cases assert (tests/linattn_cases.py: expected_forms) - a new instantiation without a case fails here."""
    src = open(os.path.join(ROOT, "dex_tts_amd", "csrc", "linattn_fused.hip")).read()
    for macro in ("KVCTX_CASE\\(CC, ", "KVHW_CASE\\("):
        line = [l for l in src.splitlines() if re.search(macro + r"\d", l) and "#define" not in l][0]
        assert sorted(int(n) for n in re.findall(macro + r"(\d+)\)", line)) == sorted(f for f in K.PRO_FLS if f % 2), line
    named = set(re.findall(r'"(linattn_out2[a-z_0-9]*kernel C=[^"]*)"', src))
    for kern, rws in (("linattn_kvctx_kernel", ("",)), ("linattn_kvctx_hw_kernel", (" ROWS=0", " ROWS=1"))):
        assert f'"{kern}"' in src
        for C in K.CS:
            for rw in rws:
                named |= {f"{kern} C={C} PRO=0 FL=-1{rw}", f"{kern} C={C} PRO=1 FL=-1{rw}"} | {f"{kern} C={C} PRO=1 FL={f}{rw}" for f in range(1, 16, 2)}
    merges = {K.merge_form(n) for n in K.MERGE_NBLK}
    assert merges == {f"linattn_merge_kernel merge_fold<{m}>" for m in re.findall(r"merge_fold<(\d+)>\(p,", src)}
    assert K.expected_forms("bf16") == named | merges
    assert K.expected_forms("fp16x2") == {f for f in named if not f.startswith("linattn_kvctx_hw_kernel C=128")} | merges
