"""The linear-attention kernels of the U-Net stages ONE LAUNCH AT A TIME against a plain fp64 reference of the same operation.

linattn_kvctx_kernel / linattn_kvctx_hw_kernel, linattn_merge_kernel and the three tail kernels (csrc/linattn_fused.hip), and the fp32
mode's linattn_ctx_kernel / linattn_combine_kernel (csrc/linattn.hip), are reached through the test-only shim (tests/kshim), which fills
the library's parameter structs and calls its own launchers.  Every case (tests/linattn_cases.py) asserts the form string the launcher
reports - kernel, C, PRO, FL, ROWS for the context pass, the form of the tail - so a launcher that picks another instantiation fails the
case instead of shrinking coverage.  Per launch: every partial (m, s, ctx) of every block, the fp64 merge of the kernel's partials
against the full reference, Xout as fp32 and as 16 bits, every W2 element at its decoded slot, every y; every element finite, the guard
regions in front of and behind every output bit-identical, every word the launch does not own still the NaN pre-fill; and where the
code comments promise equal bits - head-parallel against 4-wave, rows 1 against 0, wave-split tail against direct - equal bits at the
launch.  Every output element is held to the bound tests/linattn_reference.py derives; nothing is excluded.  Each comparison records
max(err / tol) (profiles/linattn_kernel_parity_measured.jsonl holds a run's lines).

No case skips: the one form a build lacks (the head-parallel context pass at C = 128 with split weights) must be a shim error."""
import os

import numpy as np
import pytest
import torch

from tests import conv_reference as CR
from tests import linattn_cases as K
from tests import linattn_reference as R

pytestmark = pytest.mark.gpu
FILL = 0x7FC07FC0                     # a NaN as fp32 AND as two 16-bit values of either type
GUARD = 0x5A5AA5A5
GUARD_WORDS = 1024
PRECS = K.PRECS


@pytest.fixture
def knobs():
    """The case's DEX_* knobs for one launch (the launcher reads DEX_OUT2_MIN), restored afterwards."""
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


@pytest.fixture(scope="module")
def ks():
    from tests import kshim
    kshim.load()
    return kshim


def _dev():
    return torch.device("cuda", 0)


def _guarded(nwords):
    buf = torch.full((nwords + 2 * GUARD_WORDS,), FILL, dtype=torch.int32, device=_dev())
    buf[:GUARD_WORDS] = GUARD
    buf[GUARD_WORDS + nwords:] = GUARD
    return buf, buf[GUARD_WORDS:GUARD_WORDS + nwords]


def _guards_intact(buf, nwords):
    h = buf.cpu().numpy()
    assert (h[:GUARD_WORDS] == GUARD).all() and (h[GUARD_WORDS + nwords:] == GUARD).all(), "a guard region was written"
    return h[GUARD_WORDS:GUARD_WORDS + nwords]


def _f32(words):
    return torch.from_numpy(words.view(np.float32).copy())


def _lp(words, lp):
    return torch.from_numpy(words.copy()).view(lp)


def _record(tag, ratios):
    from tests import gpu_util
    gpu_util.record(tag, **ratios)
    print(tag, ratios)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert ratios and not bad, (tag, ratios)


_W = {}


def _weights(ks, C, prec, swap_kv=False):
    """The case's weights on the host and packed by the library on the device: Wkv (row-major cast), Wq (fragment order)."""
    key = (C, prec, swap_kv)
    if key not in _W:
        Wqkv, Wout, bout = K.make_weights(C, prec)
        kv = Wqkv[128:]
        if swap_kv:
            kv = torch.cat([kv[128:], kv[:128]])
        wkv, kv_lo = ks.pack("cast", kv.contiguous().to(_dev()), prec)
        wq, q_lo = ks.pack("frag_nk", Wqkv[:128].contiguous().to(_dev()), prec)
        _W[key] = dict(Wqkv=Wqkv, Wout=Wout, bout=bout, wkv=wkv, kv_lo=kv_lo, wq=wq, q_lo=q_lo)
    return _W[key]


class Parts:
    """Guarded, NaN-filled partial buffers of one context-pass launch."""

    def __init__(self, B, nblk):
        self.B, self.nblk = B, nblk
        self.n = (B * 4 * nblk * 32, B * 4 * nblk * 32, B * 4 * nblk * 1024)
        self.bufs = [_guarded(n) for n in self.n]

    def tensors(self):
        return dict(zip(("part_m", "part_s", "part_c"), (b[1].view(torch.float32) for b in self.bufs)))

    def read(self):
        """[(m, s, c)] per block (fp32 on the host) after the guard check, and the raw words."""
        w = [_guards_intact(b[0], n) for b, n in zip(self.bufs, self.n)]
        B, nb = self.B, self.nblk
        m, s, c = _f32(w[0]).reshape(B, 4, nb, 32), _f32(w[1]).reshape(B, 4, nb, 32), _f32(w[2]).reshape(B, 4, nb, 32, 32)
        assert bool(torch.isfinite(m).all() and torch.isfinite(s).all() and torch.isfinite(c).all()), "non-finite partials"
        return [(m[:, :, i], s[:, :, i], c[:, :, i]) for i in range(nb)], np.concatenate(w)


def _partial_checks(got, k, v, npix, nsub, prec, dk=None, dv=None):
    worst = [0.0, 0.0, 0.0]
    refs, tols = [], []
    for (lo, hi), g in zip(R.blocks(npix, nsub), got):
        ref, tol = R.partial(k, v, lo, hi), R.partial_tolerance(k, v, lo, hi, prec, nsub, dk, dv)
        refs.append(ref), tols.append(tol)
        worst = [max(a, b) if b == b else float("nan") for a, b in zip(worst, R.partial_ratios(g, ref, tol, prec))]
    ms, mc = R.merged_ratios(got, refs, tols)
    return dict(m=worst[0], s=worst[1], c=worst[2], merged_s=ms, merged_c=mc)


# ---- context pass, x given --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", K.CS)
@pytest.mark.parametrize("npix,nsub,B", K.CTX_SHAPES)
def test_context_pass(npix, nsub, B, C, prec, ks, knobs):
    knobs({})
    Wt = _weights(ks, C, prec)
    x = K.make_x(C, B, npix)
    _, k, v = R.project(x, Wt["Wqkv"], prec)
    nblk = K.nblk_of(npix, nsub)
    first = None
    for strided in (False, True):
        ldx, x_coff = (2 * C, C) if strided else (C, 0)
        X = torch.full((B, npix, ldx), 1.0e30, dtype=torch.float32)                 # (the other half of a strided row must not be read)
        X[:, :, x_coff:x_coff + C] = x
        X = X.to(_dev())
        for hw, rows in K.CTX_FORMS:
            P = Parts(B, nblk)
            call = lambda: ks.linattn_kvctx(prec, dict(X=X, Wkv=Wt["wkv"], **P.tensors()), npix=npix, C_=C, B=B, nsub=nsub, nblk=nblk,
                                            ldx=ldx, x_coff=x_coff, headwaves=hw, rows=rows, wkv_lo_off=Wt["kv_lo"])
            if hw and not K.hw_supported(C, prec):
                with pytest.raises(ks.ShimError):
                    call()
                continue
            form = call()
            torch.cuda.synchronize()
            assert form == K.kvctx_form(C, hw, rows), form
            got, words = P.read()
            if first is None:
                first = words
                _record(f"linattn:ctx:{npix}x{nsub}x{B}:C{C}:{prec}", _partial_checks(got, k, v, npix, nsub, prec))
            else:                                                                    # the same bits in every form and layout
                assert (words == first).all(), (form, strided, "partials differ from the 4-wave form's")


# ---- context pass, PRO forms -------------------------------------------------------------------------------------------------------
def _run_pro(fl, C, prec, ks, swap_kv=False):
    """H = 40, W = 5 (200 pixels: a ragged last sub-tile, mask zeros inside every sub-tile), B = 2; one flag set - compile-time (odd fl)
    or the run-time-flag form (even fl: fp32 h2) - at mask_ws 1 and 2, with and without a residual (ldres = C + 8), in all three forms.
    Returns the ratios by with / without residual (swap_kv: the negative control, nothing recorded or asserted on them)."""
    Wt = _weights(ks, C, prec, swap_kv)
    lp = ks.LP_DTYPE[prec]
    B, W, npix, nsub = K.PRO_B, K.PRO_W, K.PRO_H * K.PRO_W, 1
    nblk = K.nblk_of(npix, nsub)
    h2_lp, res_lp, xout_lp, under = bool(fl & 1), bool(fl & 2), bool(fl & 4), bool(fl & 8)
    out = {}
    for with_res in (True, False):
        I = K.make_pro(C, prec, fl, with_res)
        fix = CR.encode_stats(I["mean"], I["meansq"], seed=fl)
        mean, meansq = CR.decode_stats(fix)
        x, scale = R.prologue(I["h2"], mean, meansq, I["gamma"], I["beta"], I["res"], K.mask_of(I["cols"], 1), 1, W, under)
        tolx, delta = R.xout_tolerance(x, scale, prec, xout_lp)
        err, share = R.operand_error(x, delta, Wt["Wqkv"][128:], prec)
        assert share <= R.AMB_SHARE_MAX, share
        _, k, v = R.project(x, Wt["Wqkv"], prec)
        t = dict(H2=(I["h2"].to(lp) if h2_lp else I["h2"]).contiguous().to(_dev()), gn_stats=fix.contiguous().to(_dev()),
                 gamma=I["gamma"].to(_dev()), beta=I["beta"].to(_dev()), Wkv=Wt["wkv"])
        ldres = 0
        if with_res:
            ldres = C + 8
            r = torch.full((B, npix, ldres), 3.0e4, dtype=torch.float32)
            r[:, :, :C] = I["res"]
            t["res"] = (r.to(lp) if res_lp else r).contiguous().to(_dev())
        first = None
        for mask_ws in (1, 2):
            t["mask"] = K.mask_of(I["cols"], mask_ws).contiguous().to(_dev())
            for hw, rows in K.CTX_FORMS:
                if hw and not K.hw_supported(C, prec):
                    continue
                P = Parts(B, nblk)
                nx = B * npix * C // (2 if xout_lp else 1)
                xbuf, xo = _guarded(nx)
                form = ks.linattn_kvctx(prec, dict(Xout=xo.view(lp if xout_lp else torch.float32), **t, **P.tensors()), npix=npix, C_=C, B=B,
                                        nsub=nsub, nblk=nblk, headwaves=hw, rows=rows, W=W, mask_ws=mask_ws, mask_bstride=W * mask_ws,
                                        ldres=ldres, res_under_mask=under, h2_bf16=h2_lp, res_lp=res_lp, xout_lp=xout_lp,
                                        wkv_lo_off=Wt["kv_lo"])
                torch.cuda.synchronize()
                assert form == K.kvctx_form(C, hw, rows, True, fl), form
                got, words = P.read()
                xw = _guards_intact(xbuf, nx)
                words = np.concatenate([words, xw])
                if first is None:
                    first = words
                    xg = (_lp(xw, lp) if xout_lp else _f32(xw)).reshape(B, npix, C)
                    assert bool(torch.isfinite(xg.float()).all())
                    ratios = _partial_checks(got, k, v, npix, nsub, prec, err[..., :128], err[..., 128:])
                    ratios["xout"] = R.ratio(xg, x, tolx)
                    out[with_res] = ratios
                    if not swap_kv:
                        _record(f"linattn:pro:fl{fl}:res{int(with_res)}:C{C}:{prec}", ratios)
                else:
                    assert (words == first).all(), (form, mask_ws, "partials or Xout differ from the 4-wave form's")
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", K.CS)
@pytest.mark.parametrize("fl", K.PRO_FLS)
def test_context_pass_with_prologue(fl, C, prec, ks, knobs):
    knobs({})
    _run_pro(fl, C, prec, ks)


# ---- merge ------------------------------------------------------------------------------------------------------------------------
def _run_merge(ks, prec, pm, ps, pc, Wout, C, B):
    nblk = pm.shape[2]
    nw = B * C * 128 // 2
    wbuf, w2 = _guarded(nw)
    form = ks.linattn_merge(prec, dict(part_m=pm.contiguous().to(_dev()), part_s=ps.contiguous().to(_dev()), part_c=pc.contiguous().to(_dev()),
                                       Wout=Wout.contiguous().to(_dev()), g=torch.tensor([K.G], device=_dev()), W2=w2.view(torch.int16)),
                            nblk=nblk, C_=C, B=B)
    torch.cuda.synchronize()
    assert form == K.merge_form(nblk), form
    words = _guards_intact(wbuf, nw)
    vals = _lp(words, ks.LP_DTYPE[prec]).reshape(B, C * 128)
    assert bool(torch.isfinite(vals.float()).all()), "W2 words left unwritten or non-finite"      # every slot is owned: none keeps the fill
    return R.unpack_w2(vals.float(), C), w2


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", K.CS)
@pytest.mark.parametrize("nblk", K.MERGE_NBLK)
def test_merge(nblk, C, prec, ks, knobs):
    knobs({})
    Wt = _weights(ks, C, prec)
    pm, ps, pc = K.make_partials(nblk, 2)
    W2, tol, _ = R.merge_reference(pm, ps, pc, Wt["Wout"], K.G, prec)
    got, _ = _run_merge(ks, prec, pm, ps, pc, Wt["Wout"], C, 2)
    _record(f"linattn:merge:{nblk}:C{C}:{prec}", dict(W2=R.ratio(got, W2, tol)))


# ---- tail -------------------------------------------------------------------------------------------------------------------------
LDY, Y_COFF, LDY2, Y2_COFF = 256, 128, 192, 64


def _run_tail(ks, prec, kind, X, w2, Wt, C, B, npix, ldx=None, x_coff=0, lp_io=False):
    """One tail launch into Y rows of 256 with y_coff = 128 (lp_io: 16-bit X, Y and a Y2 with its own ldy2 / y2_coff).  Returns the y
    words' values [B, npix, C] (and Y2's); the other parts of every row must still be the pre-fill."""
    lp = ks.LP_DTYPE[prec]
    ldx = C if ldx is None else ldx
    ny = B * npix * LDY // (2 if lp_io else 1)
    ybuf, Y = _guarded(ny)
    t = dict(X=X, Wq=Wt["wq"], W2=w2, bias=(K.G * Wt["bout"]).to(_dev()), Y=Y.view(lp if lp_io else torch.float32))
    kw = {}
    if lp_io:
        ny2 = B * npix * LDY2 // 2
        y2buf, Y2 = _guarded(ny2)
        t["Y2"] = Y2.view(lp)
        kw = dict(ldy2=LDY2, y2_coff=Y2_COFF, x_lp=True, y_lp=True)
    form = ks.linattn_out2(prec, t, npix=npix, C_=C, B=B, ldx=ldx, x_coff=x_coff, ldy=LDY, y_coff=Y_COFF, hw=kind.startswith("hw"),
                           rows=kind == "hw1", wq_lo_off=Wt["q_lo"], **kw)
    torch.cuda.synchronize()
    assert form == K.tail_form(C, "throughput" if lp_io else kind), form

    def rows_of(buf, n, ld, coff):
        w = _guards_intact(buf, n)
        vals = (_lp(w, lp) if lp_io else _f32(w)).reshape(B, npix, ld)
        raw = torch.from_numpy(w.copy()).view(torch.int16 if lp_io else torch.int32).reshape(B, npix, ld)
        own = torch.zeros(ld, dtype=torch.bool)
        own[coff:coff + C] = True
        fill = FILL & 0xFFFF if lp_io else FILL
        assert bool((raw[:, :, ~own] == fill).all()), "a word outside the y columns was written"
        y = vals[:, :, coff:coff + C]
        assert bool(torch.isfinite(y.float()).all()), "non-finite or unwritten y"
        return y
    y = rows_of(ybuf, ny, LDY, Y_COFF)
    return (y, rows_of(y2buf, ny2, LDY2, Y2_COFF)) if lp_io else (y, None)


def _w2_device(W2h, prec, ks, permute=True):
    return R.pack_w2(W2h, permute).to(ks.LP_DTYPE[prec]).contiguous().to(_dev())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", K.CS)
@pytest.mark.parametrize("npix,B", [(n, b) for n in K.TAIL_NPIX for b in K.TAIL_B])
def test_tail(npix, B, C, prec, ks, knobs):
    Wt = _weights(ks, C, prec)
    lp = ks.LP_DTYPE[prec]
    x, W2h = K.make_x(C, B, npix), K.make_w2(C, B, prec)
    w2 = _w2_device(W2h, prec, ks)
    y, tol, _ = R.tail_reference(x, Wt["Wqkv"][:128], W2h, K.G * Wt["bout"], prec)
    Xd = x.contiguous().to(_dev())
    Xs = torch.full((B, npix, 2 * C), 1.0e30)
    Xs[:, :, C:] = x
    Xs = Xs.to(_dev())
    ratios, bits = {}, {}
    for kind in ("direct", "hw0", "hw1", "throughput"):
        knobs({"DEX_OUT2_MIN": 1} if kind == "throughput" else {})
        strided = kind in ("throughput", "hw1")
        got, _ = _run_tail(ks, prec, kind, Xs if strided else Xd, w2, Wt, C, B, npix, ldx=2 * C if strided else C, x_coff=C if strided else 0)
        ratios[kind] = R.ratio(got, y, tol)
        bits[kind] = got.view(torch.int32)
    assert torch.equal(bits["hw0"], bits["direct"]) and torch.equal(bits["hw1"], bits["direct"]), "the wave-split tail's bits differ from the direct form's"
    # 16-bit X, Y and Y2 (throughput form): x IS the stored 16-bit value, also as the residual
    xh = x.to(lp)
    yl, _, tol_lp = R.tail_reference(xh.float(), Wt["Wqkv"][:128], W2h, K.G * Wt["bout"], prec)
    knobs({"DEX_OUT2_MIN": 1})
    gy, gy2 = _run_tail(ks, prec, "throughput", xh.contiguous().to(_dev()), w2, Wt, C, B, npix, lp_io=True)
    ratios["y_lp"], ratios["y2"] = R.ratio(gy.float(), yl, tol_lp), R.ratio(gy2.float(), yl, tol_lp)
    assert torch.equal(gy.view(torch.int16), gy2.view(torch.int16))                  # one rounding of the same fp32 value
    _record(f"linattn:tail:{npix}x{B}:C{C}:{prec}", ratios)


# ---- the three launches chained ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", K.CS)
def test_chain(C, prec, ks, knobs):
    """The kernel's own partials to its merge, that W2 to its tail, against the full reference with the composed bound; and the
    library's packs of Wq and Wkv against the layouts the reference states."""
    knobs({})
    Wt = _weights(ks, C, prec)
    lp = ks.LP_DTYPE[prec]
    npix, nsub, B = K.CHAIN["npix"], K.CHAIN["nsub"], K.CHAIN["B"]
    nblk = K.nblk_of(npix, nsub)
    Wqkv = Wt["Wqkv"].double()
    hi = CR.round_lp(Wqkv, prec)
    halves = [hi] + ([CR.round_lp(Wqkv - hi, prec)] if prec == "fp16x2" else [])
    for i, h in enumerate(halves):                                                   # the split mode's lo half behind the hi half
        want_q = R.pack_wq(h[:128]).to(lp).view(torch.int16)
        assert torch.equal(Wt["wq"][i * Wt["q_lo"]:i * Wt["q_lo"] + 128 * C].cpu(), want_q), "launch_pack_lp_frag_nk layout"
        want_kv = h[128:].reshape(-1).to(lp).view(torch.int16)
        assert torch.equal(Wt["wkv"][i * Wt["kv_lo"]:i * Wt["kv_lo"] + 256 * C].cpu(), want_kv), "row-major cast"
    x = K.make_x(C, B, npix)
    q, k, v = R.project(x, Wqkv, prec)
    X = x.contiguous().to(_dev())
    P = Parts(B, nblk)
    ks.linattn_kvctx(prec, dict(X=X, Wkv=Wt["wkv"], **P.tensors()), npix=npix, C_=C, B=B, nsub=nsub, nblk=nblk, ldx=C, wkv_lo_off=Wt["kv_lo"])
    torch.cuda.synchronize()
    got, _ = P.read()
    ratios = _partial_checks(got, k, v, npix, nsub, prec)
    pm, ps, pc = (torch.stack([g[i] for g in got], dim=2) for i in range(3))
    W2k, tolk, _ = R.merge_reference(pm, ps, pc, Wt["Wout"], K.G, prec)               # the merge of the kernel's OWN partials
    W2g, w2dev = _run_merge(ks, prec, pm, ps, pc, Wt["Wout"], C, B)
    ratios["W2_own"] = R.ratio(W2g, W2k, tolk)
    # W2 against the full reference: the partials' merged bounds carried through the normalisation and Wout
    M, S, Cx, _ = R.partial(k, v)
    tols = [R.partial_tolerance(k, v, lo, hi_, prec, nsub) for lo, hi_ in R.blocks(npix, nsub)]
    refs = [R.partial(k, v, lo, hi_) for lo, hi_ in R.blocks(npix, nsub)]
    w = [torch.exp(p[0] - M) for p in refs]
    ts, tc = sum(wi * t[1] for wi, t in zip(w, tols)), sum(wi[..., None] * t[2] for wi, t in zip(w, tols))
    ctx = Cx / S[..., None]
    dctx = (tc + ctx.abs() * ts[..., None]) / (S - ts)[..., None]
    W2t, _ = R.w2_of(ctx, Wt["Wout"], K.G)
    dW2, _ = R.w2_of(dctx, Wt["Wout"].abs(), K.G)
    dW2 = dW2 + tolk
    ratios["W2"] = R.ratio(W2g, W2t, dW2)
    y_own, tol_own, _ = R.tail_reference(x, Wqkv[:128], W2g, K.G * Wt["bout"], prec)
    y_full, tol_full, _ = R.tail_reference(x, Wqkv[:128], W2t, K.G * Wt["bout"], prec, dW2=dW2)
    yg, _ = _run_tail(ks, prec, "direct", X, w2dev.view(lp), Wt, C, B, npix)
    ratios["y_own"], ratios["y"] = R.ratio(yg, y_own, tol_own), R.ratio(yg, y_full, tol_full)
    _record(f"linattn:chain:C{C}:{prec}", ratios)


# ---- fp32 mode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.FP32_N)
def test_fp32_context_and_combine(n, ks, knobs):
    knobs({})
    B, chunk = 2, 512
    nch = (n + chunk - 1) // chunk
    qkv = K.make_qkv(n, B)
    k, v = qkv[..., 128:256].double(), qkv[..., 256:].double()
    P = Parts(B, nch)
    form = ks.linattn_ctx(dict(qkv=qkv.contiguous().to(_dev()), **P.tensors()), n=n, B=B)
    torch.cuda.synchronize()
    assert form == "linattn_ctx_kernel"
    got, _ = P.read()
    worst = [0.0, 0.0, 0.0]
    for c, g in enumerate(got):
        lo, hi = c * chunk, min(n, (c + 1) * chunk)
        tol = R.partial_tolerance(k, v, lo, hi, None, 0, fp32_mode=True, chunk_subtiles=4)
        worst = [max(a, b) if b == b else float("nan") for a, b in zip(worst, R.partial_ratios(g, R.partial(k, v, lo, hi), tol, None))]
    ratios = dict(m=worst[0], s=worst[1], c=worst[2])
    pm, ps, pc = (torch.stack([g[i] for g in got], dim=2) for i in range(3))
    for C in K.CS:
        _, Wout, _ = K.make_weights(C, "bf16")
        W2, tol, _ = R.merge_reference(pm, ps, pc, Wout, K.G, None, combine=True)
        nw = B * 128 * C
        wbuf, we = _guarded(nw)
        form = ks.linattn_combine(dict(part_m=pm.contiguous().to(_dev()), part_s=ps.contiguous().to(_dev()), part_c=pc.contiguous().to(_dev()),
                                       Wout=Wout.contiguous().to(_dev()), g=torch.tensor([K.G], device=_dev()), Weff=we.view(torch.float32)),
                                  nchunks=nch, C_=C, B=B)
        torch.cuda.synchronize()
        assert form == "linattn_combine_kernel"
        Weff = _f32(_guards_intact(wbuf, nw)).reshape(B, 128, C)
        assert bool(torch.isfinite(Weff).all())
        ratios[f"Weff{C}"] = R.ratio(Weff.transpose(1, 2), W2, tol)
    _record(f"linattn:fp32:{n}", ratios)


# ---- negative controls, forms, rejects ----------------------------------------------------------------------------------------------
def test_w2_without_the_permutation_breaks_the_bound(ks, knobs):
    """Negative control of this file's own decoding and comparison, on the device: the tail on a W2 packed in plain fragment order
    computes a wrong (finite, in-bounds) y, far outside the bound; the columns the launch does not own stay untouched."""
    knobs({})
    C, B, npix, prec = 64, 1, 129, "bf16"
    Wt = _weights(ks, C, prec)
    x, W2h = K.make_x(C, B, npix), K.make_w2(C, B, prec)
    y, tol, _ = R.tail_reference(x, Wt["Wqkv"][:128], W2h, K.G * Wt["bout"], prec)
    good, _ = _run_tail(ks, prec, "direct", x.contiguous().to(_dev()), _w2_device(W2h, prec, ks), Wt, C, B, npix)
    bad, _ = _run_tail(ks, prec, "direct", x.contiguous().to(_dev()), _w2_device(W2h, prec, ks, permute=False), Wt, C, B, npix)
    assert R.ratio(good, y, tol) <= 1.0 and R.ratio(bad, y, tol) > 10.0


def test_swapped_k_and_v_rows_break_the_bound(ks, knobs):
    """Wkv with the k and the v row blocks swapped: every partial lands far outside, Xout - which no weight touches - stays inside."""
    knobs({})
    out = _run_pro(9, 64, "bf16", ks, swap_kv=True)
    for r in out.values():
        assert r["xout"] <= 1.0 and r["c"] > 10.0 and r["s"] > 10.0 and r["m"] > 10.0, r


@pytest.mark.parametrize("prec", PRECS)
def test_cases_name_every_instantiation(prec):
    """The form strings the cases above assert, collected the way they build them, are the launchers' whole set (the CPU test holds that
    set against the source)."""
    named = {K.merge_form(n) for n in K.MERGE_NBLK}
    for C in K.CS:
        for hw, rows in K.CTX_FORMS:
            if hw and not K.hw_supported(C, prec):
                continue
            named.add(K.kvctx_form(C, hw, rows))
            named |= {K.kvctx_form(C, hw, rows, True, fl) for fl in K.PRO_FLS}
        named |= {K.tail_form(C, kind) for kind in ("direct", "hw0", "hw1", "throughput")}
    assert named == K.expected_forms(prec)


def test_shim_rejects_descriptors_outside_the_launchers_contract(ks, knobs):
    """Every descriptor outside what the launchers document is an error code, never a launch."""
    knobs({})
    d = _dev()
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=d)

    def kv(prec="bf16", C=64, npix=200, B=1, nsub=1, nblk=None, pro=False, **kw):
        nblk = K.nblk_of(max(npix, 1), nsub) if nblk is None else nblk
        t = dict(Wkv=z(2 * 256 * C, torch.int16), part_m=z(B * 4 * nblk * 32), part_s=z(B * 4 * nblk * 32), part_c=z(B * 4 * nblk * 1024))
        if pro:
            t.update(H2=z(B * max(npix, 1) * C), gn_stats=z(B * 8 * 32 * 2, torch.int64), gamma=z(C), beta=z(C), mask=z(64), Xout=z(B * max(npix, 1) * C))
            kw.setdefault("mask_ws", 1)
        else:
            t["X"] = z(B * max(npix, 1) * C)
            kw.setdefault("ldx", C)
        return ks.linattn_kvctx(prec, t, npix=npix, C_=C, B=B, nsub=nsub, nblk=nblk, wkv_lo_off=256 * C if prec == "fp16x2" else 0, **kw)

    def out2(prec="bf16", C=64, npix=200, B=1, **kw):
        t = dict(X=z(B * max(npix, 1) * C, kw.pop("xdt", torch.float32)), Wq=z(2 * 128 * C, torch.int16), W2=z(B * C * 128, torch.int16), bias=z(C),
                 Y=z(B * max(npix, 1) * C))
        return ks.linattn_out2(prec, t, npix=npix, C_=C, B=B, ldx=C, ldy=C, wq_lo_off=128 * C if prec == "fp16x2" else 0, **kw)

    bad = [lambda: kv(C=96), lambda: kv(C=256), lambda: out2(C=32),                   # C not 64 or 128
           lambda: kv(nblk=3), lambda: kv(npix=300, nsub=2, nblk=3), lambda: kv(nsub=9, nblk=1),      # nblk != ceil(npix / (128 nsub))
           lambda: kv(prec="fp16x2", C=128, headwaves=True),                         # no head-parallel form in the split build at C = 128
           lambda: kv(npix=0, nblk=1), lambda: out2(npix=0),                          # npix <= 0
           lambda: kv(pro=True, W=7), lambda: kv(pro=True, W=0),                      # W does not divide npix in a PRO launch
           lambda: kv(rows=True),                                                     # rows without the head-parallel form
           lambda: kv(xout_lp=True), lambda: kv(W=5),                                 # PRO members without H2
           lambda: kv(ldx=60), lambda: kv(ldx=66, x_coff=2),                          # rows narrower than C / unaligned
           lambda: out2(hw=True, x_lp=True, xdt=torch.bfloat16), lambda: out2(hw=True, y_lp=True),    # hw together with 16-bit I/O
           lambda: out2(rows=True),
           lambda: out2(y_lp=True)]                                                   # 16-bit Y where the direct form would run
    for i, f in enumerate(bad):
        with pytest.raises(ks.ShimError):
            f()
            raise AssertionError(f"descriptor {i} was launched")
    with pytest.raises(ks.ShimError):                                                # partials shorter than the descriptor implies
        ks.linattn_kvctx("bf16", dict(X=z(200 * 64), Wkv=z(256 * 64, torch.int16), part_m=z(2 * 4 * 32 - 1), part_s=z(2 * 4 * 32), part_c=z(2 * 4 * 1024)),
                         npix=200, C_=64, B=1, nsub=1, nblk=2, ldx=64)
    with pytest.raises(ks.ShimError):
        ks.linattn_merge("bf16", dict(part_m=z(4 * 32), part_s=z(4 * 32), part_c=z(4 * 1024), Wout=z(64 * 128), g=z(1), W2=z(64 * 128 - 1, torch.int16)),
                         nblk=1, C_=64, B=1)
    with pytest.raises(ks.ShimError):
        ks.linattn_ctx(dict(qkv=z(300 * 384), part_m=z(4 * 32), part_s=z(4 * 32), part_c=z(4 * 1024)), n=300, B=1, nchunks=2)
    assert kv() == K.kvctx_form(64, False, False) and out2() == K.tail_form(64, "direct")     # (the helpers themselves are valid)
    torch.cuda.synchronize()


def test_device_reference_agrees_with_cpu():
    """The same reference functions on the device in fp64 against the CPU's."""
    Wqkv, _, _ = K.make_weights(64, "fp16x2")
    x = K.make_x(64, 2, 300)
    _, k, v = R.project(x, Wqkv, "fp16x2")
    _, kd, vd = R.project(x.to(_dev()), Wqkv.to(_dev()), "fp16x2")
    assert torch.equal(k, kd.cpu()) and torch.equal(v, vd.cpu())
    cpu, dev = R.partial(k, v, 128, 300), R.partial(kd, vd, 128, 300)
    for a, b in zip(cpu, dev):
        assert ((a - b.cpu()).abs() / a.abs().clamp(min=1e-300)).max().item() <= 1e-12 or (a - b.cpu()).abs().max().item() <= 1e-12 * a.abs().max().item()
