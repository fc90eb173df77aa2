"""The fused DiT row chain ONE LAUNCH AT A TIME against a plain fp64 reference of the same operation.

dit_rowchain_kernel<false / true>, dit_rowchain64_kernel, dit_rowchain64a_kernel and the three dit_rowchain_cluster_kernel
instantiations (csrc/dit_rowchain.hip) are reached through the test-only shim (tests/kshim), which fills DitChainP and calls the
library's own launch_dit_rowchain.  Each case (tests/rowchain_cases.py) asserts the form string the launcher reports, so a launcher
that re-plans fails the case instead of shrinking coverage.  Per case and mode:

    x2 (X rows < N)      every element within the hard bound of tests/rowchain_reference.py, and the rms error within RATIO_MAX of the
                         fp32 evaluation's - over the whole output, per 32-column tile and per row tile; bitwise unchanged in a
                         qkv_only launch
    q / k / v (rows < N) within the sharp single-stage bound anchored on the x2 the launch itself wrote
    pad rows             finite where the form owns them; every word no tile owns, and all three buffers of a last-block launch,
                         still the NaN pre-fill
    guards               the 1024-word regions around X, O, ml, Qh / Kh / Vt (and the cluster slabs and flags) bit-identical
    cluster forms        xerr == 0, and a second launch with the next epoch from the same inputs gives the same bits

Each comparison records max(err / tol) and the three ratios (profiles/rowchain_kernel_parity_measured.jsonl holds a run's lines).
No case skips: every mode's build has every form."""
import os

import numpy as np
import pytest
import torch

from tests import attn_reference as AR
from tests import rowchain_cases as K
from tests import rowchain_reference as R

pytestmark = pytest.mark.gpu
FILL = 0x7FC07FC0                     # a NaN as fp32 AND as two 16-bit values of either type
GUARD = 0x5A5AA5A5
GUARD_WORDS = 1024
NAN = float("nan")


@pytest.fixture
def knobs():
    """The case's DEX_* knobs for one launch (the launcher reads the environment outside a C-ABI call), restored afterwards."""
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


def _guarded(nwords, fill=FILL):
    buf = torch.full((nwords + 2 * GUARD_WORDS,), fill, dtype=torch.int32, device=_dev())
    buf[:GUARD_WORDS] = GUARD
    buf[GUARD_WORDS + nwords:] = GUARD
    return buf, buf[GUARD_WORDS:GUARD_WORDS + nwords]


def _guards_intact(buf, nwords, what):
    h = buf.cpu().numpy()
    assert (h[:GUARD_WORDS] == GUARD).all() and (h[GUARD_WORDS + nwords:] == GUARD).all(), f"a guard region of {what} was written"
    return h[GUARD_WORDS:GUARD_WORDS + nwords]


def _put(view, t, dtype=torch.float32):
    """Copy values into (the front of) a guarded int32 view, as `dtype` elements."""
    flat = t.to(dtype).contiguous().reshape(-1)
    view.view(dtype)[:flat.numel()] = flat.to(_dev())


_SHARED = {}


def _shared(prec, ks, zero_lo=False):
    """Device side of K.shared_weights(): the four packs of the mode (hi, then lo in fp16x2), biases and conditioning tables."""
    key = (prec, zero_lo)
    if key not in _SHARED:
        w = K.shared_weights()
        d = {}
        for k in ("Wp", "W1", "W2", "Wq"):
            pack, lo_off = ks.pack("frag", w[k].to(torch.float32).contiguous().to(_dev()), prec)
            if zero_lo:
                assert prec == "fp16x2" and lo_off == w[k].numel()
                pack[lo_off:] = 0
            d[k] = pack
        for k in ("bp", "b1", "b2", "bq"):
            d[k] = w[k].to(torch.float32).to(_dev())
        d["ada"] = w["ada"].to(torch.float32).reshape(K.N_STEPS, 6 * 256).contiguous().to(_dev())
        for k in ("next_shift", "next_scale"):                          # rows NEXT_STRIDE apart, NaN between them
            t = torch.full((K.N_STEPS, K.NEXT_STRIDE), NAN, dtype=torch.float32)
            t[:, :256] = w[k].to(torch.float32)
            d[k] = t.reshape(-1).contiguous().to(_dev())
        _SHARED[key] = d
    return _SHARED[key]


def _attention_inputs(case, inp, lp):
    """O / ml buffers of a launch whose attention ran separately: (O guarded pair, words, ml guarded pair or None, words, o_sstride)."""
    B, N = case["B"], case["N"]
    rows = B * N * 256
    sstride = rows + K.O_PAD
    if case["o_lp"]:
        nO = rows // 2
        obuf, O = _guarded(nO)
        _put(O, inp["O"], lp)
        return (obuf, O), nO, None, 0, sstride
    tk, t0 = case["tail_ks"], case["tail_row0"]
    slots = 1 + tk if tk > 1 else max(case["ksplit"], 1)
    nO = slots * sstride
    obuf, O = _guarded(nO)
    Of = O.view(torch.float32)
    parts = inp.get("parts") or []
    if case["ksplit"] <= 1:
        o0 = inp["O"].clone()
        if tk > 1:
            o0[:, t0:] = NAN                                           # rows of the tail split: slot 0 is not theirs to read
        Of[:rows] = o0.to(torch.float32).reshape(-1).to(_dev())
    for s, (_, _, Os) in enumerate(parts):
        Of[s * sstride:s * sstride + rows] = Os.to(torch.float32).reshape(-1).to(_dev())
    nml = max(case["ksplit"], tk) * B * 2 * N * 2
    mpair = None
    if nml and (case["ksplit"] > 1 or tk > 1):
        mbuf, ml = _guarded(nml)
        src = parts if case["ksplit"] > 1 else inp["tail_parts"]
        mlv = torch.stack([torch.stack([m, l], -1) for m, l, _ in src])   # [s, B, 2, N, 2]
        if tk > 1:
            mlv[:, :, :, :t0] = NAN
            for s, (_, _, Os) in enumerate(src):
                o = Os.clone()
                o[:, :t0] = NAN
                Of[(1 + s) * sstride:(1 + s) * sstride + rows] = o.to(torch.float32).reshape(-1).to(_dev())
        _put(ml, mlv)
        mpair = (mbuf, ml)
    else:
        nml = 0
    return (obuf, O), nO, mpair, nml, sstride


def _decode(words, lp, B, Npad, kind):
    """Raw words of an operand buffer -> fp64 rows [2 B, Npad, 128]."""
    f = torch.from_numpy(words.copy()).view(lp).reshape(2 * B, Npad * 128)
    return (AR.unpack_qk if kind < 2 else AR.unpack_vt)(f).to(torch.float64)


def _rows(x, B, N):
    """[2 B, Npad, 128] -> the live rows [B, N, 256]."""
    return x.reshape(B, 2, -1, 128)[:, :, :N].permute(0, 2, 1, 3).reshape(B, N, 256)


def run_case(case, prec, ks, zero_lo=False):
    """One launch (two for the cluster forms) and all its checks.  zero_lo: the packs without their lo halves - returns the rms
    ratios instead of asserting them (the negative control below)."""
    B, N, Npad = case["B"], case["N"], case["Npad"]
    lp = ks.LP_DTYPE[prec]
    inp = K.make_inputs(case)
    sh = _shared(prec, ks, zero_lo)
    nX, nQ = B * N * 256, B * 2 * Npad * 64
    xbuf, X = _guarded(nX)
    _put(X, inp["X"])
    t = dict(X=X.view(torch.float32), ada=sh["ada"])
    kw = dict(B=B, N=N, Npad=Npad, ksplit=case["ksplit"], qkv_only=case["qkv_only"], attn_inline=case["attn_inline"], step=case["step"],
              row_bstride=case["row_bstride"], o_lp=case["o_lp"], tail_row0=case["tail_row0"], tail_ks=case["tail_ks"], qscale=case["qscale"])
    if not case["qkv_only"]:
        t.update({k: sh[k] for k in ("Wp", "W1", "W2", "bp", "b1", "b2")})
    if not case["last"]:
        t.update(Wq=sh["Wq"], bq=sh["bq"], next_shift=sh["next_shift"], next_scale=sh["next_scale"])
        kw["next_step_stride"] = K.NEXT_STRIDE
    qbufs = [_guarded(nQ) for _ in range(3)]
    for name, (_, v) in zip(("Qh", "Kh", "Vt"), qbufs):
        t[name] = v.view(lp)
    guarded = [("X", xbuf, nX)] + [(n, b, nQ) for n, (b, _) in zip(("Qh", "Kh", "Vt"), qbufs)]
    if case["attn_inline"]:
        for name, pack, src in (("Qin", AR.pack_qk, "q"), ("Kin", AR.pack_qk, "k"), ("Vin", AR.pack_vt, "v")):
            t[name] = pack(inp[src]).to(lp).contiguous().to(_dev())
    elif not case["qkv_only"]:
        (obuf, O), nO, mpair, nml, sstride = _attention_inputs(case, inp, lp)
        t["O"], kw["o_sstride"] = O.view(torch.float32), sstride
        guarded.append(("O", obuf, nO))
        if mpair is not None:
            t["ml"] = mpair[1].view(torch.float32)
            guarded.append(("ml", mpair[0], nml))
    epochs = [0]
    if case["cluster"]:
        xlocal = case["cluster"] == "local"
        assert ks.predicate("dit_rowchain_cluster_form", prec, N, B)
        assert ks.predicate("dit_rowchain_cluster_local_fits", prec, N, B) == xlocal, "the case's knobs decide where the hand-offs go"
        gt = ks.cluster_grid_tiles(prec, N, B, xlocal)
        nS, nF = B * ((N + 31) // 32) * ks.DIT_CLUSTER_SLAB_FLOATS, gt * ks.DIT_CLUSTER_FLAG_WORDS + 1
        sbuf, slab = _guarded(nS, 0)
        fbuf, flag = _guarded(nF, 0)                                   # zeroed ONCE; the launches' epochs are 1, 2
        t.update(xslab=slab.view(torch.float32), xflag=flag)
        kw["xlocal"] = xlocal
        guarded += [("xslab", sbuf, nS), ("xflag", fbuf, nF)]
        epochs = [1, 2]
    results = []
    for epoch in epochs:
        if epoch > 1:                                                   # the same inputs again
            _put(X, inp["X"])
            for _, v in qbufs:
                v.fill_(FILL)
        form = ks.dit_rowchain(prec, t, epoch=epoch, **kw)
        torch.cuda.synchronize()
        assert form == case["form"], (case["name"], form)
        res = {n: _guards_intact(b, nw, n) for n, b, nw in guarded}
        if case["cluster"]:
            assert res["xflag"][-1] == 0, (case["name"], "xerr", int(res["xflag"][-1]))
        results.append(res)
    if len(results) == 2:
        for n in ("X", "Qh", "Kh", "Vt"):
            assert np.array_equal(results[0][n], results[1][n]), (case["name"], n, "differs between two launches of the same inputs")
    res = results[0]
    # ---- x2
    got = torch.from_numpy(res["X"].view(np.float32).copy()).reshape(B, N, 256)
    ref = R.reference(case, inp, prec)
    out = {}
    if case["qkv_only"]:
        assert torch.equal(got, inp["X"].to(torch.float32)), (case["name"], "a qkv_only launch changed X")
    else:
        assert bool(torch.isfinite(got).all()), (case["name"], "non-finite x2")
        ev = R.evaluate(case, inp, prec)
        out["hard"] = R.ratio(got, ref["x2"], ref["tol_x2"])
        out["r_all"], out["r_col"], out["r_row"] = R.rms_ratios(got, ref["x2"], ev["x2"], R.FORM_ROWS[case["form"]])
    # ---- q / k / v
    own = R.owned_rows(case["form"], N, Npad)
    if case["last"]:
        for n in ("Qh", "Kh", "Vt"):
            assert (res[n] == FILL).all(), (case["name"], n, "written by a launch without a qkv stage")
    else:
        q = R.qkv_reference(case, inp, prec, got.to(torch.float64))
        out["amb"] = q["amb_share"]
        assert q["amb_share"] <= R.AMB_SHARE_MAX, (case["name"], q["amb_share"])
        for kind, n in enumerate(("Qh", "Kh", "Vt")):
            tiles = res[n].reshape(2 * B, Npad // 32, 2048)
            assert (tiles[:, len(own) // 32:] == FILL).all(), (case["name"], n, "words that belong to no row tile were written")
            rows = _decode(res[n], lp, B, Npad, kind)
            assert bool(torch.isfinite(rows[:, :len(own)]).all()), (case["name"], n, "non-finite rows a tile owns")
            sl = slice(256 * kind, 256 * kind + 256)
            out["qkv"[kind]] = R.ratio(_rows(rows, B, N), q["qkv"][..., sl], q["tol"][..., sl])
    if zero_lo:
        return out
    from tests import gpu_util
    gpu_util.record(f"rowchain:{case['name']}:{prec}", **out)
    print(case["name"], prec, form, {k: round(v, 4) for k, v in out.items()})
    bad = {k: v for k, v in out.items() if k in ("hard", "q", "k", "v") and not v <= 1.0}
    bad.update({k: v for k, v in out.items() if k.startswith("r_") and not v <= R.RATIO_MAX})
    assert not bad, (case["name"], prec, out)


@pytest.mark.parametrize("case,prec", [(c, p) for c in K.ALL for p in K.PRECS], ids=[f"{c['name']}-{p}" for c in K.ALL for p in K.PRECS])
def test_rowchain_launch(case, prec, ks, knobs):
    knobs(case["env"])
    if case is K.PERSISTENT:
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        assert case["B"] * ((case["N"] + 63) // 64) > ncu, "the persistent form must walk more row tiles than it has workgroups"
    run_case(case, prec, ks)


def test_dropped_lo_half_exceeds_the_ratio_limit(ks, knobs):
    """Negative control of this file's own decoding and statistic, on the device: the same launch on packs whose lo halves are
    zeroed computes a plausible result inside the hard bound, and the rms-error ratio must report it."""
    case = next(c for c in K.SEP32 if c["B"] * c["N"] >= 192 and c["ksplit"] > 1)
    knobs(case["env"])
    out = run_case(case, "fp16x2", ks, zero_lo=True)
    assert min(out["r_all"], out["r_col"], out["r_row"]) > R.RATIO_MAX, out
    assert out["hard"] <= 1.0, out


@pytest.mark.parametrize("prec", K.PRECS)
def test_predicates_the_cases_rely_on(prec, ks, knobs):
    knobs({})
    assert ks.predicate("dit_rowchain_supported", prec, 256, 512) and not ks.predicate("dit_rowchain_supported", prec, 256, 1024)
    assert not ks.predicate("dit_rowchain64_form", prec, 33, 2, 0)                     # by default a small grid keeps the 32-row form
    assert ks.predicate("dit_rowchain_cluster_form", prec, 100, 3) and not ks.predicate("dit_rowchain_cluster_form", prec, 200, 65)
    assert ks.predicate_int("dit_rowchain_cluster_xcds", prec, 100, 3) == 8
    knobs({"DEX_ROWCHAIN64": 2})
    assert ks.predicate("dit_rowchain64_form", prec, 33, 2, 0) and not ks.predicate("dit_rowchain64_form", prec, 33, 2, 1)
    knobs({"DEX_DIT_XCDS": 3})
    assert ks.predicate_int("dit_rowchain_cluster_xcds", prec, 100, 3) == 3
    knobs({"DEX_DIT_CLUSTER_LOCAL": 0})
    assert not ks.predicate("dit_rowchain_cluster_local_fits", prec, 100, 3)


def test_shim_rejects_what_the_launcher_would_not_run_as_asked(ks, knobs):
    """Every descriptor outside what the launcher and the kernels' index arithmetic cover is an error code, never a launch."""
    prec, lp, B, N, Npad = "bf16", torch.bfloat16, 2, 33, 64
    sh = _shared(prec, ks)
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=_dev())

    def call(env=None, drop=(), **over):
        knobs(env or {})
        n_, npad_ = over.get("N", N), over.get("Npad", Npad)
        t = dict(X=z(B * n_ * 256), O=z(8 * B * n_ * 256), ml=z(8 * B * 2 * n_ * 2), ada=sh["ada"], next_shift=sh["next_shift"],
                 next_scale=sh["next_scale"], **{k: sh[k] for k in ("Wp", "W1", "W2", "Wq", "bp", "b1", "b2", "bq")})
        for n in ("Qh", "Kh", "Vt", "Qin", "Kin", "Vin"):
            t[n] = z(B * 2 * npad_ * 128, lp)
        t.update(over.pop("tensors", {}))
        for n in drop:
            t.pop(n)
        kw = dict(B=B, N=n_, Npad=npad_, ksplit=1, o_sstride=B * n_ * 256, next_step_stride=K.NEXT_STRIDE, qscale=1.0)
        kw.update(over)
        return ks.dit_rowchain(prec, t, **kw)

    slabs = lambda: dict(xslab=z(B * 2 * ks.DIT_CLUSTER_SLAB_FLOATS), xflag=z(16 * ks.DIT_CLUSTER_FLAG_WORDS + 1, torch.int32))
    bad = [dict(tensors=slabs(), attn_inline=True, ksplit=0, epoch=0),                                  # an epoch of 0 is the flags' idle value
           dict(tensors=slabs(), attn_inline=True, ksplit=0, epoch=1 << 24, xlocal=True),               # XCD-local flags carry 24 epoch bits
           dict(tensors=slabs(), attn_inline=True, ksplit=0, epoch=1, xlocal=True, env={"DEX_DIT_CLUSTER_LOCAL": 0}),
           dict(Npad=72), dict(ksplit=9),
           dict(o_lp=True, env={"DEX_ROWCHAIN64": 0}),                                                  # 16-bit O rows: the 64-row form only
           dict(o_lp=True, ksplit=2, env={"DEX_ROWCHAIN64": 2}),
           dict(tail_row0=32, tail_ks=2, env={"DEX_ROWCHAIN64": 2}), dict(tail_row0=0, tail_ks=2, env={"DEX_ROWCHAIN64": 2}),
           dict(tail_row0=64, tail_ks=2, N=100, Npad=128, env={"DEX_ROWCHAIN64": 0}),
           dict(tensors=slabs(), epoch=1),                                                              # slabs, but not a launch the cluster form takes
           dict(xlocal=True), dict(qkv_only=True, attn_inline=True), dict(drop=("Wq",)), dict(drop=("ml",), ksplit=2),
           dict(drop=("Qin",), attn_inline=True, ksplit=0), dict(step=-1)]
    for kw in bad:
        with pytest.raises(ks.ShimError):
            call(**kw)
    with pytest.raises(ks.ShimError):                                   # a tensor shorter than the descriptor implies
        call(tensors=dict(X=z(B * N * 256 - 1)))
    with pytest.raises(ks.ShimError):
        call(step=K.N_STEPS)                                            # a step row past the table
