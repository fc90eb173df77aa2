"""The fragment-operand softmax attention kernels ONE LAUNCH AT A TIME against a plain fp64 reference of the same operation.

attn_direct_kernel, attn_direct_ring_kernel (csrc/attention_direct.hip) and attn_q64_kernel (csrc/attention_q64.hip) are reached
through the test-only shim (tests/kshim), which fills AttnDirectP and calls the library's own launchers.  Each case
(tests/attn_cases.py) asserts the form string the shim returns - the kernel, its xcd_map, or the 64-query form's whole unit plan - so a
launcher that re-plans fails the case instead of shrinking coverage.  Per case: every partial of every row range against the fp64
attention over its own key range, its (m, l), the fp64 merge of the kernel's partials against the full reference, every live element
finite, the guard regions in front of and behind O and ml bit-identical, and every word no unit owns still the NaN pre-fill.  Every
output element is held to the bound tests/attn_reference.py derives; nothing is excluded.  Each comparison records max(err / tol)
(profiles/attention_kernel_parity_measured.jsonl holds a run's lines).

No case skips: every mode's build has all three kernels."""
import os

import numpy as np
import pytest
import torch

from tests import attn_cases as K
from tests import attn_reference as R

pytestmark = pytest.mark.gpu
FILL = 0x7FC07FC0                     # a NaN as fp32 AND as two 16-bit values of either type
GUARD = 0x5A5AA5A5
GUARD_WORDS = 1024


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


_PACKED, _REF = {}, {}


def _packed(case, lp, vt_swap=True):
    key = (case["B"], case["N"], case["spikes"], lp, vt_swap)
    if key not in _PACKED:
        _PACKED.clear()
        q, k, v = K.make_operands(case["B"], case["N"], case["spikes"])
        _PACKED[key] = tuple(t.to(lp).contiguous().to(_dev()) for t in (R.pack_qk(q), R.pack_qk(k), R.pack_vt(v, swap=vt_swap)))
    return _PACKED[key]


def _ref(case, rows, keys):
    """fp64 (O, A, M, L, max|v|) of a row range over a key range, computed once and shared by the modes and plans of a shape."""
    shape = (case["B"], case["N"], case["spikes"])
    if _REF.get("shape") != shape:
        _REF.clear()
        _REF["shape"] = shape
    if (rows, keys) not in _REF:
        assert case["B"] * case["N"] * case["N"] <= 2 ** 25                           # (the CPU reference's range)
        q, k, v = K.make_operands(*shape)
        O, A, M, L = R.attention_qkv(q, k, v, case["N"], keys[0], keys[1], slice(*rows))
        _REF[(rows, keys)] = (O, A, M, L, v[:, keys[0]:keys[1]].abs().max(dim=1).values)
    return _REF[(rows, keys)]


def _gh(x, B):
    """[B, R, 2, 128] -> [2 B, R, 128]: (element, head) pairs as the operands order them."""
    return x.permute(0, 2, 1, 3).reshape(2 * B, x.shape[1], 128)


def run_case(case, prec, ks, vt_swap=True):
    """One launch and all its checks.  vt_swap=False packs v^T WITHOUT the bit-2/3 swap and returns the ratios instead of asserting
    them (the negative control below)."""
    B, N = case["B"], case["N"]
    npad = (N + 31) // 32 * 32
    lp = ks.LP_DTYPE[prec]
    Qh, Kh, Vt = _packed(case, lp, vt_swap)
    sstride = B * N * 256
    nO, nML = K.n_slots(case) * sstride, K.n_ml(case) * B * 2 * N * 2
    obuf, O = _guarded(nO)
    mbuf, ml = _guarded(nML)
    entry = ks.attn_direct if case["kind"] == "direct" else ks.attn_q64
    form = entry(prec, dict(Qh=Qh, Kh=Kh, Vt=Vt, O=O.view(torch.float32), ml=ml.view(torch.float32)), N=N, Npad=npad, B=B,
                 ksplit=case["ksplit"], o_sstride=sstride, o_lp=case["o_lp"], tail_g=case["tail_g"], tail_ks=case["tail_ks"],
                 half_g=case["half_g"], half_n=case["half_n"])
    torch.cuda.synchronize()
    assert form == case["form"], (case["name"], form)
    ow, mw = _guards_intact(obuf, nO), _guards_intact(mbuf, nML)
    o_owned, m_owned = np.zeros(nO, dtype=bool), np.zeros(nML, dtype=bool)
    o32 = torch.from_numpy(ow.view(np.float32).reshape(K.n_slots(case), B, N, 2, 128))
    o16 = torch.from_numpy(ow[:sstride // 2].copy()).view(lp).reshape(B, N, 2, 128)  # 16-bit rows: the front half of slot 0
    mlv = torch.from_numpy(mw.view(np.float32).reshape(K.n_ml(case), B, 2, N, 2))
    ratios = {}
    worst = lambda name, v: ratios.__setitem__(name, max(ratios.get(name, 0.0), v) if v == v else float("nan"))
    by_rows = {}
    for part in K.parts_of(case):
        r0, r1 = part["rows"]
        if r0 == r1:
            continue
        Or, Ar, Mr, Lr, vmax = _ref(case, part["rows"], part["keys"])
        if part["lp"]:
            got = _gh(o16[:, r0:r1].to(torch.float64), B)
            own = o_owned[:sstride // 2].reshape(B, N, 128)
        else:
            got = _gh(o32[part["slot"], :, r0:r1].to(torch.float64), B)
            own = o_owned[part["slot"] * sstride:(part["slot"] + 1) * sstride].reshape(B, N, 256)
        own[:, r0:r1] = True
        assert bool(torch.isfinite(got).all()), (case["name"], part, "non-finite live elements")
        tol = R.tolerance(Or, Ar, vmax, N, prec, part["lp"])
        worst("O", ((got - Or).abs() / tol).max().item())
        m = l = None
        if part["ml"] is not None:
            g = mlv[part["ml"]].reshape(2 * B, N, 2)[:, r0:r1]
            m, l = g[..., 0].to(torch.float64), g[..., 1].to(torch.float64)
            m_owned[part["ml"] * B * 2 * N * 2:(part["ml"] + 1) * B * 2 * N * 2].reshape(2 * B, N, 2)[:, r0:r1] = True
            assert bool(torch.isfinite(m).all() and torch.isfinite(l).all()), (case["name"], part, "non-finite (m, l)")
            r_m, r_l = R.ml_ratios(m, l, Mr, Lr, N)
            worst("m", r_m)
            worst("l", r_l)
        by_rows.setdefault(part["rows"], []).append(((m, l, got), (Mr, Lr, Or), tol))
    for rows, parts in by_rows.items():
        if len(parts) < 2:
            continue
        got, _, _ = R.merge([p[0] for p in parts])
        full, _, _ = R.merge([p[1] for p in parts])                                   # (fp64: the full-range reference to 1e-15)
        tol = R.merged_tolerance([p[1] for p in parts], [p[2] for p in parts], N)
        worst("merged", ((got - full).abs() / tol).max().item())
    assert (ow[~o_owned] == FILL).all(), (case["name"], "O words that belong to no unit were written")
    assert (mw[~m_owned] == FILL).all(), (case["name"], "(m, l) words that belong to no unit were written")
    if not vt_swap:
        return ratios
    from tests import gpu_util
    gpu_util.record(f"attnk:{case['name']}:{prec}", **ratios)
    print(case["name"], prec, form, ratios)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert "O" in ratios and not bad, (case["name"], prec, ratios)


@pytest.mark.parametrize("case,prec", [(c, p) for c in K.ALL for p in K.PRECS], ids=[f"{c['name']}-{p}" for c in K.ALL for p in K.PRECS])
def test_attention_launch(case, prec, ks, knobs):
    knobs(case["env"])
    run_case(case, prec, ks)


@pytest.mark.parametrize("kind", ("waves", "ring", "q64"))
def test_wrong_operand_layout_breaks_the_bound(kind, ks, knobs):
    """Negative control of this file's own decoding and comparison, on the device: the same launch on a v^T packed without the
    bit-2/3 swap computes a wrong (finite, in-bounds) result, and every kernel's case must report it far outside the bound."""
    knobs({})
    case = {"waves": K.direct(2, 257, 2), "ring": K.direct(256, 33, xcd_map=1), "q64": K.q64(2, 257, 2)}[kind]
    ratios = run_case(case, "bf16", ks, vt_swap=False)
    assert ratios["O"] > 10 and ratios["merged" if case["ksplit"] > 1 else "O"] > 10, ratios
    assert ratios["m"] <= 1.0 and ratios["l"] <= 1.0, ratios                          # (m, l) do not depend on v


@pytest.mark.parametrize("prec", K.PRECS)
def test_plans_the_cases_rely_on(prec, ks, knobs):
    knobs({})
    for c in K.ALL:
        if c["kind"] == "direct":
            ring = ks.attn_plan("attention_direct_batch_regime", prec, c["N"], c["B"])
            assert bool(ring) == c["form"].startswith("attn_direct_ring_kernel"), c["name"]
    assert ks.attn_plan("attention_direct_ksplit", prec, 1025, 16) == K.RING_KS_B16_N1025
    assert ks.attn_plan("attention_q64_ksplit", prec, 520, 1, 8) == K.Q64_AUTO_KS_B1_N520


def test_shim_rejects_unreachable_plans(ks, knobs):
    """Every plan outside what the launchers document is an error code, never a launch."""
    knobs({})
    lp = torch.bfloat16

    def call(entry, B, N, **kw):
        npad = kw.pop("Npad", (N + 31) // 32 * 32)
        ops = torch.zeros(B * 2 * npad * 128, dtype=lp, device=_dev())
        O = torch.zeros(8 * B * N * 256, dtype=torch.float32, device=_dev())
        ml = torch.zeros(5 * B * 2 * N * 2, dtype=torch.float32, device=_dev())
        return entry("bf16", dict(Qh=ops, Kh=ops, Vt=ops, O=O, ml=ml), N=N, Npad=npad, B=B, o_sstride=B * N * 256, **kw)

    bad = [(ks.attn_direct, 3, 33, dict(ksplit=3)),                                  # more splits than 32-key tiles
           (ks.attn_q64, 3, 33, dict(ksplit=2)),                                     # more splits than 64-key tiles
           (ks.attn_direct, 256, 33, dict(ksplit=2)),                                # ring kernel: not attention_direct_ksplit's value
           (ks.attn_direct, 2, 257, dict(o_lp=True)),                                # 16-bit rows: not the key-splitting waves
           (ks.attn_direct, 2, 257, dict(tail_g=1, tail_ks=2)),
           (ks.attn_q64, 1, 520, dict(tail_g=1, tail_ks=5)), (ks.attn_q64, 1, 520, dict(tail_g=0, tail_ks=2)),
           (ks.attn_q64, 1, 520, dict(tail_g=3, tail_ks=2)), (ks.attn_q64, 2, 70, dict(tail_g=1, tail_ks=2)),
           (ks.attn_q64, 1, 520, dict(tail_g=1, tail_ks=2, ksplit=2)),                # a tail split together with a key split
           (ks.attn_q64, 1, 520, dict(half_g=1, half_n=2)), (ks.attn_q64, 1, 520, dict(half_g=3, half_n=1)),
           (ks.attn_q64, 1, 520, dict(half_g=0, half_n=5, ksplit=2)),
           (ks.attn_q64, 2, 257, dict(ksplit=2, o_lp=True)),                          # 16-bit rows with a key split
           (ks.attn_q64, 2, 257, dict(Npad=320)), (ks.attn_direct, 2, 257, dict(Npad=320))]
    for entry, B, N, kw in bad:
        with pytest.raises(ks.ShimError):
            call(entry, B, N, **kw)
    with pytest.raises(ks.ShimError):                                                # operands shorter than the descriptor implies
        ops = torch.zeros(2 * 2 * 288 * 128 - 1, dtype=lp, device=_dev())
        ks.attn_q64("bf16", dict(Qh=ops, Kh=ops, Vt=ops, O=torch.zeros(2 * 257 * 256, device=_dev())), N=257, Npad=288, B=2,
                    o_sstride=2 * 257 * 256)


def test_device_reference_agrees_with_cpu():
    """The same reference function on the device in fp64 (allowed for shapes past the CPU's range) against the CPU's."""
    q, k, v = K.make_operands(2, 257)
    cpu = R.attention_qkv(q, k, v, 257, 64, 257)
    dev = R.attention_qkv(q.to(_dev()), k.to(_dev()), v.to(_dev()), 257, 64, 257)
    for a, b in zip(cpu, dev):
        assert (a - b.cpu()).abs().max().item() <= 1e-12
