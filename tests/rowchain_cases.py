"""The launches tests/test_gpu_rowchain_kernels.py runs one at a time, and their operands (shared with
tests/test_rowchain_reference_cpu.py).

Each case names the form string launch_dit_rowchain must report (g_last_symbol through the shim) and the DEX_* knobs it sets: a
launcher that re-plans fails the case.  Hidden size 256 / mlp 512 - the only size the kernels have.

OPERANDS (make_inputs): seeded fp32 values held in fp64.  X ~ N(0, 1); weights ~ N(0, 1 / K) (ONE set for every case: the packs are
made once per mode); biases and the adaLN rows ~ 0.5 N(0, 1), gates +-(0.6 .. 1.4), and every step row of the tables carries an
offset of its own of order 1, so a dropped bias or gate or a wrong row is far outside the bound.  Attention output given: O ~ 0.7
N(0, 1) (on the 2^-6 grid below 2 for 16-bit rows: exact in bf16 and fp16).  Key-split partials: normalised O_s ~ 0.7 N(0, 1), m_s
uniform over +-30, l_s over 1 .. 50, and split 1 at m = -100 (a negligible weight).  In-kernel attention: tests/attn_cases.py's
operands (spikes, edge sentinel, pad rows)."""
import math

import torch

from tests import attn_cases
from tests import rowchain_reference as R

PRECS = ("bf16", "fp16", "fp16x2")
KNOBS = ("DEX_ROWCHAIN64", "DEX_ROWCHAIN64A", "DEX_DIT_CLUSTER", "DEX_DIT_CLUSTER_LOCAL", "DEX_DIT_XCDS", "DEX_XCD_MAP")
QSCALE = float(torch.tensor(1.4426950408889634 / math.sqrt(128.0), dtype=torch.float32))      # log2(e) / sqrt(head_dim), as dex_api.hip folds it
N_STEPS = 6
NEXT_STRIDE = 320                               # floats between the step rows of next_shift / next_scale (not 256: the stride is used)
SEED = 6                                        # (a single-row case has 256 elements: its mutant ratios scatter by +-0.1 and its cap of 1 % ambiguous a2
                                                # elements is 2 of them against ~1 expected; at this seed every single-row case and mode meets what
                                                # tests/test_rowchain_reference_cpu.py asks of all cases; the larger cases meet it at any seed)
O_PAD = 256                                     # floats between the O slots beyond B * N * 256 (o_sstride is used)
F32, F_TT, F_64, F_64A = "dit_rowchain_kernel<false>", "dit_rowchain_kernel<true> xcd_map=", "dit_rowchain64_kernel", "dit_rowchain64a_kernel"
F_CQ, F_CG, F_CL = ("dit_rowchain_cluster_kernel<true,false>", "dit_rowchain_cluster_kernel<false,false>",
                    "dit_rowchain_cluster_kernel<false,true>")


def case(form, B, N, *, ksplit=1, o_lp=False, last=False, qkv_only=False, inline=False, step=1, row_bstride=0, tail=None, env=None,
         cluster=None, Npad=None, tag=""):
    """cluster: None | "local" | "global" (slabs and flags are given; XCD-local hand-offs or not)."""
    npad = (N + 31) // 32 * 32 if Npad is None else Npad
    t0, tk = tail or (0, 0)
    name = f"{tag}_B{B}_N{N}" + (f"_ks{ksplit}" if ksplit != 1 else "") + ("_olp" if o_lp else "") + ("_last" if last else "")
    name += ("_qkv" if qkv_only else "") + (f"_rbs{row_bstride}" if row_bstride else "") + (f"_tail{t0}x{tk}" if tk else "")
    name += (f"_npad{npad}" if Npad is not None else "")
    for kk, vv in (env or {}).items():
        name += f"_{kk[4:].lower()}{vv}"
    assert not (qkv_only and (last or inline)) and step >= 1
    return dict(name=name, form=form, B=B, N=N, Npad=npad, ksplit=0 if (qkv_only or inline) else ksplit, o_lp=o_lp, last=last,
                qkv_only=qkv_only, attn_inline=inline, step=step, row_bstride=row_bstride, tail_row0=t0, tail_ks=tk, env=env or {},
                cluster=cluster, qscale=QSCALE)


# ---- 32-row form, attention separate
_E32 = {"DEX_ROWCHAIN64": 0}
SEP32 = [case(F32, 1, 1, env=_E32, tag="r32"), case(F32, 2, 33, ksplit=3, env=_E32, tag="r32"), case(F32, 3, 64, ksplit=4, env=_E32, tag="r32"),
         case(F32, 2, 33, ksplit=8, env=_E32, tag="r32"), case(F32, 1, 1, last=True, env=_E32, tag="r32"),
         case(F32, 2, 33, last=True, env=_E32, tag="r32"), case(F32, 1, 1, qkv_only=True, env=_E32, tag="r32"),
         case(F32, 3, 64, qkv_only=True, env=_E32, tag="r32"), case(F32, 3, 64, step=2, row_bstride=1, env=_E32, tag="r32"),
         case(F32, 2, 33, env=_E32, Npad=96, tag="r32")]
# ---- 32-row form, attention inline (no slabs)
INL32 = [case(F_TT + "0", 1, 1, inline=True, tag="inl"), case(F_TT + "0", 2, 33, inline=True, tag="inl"),
         case(F_TT + "0", 1, 129, inline=True, tag="inl"), case(F_TT + "0", 2, 33, inline=True, last=True, tag="inl"),
         case(F_TT + "1", 8, 40, inline=True, tag="inl"), case(F_TT + "0", 8, 40, inline=True, env={"DEX_XCD_MAP": 0}, tag="inl")]
# ---- 64-row round-3 kernel
_E64 = {"DEX_ROWCHAIN64": 2, "DEX_ROWCHAIN64A": 0}
R64 = [case(F_64, 1, 1, env=_E64, tag="r64"), case(F_64, 2, 33, ksplit=2, env=_E64, tag="r64"), case(F_64, 2, 65, ksplit=6, env=_E64, tag="r64"),
       case(F_64, 1, 128, ksplit=8, env=_E64, tag="r64"), case(F_64, 2, 65, o_lp=True, env=_E64, tag="r64"),
       case(F_64, 2, 300, tail=(256, 3), env=_E64, tag="r64"), case(F_64, 2, 33, step=2, row_bstride=1, env=_E64, tag="r64"),
       case(F_64, 2, 33, qkv_only=True, env=_E64, tag="r64"), case(F_64, 2, 65, last=True, env=_E64, tag="r64"),
       case(F_64, 1, 1, env=_E64, Npad=64, tag="r64")]
# ---- 64-row generated streams, and the launcher's fall-backs to the round-3 kernel
_E64A = {"DEX_ROWCHAIN64": 2}
PERSISTENT = case(F_64A, 65, 200, o_lp=True, env=_E64A, tag="r64a")             # 260 tiles > CUs; every element's last tile: 8 live rows
R64A = ([case(F_64A, b, n, qkv_only=True, env=_E64A, tag="r64a") for b, n in ((1, 1), (2, 33), (3, 65), (1, 128))]
        + [case(F_64A, b, n, o_lp=True, env=_E64A, tag="r64a") for b, n in ((1, 1), (2, 33), (3, 65), (1, 128))]
        + [case(F_64A, 2, 33, o_lp=True, last=True, env=_E64A, tag="r64a"), case(F_64A, 1, 1, o_lp=True, env=_E64A, Npad=64, tag="r64a"),
           PERSISTENT,
           case(F_64, 2, 33, env=_E64A, tag="r64fb"), case(F_64, 2, 33, ksplit=2, env=_E64A, tag="r64fb"),
           case(F_64, 2, 33, o_lp=True, step=2, row_bstride=1, env=_E64A, tag="r64fb")])
# ---- cluster forms
_SHAPES = ((1, 1), (2, 33), (1, 129), (3, 100))
_EG = {"DEX_DIT_CLUSTER_LOCAL": 0}
CLUSTER = ([case(F_CQ, b, n, qkv_only=True, cluster="local", tag="clq") for b, n in _SHAPES]
           + [case(F_CQ, 3, 100, qkv_only=True, cluster="global", env=_EG, tag="clq")]
           + [case(F_CG, b, n, inline=True, cluster="global", env=_EG, tag="clg") for b, n in _SHAPES]
           + [case(F_CL, b, n, inline=True, cluster="local", tag="cll") for b, n in _SHAPES]
           + [case(F_CL, b, n, inline=True, cluster="local", env={"DEX_DIT_XCDS": 3}, tag="cll") for b, n in _SHAPES]
           + [case(F_CL, 2, 33, inline=True, last=True, cluster="local", tag="cll")])
ALL = SEP32 + INL32 + R64 + R64A + CLUSTER
assert len({c["name"] for c in ALL}) == len(ALL)


# ---- operands --------------------------------------------------------------------------------------------------------------------
def _f32(t):
    return t.to(torch.float32).to(torch.float64)


_WEIGHTS = None


def shared_weights():
    """The four weight matrices [K, N], biases and the conditioning tables: one set for every case."""
    global _WEIGHTS
    if _WEIGHTS is None:
        g = torch.Generator().manual_seed(20240607)
        n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        w = {"Wp": n(256, 256) / 16, "W1": n(256, 512) / 16, "W2": n(512, 256) / math.sqrt(512.0), "Wq": n(256, 768) / 16,
             "bp": 0.5 * n(256), "b1": 0.5 * n(512), "b2": 0.5 * n(256), "bq": 0.5 * n(768)}
        step_off = torch.linspace(-2.5, 2.5, N_STEPS, dtype=torch.float64)[:, None, None] * torch.tensor([1.0, 0.1, 0.0, -1.0, 0.1, 0.0])[None, :, None]
        ada = 0.5 * n(N_STEPS, 6, 256) * torch.tensor([1.0, 0.5, 0.0, 1.0, 0.5, 0.0])[None, :, None] + step_off
        sign = torch.where(torch.rand(N_STEPS, 2, 256, generator=g) < 0.5, -1.0, 1.0).double()
        gates = sign * (0.6 + 0.8 * torch.rand(N_STEPS, 2, 256, generator=g, dtype=torch.float64))
        ada[:, 2], ada[:, 5] = gates[:, 0], gates[:, 1]
        w["ada"] = ada
        # the next block's shift rows sit at 3 + step: a2 stays away from zero, where the 16-bit grid is fine against the fp32 LayerNorm's
        # error and the share of ambiguous elements would pass the project's cap in the fp16 modes (tests/rowchain_reference.py)
        w["next_shift"] = 0.5 * n(N_STEPS, 256) + 3.0 + torch.arange(N_STEPS, dtype=torch.float64)[:, None]
        w["next_scale"] = 0.25 * n(N_STEPS, 256) + 0.1 * step_off[:, 0]
        _WEIGHTS = {k: _f32(v) for k, v in w.items()}
    return _WEIGHTS


_INP = {}


def make_inputs(c):
    """fp64 tensors (fp32 values) of a case, cached one case at a time."""
    if _INP.get("name") == c["name"]:
        return _INP["inp"]
    B, N = c["B"], c["N"]
    g = torch.Generator().manual_seed(SEED + 7919 * B + 104729 * N + 13 * c["ksplit"] + 5 * c["tail_ks"] + int(c["o_lp"]) + 101 * int(c["attn_inline"]))
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    inp = dict(shared_weights())
    inp["X"] = _f32(n(B, N, 256))

    def parts(k):
        out = []
        for s in range(k):
            m = torch.rand(B, 2, N, generator=g, dtype=torch.float64) * 60 - 30
            if s == 1:
                m = torch.full_like(m, -100.0)
            l = 1 + 49 * torch.rand(B, 2, N, generator=g, dtype=torch.float64)
            out.append((_f32(m), _f32(l), _f32(0.7 * n(B, N, 256))))
        return out
    if c["attn_inline"]:
        q, k, v = attn_cases.make_operands(B, N)
        inp["q"], inp["k"], inp["v"] = q.clone(), k.clone(), v.clone()
    elif not c["qkv_only"]:
        if c["ksplit"] > 1:
            inp["parts"] = parts(c["ksplit"])
        else:
            O = 0.7 * n(B, N, 256)
            inp["O"] = (torch.round(O * 64).clamp(-127, 127) / 64) if c["o_lp"] else _f32(O)
        if c["tail_ks"] > 1:
            inp["tail_parts"] = parts(c["tail_ks"])
    _INP.clear()
    _INP.update(name=c["name"], inp=inp)
    return inp


def measure_ln_fp32_error():
    """max over every case with a qkv stage and every mode of R.ln_fp32_error_ulps on the reference's own x2 (module docstring of
    tests/rowchain_reference.py)."""
    worst = 0.0
    for c in ALL:
        if c["last"]:
            continue
        inp = make_inputs(c)
        for prec in PRECS:
            x2 = R.reference(c, inp, prec)["x2"]
            worst = max(worst, R.ln_fp32_error_ulps(c, inp, prec, x2.to(torch.float32).to(torch.float64)))
    return worst
