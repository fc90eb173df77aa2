"""CPU checks of tests/rowchain_reference.py and tests/rowchain_cases.py, for every case and mode of the GPU file
(tests/test_gpu_rowchain_kernels.py): the fp32 evaluation with the kernels' rounding points is within both derived bounds, a second
faithful fp32 evaluation in another summation order stays within 2 % of it in the rms-error statistic, every mutant breaks the check
that is there for it, the ambiguity set stays small, the measured delta leaves its margin, and the row sets and packers the GPU file
decodes with agree with a scalar re-statement of the kernels' store indices."""
import pytest
import torch

from tests import attn_reference as AR
from tests import rowchain_cases as K
from tests import rowchain_reference as R

PAIRS = [(c, p) for c in K.ALL for p in K.PRECS]
IDS = [f"{c['name']}-{p}" for c, p in PAIRS]


@pytest.mark.parametrize("case,prec", PAIRS, ids=IDS)
def test_evaluation_within_bounds_and_mutants_break_them(case, prec, golden_threads):
    # (golden_threads: torch's fp32 products split their sums by the thread count; the statistics of the single-row cases are pinned to one)
    inp = K.make_inputs(case)
    ref = R.reference(case, inp, prec)
    ev = R.evaluate(case, inp, prec)
    rows = R.FORM_ROWS[case["form"]]
    if case["qkv_only"]:
        assert torch.equal(ev["x2"].double(), inp["X"])
    else:
        hard = R.ratio(ev["x2"], ref["x2"], ref["tol_x2"])
        assert hard <= 1.0, (case["name"], prec, hard)
        again = R.evaluate(case, inp, prec, reorder=True)
        spread = max(R.rms_ratios(again["x2"], ref["x2"], ev["x2"], rows))
        assert spread <= 1.02, (case["name"], prec, spread)
        for m in ("gate_swap", "merge_unweighted", "ln_affine_prev_step"):
            if m == "merge_unweighted" and not (case["ksplit"] > 1 or case["tail_ks"] > 1):
                continue                                               # (nothing to merge: the mutant is the identity)
            got = R.evaluate(case, inp, prec, mutant=m)
            assert R.ratio(got["x2"], ref["x2"], ref["tol_x2"]) > 1.0, (case["name"], prec, m)
        for m in ("trunc_a1", "trunc_h") + (("drop_lo",) if prec == "fp16x2" else ()):
            got = R.evaluate(case, inp, prec, mutant=m)
            whole, col, row = R.rms_ratios(got["x2"], ref["x2"], ev["x2"], rows)
            assert whole >= 1.3 and max(col, row) >= 1.3, (case["name"], prec, m, whole, col, row)
    if not case["last"]:
        x2 = ev["x2"].double()                                         # the anchor: the fp32 x2 of the evaluation under test
        q = R.qkv_reference(case, inp, prec, x2)
        sharp = R.ratio(ev["qkv"], q["qkv"], q["tol"])
        assert sharp <= 1.0, (case["name"], prec, sharp)
        assert q["amb_share"] <= R.AMB_SHARE_MAX / 2, (case["name"], prec, q["amb_share"])
        measured = R.ln_fp32_error_ulps(case, inp, prec, x2)
        assert 4 * measured <= R.DELTA_ULPS, (case["name"], prec, measured)
        # a wrong q scale, or the bias added after it, is outside the sharp bound
        bad = ev["qkv"].double().clone()
        bad[..., :R.H] = R.round_lp((q["qkv"][..., :R.H] / case["qscale"]) * (case["qscale"] * (1 + 2.0 ** -6)), prec)
        assert R.ratio(bad, q["qkv"], q["tol"]) > 1.0


def test_measured_delta_is_the_documented_one(golden_threads):
    assert abs(K.measure_ln_fp32_error() - R.LN_FP32_ULPS_MEASURED) <= 0.25 * R.LN_FP32_ULPS_MEASURED
    assert R.DELTA_ULPS == 8 * R.LN_FP32_ULPS_MEASURED


def _stored_rows(form, N, Npad):
    """Scalar re-statement of the stores: which rows of a (element, head) operand the row tiles of a launch write."""
    rows = set()
    if R.FORM_ROWS[form] == 32:                                        # store_qkv_tile_d: tile n0 >> 5, all 32 rows of it
        for n0 in range(0, N, 32):
            rows.update(range(n0, n0 + 32))
    else:                                                              # two halves per 64-row tile; one at or past Npad is not stored
        for n0 in range(0, N, 64):
            for m in range(2):
                if n0 + 32 * m >= Npad:
                    break
                rows.update(range(n0 + 32 * m, n0 + 32 * m + 32))
    return rows


@pytest.mark.parametrize("form", sorted(R.FORM_ROWS))
def test_owned_rows_match_the_store_indices(form):
    for N in (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 200, 300):
        base = (N + 31) // 32 * 32
        for Npad in (base, base + 32, base + 64):
            own = R.owned_rows(form, N, Npad)
            assert set(own) == _stored_rows(form, N, Npad), (form, N, Npad)
            assert max(own) < Npad and set(range(N)) <= set(own)


@pytest.mark.parametrize("N,Npad", [(1, 32), (1, 64), (33, 64), (33, 96), (65, 96), (129, 160)])
def test_operand_layouts_round_trip(N, Npad):
    """pack / unpack of the q / k / v^T layouts at Npad != N, against the element offsets of store_qkv_tile (dit_rowchain.hip)."""
    g = torch.Generator().manual_seed(N * 1000 + Npad)
    x = torch.randn(3, Npad, 128, generator=g, dtype=torch.float64)
    for pack, unpack in ((AR.pack_qk, AR.unpack_qk), (AR.pack_vt, AR.unpack_vt)):
        f = pack(x)
        assert f.shape == (3, Npad * 128) and torch.equal(unpack(f), x)
    fq, fv = AR.pack_qk(x), AR.pack_vt(x)
    for r, d in ((0, 0), (N - 1, 127), (Npad - 1, 5), (min(N, Npad - 1), 64), (Npad - 32, 31)):
        base, row = (r >> 5) * 4096, r & 31
        off = (((d >> 4) * 64 + ((d >> 3) & 1) * 32 + row) << 3) + (d & 7)                 # q / k: chunk (row, d / 8), 8 consecutive d
        assert fq[1, base + off] == x[1, r, d]
        pos = (row & ~12) | ((row & 4) << 1) | ((row & 8) >> 1)                           # v^T: the position that holds key row `row`
        off = ((((d >> 5) * 2 + (pos >> 4)) * 64 + ((pos >> 3) & 1) * 32 + (d & 31)) << 3) + (pos & 7)
        assert fv[1, base + off] == x[1, r, d]


def test_row_groups_fold_short_tiles():
    assert R.row_groups(1, 200, 64) == [[(0, 0, 64)], [(0, 64, 128)], [(0, 128, 192)], [(0, 192, 200)]]      # 8 live rows stand alone
    assert R.row_groups(1, 199, 64) == [[(0, 0, 64)], [(0, 64, 128)], [(0, 128, 192), (0, 192, 199)]]
    assert R.row_groups(2, 33, 32) == [[(0, 0, 32), (0, 32, 33)], [(1, 0, 32), (1, 32, 33)]]
    assert all(sum(r1 - r0 for _, r0, r1 in g) >= 8 for g in R.row_groups(65, 200, 64))


def test_cases_cover_what_the_launcher_chooses_between():
    forms = {c["form"] for c in K.ALL}
    assert forms == set(R.FORM_ROWS)
    assert {c["ksplit"] for c in K.ALL if c["form"] == K.F32} >= {0, 1, 3, 4, 8}
    assert {c["ksplit"] for c in K.ALL if c["form"] == K.F_64} >= {2, 6, 8}
    assert K.PERSISTENT["B"] * ((K.PERSISTENT["N"] + 63) // 64) == 260 and K.PERSISTENT["N"] % 64 == 8
    for c in K.ALL:
        assert set(c["env"]) <= set(K.KNOBS) and c["Npad"] % 32 == 0 and c["Npad"] >= c["N"]
        assert c["B"] * c["N"] <= 13000
