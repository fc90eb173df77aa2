"""tests/attn_reference.py and tests/attn_cases.py on the CPU: the packers against the layout and the MFMA contraction they serve, an
emulation of the kernels' arithmetic inside the derived bound, and the mutants of that emulation outside it - at the same inputs, in
every mode.  A bound that a subtly wrong kernel would still meet fails here, without a GPU."""
import pytest
import torch

from tests import attn_cases as K
from tests import attn_reference as R

NS = (33, 257, 520)


def _lp_ops(B, N, spikes=True):
    q, k, v = K.make_operands(B, N, spikes)
    return q, k, v, R.pack_qk(q).to(torch.float32), R.pack_qk(k).to(torch.float32), R.pack_vt(v).to(torch.float32)


# ---- packers ------------------------------------------------------------------------------------------------------------------
def test_pack_round_trips():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 96, 128, generator=g, dtype=torch.float64)
    for pack, unpack in ((R.pack_qk, R.unpack_qk), (R.pack_vt, R.unpack_vt)):
        f = pack(x)
        assert f.shape == (3, 96 * 128) and torch.equal(unpack(f), x)
        assert torch.equal(torch.sort(f, dim=-1).values, torch.sort(x.reshape(3, -1), dim=-1).values)
        assert torch.equal(pack(x.to(torch.bfloat16)).to(torch.float64), pack(x.to(torch.bfloat16).to(torch.float64)))
    assert not torch.equal(R.pack_vt(x), R.pack_vt(x, swap=False))


def test_pack_offsets_as_stated():
    """Spot values of the two formulas, and the producer's chunking: a 16-byte chunk is 8 consecutive d of one row (q / k), 8
    consecutive POSITIONS of one feature (v^T)."""
    x = torch.arange(64 * 128, dtype=torch.float64).reshape(1, 64, 128)               # value = row * 128 + d
    f = R.pack_qk(x)[0]
    for r, d in ((0, 0), (5, 8), (31, 127), (33, 16), (63, 9)):
        off = (r >> 5) * 4096 + ((((d >> 4) * 64 + ((d >> 3) & 1) * 32 + (r & 31)) << 3) + (d & 7))
        assert f[off] == r * 128 + d
    assert torch.equal(f[8:16], x[0, 1, 0:8])                                          # lane 1 of K-step 0: row 1, d 0..7
    assert torch.equal(f[32 * 8:32 * 8 + 8], x[0, 0, 8:16])                            # lane 32: row 0, d 8..15
    fv = R.pack_vt(x)[0]
    assert [R.swz(p) for p in (0, 4, 8, 12, 5, 10, 31)] == [0, 8, 4, 12, 9, 6, 31]
    for p, d in ((0, 0), (4, 3), (9, 40), (31, 127), (32 + 6, 70)):
        pp = p & 31
        off = (p >> 5) * 4096 + (((((d >> 5) * 2 + (pp >> 4)) * 64 + ((pp >> 3) & 1) * 32 + (d & 31)) << 3) + (pp & 7))
        assert fv[off] == ((p & ~31) + R.swz(pp)) * 128 + d
    assert fv[0:8].tolist() == [r * 128 for r in (0, 1, 2, 3, 8, 9, 10, 11)]            # positions 0..7 of feature 0


def test_packers_against_the_mfma_contraction():
    """The transposed flash formulation on one (key tile, query tile) as the layout comment of attention_direct.hip describes it:
    S^T = K Q^T with A = K rows (lane = hh * 32 + key, 8 consecutive d per K-step), B = Q rows; O^T += V^T P^T with A = V^T rows
    (lane = hh * 32 + d, 8 consecutive positions) and B taken from the S^T accumulator in place: slot j of K-step k2 of lane
    (query, hh) holds key (j & 3) + 8 * (2 * k2 + (j >> 2)) + 4 * hh."""
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(1, 64, 128, generator=g, dtype=torch.float64) for _ in range(3))
    Qf, Kf, Vf = (R.pack_qk(q)[0].reshape(2, 8, 64, 8), R.pack_qk(k)[0].reshape(2, 8, 64, 8), R.pack_vt(v)[0].reshape(2, 4, 2, 64, 8))
    for kt in range(2):
        for qt in range(2):
            S = torch.zeros(32, 32, dtype=torch.float64)                               # [key][query]
            for ks in range(8):
                for hh in range(2):
                    S += Kf[kt, ks, hh * 32:hh * 32 + 32] @ Qf[qt, ks, hh * 32:hh * 32 + 32].t()
            want = k[0, kt * 32:kt * 32 + 32] @ q[0, qt * 32:qt * 32 + 32].t()
            assert torch.allclose(S, want, rtol=0, atol=1e-12)
            # the accumulator registers of lane (query i, hh): slot r <-> key (r & 3) + 8 (r >> 2) + 4 hh
            P = torch.randn(32, 32, generator=g, dtype=torch.float64)                  # [key][query]
            OT = torch.zeros(128, 32, dtype=torch.float64)                             # [d][query]
            for t in range(4):
                for k2 in range(2):
                    for hh in range(2):
                        keys = [(j & 3) + 8 * (2 * k2 + (j >> 2)) + 4 * hh for j in range(8)]
                        OT[t * 32:t * 32 + 32] += Vf[kt, t, k2, hh * 32:hh * 32 + 32] @ P[keys]
            assert torch.allclose(OT, v[0, kt * 32:kt * 32 + 32].t() @ P, rtol=0, atol=1e-12)


# ---- cases --------------------------------------------------------------------------------------------------------------------
def test_case_operands():
    names = [c["name"] for c in K.ALL]
    assert len(set(names)) == len(names)
    for B, N, spikes in ((2, 1, True), (3, 33, True), (1, 64, False), (2, 257, True), (1, 520, True)):
        q, k, v = K.make_operands(B, N, spikes)
        npad = (N + 31) // 32 * 32
        assert q.shape == (2 * B, npad, 128)
        assert K.grids_ok(q, k) and all(K.representable(x) for x in (q, k, v))
        if npad > N:
            assert torch.equal(k[:, N:], k[:, N - 1:N].expand(-1, npad - N, -1)) and bool((v[:, N:] == 100).all())
        s = R.scores(q, k, N)
        assert torch.equal(s.to(torch.float32).to(torch.float64), s)                  # exact in fp32
        if N > 40:
            plain = s[:, torch.arange(N) % 4 != 1]
            p_last = torch.exp2(plain[..., N - 1] - plain.max(dim=-1).values)
            assert p_last.median() >= 0.3, float(p_last.median())                      # the sentinel is near the row maximum
            if spikes:
                spiked = s[:, torch.arange(N) % 4 == 1]
                js = K.spike_keys(N)
                assert len(js) == 3
                for j in js:                                                          # every spike is a move of the reference maximum
                    before = spiked[..., :j].max(dim=-1).values
                    assert bool((spiked[..., j] > before + R.LAG).all())


def test_parts_cover_every_row_once_per_slot():
    for c in K.ALL:
        N = c["N"]
        parts = K.parts_of(c)
        by_rows = {}
        for p in parts:
            by_rows.setdefault(p["rows"], []).append(p["keys"])
            assert p["keys"][0] < p["keys"][1] or p["rows"][0] == p["rows"][1], (c["name"], p)
        assert sorted(by_rows)[0][0] == 0 and max(r[1] for r in by_rows) == N
        for rows, keys in by_rows.items():
            keys = sorted(keys)
            assert keys[0][0] == 0 and keys[-1][1] == N and all(a[1] == b[0] for a, b in zip(keys, keys[1:])), (c["name"], keys)


def test_merge_of_reference_partials_is_the_full_reference():
    q, k, v = K.make_operands(2, 257)
    s = R.scores(q, k, 257)
    O, A, M, L = R.attention(s, v)
    cuts = (0, 96, 160, 257)
    parts = [R.attention(s, v, lo, hi) for lo, hi in zip(cuts, cuts[1:])]
    Om, Mm, Lm = R.merge([(p[2], p[3], p[0]) for p in parts])
    assert torch.allclose(Om, O, rtol=0, atol=1e-13) and torch.equal(Mm, M) and torch.allclose(Lm, L, rtol=1e-13, atol=0)


# ---- the bound: the emulation inside, every mutant outside -------------------------------------------------------------------
def _ratio(O, ref, tol):
    return ((O.to(torch.float64) - ref).abs() / tol).max().item()


_FULL = {}


def _full(N):
    if N not in _FULL:
        _FULL[N] = _full_uncached(N)
    return _FULL[N]


def _full_uncached(N):
    q, k, v, Qf, Kf, Vf = _lp_ops(2, N)
    s = R.scores(q, k, N)
    O, A, M, L = R.attention(s, v)
    return q, k, v, Qf, Kf, Vf, s, O, A, M, L


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("prec", K.PRECS)
def test_emulation_within_bound(N, prec):
    q, k, v, Qf, Kf, Vf, s, O, A, M, L = _full(N)
    vmax = v[:, :N].abs().max(dim=1).values
    for out_lp in (False, True):
        Oe, me, le = R.emulate(Qf, Kf, Vf, N, prec, out_lp=out_lp)
        r = _ratio(Oe, O, R.tolerance(O, A, vmax, N, prec, out_lp))
        r_m, r_l = R.ml_ratios(me, le, M, L, N)
        print(f"N={N} {prec} out_lp={out_lp}: max err/tol {r:.4f}  m {r_m:.4f}  l {r_l:.4f}")
        assert r <= 1.0 and r_m <= 1.0 and r_l <= 1.0, (r, r_m, r_l)
        assert bool((me < M).any()), "the inputs never make the reference maximum lag"
    # key split by 32-key tiles, merged in fp64
    nt = (N + 31) // 32
    cut = nt // 2
    a, b = R.emulate(Qf, Kf, Vf, N, prec, 0, cut), R.emulate(Qf, Kf, Vf, N, prec, cut, nt)
    refs, tols = [], []
    for (lo, hi), (Oe, me, le) in (((0, cut * 32), a), ((cut * 32, N), b)):
        Or, Ar, Mr, Lr = R.attention(s, v, lo, hi)
        tol = R.tolerance(Or, Ar, v[:, lo:hi].abs().max(dim=1).values, N, prec, False)
        assert _ratio(Oe, Or, tol) <= 1.0 and max(R.ml_ratios(me, le, Mr, Lr, N)) <= 1.0
        refs.append((Mr, Lr, Or)); tols.append(tol)
    Om, _, _ = R.merge([(x[1].to(torch.float64), x[2].to(torch.float64), x[0].to(torch.float64)) for x in (a, b)])
    r = _ratio(Om, O, R.merged_tolerance(refs, tols, N))
    print(f"N={N} {prec} merged: max err/tol {r:.4f}")
    assert r <= 1.0


MUTANTS = ("drop_last", "admit_pad", "no_swap", "skip_tile", "tile_twice", "wrong_m", "row_off", "heads_swapped")


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("prec", K.PRECS)
def test_mutants_exceed_bound(N, prec, mutant):
    q, k, v, Qf, Kf, Vf, s, O, A, M, L = _full(N)
    nt = (N + 31) // 32
    cut = max(nt // 2, 1)
    d64 = lambda x: tuple(t.to(torch.float64) for t in x)
    if mutant in ("tile_twice", "wrong_m"):
        hi0 = cut + 1 if mutant == "tile_twice" else cut                               # tile `cut` counted in both splits
        a, b = d64(R.emulate(Qf, Kf, Vf, N, prec, 0, hi0)), d64(R.emulate(Qf, Kf, Vf, N, prec, cut, nt))
        if mutant == "wrong_m":
            a, b = (a[0], b[1], a[2]), (b[0], a[1], b[2])
        Oe, _, _ = R.merge([(a[1], a[2], a[0]), (b[1], b[2], b[0])])
        refs, tols = [], []
        for lo, hi in ((0, cut * 32), (cut * 32, N)):
            Or, Ar, Mr, Lr = R.attention(s, v, lo, hi)
            refs.append((Mr, Lr, Or)); tols.append(R.tolerance(Or, Ar, v[:, lo:hi].abs().max(dim=1).values, N, prec, False))
        tol = R.merged_tolerance(refs, tols, N)
    else:
        m = ("skip_tile", nt // 3) if mutant == "skip_tile" else None if mutant == "heads_swapped" else mutant
        Oe, _, _ = R.emulate(Qf, Kf, Vf, N, prec, mutant=m)
        if mutant == "heads_swapped":
            Oe = Oe.reshape(2, 2, N, 128).flip(1).reshape(4, N, 128)
        tol = R.tolerance(O, A, v[:, :N].abs().max(dim=1).values, N, prec, False)
    r = _ratio(Oe, O, tol)
    print(f"N={N} {prec} {mutant}: max err/tol {r:.1f}")
    assert r > 1.0, r
