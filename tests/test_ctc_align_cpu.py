"""CPU: the float64 restatement of the CTC alignment contract (tests/ctc_ref.py) against torch's ``F.ctc_loss`` in double precision
and against brute-force enumeration, and the host side of dex_tts_amd/ctc_align.py.  The GPU tests hold the device to the
restatement (tests/test_gpu_ctc_align.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ctc_ref as R

EPS = 2.0 ** -53


def bound(T, v):
    """Each of the T steps costs a handful of fp64 roundings of the running magnitude, on both sides."""
    return 16 * T * EPS * max(1.0, abs(v))


def torch_nll(x, y):
    lp = torch.log_softmax(torch.from_numpy(x).double(), dim=-1)[:, None, :]
    return float(F.ctc_loss(lp, torch.from_numpy(np.asarray(y, np.int64))[None], torch.tensor([x.shape[0]]), torch.tensor([len(y)]),
                            blank=0, reduction="none", zero_infinity=False)[0])


_NLL = {}


def nll_of(case):
    if case not in _NLL:
        x, y = R.make_case(*case)
        _NLL[case] = (R.ctc_nll(x, y), torch_nll(x, y))
    return _NLL[case]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "seed%d_T%d_L%d_V%d" % c)
def test_restatement_nll_is_torch_ctc_loss(case):
    got, ref = nll_of(case)
    d, b = abs(got - ref), bound(case[1], ref)
    print(f"{case}: nll {got:.6f}, |d| {d:.3e}, bound {b:.3e}, share {d / b:.3f}")
    assert np.isfinite(ref) and d <= b


def test_exact_fit_and_infeasible_row():
    x, y = R.make_case(2, 33, 7, 32)
    need = len(y) + R.repeats(y)
    assert need == 10, "seed 2 is the exact-fit case: L + R = 10"
    got, ref = R.ctc_nll(x[:10], y), torch_nll(x[:10], y)
    assert np.isfinite(ref) and abs(got - ref) <= bound(10, ref)
    assert R.ctc_nll(x[:9], y) == np.inf and torch_nll(x[:9], y) == np.inf
    al = R.ctc_align(x[:10], y)
    assert (al["spans"][:, 1] - al["spans"][:, 0] == 1).all()          # one frame per symbol, a blank between equal neighbours
    assert al["score"] <= -got + bound(10, got)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "seed%d_T%d_L%d_V%d" % c)
def test_best_path_is_no_likelier_than_the_text(case):
    x, y = R.make_case(*case)
    al, nll = R.ctc_align(x, y), nll_of(case)[0]
    assert al["score"] <= -nll + bound(case[1], nll)
    st = al["states"]
    assert st[0] in (0, 1) and st[-1] in (2 * len(y), 2 * len(y) - 1 if len(y) else 0)
    assert (al["spans"][:, 1] > al["spans"][:, 0]).all()
    assert ((al["token_scores"] > 0) & (al["token_scores"] <= 1)).all()


def small_cases():
    """Everything brute force can enumerate: T <= 6, L <= 3, V <= 4, repeats included, seeded normal logits and the tie cases."""
    out = []
    for seed, (T, y, V) in enumerate([(1, [1], 2), (2, [1], 2), (3, [1, 1], 3), (4, [1, 2], 3), (5, [2, 2, 1], 4), (6, [1, 2, 3], 4), (6, [3, 3, 3], 4),
                                      (6, [1, 1], 2), (5, [], 3), (6, [2, 1, 2], 4), (6, [1, 2, 2], 4)]):
        g = np.random.default_rng(200 + seed)
        out.append((f"normal_T{T}_{y}", (g.standard_normal((T, V)) * 3).astype(np.float32), np.array(y, np.int64)))
        out.append((f"ints_T{T}_{y}", g.integers(-1, 2, (T, V)).astype(np.float32), np.array(y, np.int64)))
        out.append((f"zeros_T{T}_{y}", np.zeros((T, V), np.float32), np.array(y, np.int64)))
    return out + [c for c in R.tie_cases() if c[1].shape[0] <= 6 and len(c[2]) <= 3]


@pytest.mark.parametrize("name,x,y", small_cases(), ids=[c[0] for c in small_cases()])
def test_viterbi_against_brute_force(name, x, y):
    feasible = len(y) + R.repeats(y) <= x.shape[0]
    best, arg = R.brute_force(x, y)
    al = R.ctc_align(x, y)
    if not feasible:
        assert best == -np.inf and not arg and al["raw_score"] == -np.inf and (al["states"] == -1).all()
        return
    assert al["raw_score"] == best                                    # the same fp64 adds in the same order: equal, not close
    assert tuple(al["states"]) in arg
    assert R.path_score(x, y, al["states"]) == best


def test_tie_rule_goldens():
    """Worked by hand from the rule (stay, then step, then skip; the last state unless the one before is strictly better)."""
    t = {c[0]: c for c in R.tie_cases()}
    assert R.ctc_align(*t["zeros_T4_y1"][1:])["states"].tolist() == [1, 2, 2, 2]
    assert R.ctc_align(*t["zeros_T4_y12"][1:])["states"].tolist() == [1, 3, 4, 4]
    al = R.ctc_align(*t["zeros_T4_y12"][1:])
    assert al["spans"].tolist() == [[0, 1], [1, 2]]
    np.testing.assert_allclose(al["token_scores"], [0.25, 0.25], rtol=1e-15)
    # a strictly better last symbol is the final state
    x = np.zeros((3, 3), np.float32)
    x[2, 1] = 1.0
    assert R.ctc_align(x, np.array([1]))["states"].tolist() == [1, 1, 1]
    x[2, 0] = 1.0
    assert R.ctc_align(x, np.array([1]))["states"].tolist() == [1, 2, 2]


# ---------------------------------------------------------------------------------------------------------------- host functions
def test_text_to_targets():
    from dex_tts_amd import asr
    from dex_tts_amd.ctc_align import text_to_targets
    V = {s: i for i, s in enumerate(asr.VOCAB)}
    ids, words = text_to_targets("  Don't stop,  now! ")
    assert words == ["DON'T", "STOP", "NOW"]
    assert ids == [V[c] for c in "DON'T|STOP|NOW"]
    assert ids[0] != V["|"] and ids[-1] != V["|"]
    with pytest.raises(ValueError, match=r"'7'.*position 5"):
        text_to_targets("room 7")
    assert text_to_targets("room 7 , here", unknown="drop") == ([V[c] for c in "ROOM|HERE"], ["ROOM", "HERE"])
    assert text_to_targets(" -- ... ") == ([], [])
    assert text_to_targets("") == ([], [])
    with pytest.raises(ValueError, match="position 1"):
        text_to_targets("né")
    with pytest.raises(ValueError):
        text_to_targets("a", unknown="keep")


@pytest.fixture(scope="module")
def lib():
    from dex_tts_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from dex_tts_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_workspace_bytes_refuses_bad_arguments(lib):
    assert lib.dex_ctc_workspace_bytes(1, 199, 32, 60) > 199 * 8
    assert lib.dex_ctc_workspace_bytes(1024, 4096, 65536, 0) > 0
    for bad in [(0, 10, 32, 4), (1025, 10, 32, 4), (1, 0, 32, 4), (1, 4097, 32, 4), (1, 10, 0, 4), (1, 10, 65537, 4), (1, 10, 32, -1), (1, 10, 32, 1024)]:
        assert lib.dex_ctc_workspace_bytes(*bad) == 0, bad
    # back-pointers that fit LDS need no room; the others get (2 Lmax + 1) ceil(T / 16) words per row
    small, large = lib.dex_ctc_workspace_bytes(1, 199, 32, 60), lib.dex_ctc_workspace_bytes(1, 4096, 32, 1023)
    assert small < 8192 and large >= 2047 * 256 * 4
    assert lib.dex_ctc_workspace_bytes(2, 4096, 32, 1023) - large >= 2047 * 256 * 4


def test_python_refusals():
    from dex_tts_amd.ctc_align import check_targets
    fr, tg, tl = check_targets(2, 10, 5, None, [[1, 2], []], feasible=True)
    assert fr.tolist() == [10, 10] and tg.tolist() == [[1, 2], [0, 0]] and tl.tolist() == [2, 0]
    assert fr.dtype == tg.dtype == tl.dtype == np.int32
    fr, tg, tl = check_targets(1, 10, 5, [4], np.array([[1, 1, 3, 9]]), [3])
    assert tg.tolist() == [[1, 1, 3]] and tl.tolist() == [3]
    with pytest.raises(ValueError, match="row 1 holds the blank"):
        check_targets(2, 10, 5, None, [[1], [2, 0]])
    with pytest.raises(ValueError, match="row 0 holds the id 5"):
        check_targets(1, 10, 5, None, [[1, 5]])
    with pytest.raises(ValueError, match="row 1 cannot be aligned.*need 4 frames.*has 3"):
        check_targets(2, 10, 5, [10, 3], [[1, 1], [1, 1, 2]], feasible=True)
    check_targets(2, 10, 5, [10, 3], [[1, 1], [1, 1, 2]], feasible=False)      # the likelihood takes it (+inf)
    with pytest.raises(ValueError, match="1024 target symbols"):
        check_targets(1, 4096, 5, None, [[1, 2] * 512])
    with pytest.raises(ValueError, match="4097 frames"):
        check_targets(1, 4097, 5, None, [[1]])
    with pytest.raises(ValueError, match="blank 5"):
        check_targets(1, 10, 5, None, [[1]], blank=5)
    with pytest.raises(ValueError):
        check_targets(1, 10, 5, [11], [[1]])
    with pytest.raises(ValueError, match="2 targets for 1 rows"):
        check_targets(1, 10, 5, None, [[1], [2]])
    with pytest.raises(ValueError, match="MI355X only"):
        from dex_tts_amd.ctc_align import ctc_align
        ctc_align(torch.zeros(4, 5), None, [1])


def test_speaking_rate_and_word_alignment():
    from dex_tts_amd import asr
    from dex_tts_amd.ctc_align import speaking_rate, text_to_targets, word_alignment
    al = {"words": [{"word": "A", "start": 0.5, "end": 0.9, "score": 1.0}, {"word": "B", "start": 1.0, "end": 1.5, "score": 1.0},
                    {"word": "C", "start": 2.0, "end": 2.5, "score": 1.0}]}
    assert speaking_rate(al) == 3 / 2.0
    with pytest.raises(ValueError):
        speaking_rate({"words": []})
    ids, words = text_to_targets("it's ok")
    spans = np.array([[0, 2], [2, 3], [4, 5], [5, 6], [6, 8], [9, 10], [10, 13]])
    tok = np.array([0.5, 1.0, 0.25, 0.75, 0.125, 0.5, 1.0])
    row = word_alignment(ids, words, spans, tok, -3.0, 4.0, 13, 4100, 320, asr.VOCAB)
    assert [c["char"] for c in row["chars"]] == list("IT'SOK")
    assert [w["word"] for w in row["words"]] == ["IT'S", "OK"]
    assert row["words"][0]["start"] == 0.0 and row["words"][0]["end"] == 6 * 320 / 16000
    assert row["words"][0]["score"] == (2 * 0.5 + 1.0 + 0.25 + 0.75) / 5
    assert row["words"][1]["start"] == 9 * 320 / 16000 and row["words"][1]["end"] == 4100 / 16000     # clipped to the row's samples
    assert row["words"][1]["score"] == (0.5 + 3 * 1.0) / 4
    assert row["score"] == -3.0 and row["nll"] == 4.0 and row["frames"] == 13
    assert speaking_rate(row) == 2 / (4100 / 16000)
