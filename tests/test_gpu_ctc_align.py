"""GPU: CTC forced alignment and text likelihood (dex_tts_amd/ctc_align.py, csrc/ctc_align.hip) against the float64 restatement
(tests/ctc_ref.py, itself held to ``F.ctc_loss`` and to brute force by tests/test_ctc_align_cpu.py).

Paths and spans must be IDENTICAL to the restatement: the path is decided by exact fp64 adds and compares on the raw logits, so no
margin condition is needed and the tie cases are included.  Values: ``16 T 2^-53 max(1, |v|)`` for the two sums (``score``, ``nll``),
``1e-12`` absolute for the token probabilities (a mean of values <= 1, each exact to a few ulp of ``|log p| <= ~40``).

Which kernel form and which back-pointer placement a case exercises (``FORMS``; ``test_forms_are_what_the_table_says`` recomputes
the table from the launch rule so that it cannot go stale): the register form holds R states per lane of one wave (S <= 512), the
LDS form one or two states per thread; the back-pointers sit in LDS while S ceil(T / 16) words fit beside the column, else in the
workspace."""
import numpy as np
import pytest
import torch

from tests import asr_ref as A
from tests import ctc_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
EXTRA = [(18, 4096, 100, 32)]                 # the register form with its back-pointers in the workspace
# (seed, T, L, V) -> (form, states per thread, back-pointer placement); the seam each case sits on
FORMS = {
    (0, 1, 1, 5): ("reg", 1, "lds"),          # one frame
    (1, 4, 3, 5): ("reg", 1, "lds"),
    (2, 33, 7, 32): ("reg", 1, "lds"),        # T = 33: the third back-pointer word holds one frame
    (3, 65, 31, 32): ("reg", 1, "lds"),       # S = 63: the last lane idle; T = 65
    (4, 70, 32, 32): ("reg", 2, "lds"),       # S = 65: two states per lane
    (5, 199, 40, 32): ("reg", 2, "lds"),
    (6, 130, 33, 300): ("reg", 2, "lds"),     # V = 300: five passes of the normaliser
    (7, 12, 0, 32): ("reg", 1, "lds"),        # L = 0
    (8, 300, 120, 32): ("reg", 4, "lds"),
    (9, 2100, 1023, 32): ("lds", 2, "workspace"),
    (10, 4096, 512, 32): ("lds", 2, "workspace"),
    (11, 40, 20, 3): ("reg", 1, "lds"),
    (12, 600, 255, 32): ("reg", 8, "lds"),    # S = 511: the widest register form
    (13, 600, 256, 32): ("lds", 1, "lds"),    # S = 513: the LDS form
    (14, 1100, 511, 32): ("lds", 1, "workspace"),   # S = 1023: one state per thread
    (15, 1100, 512, 32): ("lds", 2, "workspace"),   # S = 1025: two states per thread
    (17, 2, 1, 2): ("reg", 1, "lds"),         # V = 2
    (18, 4096, 100, 32): ("reg", 4, "workspace"),
}
ALL = R.CASES + EXTRA


def launch_rule(T, L):
    """csrc/ctc_align.hip plan_for / run, restated."""
    S = 2 * L + 1
    if S <= 512:
        form, r = "reg", 1
        while r * 64 < S:
            r *= 2
        ns = 0
    else:
        form, r = "lds", 1 if S <= 1024 else 2
        ns = (-(-S // r) + 63) // 64 * 64 * r
    fits = 32 + 2 * ns * 8 + 4 * S * ((T + 15) // 16) <= 160 * 1024
    return form, r, "lds" if fits else "workspace"


def test_forms_are_what_the_table_says():
    assert set(FORMS) == set(ALL)
    for (seed, T, L, V), want in FORMS.items():
        assert launch_rule(T, L) == want, (seed, T, L, V)
    assert {f[:1] + f[2:] for f in FORMS.values()} == {("reg", "lds"), ("reg", "workspace"), ("lds", "lds"), ("lds", "workspace")}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_REF = {}


def ref_of(key, x=None, y=None):
    """The restatement of one utterance: computed once and shared, never changed."""
    if key not in _REF:
        if x is None:
            x, y = R.make_case(*key)
        _REF[key] = (x, y, R.ctc_align(x, y), R.ctc_nll(x, y))
    return _REF[key]


def sum_bound(T, v):
    return 16 * T * EPS * max(1.0, abs(v))


def check_row(what, got, x, y, al, nll):
    """One row of the device's outputs (host arrays) against the restatement; figures first, then the assertions."""
    T, L = x.shape[0], len(y)
    ds, dn = abs(got["score"] - al["score"]), abs(got["nll"] - nll)
    dp = float(np.abs(got["token_scores"][:L] - al["token_scores"]).max()) if L else 0.0
    print(f"{what}: states equal {np.array_equal(got['states'][:T], al['states'])}, spans equal {np.array_equal(got['spans'][:L], al['spans'])}, "
          f"|d score| {ds:.3e} (bound {sum_bound(T, al['score']):.3e}), |d nll| {dn:.3e} (bound {sum_bound(T, nll):.3e}), "
          f"|d p| max {dp:.3e} (bound 1e-12)")
    assert np.array_equal(got["states"][:T], al["states"])
    assert np.array_equal(got["spans"][:L], al["spans"])
    assert ds <= sum_bound(T, al["score"]) and dn <= sum_bound(T, nll)
    assert dp <= 1e-12


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def align_one(x, y):
    from dex_tts_amd.ctc_align import ctc_align
    return host(ctc_align(cuda(x), None, [int(v) for v in y]))


@pytest.mark.parametrize("case", ALL, ids=lambda c: "seed%d_T%d_L%d_V%d" % c)
def test_paths_bitwise_and_values(case):
    x, y, al, nll = ref_of(case)
    got = align_one(x, y)
    assert got["states"].shape == (x.shape[0],) and got["spans"].shape == (max(len(y), 1), 2)
    check_row(f"{case} {FORMS[case]}", got, x, y, al, nll)


@pytest.mark.parametrize("name", [c[0] for c in R.tie_cases()])
def test_tie_cases_bitwise(name):
    _, x, y = next(c for c in R.tie_cases() if c[0] == name)
    x, y, al, nll = ref_of(("tie", name), x, y)
    check_row(name, align_one(x, y), x, y, al, nll)


def test_exact_fit_and_infeasible_row():
    from dex_tts_amd.ctc_align import ctc_align, ctc_nll
    x, y = R.make_case(2, 33, 7, 32)
    assert len(y) + R.repeats(y) == 10
    x10, y, al, nll = ref_of(("fit", 10), x[:10], y)
    check_row("exact fit", align_one(x10, y), x10, y, al, nll)
    # the same utterance inside a longer buffer, cut by frames
    got = host(ctc_align(cuda(x), [10], [int(v) for v in y]))
    check_row("exact fit by frames", got, x10, y, al, nll)
    assert (got["states"][10:] == -1).all()
    inf = ctc_nll(cuda(x[None]), [9], [[int(v) for v in y]]).cpu().numpy()
    print("infeasible row: nll", inf)
    assert inf.shape == (1,) and inf[0] == np.inf
    with pytest.raises(ValueError, match="row 0 cannot be aligned"):
        ctc_align(cuda(x[None]), [9], [[int(v) for v in y]])


RAGGED = [R.CASES[i] for i in (1, 2, 5, 7, 8)]


def ragged_batch():
    """Cases 1, 2, 5, 7, 8 as the rows of one call, padded to T = 300 and Lmax = 120 with garbage behind each row's frames and target."""
    g = np.random.default_rng(77)
    B, T, Lm, V = len(RAGGED), 300, 120, 32
    x = (g.standard_normal((B, T, V)) * 50).astype(np.float32)
    tg = g.integers(0, 1000, (B, Lm)).astype(np.int64)                # garbage ids: the blank and ids >= V among them
    fr, tl = [], []
    for b, c in enumerate(RAGGED):
        xb, yb = R.make_case(*c)
        xb = np.pad(xb, ((0, 0), (0, V - xb.shape[1])), constant_values=-np.inf) if xb.shape[1] < V else xb
        x[b, :xb.shape[0]] = xb
        tg[b, :len(yb)] = yb
        fr.append(xb.shape[0])
        tl.append(len(yb))
    return x, tg, fr, tl


def test_ragged_batch_rows_are_the_rows_alone():
    from dex_tts_amd.ctc_align import ctc_align, ctc_nll
    x, tg, fr, tl = ragged_batch()
    got = host(ctc_align(cuda(x), fr, tg, tl))
    nll = ctc_nll(cuda(x), fr, tg, tl).cpu().numpy()
    assert got["states"].shape == (5, 300) and got["spans"].shape == (5, 120, 2) and got["token_scores"].shape == (5, 120)
    for b, c in enumerate(RAGGED):
        T, L = fr[b], tl[b]
        xa = np.ascontiguousarray(x[b, :T])
        alone = align_one(xa, tg[b, :L])
        for k in ("states", "spans", "token_scores", "score", "nll"):
            n = {"states": T, "spans": L, "token_scores": L}.get(k)
            a, g = (alone[k], got[k][b]) if n is None else (alone[k][:n], got[k][b][:n])
            assert np.asarray(a).tobytes() == np.asarray(g).tobytes(), (c, k)
        assert nll[b].tobytes() == got["nll"][b].tobytes()
        assert (got["states"][b, T:] == -1).all() and (got["spans"][b, L:] == -1).all() and np.isnan(got["token_scores"][b, L:]).all()
        if c[3] == 32:                                                  # (case 1 has V = 5: padded with -inf columns, another utterance)
            xr, yr, al, nl = ref_of(c)
            check_row(f"ragged row {b}", {k: got[k][b] for k in got}, xr, yr, al, nl)


def test_rows_without_an_alignment():
    from dex_tts_amd.ctc_align import ctc_align
    x, tg, fr, tl = ragged_batch()
    base = host(ctc_align(cuda(x), fr, tg, tl))
    for what, row in (("-inf", 2), ("nan", 4)):
        xe = x.copy()
        if what == "-inf":
            xe[row, :, tg[row, 3]] = -np.inf                           # one of the row's target ids in every frame
        else:
            xe[row, 17, 5] = np.nan                                    # one logit
        got = host(ctc_align(cuda(xe), fr, tg, tl))
        T, L = fr[row], tl[row]
        print(f"{what}: score {got['score'][row]}, nll {got['nll'][row]}")
        if what == "-inf":
            assert got["score"][row] == -np.inf and got["nll"][row] == np.inf
        else:
            assert np.isnan(got["score"][row]) and np.isnan(got["nll"][row])
        assert (got["states"][row] == -1).all() and (got["spans"][row] == -1).all() and np.isnan(got["token_scores"][row]).all()
        for b in range(len(fr)):
            if b != row:
                for k in got:
                    assert got[k][b].tobytes() == base[k][b].tobytes(), (what, b, k)


# ---------------------------------------------------------------------------------------------------------------- through the network
_MODEL = {}


def model():
    if "m" not in _MODEL:
        from dex_tts_amd import asr
        sd = A.make_weights(A.TINY, 0)
        m = asr.Wav2Vec2CTC(A.library_config(A.TINY), "cuda")
        _MODEL["m"] = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return _MODEL["m"]


TEXTS = ["It's a cab, ok", "no way"]
SAMPLES = [6000, 4100]


def check_alignment_rows(rows, logits, ln, texts, m):
    """``align``'s rows against ``ctc_align`` of the same logits: bit for bit, words rebuilt on the host from the states, times by the
    stated arithmetic."""
    from dex_tts_amd import asr
    from dex_tts_amd.ctc_align import ctc_align, ctc_nll, text_to_targets
    pairs = [text_to_targets(t, m.vocab) for t in texts]
    fr = [asr.num_frames(int(n), m.config) for n in ln]
    got = host(ctc_align(logits, fr, [p[0] for p in pairs]))
    nll = ctc_nll(logits, fr, [p[0] for p in pairs]).cpu().numpy()
    for b, (ids, words) in enumerate(pairs):
        row = rows[b]
        assert row["frames"] == fr[b] and row["score"] == got["score"][b] and row["nll"] == got["nll"][b] == nll[b]
        st = got["states"][b, :fr[b]]
        keep = [l for l, i in enumerate(ids) if m.vocab[i] != "|"]
        assert [c["char"] for c in row["chars"]] == [m.vocab[ids[l]] for l in keep]
        for c, l in zip(row["chars"], keep):
            t = np.nonzero(st == 2 * l + 1)[0]
            assert c["start"] == t[0] * 320 / 16000 and c["end"] == min((t[-1] + 1) * 320, int(ln[b])) / 16000
            assert c["score"] == got["token_scores"][b, l]
        assert [w["word"] for w in row["words"]] == words
        first = 0
        for w, word in zip(row["words"], words):                      # a word's symbols are consecutive target positions
            ls = list(range(first, first + len(word)))
            first += len(word) + 1
            t0 = np.nonzero(st == 2 * ls[0] + 1)[0][0]
            t1 = np.nonzero(st == 2 * ls[-1] + 1)[0][-1] + 1
            assert w["start"] == t0 * 320 / 16000 and w["end"] == min(t1 * 320, int(ln[b])) / 16000
            n = [int((st == 2 * l + 1).sum()) for l in ls]
            want = sum(k * got["token_scores"][b, l] for k, l in zip(n, ls)) / sum(n)
            assert abs(w["score"] - want) <= 4 * EPS
    return got


def test_align_through_the_network():
    from dex_tts_amd.ctc_align import speaking_rate
    m = model()
    x = np.zeros((2, max(SAMPLES)), np.float32)
    for b, n in enumerate(SAMPLES):
        x[b, :n] = A.synth_wav(n, 40 + b)
    wav = cuda(x)
    logits = m.forward(wav, SAMPLES)
    rows = m.align(wav, TEXTS, lengths=SAMPLES)
    got = check_alignment_rows(rows, logits, SAMPLES, TEXTS, m)
    assert rows[0]["frames"] == 18 and rows[1]["frames"] == 12
    tn = m.text_nll(wav, TEXTS, lengths=SAMPLES)
    assert tn.dtype == torch.float64 and tn.is_cuda and tn.cpu().numpy().tobytes() == got["nll"].tobytes()
    assert speaking_rate(rows[0]) > 0
    with pytest.raises(ValueError, match="row 1 cannot be aligned"):
        m.align(wav, [TEXTS[0], "far too many symbols for twelve frames"], lengths=SAMPLES)
    with pytest.raises(ValueError, match="'7'"):
        m.align(wav, ["a 7", "b"], lengths=SAMPLES)


def test_align_scores_resamples_int16_waveforms():
    from dex_tts_amd import synthesize
    from dex_tts_amd._native import pad_wavs, resample_to_16k
    m = model()
    audio = [(A.synth_wav(n, 50 + b, amp=0.3) * 32767).astype(np.int16) for b, n in enumerate((8400, 6100))]
    rows, mean, err = synthesize.align_scores(m, audio, TEXTS, sr=22050)
    xw, lw = pad_wavs(audio, m.device, scale_int16=True)
    x16, l16 = resample_to_16k(xw, lw, 22050)
    want = m.align(x16, TEXTS, lengths=l16)
    assert rows == want
    check_alignment_rows(rows, m.forward(x16, l16), l16, TEXTS, m)
    per = [r["nll"] / n for r, n in zip(rows, (13, 6))]                 # "IT'S|A|CAB|OK" has 13 symbols, "NO|WAY" 6
    assert mean == sum(per) / 2 and err == float(np.std(per) / np.sqrt(2))
