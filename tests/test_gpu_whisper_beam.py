"""GPU: Whisper beam search (dex_tts_amd/whisper.py ``generate_beam``, csrc/whisper.hip) - the two beam attention forms and the step
tail one launch at a time, then the whole search against its float64 restatement (tests/whisper_beam_ref.py, itself held to
``transformers``' beam search by tests/test_whisper_beam_cpu.py).  Tolerances of float results are those of tests/test_gpu_whisper.py
(``whisper_ref.tolerance`` with the fp32 CPU yardstick); selections are compared exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_gpu_whisper as G
from tests import whisper_beam_ref as BR
from tests import whisper_ref as R

pytestmark = pytest.mark.gpu

cuda, check = G.cuda, G.check
SHAPES = [(U, K, H) for U in (1, 3) for K in (2, 5, 8) for H in (1, 3)]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from dex_tts_amd import _lib
    return _lib.load()


def _attend(q, k, v, n, cap, nk=None, nv=None):
    """dex_whisper_attend on rows q [B, H, 64] against k, v [B, cap, H, 64] (device tensors; k and v are written where nk is given)."""
    B, H = q.shape[:2]
    out = torch.full((B, H * 64), float("nan"), device="cuda")
    rc = _lib().dex_whisper_attend(q.data_ptr(), k.data_ptr(), v.data_ptr(), nk.data_ptr() if nk is not None else None,
                                   nv.data_ptr() if nv is not None else None, out.data_ptr(), B, H, n, cap, _stream())
    assert rc == 0
    return out.cpu().numpy().reshape(B, H, 64)


def _attend_beam(q, k, v, n, cap, U, K, anc=None, nk=None, nv=None):
    H = q.shape[1]
    out = torch.full((U * K, H * 64), float("nan"), device="cuda")
    rc = _lib().dex_whisper_attend_beam(q.data_ptr(), k.data_ptr(), v.data_ptr(), nk.data_ptr() if nk is not None else None,
                                        nv.data_ptr() if nv is not None else None, anc.data_ptr() if anc is not None else None,
                                        anc.shape[1] if anc is not None else 0, out.data_ptr(), U, K, H, n, cap, _stream())
    assert rc == 0
    return out.cpu().numpy().reshape(U * K, H, 64)


# ---------------------------------------------------------------------------------------------------- beam attention, cross form
@pytest.mark.parametrize("U,K,H", SHAPES)
@pytest.mark.parametrize("S", [50, 150, 1500])
def test_attend_beam_cross(S, U, K, H):
    """One workgroup per (head, utterance) serves the K queries from one pass over the utterance's keys: every row is BITWISE
    dex_whisper_attend of that query against its utterance's K / V, and within the bound of float64."""
    rng = np.random.default_rng(S + 10 * K + U + H)
    q = rng.standard_normal((U * K, H, 64)).astype(np.float32) * 2
    k = rng.standard_normal((U, S, H, 64)).astype(np.float32)
    v = rng.standard_normal((U, S, H, 64)).astype(np.float32)
    got = _attend_beam(cuda(q), cuda(k), cuda(v), S, S, U, K)
    kr, vr = np.repeat(k, K, axis=0), np.repeat(v, K, axis=0)
    alone = _attend(cuda(q), cuda(kr), cuda(vr), S, S)
    assert np.array_equal(got, alone), f"differs from the plain kernel by {np.abs(got - alone).max():.3e}"
    check(f"attend_beam cross S={S} U={U} K={K} H={H}", got, G._softmax_attend(q, kr, vr, np.float64), G._softmax_attend(q, kr, vr, np.float32))


def test_attend_beam_refuses_more_scores_than_lds_holds():
    z = torch.zeros(8 * 2000 * 64, device="cuda")
    lib = _lib()
    args = (z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, None, 0, z.data_ptr(), 1)
    assert lib.dex_whisper_attend_beam(*args, 8, 1, 2000, 2000, _stream()) != 0          # 16000 scores
    assert lib.dex_whisper_attend_beam(*args, 9, 1, 50, 50, _stream()) != 0
    assert lib.dex_whisper_attend_beam(*args, 1, 1, 50, 50, _stream()) != 0


# ---------------------------------------------------------------------------------------------------- beam attention, self form
@pytest.mark.parametrize("U,K,H", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 448])
def test_attend_beam_self(n, U, K, H):
    """Row r appends its k and v at position n - 1 of its own row and reads position t < n - 1 from row anc[r][t] of its utterance:
    held to float64 on the gathered keys; with the identity table BITWISE dex_whisper_attend; the appended key lands in the row's own
    slot and a 1e30 sentinel everywhere else in the cache is intact."""
    rng = np.random.default_rng(n * 7 + 10 * K + U + H)
    B, cap = U * K, n + 3
    q = rng.standard_normal((B, H, 64)).astype(np.float32) * 2
    k = rng.standard_normal((B, cap, H, 64)).astype(np.float32)
    v = rng.standard_normal((B, cap, H, 64)).astype(np.float32)
    kd, vd = k.copy(), v.copy()
    kd[:, n - 1:], vd[:, n - 1:] = 1e30, -1e30
    nk, nv = cuda(k[:, n - 1]), cuda(v[:, n - 1])
    ident = np.tile((np.arange(B) % K)[:, None], (1, cap)).astype(np.int32)
    anc = rng.integers(0, K, (B, cap)).astype(np.int32)
    anc[:, n - 1:] = -7                                                  # never read: the appended position is the row's own
    rows = (np.arange(B) // K * K)[:, None] + anc[:, : n - 1]            # the cache row that holds position t of row r
    kg, vg = k[:, :n].copy(), v[:, :n].copy()
    kg[:, : n - 1], vg[:, : n - 1] = k[rows, np.arange(n - 1)[None]], v[rows, np.arange(n - 1)[None]]
    tk, tv = cuda(kd), cuda(vd)
    got = _attend_beam(cuda(q), tk, tv, n, cap, U, K, cuda(anc), nk, nv)
    check(f"attend_beam self n={n} U={U} K={K} H={H}", got, G._softmax_attend(q, kg, vg, np.float64), G._softmax_attend(q, kg, vg, np.float32))
    for t, ref, sentinel in ((tk, k, 1e30), (tv, v, -1e30)):
        c = t.cpu().numpy()
        assert np.array_equal(c[:, n - 1], ref[:, n - 1]) and np.array_equal(c[:, : n - 1], ref[:, : n - 1]) and (c[:, n:] == sentinel).all()
    same = _attend_beam(cuda(q), cuda(kd), cuda(vd), n, cap, U, K, cuda(ident), nk, nv)
    plain = _attend(cuda(q), cuda(kd), cuda(vd), n, cap, nk, nv)
    assert np.array_equal(same, plain), f"identity ancestry differs from the plain kernel by {np.abs(same - plain).max():.3e}"


# ---------------------------------------------------------------------------------------------------- the step tail on scripted logits
class _State:
    """The caller-held state of dex_whisper_beam_pick: U utterances of K beams, as ``new_state`` starts them."""

    def __init__(self, U, K, ld_seq, ld_anc):
        from dex_tts_amd._lib import DexWhisperBeamState
        R_ = U * K
        i32 = dict(dtype=torch.int32, device="cuda")
        self.U, self.K = U, K
        self.run = cuda(np.tile(np.array([0.0] + [-1e9] * (K - 1)), U))
        self.pool_score = torch.full((R_,), float("-inf"), dtype=torch.float64, device="cuda")
        self.seq = [torch.full((R_, ld_seq), -5, **i32) for _ in range(2)]
        self.anc = [cuda(np.tile((np.arange(R_) % K)[:, None], (1, ld_anc)).astype(np.int32)) for _ in range(2)]
        self.pool_ids, self.pool_len = torch.full((R_, ld_seq), -5, **i32), torch.zeros(R_, **i32)
        self.pool_order, self.pool_n = cuda((np.arange(R_) % K).astype(np.int32)), torch.zeros(U, **i32)
        self.done, self.count, self.tok, self.par = torch.zeros(U, **i32), torch.zeros(1, **i32), torch.full((R_,), -1, **i32), torch.full((R_,), -1, **i32)
        self.c = DexWhisperBeamState(run_score=self.run.data_ptr(), pool_score=self.pool_score.data_ptr(), pool_ids=self.pool_ids.data_ptr(),
                                     pool_len=self.pool_len.data_ptr(), pool_order=self.pool_order.data_ptr(), pool_n=self.pool_n.data_ptr(),
                                     done=self.done.data_ptr(), count=self.count.data_ptr(), ld_seq=ld_seq, ld_anc=ld_anc)
        self.parity = 0

    def step(self, logits, mask, eos, i, pos, last, lp):
        U, K, V = self.U, self.K, logits.shape[-1]
        a, b = self.parity, self.parity ^ 1
        self.c.seq_in, self.c.seq_out, self.c.anc_in, self.c.anc_out = (self.seq[a].data_ptr(), self.seq[b].data_ptr(), self.anc[a].data_ptr(),
                                                                       self.anc[b].data_ptr())
        lg = cuda(logits.reshape(U * K, V).astype(np.float32))
        scratch = torch.empty(_lib().dex_whisper_beam_pick_scratch_bytes(U, K, V), dtype=torch.uint8, device="cuda")
        rc = _lib().dex_whisper_beam_pick(lg.data_ptr(), U, K, V, cuda(mask).data_ptr(), eos, i, pos, int(last), lp, C.byref(self.c),
                                          self.tok.data_ptr(), self.par.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream())
        assert rc == 0
        self.parity = b
        host = lambda t, *shape: t.cpu().numpy().reshape(*shape)
        order = host(self.pool_order, U, K)
        return dict(tokens=host(self.tok, U, K), parents=host(self.par, U, K), run=host(self.run, U, K), seq=host(self.seq[b], U, K, -1),
                    anc=host(self.anc[b], U, K, -1), done=host(self.done, U), count=int(self.count.item()), pool_n=host(self.pool_n, U),
                    pool_ids=np.take_along_axis(host(self.pool_ids, U, K, -1), order[:, :, None], 1),
                    pool_len=np.take_along_axis(host(self.pool_len, U, K), order, 1), pool_score=np.take_along_axis(host(self.pool_score, U, K), order, 1))


def _row(V, highs):
    x = (-8.0 - np.arange(V) * 1e-4).astype(np.float32)                   # a background that decreases with the id: no two values equal
    for t, val in highs.items():
        x[t] = val
    return x


def _script(V, K, eos, kind, scale):
    """The logits [steps, K, V] of one utterance.  Steps 0 - 2 are shared: (0) beams 1 .. K - 1 hold a huge logit that must not count
    (step 0 is beam 0's alone), beam 0's largest logit is in ``begin_suppress`` and 2K ids tie exactly behind it; (1) all rows are
    equal, and so are the running scores: ids 20 (now allowed) and 21 tie within a row and across the beams, the lowest flat
    indices win and beams share a parent; (2) equal rows again with the eos second: the K eos candidates have ranks K .. 2K - 1 and
    are dropped.  ``stop``: step 3 has the eos first in equal rows - all top K candidates are eos, the pool fills and the stop fires;
    what follows must not change the state.  ``long``: (3) and (4) rows that differ by beam, (5) the eos first in beam 0's row only,
    (6) the last step, which pools the top K whatever they are."""
    s = np.float32(scale)
    steps = [np.stack([_row(V, {20: 9 * s, **{40 + j: 5 * s for j in range(2 * K)}})] + [_row(V, {30: 50.0})] * (K - 1)),
             np.stack([_row(V, {20: 6 * s, 21: 6 * s})] * K),
             np.stack([_row(V, {50: 7 * s, eos: 6.5 * s})] * K)]
    if kind == "stop":
        steps += [np.stack([_row(V, {eos: 8 * s, 60: 5 * s, 61: 4 * s})] * K)]
        steps += [np.stack([_row(V, {70 + r: 9.0 - r}) for r in range(K)])] * 3
    else:
        steps += [np.stack([_row(V, {60 + r: (7 - 0.3 * r) * s, eos: (6.0 - r) * s}) for r in range(K)]),
                  np.stack([_row(V, {70 + r: (8 - 0.5 * r) * s, 80 + r: 5 * s}) for r in range(K)]),
                  np.stack([_row(V, {eos: 9 * s, 85: 6 * s})] + [_row(V, {85 + r: (6 - 0.2 * r) * s}) for r in range(1, K)]),
                  np.stack([_row(V, {22 + r: (7 - 0.4 * r) * s, eos: (6.9 - 1.1 * r) * s}) for r in range(K)])]
    return np.stack(steps)


@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("K,lp", [(2, 1.0), (5, 0.6)])
@pytest.mark.parametrize("V", [96, 51866])
def test_beam_pick_scripted(V, K, lp, U):
    """Seven steps of the tail alone on scripted logits, compared after every step with ``select`` on the same fp32 logits: tokens, parents,
    sequences, ancestry, pool ids and lengths, done flags and the done count are equal, running and pool scores agree within 1e-12
    relative.  Every distance a decision of the script compares is exactly 0 (a tie, decided by the index) or above 1e-6."""
    eos, P, n = V - 2, 3, 7
    kinds = ["long", "stop", "long"][:U]
    logits = np.stack([_script(V, K, eos, kind, 1.0 - 0.1 * u) for u, kind in enumerate(kinds)], axis=1)          # [steps, U, K, V]
    sp = R.spec((1, 5, 7), (0, 3), (20,), eos)
    sup = np.zeros(V, np.uint8); sup[[0, 3]] = 1
    beg = sup.copy(); beg[20] = 1
    dev = _State(U, K, n + 1, P + n + 1)
    ref = [BR.new_state(K, P + n + 1) for _ in range(U)]
    seen = dict(tie_across=False, all_eos=False, eos_dropped=False, frozen=False, last_pool=False)
    for i in range(n):
        last = i == n - 1
        got = dev.step(logits[i], beg if i == 0 else sup, eos, i, P - 1 + i, last, lp)
        for u in range(U):
            was_done, before = ref[u].done, ref[u]
            ref[u], info = BR.select(logits[i, u], ref[u], sp, i, last, lp, P - 1 + i)
            assert all(g == 0.0 or g > 1e-6 for g in info.gaps), (i, u, info.gaps)
            if was_done:
                seen["frozen"] = True
            elif not last:
                assert got["tokens"][u].tolist() == info.tokens and got["parents"][u].tolist() == info.parents, (i, u)
                cand = [(int(f) // V, int(f) % V) for f in info.candidates]
                if i == 0:
                    assert info.parents == [0] * K and 20 not in info.tokens and info.tokens == list(range(40, 40 + K))
                if i == 1:
                    assert 20 in info.tokens and cand[:4] == [(0, 20), (0, 21), (1, 20), (1, 21)]
                    seen["tie_across"] = True
                if [t for _, t in cand[K:]] == [eos] * K and len(ref[u].pool) == len(before.pool):
                    seen["eos_dropped"] = True
                if [t for _, t in cand[:K]] == [eos] * K:
                    assert ref[u].done and len(ref[u].pool) == K
                    seen["all_eos"] = True
            else:
                assert len(ref[u].pool) == K and ref[u].done
                seen["last_pool"] = True
            st = ref[u]
            assert np.allclose(got["run"][u], st.run, rtol=1e-12, atol=0), (i, u, got["run"][u], st.run)
            m = len(st.seqs[0])
            assert got["seq"][u][:, :m].tolist() == st.seqs and got["anc"][u].tolist() == st.anc.tolist(), (i, u)
            assert int(got["pool_n"][u]) == len(st.pool) and int(got["done"][u]) == int(st.done)
            for j, e in enumerate(st.pool):
                assert got["pool_ids"][u, j, : len(e["ids"])].tolist() == e["ids"] and int(got["pool_len"][u, j]) == e["length"]
                assert (got["pool_ids"][u, j, len(e["ids"]):] == eos).all()
                assert np.isclose(got["pool_score"][u, j], e["score"], rtol=1e-12, atol=0)
        assert got["count"] == sum(int(s.done) for s in ref)
    assert seen["tie_across"] and seen["eos_dropped"] and seen["last_pool"] and (U == 1 or (seen["all_eos"] and seen["frozen"])), seen


# ---------------------------------------------------------------------------------------------------- the whole search
# Utterance seeds and the eos of a run, picked on the CPU: the float64 restatement's smallest decision gap is 6.3e-3 / 7.8e-3 / 3.7e-3
# (TINY, K = 3) and 1.3e-3 / 1.5e-3 (WIDE, K = 5); TINY's utterances stop early after 7 and 10 steps and run to the cap of 12,
# WIDE's after 4 steps and at the cap with hypotheses of 7 and 12 tokens in its pool.
RUN = {"TINY": dict(K=3, seeds=(20, 27, 23), eos=94, begin=(55, 69)), "WIDE": dict(K=5, seeds=(31, 25), eos=978, begin=(253, 351, 982))}
MAX_NEW = 12
_RUN = {}


def _specs(name):
    from dex_tts_amd.whisper import GenerationSpec
    r = RUN[name]
    return GenerationSpec(G.PROMPT, (0, 3), r["begin"], r["eos"]), R.spec(G.PROMPT, (0, 3), r["begin"], r["eos"])


def run_case(name):
    """One traced device run per config, shared and never changed."""
    if name not in _RUN:
        r, cfg = RUN[name], G.CFG[name]
        feats = np.stack([R.make_features(cfg, s) for s in r["seeds"]])
        ids, lens, scores, tr = G.model(name).generate_beam(cuda(feats), _specs(name)[0], r["K"], max_new_tokens=MAX_NEW, trace=True)
        _RUN[name] = (feats, ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy(), {k: v.cpu().numpy() for k, v in tr.items()})
    return _RUN[name]


def _replay(name, u):
    _, _, _, _, tr = run_case(name)
    cfg, sp = G.CFG[name], _specs(name)[1]
    return BR.beam_search(cfg, None, None, sp, RUN[name]["K"], MAX_NEW, 1.0, step_fn=lambda i, tokens, parents: tr["logits"][i, u])


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_generate_beam_is_the_restatement_on_its_own_logits(name):
    """``beam_search`` replayed on the traced device logits reproduces the device's tokens, parents, running scores, pool, ids,
    lengths and scores; the replay's smallest decision gap is above 1e-9, so nothing here is a coincidence of rounding."""
    feats, ids, lens, scores, tr = run_case(name)
    K, eos = RUN[name]["K"], RUN[name]["eos"]
    assert ids.dtype == np.int32 and ids.shape[0] == len(feats) and scores.dtype == np.float64
    ended = []
    for u in range(len(feats)):
        hyp, pool, trace, gap = _replay(name, u)
        print(f"{name} utterance {u}: {len(trace)} steps, gap {gap:.3e}, pool lengths {[e['length'] for e in pool]}, score {hyp['score']:.6f}")
        assert gap > 1e-9
        ended.append(len(trace))
        for i, t in enumerate(trace):
            if t["tokens"] is None:
                assert (tr["tokens"][i, u] == -1).all() and (tr["parents"][i, u] == -1).all()
                continue
            assert tr["tokens"][i, u].tolist() == t["tokens"] and tr["parents"][i, u].tolist() == t["parents"], (u, i)
            assert np.allclose(tr["scores"][i, u], t["run"], rtol=1e-12, atol=0)
        assert (tr["tokens"][len(trace):, u] == -1).all()                                   # done is sticky
        assert int(tr["pool_n"][u]) == len(pool) == K
        for j, e in enumerate(pool):
            assert tr["pool_ids"][u, j, : len(e["ids"])].tolist() == e["ids"] and (tr["pool_ids"][u, j, len(e["ids"]):] == eos).all()
            assert int(tr["pool_lengths"][u, j]) == e["length"] and np.isclose(tr["pool_scores"][u, j], e["score"], rtol=1e-12, atol=0)
        assert ids[u, : len(hyp["ids"])].tolist() == hyp["ids"] and (ids[u, len(hyp["ids"]):] == eos).all()
        assert int(lens[u]) == hyp["length"] and np.isclose(scores[u], hyp["score"], rtol=1e-12, atol=0) and scores[u] == tr["pool_scores"][u, 0]
    assert min(ended) < MAX_NEW == max(ended) == ids.shape[1], ended                         # one stops early while another goes on


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_generate_beam_logits_follow_each_beams_own_prefix(name):
    """EVERY traced logits row lies within ``whisper_ref.tolerance`` of the teacher-forced float64 logits of that beam's own prefix
    (the prompt and its tokens from the trace): a cache that followed the wrong parent fails by orders of magnitude.  The bound of
    an utterance is the rule's over all of its traced rows: 8 x the largest distance of the fp32 CPU evaluation of those same rows
    from float64."""
    feats, _, _, _, tr = run_case(name)
    cfg, sd, K = G.CFG[name], G.weights(name), RUN[name]["K"]
    for u in range(len(feats)):
        n = len(_replay(name, u)[2])
        prefixes, seqs = [], [[] for _ in range(K)]
        for i in range(n):
            prefixes.append([tuple(s) for s in seqs])
            if i + 1 < n:
                seqs = [seqs[p] + [int(t)] for p, t in zip(tr["parents"][i, u], tr["tokens"][i, u])]
        known = {}                                                                           # prefix -> (float64 logits, the yardstick's)
        for i in reversed(range(n)):                                                         # the longest prefixes first: they hold the others
            for r in range(K):
                if prefixes[i][r] not in known:
                    seq = list(G.PROMPT) + list(prefixes[i][r])
                    _, ref = R.forward(cfg, sd, feats[u], seq)
                    _, yard = R.torch_forward_fp32(cfg, sd, feats[u], seq)
                    for m in range(len(prefixes[i][r]) + 1):
                        known.setdefault(prefixes[i][r][:m], (ref[len(G.PROMPT) - 1 + m], yard[len(G.PROMPT) - 1 + m]))
        rows = [known[prefixes[i][r]] for i in range(n) for r in range(K)]
        got = tr["logits"][:n, u].reshape(n * K, -1)
        tol = check(f"beam logits {name} utterance {u}: {n} steps x {K} beams", got, np.stack([a for a, _ in rows]), np.stack([b for _, b in rows]))
        err = np.abs(got.astype(np.float64) - np.stack([a for a, _ in rows])).max(axis=1)
        assert (err <= tol).all()


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_generate_beam_rows_are_the_utterance_alone(name):
    feats, ids, lens, scores, _ = run_case(name)
    m, sp, K = G.model(name), _specs(name)[0], RUN[name]["K"]
    for u in range(len(feats)):
        a_ids, a_lens, a_scores = m.generate_beam(cuda(feats[u:u + 1]), sp, K, max_new_tokens=MAX_NEW)
        a_ids = a_ids.cpu().numpy()[0]
        assert np.array_equal(a_ids, ids[u, : len(a_ids)]) and (ids[u, len(a_ids):] == RUN[name]["eos"]).all()
        assert int(a_lens[0]) == lens[u] and float(a_scores[0]) == scores[u]
    g_ids, g_lens = m.generate(cuda(feats), sp, MAX_NEW, num_beams=K)
    assert np.array_equal(g_ids.cpu().numpy(), ids) and np.array_equal(g_lens.cpu().numpy(), lens)


def test_groups_of_utterances_and_one_beam():
    """K = 8 takes 32 // 8 = 4 utterances per network call: five utterances run as 4 + 1 and each is the utterance alone.
    ``num_beams=1`` is greedy decoding, bitwise."""
    m, sp = G.model("TINY"), _specs("TINY")[0]
    feats = cuda(np.stack([R.make_features(R.TINY, s) for s in (20, 27, 23, 21, 24)]))
    ids, lens, scores = m.generate_beam(feats, sp, 8, 0.6, max_new_tokens=6)
    for u in (0, 3, 4):
        a = m.generate_beam(feats[u:u + 1], sp, 8, 0.6, max_new_tokens=6)
        assert np.array_equal(a[0].cpu().numpy()[0], ids[u].cpu().numpy()) and int(a[1][0]) == int(lens[u]) and float(a[2][0]) == float(scores[u])
    want, got = m.generate(feats, sp), m.generate(feats, sp, num_beams=1, length_penalty=0.6)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])


def test_transcribe_and_score_with_beams():
    from dex_tts_amd import synthesize, whisper
    from dex_tts_amd.asr import score_transcripts
    m, sp = G.model("TINY"), _specs("TINY")[0]
    vocab = [f"Ġw{i}" for i in range(R.TINY.vocab_size)]
    audio = [(R.synth_wav(n, 70 + i) * 32767.0).astype(np.int16) for i, n in enumerate((9000, 12001))]
    texts = ["w1 w2 w3", "w4, w5!"]
    ids, lens, _ = m.generate_beam(m.log_mel(audio, sr=22050), sp, 3)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    want = [whisper.decode(ids[b, : lens[b]], vocab, sp.eos_token_id) for b in range(2)]
    preds, *score = synthesize.whisper_scores(m, sp, vocab, audio, texts, sr=22050, num_beams=3)
    assert preds == want and any(preds) and tuple(score) == score_transcripts(texts, preds)
    assert m.transcribe(audio, sp, vocab, sr=22050, num_beams=3) == want
    assert whisper.whisper_score(audio, texts, model=m, spec=sp, vocab=vocab, sr=22050, num_beams=3)[0] == want


# ---------------------------------------------------------------------------------------------------- errors
def test_beam_errors():
    from dex_tts_amd import whisper
    m, sp = G.model("TINY"), _specs("TINY")[0]
    feat = cuda(R.make_features(R.TINY, 20)[None])
    for bad in (1, 9, 0):
        with pytest.raises(ValueError, match="num_beams"):
            m.generate_beam(feat, sp, bad)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(feat, sp, num_beams=9)
    with pytest.raises(ValueError, match="timestamps"):
        m.generate(feat, sp, timestamps=True, num_beams=3)
    with pytest.raises(ValueError, match="early_stopping"):
        m.generate(feat, sp, num_beams=3, early_stopping=True)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(feat, sp, num_beams=3, num_return_sequences=3)
    with pytest.raises(ValueError, match="long_form"):
        whisper.whisper_score([np.zeros(1000, np.float32)], ["a"], model=m, spec=sp, vocab=["a"] * 96, long_form=True, num_beams=3)
    with pytest.raises(ValueError, match="leave 5 ids"):
        m.generate_beam(feat, whisper.GenerationSpec(G.PROMPT, tuple(range(0, 80)), tuple(range(80, 91)), 91), 3)
    with pytest.raises(ValueError, match="max_new_tokens"):
        m.generate_beam(feat, sp, 3, max_new_tokens=0)
    with pytest.raises(ValueError, match="CUDA"):
        m.generate_beam(torch.zeros(1, R.TINY.num_mel_bins, 2 * R.TINY.max_source_positions), sp, 3)
    with pytest.raises(ValueError, match="not loaded"):
        whisper.Whisper(R.library_config(R.TINY), "cuda").generate_beam(feat, sp, 3)
    lib, h = _lib(), m._ctx.h
    assert lib.dex_whisper_beam_workspace_bytes(h, 4, 8) > lib.dex_whisper_workspace_bytes(h, 4) and lib.dex_whisper_beam_workspace_bytes(h, 5, 8) == 0
    assert lib.dex_whisper_beam_workspace_bytes(h, 1, 1) == 0 and lib.dex_whisper_beam_workspace_bytes(h, 1, 9) == 0
