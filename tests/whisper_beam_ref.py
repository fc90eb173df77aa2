"""Restatement of the beam search of dex_tts_amd/whisper.py (the definition in its docstring) in float64 numpy, on top of
``whisper_ref.Decoder``.  tests/test_whisper_beam_cpu.py holds it to ``transformers``' own beam search in double precision.

``select`` is one step of pure selection logic on given fp32 logits and state; ``beam_search`` loops it over a decoder (the float64
restatement, or recorded logits through ``step_fn``).  Both report the smallest *decision gap* they met: the distance between
consecutive candidates among the top 2K + 1 accumulated scores, between a pooled score and every pool entry it is merged against, and
of the stop comparison.  A caller that compares against another precision asserts on it, so a coincidence cannot pass silently."""
import copy
import types

import numpy as np

from tests import whisper_ref as R


def log_softmax(row):
    """fp64 log-softmax of the whole row of logits (fp32 from the device, exact in fp64): x - (max + log sum exp(x - max))."""
    x = np.asarray(row).astype(np.float64)
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum()))


def new_state(K, n_positions=0):
    """Before the first step: scores [0, -1e9, ...], empty sequences, identity ancestry, an empty pool."""
    return types.SimpleNamespace(run=np.array([0.0] + [-1e9] * (K - 1)), seqs=[[] for _ in range(K)],
                                 anc=np.tile(np.arange(K)[:, None], (1, n_positions)), pool=[], done=False)


def select(logits, state, sp, i, last, length_penalty=1.0, pos=None):
    """One step of an utterance: ``logits`` [K, V] fp32 of the K running beams at new-token step ``i`` (``last``: the last step),
    ``state`` from ``new_state`` / an earlier call (not modified) -> (the next state, info) with info.tokens / parents (the new
    running set; None on the last step), info.candidates (flat indices of the 2K best), info.gaps (every distance a decision
    compared) and info.gap, their minimum.  A done state comes back as it is.  ``pos``: the cache position of the step, for the ancestry table (left alone when None)."""
    if state.done:
        return state, types.SimpleNamespace(tokens=None, parents=None, candidates=None, gaps=[], gap=np.inf)
    K, V = np.shape(logits)
    acc = np.stack([log_softmax(row) for row in logits])
    acc[:, list(sp.suppress_tokens)] = -np.inf
    if i == 0:
        acc[:, list(sp.begin_suppress_tokens)] = -np.inf
    if int(np.isfinite(acc[0]).sum()) < 2 * K:
        raise ValueError(f"{int(np.isfinite(acc[0]).sum())} unmasked ids, num_beams = {K} needs {2 * K}")
    flat = (acc + state.run[:, None]).ravel()
    order = np.lexsort((np.arange(flat.size), -flat))[: 2 * K + 1]           # descending, ties to the lowest flat index
    top = flat[order]
    gaps = [float(g) for g in top[:-1] - top[1:]]
    div = float(i + 1) ** length_penalty
    st = types.SimpleNamespace(run=state.run.copy(), seqs=[list(s) for s in state.seqs], anc=state.anc.copy(),
                               pool=[dict(e) for e in state.pool], done=False)
    run, tokens, parents = [], [], []
    for rank, f in enumerate(order[: 2 * K]):
        r, tok = int(f) // V, int(f) % V
        if not last and tok != sp.eos_token_id:
            if len(run) < K:
                run.append(float(flat[f])); tokens.append(tok); parents.append(r)
            continue
        if rank >= K:
            continue
        score = float(flat[f]) / div
        gaps += [abs(e["score"] - score) for e in st.pool]
        t = 0
        while t < len(st.pool) and not st.pool[t]["score"] < score:          # behind every entry that is at least as good
            t += 1
        st.pool.insert(t, dict(score=score, ids=state.seqs[r] + [tok], length=i if tok == sp.eos_token_id else i + 1))
        del st.pool[K:]
    if last:
        st.done = True
        return st, types.SimpleNamespace(tokens=None, parents=None, candidates=order[: 2 * K], gaps=gaps, gap=min(gaps))
    st.run = np.array(run)
    st.seqs = [state.seqs[r] + [tok] for r, tok in zip(parents, tokens)]
    if pos is not None:
        st.anc = state.anc[parents].copy()
        st.anc[:, pos + 1:] = np.arange(K)[:, None]
    if len(st.pool) == K:
        gaps.append(abs(run[0] / div - st.pool[-1]["score"]))
        st.done = run[0] / div <= st.pool[-1]["score"]
    return st, types.SimpleNamespace(tokens=tokens, parents=parents, candidates=order[: 2 * K], gaps=gaps, gap=min(gaps))


def beam_search(cfg, sd, feat, sp, K, max_new=None, length_penalty=1.0, step_fn=None):
    """Beam search of one utterance -> (hypothesis, pool, trace, gap): the pool's best entry {"ids" (its eos included), "length",
    "score"}, the pool best first, per step {"tokens", "parents", "run", "logits"} and the smallest decision gap.
    ``step_fn(i, tokens, parents) -> logits [K, V]`` replaces the float64 decoder: ``tokens`` are the K ids fed at new-token step i
    (the prompt's last at i = 0) and ``parents`` the beams whose caches they continue (None at i = 0)."""
    P = len(sp.prompt_ids)
    room = cfg.max_target_positions - P
    n_new = room if max_new is None else min(max_new, room)
    if step_fn is None:
        w = R._f64(sd)
        first = R.Decoder(cfg, sd, R.encode(cfg, sd, feat, w), w)
        for p, t in enumerate(sp.prompt_ids[:-1]):
            first.step_logits(int(t), p)
        decs = [first] + [copy.copy(first) for _ in range(K - 1)]

        def step_fn(i, tokens, parents):
            nonlocal decs
            if parents is not None:
                forks = []
                for r in parents:
                    d = copy.copy(decs[r])
                    d.k, d.v = list(decs[r].k), list(decs[r].v)              # step_logits rebinds the arrays, it never writes into them
                    forks.append(d)
                decs = forks
            else:
                for d in decs:
                    d.k, d.v = list(first.k), list(first.v)
            return np.stack([d.step_logits(int(t), P - 1 + i) for d, t in zip(decs, tokens)])

    state, trace, gap = new_state(K, cfg.max_target_positions), [], np.inf
    tokens, parents = [int(sp.prompt_ids[-1])] * K, None
    for i in range(n_new):
        logits = np.asarray(step_fn(i, tokens, parents))
        state, info = select(logits, state, sp, i, i == n_new - 1, length_penalty, P - 1 + i)
        gap = min(gap, info.gap)
        trace.append(dict(tokens=info.tokens, parents=info.parents, run=state.run.copy(), logits=logits))
        if state.done:
            break
        tokens, parents = info.tokens, info.parents
    return state.pool[0], state.pool, trace, gap
