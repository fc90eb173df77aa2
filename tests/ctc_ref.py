"""The float64 restatement of dex_tts_amd/ctc_align.py's contract, in numpy, written from the definitions with the decision order
spelt out.  One utterance at a time: ``x`` [T, V] fp32 logits, ``y`` the target ids (none equal to ``blank``).

    make_case(seed, T, L, V)      the seeded inputs the CPU and the GPU tests share
    lse_frames(x)                 [T] fp64: per frame m + log(sum exp(x - m)), lane-strided partial sums and an xor butterfly
    ctc_nll(x, y, blank=0)        -log p(y | x) by the forward recursion in fp64
    ctc_align(x, y, blank=0)      {"states", "spans", "token_scores", "score", "lse"}: the Viterbi path on the raw logits
    brute_force(x, y, blank=0)    (best score on raw logits, all best paths) by enumerating every valid state sequence

Trellis: states s = 0 .. 2 L, lab(s) = blank for even s and y[(s - 1) / 2] for odd s; into (t, s) from (t - 1, s) "stay", (t - 1, s - 1)
"step" and, for odd s >= 3 with lab(s) != lab(s - 2), (t - 1, s - 2) "skip".  Start: states 0 and 1.
"""
import itertools

import numpy as np

NEG = -np.inf


def make_case(seed, T, L, V):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((T, V)) * 3).astype(np.float32)
    y = g.integers(1, V, L)
    for i in range(1, L):
        if g.random() < 0.3:
            y[i] = y[i - 1]
    return x, y.astype(np.int64)


def repeats(y):
    y = np.asarray(y)
    return int((y[1:] == y[:-1]).sum()) if len(y) > 1 else 0


def labels(y, blank=0):
    y = np.asarray(y, dtype=np.int64)
    S = 2 * len(y) + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    can = np.zeros(S, dtype=bool)
    can[3::2] = lab[3::2] != lab[1:-2:2]
    return lab, can


def lse_frames(x):
    x = np.asarray(x, dtype=np.float32)
    T, V = x.shape
    m = np.fmax.reduce(x, axis=1)                                  # NaN is ignored, as fmaxf does
    mm = np.where(np.isfinite(m), m, np.float32(0)).astype(np.float64)
    p = np.zeros((T, 64))
    with np.errstate(all="ignore"):
        for k in range(0, V, 64):                                   # lane l sums x[l], x[l + 64], ... in that order
            c = x[:, k:k + 64].astype(np.float64)
            p[:, :c.shape[1]] += np.exp(c - mm[:, None])
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            p = p + p[:, lanes ^ o]
        return mm + np.log(p[:, 0])


def _shift(a, n):
    return np.concatenate([np.full(n, NEG), a[:-n]]) if n < len(a) else np.full(len(a), NEG)


def ctc_nll(x, y, blank=0):
    x = np.asarray(x, dtype=np.float32)
    T, L = x.shape[0], len(y)
    S = 2 * L + 1
    lab, can = labels(y, blank)
    lse = lse_frames(x)
    e = x[:, lab].astype(np.float64) - lse[:, None]
    a = np.full(S, NEG)
    a[0] = e[0, 0]
    if S > 1:
        a[1] = e[0, 1]
    with np.errstate(all="ignore"):
        for t in range(1, T):
            stay, step, skip = a, _shift(a, 1), np.where(can, _shift(a, 2), NEG)
            m = stay.copy()
            m = np.where(step > m, step, m)
            m = np.where(skip > m, skip, m)
            r = m + np.log(np.exp(stay - m) + np.exp(step - m) + np.exp(skip - m)) + e[t]
            a = np.where((stay == NEG) & (step == NEG) & (skip == NEG), NEG, r)       # (a NaN term is not -inf: it reaches the result)
        if L == 0:
            return float(-a[0])
        a1, a2 = a[S - 1], a[S - 2]
        m = a1
        if a2 > m:
            m = a2
        if a1 == NEG and a2 == NEG:
            return float(np.inf)
        return float(-(m + np.log(np.exp(a1 - m) + np.exp(a2 - m))))


def ctc_align(x, y, blank=0):
    x = np.asarray(x, dtype=np.float32)
    T, L = x.shape[0], len(y)
    S = 2 * L + 1
    lab, can = labels(y, blank)
    e = x[:, lab].astype(np.float64)                               # the raw logits: the normaliser cannot change a decision
    a = np.full(S, NEG)
    a[0] = e[0, 0]
    if S > 1:
        a[1] = e[0, 1]
    bp = np.zeros((T, S), dtype=np.int64)
    with np.errstate(all="ignore"):
        for t in range(1, T):
            stay, step, skip = a, _shift(a, 1), np.where(can, _shift(a, 2), NEG)
            best, k = stay.copy(), np.zeros(S, dtype=np.int64)    # stay wins ties, then step
            c = step > best
            best, k = np.where(c, step, best), np.where(c, 1, k)
            c = skip > best
            best, k = np.where(c, skip, best), np.where(c, 2, k)
            a = best + e[t]                                         # one fp64 add
            bp[t] = k
        final = S - 1
        if L > 0 and a[S - 2] > a[S - 1]:
            final = S - 2
        lse = lse_frames(x)
        total = 0.0
        for t in range(T):                                          # fp64, in frame order
            total += lse[t]
        score = a[final] - total
    out = {"score": float(score), "lse": lse, "raw_score": float(a[final]), "states": np.full(T, -1, dtype=np.int32),
           "spans": np.full((L, 2), -1, dtype=np.int32), "token_scores": np.full(L, np.nan)}
    if score == NEG or np.isnan(score):
        return out
    s = final
    for t in range(T - 1, -1, -1):
        out["states"][t] = s
        if t > 0:
            s = min(max(s - bp[t, s], 0), S - 1)
    for l in range(L):
        fr = np.nonzero(out["states"] == 2 * l + 1)[0]
        out["spans"][l] = (fr[0], fr[-1] + 1)
        p = 0.0
        for t in fr:
            p += np.exp(np.float64(x[t, y[l]]) - lse[t])
        out["token_scores"][l] = p / float(len(fr))
    return out


def valid_paths(T, y, blank=0):
    """Every state sequence of T frames that starts in state 0 or 1, moves by stay / step / allowed skip and ends in one of the last
    two states."""
    L = len(y)
    S = 2 * L + 1
    _, can = labels(y, blank)
    ends = {S - 1, S - 2} if L > 0 else {0}
    for path in itertools.product(range(S), repeat=T):
        if path[0] > 1 or path[-1] not in ends:
            continue
        ok = True
        for p, q in zip(path[:-1], path[1:]):
            d = q - p
            if not (d == 0 or d == 1 or (d == 2 and can[q])):
                ok = False
                break
        if ok:
            yield path


def path_score(x, y, path, blank=0):
    """The raw-logit score of a state sequence, summed in fp64 in frame order (what the recursion accumulates)."""
    lab, _ = labels(y, blank)
    s = np.float64(x[0, lab[path[0]]])
    for t in range(1, len(path)):
        s = s + np.float64(x[t, lab[path[t]]])
    return float(s)


def brute_force(x, y, blank=0):
    best, arg = NEG, []
    for path in valid_paths(x.shape[0], y, blank):
        v = path_score(x, y, path, blank)
        if v > best:
            best, arg = v, [path]
        elif v == best:
            arg.append(path)
    return best, arg


# (seed, T, L, V): the cases of the CPU and GPU tests
CASES = [(0, 1, 1, 5), (1, 4, 3, 5), (2, 33, 7, 32), (3, 65, 31, 32), (4, 70, 32, 32), (5, 199, 40, 32), (6, 130, 33, 300), (7, 12, 0, 32),
         (8, 300, 120, 32), (9, 2100, 1023, 32), (10, 4096, 512, 32), (11, 40, 20, 3), (12, 600, 255, 32), (13, 600, 256, 32),
         (14, 1100, 511, 32), (15, 1100, 512, 32), (17, 2, 1, 2)]


def tie_cases():
    """(name, x, y) with many exactly equal candidates: all-zero logits and small-integer logits (every sum is exact in fp64, so
    equal path scores are equal bit for bit).  They pin the order stay / step / skip and the final-state rule."""
    out = [("zeros_T4_y1", np.zeros((4, 4), np.float32), np.array([1])),
           ("zeros_T4_y12", np.zeros((4, 4), np.float32), np.array([1, 2])),
           ("zeros_T7_y112", np.zeros((7, 4), np.float32), np.array([1, 1, 2])),
           ("zeros_T40_L12", np.zeros((40, 5), np.float32), np.array([1, 2, 2, 3, 4, 4, 4, 1, 2, 3, 3, 1]))]
    for seed, T, y, V in ((100, 6, [1, 2, 3], 4), (101, 6, [2, 2], 4), (102, 8, [1, 2, 2, 3], 4), (103, 40, [1, 2, 2, 3, 4, 4, 4, 1, 2, 3, 3, 1], 5),
                          (104, 70, list(range(1, 5)) * 8, 5)):
        g = np.random.default_rng(seed)
        out.append((f"ints_{seed}", g.integers(-2, 3, (T, V)).astype(np.float32), np.array(y)))
    return out
