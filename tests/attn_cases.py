"""The launches tests/test_gpu_attn_kernels.py runs one at a time, and their operands (shared with tests/test_attn_reference_cpu.py).

OPERANDS (make_operands): seeded, and exactly representable in bf16 AND fp16, so one set of values and one fp64 reference serve
the three modes.  Magnitudes as in tools/attnq64.hip: q ~ +-0.35 on the 2^-6 grid, k ~ +-0.9 on the 2^-5 grid (tests/attn_reference.py
needs the grids: fp32 scores are exact), v ~ +-1 on the 2^-8 grid.  Two groups of 8 features are reserved:

    d 112..119  SPIKES.  q is 0.25 there for the query rows r % 4 == 1 and 0 for the others; k is 0 except at the spike keys, whose
                value a adds 2 a to the score of every spiked row: +18, +37 and +56 at keys N // 3, N // 2 + 5 and N - 2 (those that
                exist), each more than the lag above everything before it, so the reference maximum of every 32-query block MOVES
                at those late tiles - with lanes that exceed it and lanes that do not - and the last spike sits in the last tile of
                the last split of every plan.  Spiked rows also put most P below 2^-14 (fp16 subnormals).  spikes=False: none.
    d 120..127  EDGE SENTINEL.  q is 0.25 for every row, k is 0 except at the last live key N - 1, where 1.25 adds 2.5: its score is
                near the maximum of every unspiked row (p ~ 0.3 - 1), and its V row is +-4 alternating.  Dropping it, or admitting
                the first pad key, moves O far outside the bound in every mode.

PAD ROWS N..Npad-1 are the producer's "finite duplicates": K pad rows copy row N - 1 (an admitted pad key scores like the sentinel),
V^T pad rows are 100, Q pad rows copy live rows."""
import torch

from tests import attn_reference as R

PRECS = ("bf16", "fp16", "fp16x2")
KNOBS = ("DEX_XCD_MAP", "DEX_ATTN_Q64_HALF")
SPIKE_ADD = (9.0, 18.5, 28.0)                   # k values of the spike keys: + 2 a per spiked row


def spike_keys(N):
    cand = [N // 3, N // 2 + 5, N - 2]
    out = []
    for j in cand:
        if 1 <= j < N - 1 and j not in out:
            out.append(j)
    return out


_OPS = {}


def make_operands(B, N, spikes=True):
    """fp64 q, k, v [2 B, Npad, 128] (pad rows included), cached."""
    key = (B, N, spikes)
    if key in _OPS:
        return _OPS[key]
    _OPS.clear()                                # (one case's operands at a time: the large ones are 10s of MB)
    G, npad = 2 * B, (N + 31) // 32 * 32
    g = torch.Generator().manual_seed(1000003 * B + 31 * N + int(spikes))
    u = lambda: torch.rand(G, npad, R.HD, generator=g, dtype=torch.float64) * 2 - 1
    q = torch.round(u() * 0.35 / R.Q_GRID) * R.Q_GRID
    k = torch.round(u() * 0.9 / R.K_GRID) * R.K_GRID
    v = torch.round(u() * 256) / 256
    rows = torch.arange(npad)
    q[:, :, 112:120] = 0.0
    k[:, :, 112:128] = 0.0
    q[:, :, 120:128] = 0.25
    if spikes:
        q[:, rows % 4 == 1, 112:120] = 0.25
        for a, j in zip(SPIKE_ADD, spike_keys(N)):
            k[:, j, 112:120] = a
    k[:, N - 1, 120:128] = 1.25
    v[:, N - 1, :] = torch.where(torch.arange(R.HD) % 2 == 0, 4.0, -4.0)
    if npad > N:
        k[:, N:] = k[:, N - 1:N]
        v[:, N:] = 100.0
        q[:, N:] = q[:, :npad - N]
    _OPS[key] = (q, k, v)
    return _OPS[key]


def grids_ok(q, k):
    """The property the bound's exact-score argument needs (tests/attn_reference.py)."""
    on = lambda x, s: bool((torch.round(x / s) * s == x).all())
    bound = float(q.abs().max() * k.abs().max()) * R.HD          # every partial sum of a score stays below it
    return on(q, R.Q_GRID) and on(k, R.K_GRID) and bound < 2.0 ** 13


def representable(x):
    return bool((x.to(torch.bfloat16).to(torch.float64) == x).all() and (x.to(torch.float16).to(torch.float64) == x).all())


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def nt32(N):
    return (N + 31) // 32


def direct(B, N, ksplit=1, o_lp=False, env=None, xcd_map=None, spikes=True):
    ring = nt32(N) * 2 * B >= 1024
    form = f"attn_direct_ring_kernel xcd_map={xcd_map}" if ring else "attn_direct_kernel"
    assert ring == (xcd_map is not None)
    name = f"{'ring' if ring else 'waves'}_B{B}_N{N}_ks{ksplit}" + ("_olp" if o_lp else "") + ("_nospike" if not spikes else "")
    for kk, vv in (env or {}).items():
        name += f"_{kk[4:].lower()}{vv}"
    return dict(kind="direct", name=name, B=B, N=N, ksplit=ksplit, o_lp=o_lp, env=env or {}, form=form, spikes=spikes,
                tail_g=0, tail_ks=0, half_g=0, half_n=0, key_tile=32)


def q64(B, N, ks=1, o_lp=False, tail=None, half=None, auto_half=False, env=None, spikes=True, expect_half=None):
    """half: forced half_g (half_n follows); auto_half: leave the plan to the launcher (expect_half = the (half_g, half_n) the cost
    model must pick, asserted through the form string); default: whole units only."""
    t32 = nt32(N)
    ng = (t32 + 7) // 8
    tg, tk = tail or (0, 0)
    hg, hn = (half, (t32 - 8 * half + 3) // 4) if half is not None else (0, 0 if auto_half else -1)
    ehg, ehn = (hg, hn) if half is not None else (expect_half or (0, 0))
    nunits = 2 * B * (ehg + ehn) if ehn > 0 else 2 * B * (tg + (ng - tg) * tk) if tk > 1 else 2 * B * ng * ks
    form = (f"attn_q64_kernel nunits={nunits} grid={min(nunits, 256)} ks={ks} tail_g={tg if tk > 1 else ng} tail_ks={max(tk, 1)} "
            f"half_g={ehg} half_n={ehn} xcd_mode={int(2 * B % 8 == 0)}")
    name = f"q64_B{B}_N{N}_ks{ks}" + ("_olp" if o_lp else "") + (f"_tail{tg}x{tk}" if tk > 1 else "")
    name += (f"_half{half}" if half is not None else "_autohalf" if auto_half else "") + ("_nospike" if not spikes else "")
    for kk, vv in (env or {}).items():
        name += f"_{kk[4:].lower()}{vv}"
    return dict(kind="q64", name=name, B=B, N=N, ksplit=ks, o_lp=o_lp, env=env or {}, form=form, spikes=spikes,
                tail_g=tg, tail_ks=tk, half_g=hg, half_n=hn, key_tile=64)


# key-splitting waves: ceil(N / 32) * 2 * B < 1024
WAVES = [direct(2, 1), direct(3, 33), direct(3, 33, 2), direct(1, 64), direct(1, 64, spikes=False), direct(5, 129), direct(5, 129, 3),
         direct(2, 257), direct(2, 257, 2), direct(2, 257, 4), direct(1, 520, 4)]

# shared ring: ceil(N / 32) * 2 * B >= 1024
RING_KS_B16_N1025 = 2                           # attention_direct_ksplit(1025, 16): 9 query groups x 32 = 288 workgroups < 384, 33 tiles / 2 >= 8
RING = [direct(256, 33, xcd_map=1), direct(32, 520, xcd_map=1), direct(32, 520, o_lp=True, xcd_map=1), direct(31, 520, xcd_map=0),
        direct(32, 520, env={"DEX_XCD_MAP": 0}, xcd_map=0), direct(16, 1025, RING_KS_B16_N1025, xcd_map=1)]

# 64-query form
Q64_AUTO_KS_B1_N520 = 3                         # attention_q64_ksplit(520, 1, 8), asserted by the test through the shim
Q64_AUTO_HALF_B1_N520 = (0, 5)                  # attention_q64_half_plan(520, 1): ten half units beat six whole ones
Q64 = ([q64(2, 1), q64(3, 33), q64(4, 70), q64(4, 70, o_lp=True), q64(4, 70, spikes=False), q64(5, 129)]
       + [q64(2, 257, ks) for ks in (1, 2, 3)] + [q64(2, 257, half=h) for h in (0, 1)] + [q64(2, 257, o_lp=True)]
       + [q64(1, 520, ks) for ks in (1, 2, 3)] + [q64(1, 520, half=h) for h in (0, 1, 2)] + [q64(1, 520, auto_half=True, expect_half=Q64_AUTO_HALF_B1_N520)]
       + [q64(1, 520, tail=t, o_lp=o) for t in ((1, 2), (2, 2), (2, 3)) for o in (False, True)] + [q64(1, 520, o_lp=True)]
       + [q64(132, 70), q64(131, 70), q64(68, 300, half=1)]
       + [q64(1, 520, auto_half=True, env={"DEX_ATTN_Q64_HALF": 0})])
ALL = WAVES + RING + Q64


def parts_of(case):
    """What a launch writes: [dict(rows=(r0, r1), slot, keys=(lo, hi), ml=index or None, lp)] - the partials of every row range."""
    N, kt = case["N"], case["key_tile"]
    ntile = (nt32(N) + (kt // 32) - 1) // (kt // 32)
    rng = lambda sp, ks: (min(N, ntile * sp // ks * kt), min(N, ntile * (sp + 1) // ks * kt))
    ks, tg, tk = case["ksplit"], case["tail_g"], case["tail_ks"]
    if tk > 1:
        r0 = min(N, tg * 256)
        out = [dict(rows=(0, r0), slot=0, keys=(0, N), ml=None, lp=case["o_lp"])]
        return out + [dict(rows=(r0, N), slot=1 + sp, keys=rng(sp, tk), ml=sp, lp=False) for sp in range(tk)]
    always_ml = case["kind"] == "direct"        # (the 64-query form writes (m, l) for key splits only)
    return [dict(rows=(0, N), slot=sp, keys=rng(sp, ks), ml=sp if (ks > 1 or always_ml) else None, lp=case["o_lp"]) for sp in range(ks)]


def n_slots(case):
    return 1 + case["tail_ks"] if case["tail_ks"] > 1 else case["ksplit"]


def n_ml(case):
    return max(case["tail_ks"], case["ksplit"], 1)
