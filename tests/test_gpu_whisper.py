"""GPU: the Whisper path of dex_tts_amd/whisper.py (csrc/whisper.hip) against its float64 restatement (tests/whisper_ref.py, itself
held to transformers' model and feature extractor by tests/test_whisper_cpu.py).  Tolerances are not constants: each case measures,
on its own inputs, how far the fp32 CPU evaluation of the same graph lies from the float64 restatement, and allows the device
``NET_FACTOR`` = 8 times that distance, floored at 1e-6 of the largest magnitude (whisper_ref.tolerance, the rule of
tests/test_gpu_asr.py).  Every case prints the device error, the yardstick and the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import whisper_ref as R

pytestmark = pytest.mark.gpu

CFG = {"TINY": R.TINY, "WIDE": R.WIDE}
PROMPT = (1, 5, 7)
# Feature seeds of the three rows, and a decode run chosen on the CPU so that the restatement emits ``eos`` at different steps in
# rows 0 and 1 (TINY: steps 10 and 19, WIDE: 10 and 30) and never in row 2, which runs to the cap; ``begin`` holds the ids the rows
# would emit first without it.  Smallest float64 top-2 margin over the steps of a row against 4 x the bound of its logits, as
# measured with the fp32 CPU yardstick: TINY 1.9e-2 / 1.7e-2 / 5.8e-2 against 2.0e-3 / 5.1e-3 / 3.1e-3, WIDE 4.5e-2 / 1.5e-2 /
# 1.7e-2 against 1.8e-3 / 3.0e-3 / 5.5e-3: no step is left out.
GEN = {"TINY": dict(seeds=(19, 20, 21), eos=91, suppress=(0, 3), begin=(55, 69), ends=(10, 19, None)),
       "WIDE": dict(seeds=(10, 11, 12), eos=502, suppress=(0, 3), begin=(253, 351, 982), ends=(10, 30, None))}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SD, _MODEL, _GEN = {}, {}, {}


def weights(name):
    if name not in _SD:
        _SD[name] = R.make_weights(CFG[name], 0)
    return _SD[name]


def model(name):
    if name not in _MODEL:
        from dex_tts_amd import whisper
        m = whisper.Whisper(R.library_config(CFG[name]), "cuda")
        _MODEL[name] = m.load_state_dict({k: torch.from_numpy(v) for k, v in weights(name).items()})
    return _MODEL[name]


def spec_of(name, lib=False):
    g = GEN[name]
    if lib:
        from dex_tts_amd.whisper import GenerationSpec
        return GenerationSpec(PROMPT, g["suppress"], g["begin"], g["eos"])
    return R.spec(PROMPT, g["suppress"], g["begin"], g["eos"])


def gen_case(name):
    """Per row of the decode run, computed once and shared, never changed: (features, the restatement's ids up to and including the
    row's eos, the masked float64 logits of those steps, the sequence prompt + ids cut at max_target_positions, its float64 logits,
    the fp32 CPU yardstick's, the float64 encoder output, the yardstick's)."""
    if name not in _GEN:
        cfg, sd, rows = CFG[name], weights(name), []
        for seed in GEN[name]["seeds"]:
            feat = R.make_features(cfg, seed)
            ids, masked = R.greedy(cfg, sd, feat, spec_of(name))
            seq = (list(PROMPT) + ids)[: cfg.max_target_positions]
            enc, ref = R.forward(cfg, sd, feat, seq)
            yenc, yard = R.torch_forward_fp32(cfg, sd, feat, seq)
            rows.append((feat, ids, masked, seq, ref, yard, enc, yenc))
        _GEN[name] = rows
    return _GEN[name]


def check(what, got, ref, yard):
    tol, d = R.tolerance(yard, ref)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: device err {err:.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}, largest magnitude {np.abs(ref).max():.2f}")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert err <= tol, (what, err, tol)
    return tol


# ---------------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_log_mel_ragged_rows(name):
    """Rows of 1, 399, 400 samples and a full chunk, with garbage past each length: each meets the restatement and is BITWISE the row
    alone; a row of chunk + 1 samples raises."""
    cfg, m = CFG[name], model(name)
    N = R.n_samples(cfg)
    lens = [1, 399, 400, N]
    x = (10.0 * np.random.default_rng(3).standard_normal((4, N))).astype(np.float32)
    for b, L in enumerate(lens):
        x[b, :L] = R.synth_wav(L, 40 + b)
    got = m.log_mel(cuda(x), lens).cpu().numpy()
    assert got.shape == (4, cfg.num_mel_bins, 2 * cfg.max_source_positions)
    for b, L in enumerate(lens):
        check(f"log_mel {name} L={L}", got[b], R.log_mel(cfg, x[b, :L]), R.log_mel(cfg, x[b, :L], np.float32))
        alone = m.log_mel(cuda(x[b, :L])).cpu().numpy()
        assert np.array_equal(alone, got[b]), f"row {b} differs from the row alone by {np.abs(alone - got[b]).max():.3e}"
    with pytest.raises(ValueError, match="longer than one chunk"):
        m.log_mel(cuda(np.zeros(N + 1, np.float32)))
    with pytest.raises(ValueError, match="longer than one chunk"):
        m.log_mel(cuda(np.zeros((2, N + 1), np.float32)), [5, N + 1])


# ---------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_encode(name):
    """B = 1 and B = 3 against the restatement; the rows of the batch are BITWISE the rows alone."""
    cfg, m, rows = CFG[name], model(name), gen_case(name)
    got = m.encode(cuda(np.stack([r[0] for r in rows]))).cpu().numpy()
    assert got.shape == (3, cfg.max_source_positions, cfg.d_model)
    for b, r in enumerate(rows):
        check(f"encode {name} B=3 row {b}", got[b], r[6], r[7])
        alone = m.encode(cuda(r[0][None])).cpu().numpy()[0]
        assert np.array_equal(alone, got[b]), f"row {b} differs from the row alone by {np.abs(alone - got[b]).max():.3e}"


# ---------------------------------------------------------------------------------------------------- decoder
@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_forward_teacher_forced(name):
    """The restatement's own greedy ids fed back (row 2 never ends: the prompt plus all of its ids are max_target_positions
    positions, the cache at every length from 1 to its capacity); every position's logits.  A batch of the three rows over the
    positions they all have is BITWISE the rows alone."""
    cfg, m, rows = CFG[name], model(name), gen_case(name)
    assert len(rows[2][3]) == cfg.max_target_positions
    alone = []
    for b, r in enumerate(rows):
        got = m.forward(cuda(r[0][None]), cuda(np.asarray([r[3]], np.int32))).cpu().numpy()[0]
        check(f"forward {name} row {b}, {len(r[3])} positions", got, r[4], r[5])
        alone.append(got)
    L = min(len(r[3]) for r in rows)
    got = m.forward(cuda(np.stack([r[0] for r in rows])), cuda(np.asarray([r[3][:L] for r in rows], np.int32))).cpu().numpy()
    for b in range(3):
        assert np.array_equal(got[b], alone[b][:L]), f"row {b} differs from the row alone by {np.abs(got[b] - alone[b][:L]).max():.3e}"


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_generate(name):
    """B = 3 rows with different inputs: eos at different steps in rows 0 and 1, never in row 2, which runs to the cap.  Device ids
    equal the restatement's through the first step whose float64 top-2 margin is below 4 x the bound of the row's logits; later steps
    are left out, at most 10 % of all (with these seeds: none, see GEN).  Rows are eos-padded, the lengths are right, each row is
    the row alone, the first id is not the one ``begin_suppress_tokens`` holds, and ``max_new_tokens`` beyond the cache stops at
    ``max_target_positions`` exactly."""
    cfg, m, rows, g = CFG[name], model(name), gen_case(name), GEN[name]
    room = cfg.max_target_positions - len(PROMPT)
    feats = cuda(np.stack([r[0] for r in rows]))
    ids, lens = m.generate(feats, spec_of(name, True), max_new_tokens=1000)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    assert ids.shape == (3, room) and ids.dtype == np.int32
    total = left_out = 0
    for b, r in enumerate(rows):
        ref_ids, masked = r[1], r[2]
        end = g["ends"][b]
        assert (ref_ids.index(g["eos"]) if g["eos"] in ref_ids else None) == end and len(ref_ids) == (room if end is None else end + 1)
        unmasked_first = int(np.argmax(np.where(np.isin(np.arange(cfg.vocab_size), g["suppress"]), -np.inf, r[4][len(PROMPT) - 1])))
        assert unmasked_first in g["begin"] and ref_ids[0] != unmasked_first and ids[b, 0] not in g["begin"]
        tol, _ = R.tolerance(r[5], r[4])
        margin = R.top2_margin(masked)
        low = np.nonzero(margin < 4 * tol)[0]
        n = len(ref_ids) if len(low) == 0 else int(low[0]) + 1
        total, left_out = total + len(ref_ids), left_out + len(ref_ids) - n
        print(f"generate {name} row {b}: {len(ref_ids)} steps, smallest margin {margin.min():.3e}, 4 x bound {4 * tol:.3e}, compared {n}")
        assert ids[b, :n].tolist() == ref_ids[:n]
        if n == len(ref_ids):
            want_len = len(ref_ids) - (1 if end is not None else 0)
            assert lens[b] == want_len and (ids[b, want_len:] == g["eos"]).all()
        a_ids, a_lens = m.generate(feats[b:b + 1], spec_of(name, True))
        a_ids = a_ids.cpu().numpy()[0]
        assert int(a_lens[0]) == lens[b] and np.array_equal(a_ids, ids[b, : len(a_ids)]) and (ids[b, len(a_ids):] == g["eos"]).all()
    assert left_out * 10 <= total, (left_out, total)
    short, _ = m.generate(feats, spec_of(name, True), max_new_tokens=5)
    assert np.array_equal(short.cpu().numpy(), ids[:, :5])


def test_generate_ends_early_once_every_row_has_finished():
    """Rows 0 and 1 of the TINY run end at steps 10 and 19: the finished-count read every SYNC_EVERY = 8 steps ends the loop at 24
    of the 29 steps the cache has room for."""
    from dex_tts_amd import whisper
    rows = gen_case("TINY")
    ids, lens = model("TINY").generate(cuda(np.stack([r[0] for r in rows[:2]])), spec_of("TINY", True))
    assert whisper.SYNC_EVERY == 8 and ids.shape == (2, 24) and lens.tolist() == [10, 19]
    for b in range(2):
        assert ids[b, : lens[b]].tolist() == rows[b][1][:-1] and (ids[b, lens[b]:] == GEN["TINY"]["eos"]).all()


# ---------------------------------------------------------------------------------------------------- the two new kernels alone
def _softmax_attend(q, k, v, dtype):
    """q [B, H, 64], k / v [B, n, H, 64] -> [B, H, 64] in ``dtype``."""
    q, k, v = (a.astype(dtype) for a in (q, k, v))
    s = np.einsum("bhc,bnhc->bhn", q * dtype(0.125), k)
    s = np.exp(s - s.max(axis=-1, keepdims=True))
    return np.einsum("bhn,bnhc->bhc", s / s.sum(axis=-1, keepdims=True), v)


@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("n,append", [(1, True), (2, True), (63, True), (64, True), (65, True), (448, True),
                                      (1, False), (50, False), (64, False), (65, False), (1500, False)])
def test_attend_kernel(n, append, B, H):
    """The cached single-query attention alone at head_dim 64, B x H in {1, 6}: the self-attention use (the step's k and v appended
    at position n - 1 of a cache with room for more) at cache lengths 1 .. 448, the cross-attention use at 1 .. 1500 keys."""
    from dex_tts_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(n * 7 + B)
    cap = n + 3 if append else n
    q = rng.standard_normal((B, H, 64)).astype(np.float32) * 2
    k = rng.standard_normal((B, cap, H, 64)).astype(np.float32)
    v = rng.standard_normal((B, cap, H, 64)).astype(np.float32)
    kd, vd = k.copy(), v.copy()
    if append:                                   # the device gets garbage where the step's k and v belong
        kd[:, n - 1:], vd[:, n - 1:] = 1e30, -1e30
    tq, tk, tv, out = cuda(q), cuda(kd), cuda(vd), torch.full((B, H * 64), float("nan"), device="cuda")
    nk, nv = (cuda(k[:, n - 1]), cuda(v[:, n - 1])) if append else (None, None)
    rc = lib.dex_whisper_attend(tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), nk.data_ptr() if append else None, nv.data_ptr() if append else None,
                                out.data_ptr(), B, H, n, cap, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = out.cpu().numpy().reshape(B, H, 64)
    check(f"attend n={n} append={append} B x H = {B * H}", got, _softmax_attend(q, k[:, :n], v[:, :n], np.float64),
          _softmax_attend(q, k[:, :n], v[:, :n], np.float32))
    if append:
        assert np.array_equal(tk.cpu().numpy()[:, n - 1], k[:, n - 1]) and np.array_equal(tv.cpu().numpy()[:, n - 1], v[:, n - 1])
        assert (tk.cpu().numpy()[:, n:] == 1e30).all()


def _step_linear(x, w, form):
    from dex_tts_amd import _lib
    (M, K), N = x.shape, w.shape[1]
    tx, tw, y = cuda(x), cuda(w), torch.full((M, N), float("nan"), device="cuda")
    scratch = torch.empty((K // 64) * M * N, device="cuda")
    rc = _lib.load().dex_whisper_step_linear(tx.data_ptr(), tw.data_ptr(), y.data_ptr(), scratch.data_ptr(), scratch.numel(), M, K, N, form,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return y.cpu().numpy()


@pytest.mark.parametrize("K,N", [(64, 64), (128, 384), (384, 1152), (1536, 384), (2048, 64)])
def test_step_linear_kernel(K, N):
    """The skinny-M streaming kernel and its consumer alone: one slab with a single live wave (K = 64), one with two (K = 128) and several
    (256 rows each: K = 384 is one and a half, 1536 six, 2048 eight), every row-count form (M = 1, 3, 8, 17, 32), against float64; a row is BITWISE the row alone, whatever M is."""
    rng = np.random.default_rng(K + N)
    x, w = rng.standard_normal((32, K)).astype(np.float32), (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64)
    alone = np.concatenate([_step_linear(x[b:b + 1], w, 0) for b in (0, 2, 16, 31)])
    for M in (1, 3, 8, 17, 32):
        got = _step_linear(x[:M], w, 0)
        check(f"step linear K={K} N={N} M={M}", got, ref[:M], x[:M] @ w)
        for i, b in enumerate((0, 2, 16, 31)):
            if b < M:
                assert np.array_equal(got[b], alone[i]), f"row {b} of M={M} differs from the row alone"
    check(f"launch_igemm K={K} N={N} M=32", _step_linear(x, w, 1), ref, x @ w)


def _pick(logits, mask, eos, finished):
    from dex_tts_amd import _lib
    B, V = logits.shape
    lg, fin = cuda(logits.astype(np.float32)), cuda(np.asarray(finished, np.int32))
    mk = cuda(np.asarray(mask, np.uint8)) if mask is not None else None
    lens, count, ids = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    rc = _lib.load().dex_whisper_pick(lg.data_ptr(), B, V, mk.data_ptr() if mk is not None else None, eos, fin.data_ptr(), lens.data_ptr(),
                                      count.data_ptr(), ids.data_ptr(), 2, 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    ids = ids.cpu().numpy()
    assert (ids[:, 0] == -1).all()
    return ids[:, 1].tolist(), fin.cpu().tolist(), lens.cpu().tolist(), int(count.item())


@pytest.mark.parametrize("V", [96, 51866])
def test_pick_kernel(V):
    """The greedy step tail alone on crafted logits, exact: a V-way tie -> id 0; the maximum suppressed; the maximum in the last
    element; all but one id suppressed; an already-finished row stays eos; emitting eos finishes a row."""
    eos = V - 2
    x = np.tile(np.linspace(-1.0, 1.0, V)[None], (6, 1))
    x[0, :] = 0.25                                                     # a V-way tie
    x[1, V // 3], x[1, V // 2] = 7.0, 6.0                              # the maximum suppressed: the runner-up wins
    x[2, :] = -x[2, :]; x[2, V - 1] = 5.0                              # the maximum in the last element
    x[3, :] = 3.0                                                      # a row of its own mask below: one id left, and not the largest
    x[4, 5] = 9.0                                                      # already finished: eos whatever the logits say
    x[5, eos] = 9.0                                                    # emits eos
    mask = np.zeros(V, np.uint8)
    mask[V // 3] = 1
    ids, fin, lens, count = _pick(x, mask, eos, [0, 0, 0, 0, 1, 0])
    assert ids == [0, V // 2, V - 1, 0, eos, eos]
    assert fin == [0, 0, 0, 0, 1, 1] and lens == [1, 1, 1, 1, 0, 0] and count == 1
    only = np.ones(V, np.uint8)
    only[V - 7] = 0
    ids, fin, lens, count = _pick(x[3:4] - np.arange(V)[None] * 1e-3, only, eos, [0])
    assert ids == [V - 7] and lens == [1] and count == 0
    ids, _, _, _ = _pick(x[1:2], None, eos, [0])
    assert ids == [V // 3]


def test_transcribe_and_score():
    """``synthesize.whisper_scores`` on int16 waveforms at 22050 Hz is its pieces: resampling, ``log_mel``, ``generate``, ``decode`` and
    the reference's score of the transcripts."""
    from dex_tts_amd import synthesize, whisper
    from dex_tts_amd.asr import score_transcripts
    m, sp = model("TINY"), spec_of("TINY", True)
    vocab = [f"\u0120w{i}" for i in range(R.TINY.vocab_size)]
    audio = [(R.synth_wav(n, 70 + i) * 32767.0).astype(np.int16) for i, n in enumerate((9000, 12001))]
    texts = ["w1 w2 w3", "w4, w5!"]
    preds, *score = synthesize.whisper_scores(m, sp, vocab, audio, texts, sr=22050)
    ids, lens = m.generate(m.log_mel(audio, sr=22050), sp)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    want = [whisper.decode(ids[b, : lens[b]], vocab, sp.eos_token_id) for b in range(2)]
    assert preds == want and any(preds) and all(p == "" or p.startswith(" w") for p in preds)
    assert tuple(score) == score_transcripts(texts, preds)
    assert m.transcribe(audio[1:], sp, vocab, sr=22050) == preds[1:]
    with pytest.raises(ValueError, match="waveforms against"):
        synthesize.whisper_scores(m, sp, vocab, audio, texts[:1])


# ---------------------------------------------------------------------------------------------------- errors
def test_errors():
    from dex_tts_amd import whisper
    cfg, m, rows = R.TINY, model("TINY"), gen_case("TINY")
    feat = rows[0][0][None]
    sp = spec_of("TINY", True)
    with pytest.raises(ValueError, match="CUDA"):
        m.encode(torch.from_numpy(feat))
    with pytest.raises(ValueError, match="CUDA"):
        m.log_mel(torch.zeros(100))
    with pytest.raises(ValueError, match="CUDA"):
        m.forward(cuda(feat), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="max_target_positions"):
        m.generate(cuda(feat), whisper.GenerationSpec(tuple(range(1, cfg.max_target_positions + 2)), (), (), 91))
    with pytest.raises(ValueError, match="max_target_positions"):
        m.forward(cuda(feat), cuda(np.ones((1, cfg.max_target_positions + 1), np.int32)))
    with pytest.raises(ValueError, match="vocab"):
        m.forward(cuda(feat), cuda(np.asarray([[1, cfg.vocab_size]], np.int32)))
    with pytest.raises(ValueError, match="vocabulary"):
        m.generate(cuda(feat), whisper.GenerationSpec((1, cfg.vocab_size), (), (), 91))
    with pytest.raises(ValueError, match="features"):
        m.encode(cuda(feat[:, :, :-1]))
    empty = whisper.Whisper(R.library_config(cfg), "cuda")
    with pytest.raises(ValueError, match="not loaded"):
        empty.generate(cuda(feat), sp)
    with pytest.raises(ValueError, match="not loaded"):
        empty.encode(cuda(feat))
    sd = {k: torch.from_numpy(v) for k, v in weights("TINY").items()}
    with pytest.raises(RuntimeError, match="proj_out"):
        empty.load_state_dict(dict(sd, **{"proj_out.weight": sd["model.decoder.embed_tokens.weight"] + 1e-3}))
    stripped = {k[len("model."):]: v for k, v in sd.items()}
    stripped["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"].clone()
    assert np.array_equal(empty.load_state_dict(stripped).encode(cuda(feat)).cpu().numpy(), m.encode(cuda(feat)).cpu().numpy())
    with pytest.raises(NotImplementedError, match="scale_embedding"):
        whisper.Whisper(R.library_config(R._cfg(**dict(vars(cfg), scale_embedding=True))), "cuda")
    with pytest.raises(ValueError, match="MI355X"):
        whisper.Whisper(R.library_config(cfg), "cpu")


REFUSALS = {"prompt id": (dict(prompt=(1, 96, 7)), -1, "prompt id 96 is outside the vocabulary of 96"),
            "eos": (dict(eos=96), -1, "eos_token_id 96 is outside the vocabulary of 96"),
            "max_new": (dict(max_new=0), -1, "max_new must be >= 1 and sync_every >= 0"),
            "sync_every": (dict(sync_every=-1), -1, "max_new must be >= 1 and sync_every >= 0"),
            "not finalized": (dict(finalized=False), -2, "the whisper weights are not finalized (dex_whisper_finalize)")}


@pytest.mark.parametrize("entry", ["generate", "generate_ts", "generate_policy", "generate_beam"])
def test_refusal_parity(entry):
    """The four decoding entry points refuse the arguments they share in the same words with the same code, in host code: the
    outputs still hold what the test put there (a first launch would have filled the ids with eos)."""
    from dex_tts_amd import whisper
    cfg = R.TINY
    empty = whisper.Whisper(R.library_config(cfg), "cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mask = torch.zeros(cfg.vocab_size, dtype=torch.uint8, device="cuda")
    for what, (change, code, text) in REFUSALS.items():
        a = dict(prompt=PROMPT, eos=30, max_new=4, sync_every=2, finalized=True)
        a.update(change)
        ctx = (model("TINY") if a["finalized"] else empty)._ctx
        prompt = np.ascontiguousarray(np.asarray(a["prompt"], np.int32))
        ids, lens = torch.full((1, 4), -7, dtype=torch.int32, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda")
        stat, steps = torch.full((3,), -7.0, dtype=torch.float64, device="cuda"), C.c_int(-7)
        head = (ctx.h, prompt.ctypes.data_as(C.POINTER(C.c_int32)), len(prompt), mask.data_ptr(), mask.data_ptr(), a["eos"])
        if entry == "generate_beam":
            ws = ctx.beam_workspace(1, 2)
            rc = ctx.lib.dex_whisper_generate_beam(*head, 1, 2, 1.0, a["max_new"], a["sync_every"], ids.data_ptr(), lens.data_ptr(), stat.data_ptr(),
                                                   C.byref(steps), *[None] * 8, ws.data_ptr(), ws.numel(), st)
        else:
            ws = ctx.workspace(1)
            tail = (1, a["max_new"], a["sync_every"], ids.data_ptr(), lens.data_ptr())
            end = (C.byref(steps), ws.data_ptr(), ws.numel(), st)
            if entry == "generate":
                rc = ctx.lib.dex_whisper_generate(*head, *tail, *end)
            elif entry == "generate_ts":
                rc = ctx.lib.dex_whisper_generate_ts(*head, 40, -1, *tail, *end)
            else:
                key, zero = (C.c_uint32 * 1)(0), (C.c_int32 * 1)(0)
                rc = ctx.lib.dex_whisper_generate_policy(*head, 0, -1, -1, 0.0, 0, 0, key, zero, 1, zero, *tail, stat[:1].data_ptr(), lens.data_ptr(), 0,
                                                         None, *end)
        got = ctx.lib.dex_whisper_last_error(ctx.h).decode()
        torch.cuda.synchronize()
        assert (rc, got) == (code, text), (entry, what, rc, got)
        assert steps.value == -7 and (ids.cpu() == -7).all() and (lens.cpu() == -7).all() and (stat.cpu() == -7.0).all(), (entry, what)
