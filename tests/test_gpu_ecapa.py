"""GPU: the WavLM-large + ECAPA-TDNN path of dex_tts_amd/ecapa.py (csrc/ecapa.hip) against its float64 restatement
(tests/ecapa_ref.py, itself held to transformers' trunk and torch.nn modules by tests/test_ecapa_cpu.py).  Tolerances are not
constants: each case measures, on its own inputs, how far the torch fp32 CPU evaluation of the same graph lies from the float64
restatement, and allows the device ``NET_FACTOR`` = 8 times that distance, floored at 1e-6 of the largest magnitude
(ecapa_ref.tolerance).  Every case prints the device error, the yardstick and the bound.  The references are computed on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ecapa_ref as R

pytestmark = pytest.mark.gpu

CFG = {"TINY": R.TINY, "WIDE": R.WIDE, "TINY_GC": R.TINY_GC}
RAGGED = [32080, 720, 20880]        # 100, 2 and 65 frames
TILE = 72                           # checked against the module's RES2_TILE below


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SD, _MODEL, _CASE = {}, {}, {}


def weights(name):
    if name not in _SD:
        _SD[name] = R.make_weights(CFG[name], 0)
    return _SD[name]


def model(name, do_normalize=True):
    key = (name, do_normalize)
    if key not in _MODEL:
        from dex_tts_amd import ecapa
        m = ecapa.WavLMEcapa(R.library_config(CFG[name]), "cuda", do_normalize=do_normalize)
        _MODEL[key] = m.load_state_dict({k: torch.from_numpy(v) for k, v in weights(name).items()})
    return _MODEL[key]


def reference(name, wav, do_normalize=True):
    """(wav, float64 (mix, embedding), fp32 CPU yardstick (mix, embedding)) of one utterance."""
    return (wav, R.forward(CFG[name], weights(name), wav, do_normalize), R.torch_forward_fp32(CFG[name], weights(name), wav, do_normalize))


def case(name, n, seed):
    """``reference`` of ``synth_wav(n, seed)``: computed once and shared, never changed."""
    key = (name, n, seed)
    if key not in _CASE:
        _CASE[key] = reference(name, R.synth_wav(n, seed))
    return _CASE[key]


def check(what, got, ref, yard):
    tol, d = R.tolerance(yard, ref)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: device err {err:.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}, magnitude {np.abs(ref).max():.2f}")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert err <= tol, (what, err, tol)


def check_both(what, hid, emb, ref, yard):
    check(what + " mix", hid, ref[0], yard[0])
    check(what + " embedding", emb, ref[1], yard[1])


# ---------------------------------------------------------------------------------------------------- the Res2 chain alone
def res2_lengths(d):
    return [2, 7 * d, 7 * d + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 7 * d + 1]


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
@pytest.mark.parametrize("block", [0, 1, 2])
def test_res2_chain_alone(name, block):
    """One launch (dex_ecapa_res2) at slices of 32 (TINY) and 64 (WIDE) channels, dilations 2, 3, 4.  Two frames: every off-centre
    tap is padding.  7 d and 7 d + 1: the halo of seven stages just reaches / just misses the row's start.  TILE - 1, TILE, TILE + 1
    and 2 TILE + 7 d + 1: one workgroup, exactly one, a second with one frame, three.  Then a ragged batch of three with large
    garbage past each length: every row bitwise the row alone and exactly 0 past its frames - a stage's zero padding sits at the
    row's own end, whatever lies in the tensor there.  The eighth slice passes through bit for bit."""
    from dex_tts_amd import ecapa
    assert ecapa.RES2_TILE == TILE
    cfg, m = CFG[name], model(name)
    Cc, d = cfg.channels, cfg.dilations[block]
    w = Cc // 8
    rng = np.random.default_rng(100 + block)
    alone = {}
    for T in res2_lengths(d):
        x = rng.standard_normal((T, Cc)).astype(np.float32)
        got = m.res2(block, cuda(x)).cpu().numpy()
        check(f"{name} block {block} (d = {d}) T = {T}", got, R.res2(cfg, weights(name), block, x), R.torch_res2_fp32(cfg, weights(name), block, x))
        assert np.array_equal(got[:, 7 * w:], x[:, 7 * w:])
        alone[T] = (x, got)
    lens = [TILE + 1, 2, 2 * TILE + 7 * d + 1]
    xb = (1e3 * rng.standard_normal((3, max(lens), Cc))).astype(np.float32)
    for b, T in enumerate(lens):
        xb[b, :T] = alone[T][0]
    got = m.res2(block, cuda(xb), lens).cpu().numpy()
    for b, T in enumerate(lens):
        assert np.array_equal(got[b, :T], alone[T][1]), f"row {b} differs from the row alone by {np.abs(got[b, :T] - alone[T][1]).max():.3e}"
        assert not got[b, T:].any()


# ---------------------------------------------------------------------------------------------------- the whole network
@pytest.mark.parametrize("n", [720, 1040, 32080])
def test_single_rows_tiny(n):
    """720 samples are 2 frames, the minimum; 1040 are 3; 32080 are 100: distances past max_bucket_distance = 40 take the clamped
    far bucket on both signs, and the Res2 chains run two workgroups per row."""
    wav, ref, yard = case("TINY", n, n)
    m = model("TINY")
    hid, emb = m.hidden_states(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy()
    assert hid.shape == (R.num_frames(R.TINY, n), 128) and emb.shape == (32,)
    check_both(f"TINY n={n}", hid, emb, ref, yard)


def ragged(name):
    cases = [case(name, L, 20 + b) for b, L in enumerate(RAGGED)]
    x = (10.0 * np.random.default_rng(3).standard_normal((len(RAGGED), max(RAGGED)))).astype(np.float32)
    for b, L in enumerate(RAGGED):
        x[b, :L] = cases[b][0]
    return x, cases


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_ragged_batch_rows_are_the_rows_alone(name):
    """[32080, 720, 20880] with garbage past each length: every row meets the restatement, is BITWISE the row alone (the input
    normalisation, the attention keys, the instance norm, the squeeze-excitation means, the pooling's softmax and every
    convolution's padding end at the row's own frames), its mix is 0 past its frames, and its embedding is finite with dead ReLU
    channels before the pooling (their pooled deviation is exactly sqrt(1e-9) in the restatement)."""
    cfg, m = CFG[name], model(name)
    x, cases = ragged(name)
    hid = m.hidden_states(cuda(x), RAGGED).cpu().numpy()
    emb = m.forward(cuda(x), RAGGED).cpu().numpy()
    assert hid.shape == (3, 100, cfg.hidden_size) and emb.shape == (3, cfg.emb_dim) and np.isfinite(emb).all()
    w64 = {k: np.asarray(v, np.float64) for k, v in weights(name).items()}
    for b, L in enumerate(RAGGED):
        T = R.num_frames(cfg, L)
        wav, ref, yard = cases[b]
        check_both(f"ragged {name} row {b}", hid[b, :T], emb[b], ref, yard)
        assert not hid[b, T:].any()
        assert (R.pooled(cfg, w64, ref[0])[3 * cfg.channels:] == np.sqrt(1e-9)).any()
        alone_h, alone_e = m.hidden_states(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy()
        assert np.array_equal(alone_h, hid[b, :T]), f"row {b} mix differs from the row alone by {np.abs(alone_h - hid[b, :T]).max():.3e}"
        assert np.array_equal(alone_e, emb[b]), f"row {b} embedding differs from the row alone by {np.abs(alone_e - emb[b]).max():.3e}"


def test_global_context_attention():
    wav, ref, yard = reference("TINY_GC", R.synth_wav(20880, 14))
    m = model("TINY_GC")
    check_both("TINY global_context_att", m.hidden_states(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy(), ref, yard)


@pytest.mark.parametrize("norm", [True, False])
def test_do_normalize_with_a_dc_offset(norm):
    """0.05 + a signal of amplitude 0.01: its variance is of the order of the normalisation's eps.  With eps 1e-5 (the upstream's
    F.layer_norm) the normalised wav is about 0.7 times what eps 1e-7 (Wav2Vec2FeatureExtractor's) makes of it: the restatement
    with the other eps lies far outside the bound the device meets."""
    wav = R.dc_wav(20880, 11, dc=0.05, amp=0.01)
    _, ref, yard = reference("TINY", wav, norm)
    m = model("TINY", norm)
    hid, emb = m.hidden_states(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy()
    check_both(f"TINY do_normalize={norm}", hid, emb, ref, yard)
    if norm:
        from tests import asr_ref
        other = R.forward(R.TINY, weights("TINY"), asr_ref.normalize_input(wav), do_normalize=False)
        tol, _ = R.tolerance(yard[1], ref[1])
        gap = float(np.abs(other[1] - ref[1]).max())
        print(f"eps 1e-7 in place of 1e-5 moves the embedding by {gap:.3e}; bound {tol:.3e}")
        assert gap > 100 * tol


def test_similarity():
    """A wav with itself: 1 within fp32 rounding.  Symmetric.  A pair against the restatement's cosine."""
    from dex_tts_amd import ecapa, synthesize
    m = model("TINY")
    a, b = R.synth_wav(20880, 50), R.synth_wav(16000, 60)
    same = float(ecapa.similarity(cuda(a), cuda(a), source_sr=16000, model=m).cpu().numpy()[0])
    assert abs(same - 1.0) <= 1e-6
    ab = float(ecapa.similarity(cuda(a), cuda(b), source_sr=16000, model=m).cpu().numpy()[0])
    ba = float(ecapa.similarity(cuda(b), cuda(a), source_sr=16000, model=m).cpu().numpy()[0])
    assert abs(ab - ba) <= 1e-6
    (_, ra, ya), (_, rb, yb) = reference("TINY", a), reference("TINY", b)
    ref = R.cosine(ra[1], rb[1])
    d = abs(R.cosine(ya[1], yb[1]) - ref)
    tol = max(R.NET_FACTOR * d, R.NET_FLOOR)
    print(f"similarity: device {ab:.7f}, restatement {ref:.7f}, err {abs(ab - ref):.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}")
    assert abs(ab - ref) <= tol
    mean, err = ecapa.sim_score(cuda(a), cuda(b), source_sr=16000, model=m)
    assert abs(mean - ab) < 1e-7 and err == 0.0
    # synthesize.ecapa_sim_scores: int16 audio against float references, both at 16 kHz
    audio = [np.round(w * 32767.0).astype(np.int16) for w in (a, b)]
    cos, mean, err = synthesize.ecapa_sim_scores(m, audio, [b, a], sr=16000)
    cos = cos.cpu().numpy()
    assert cos.shape == (2,) and np.isfinite([mean, err]).all() and (mean, err) == ecapa.mean_stderr(cos)
    _, rq, yq = reference("TINY", audio[0].astype(np.float32) / 32768.0)      # what the score reads of the int16 audio
    refq = R.cosine(rq[1], rb[1])
    dq = abs(R.cosine(yq[1], yb[1]) - refq)
    print(f"ecapa_sim_scores pair 0: device {float(cos[0]):.7f}, restatement {refq:.7f}, cpu fp32 yardstick {dq:.3e}")
    assert abs(float(cos[0]) - refq) <= max(R.NET_FACTOR * dq, R.NET_FLOOR)


def test_refusals():
    """Refused before anything is enqueued: a short row, more frames than one call takes, weights that are not loaded - by the
    wrapper, and by the C ABI itself; a workspace one byte short returns the error code."""
    from dex_tts_amd import ecapa
    m = model("TINY")
    with pytest.raises(ValueError):
        m.forward(torch.zeros(32080))                             # a CPU tensor
    with pytest.raises(ValueError, match="too short"):
        m.forward(torch.zeros(719, device="cuda"))
    with pytest.raises(ValueError, match="too short"):
        m.hidden_states(torch.zeros(2, 32080, device="cuda"), [32080, 700])
    with pytest.raises(ValueError, match="at most"):
        m.forward(torch.zeros(16000 * 90, device="cuda"))         # 4499 frames > DEX_ECAPA_MAX_FRAMES
    with pytest.raises(ValueError):
        m.res2(3, torch.zeros(10, 256, device="cuda"))
    with pytest.raises(ValueError):
        m.res2(0, torch.zeros(10, 255, device="cuda"))
    fresh = ecapa.WavLMEcapa(R.library_config(R.TINY), "cuda")
    with pytest.raises(ValueError, match="not loaded"):
        fresh.forward(torch.zeros(32080, device="cuda"))
    ctx, lib = m._ctx, m._ctx.lib
    x = torch.zeros(2, 32080, device="cuda")
    out = torch.full((2, 32), 7.0, device="cuda")
    ws = ctx.workspace(2, 32080)
    need = int(lib.dex_ecapa_workspace_bytes(ctx.h, 2, 32080))
    assert 0 < need <= ws.numel()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def embed(handle, lens, n, nbytes):
        ln = np.asarray(lens, np.int32)
        return lib.dex_ecapa_embed(handle, x.data_ptr(), ln.ctypes.data_as(C.POINTER(C.c_int32)), len(lens), n, 1, out.data_ptr(), ws.data_ptr(), nbytes, st)

    assert embed(ctx.h, [32080, 700], 32080, need) == -1 and b"too short" in lib.dex_ecapa_last_error(ctx.h)
    assert embed(ctx.h, [32080, 32081], 32080, need) == -1
    assert embed(ctx.h, [32080], 16000 * 90, need) == -1 and b"at most" in lib.dex_ecapa_last_error(ctx.h)
    assert embed(ctx.h, [32080, 32080], 32080, need - 1) not in (0, -1) and b"workspace" in lib.dex_ecapa_last_error(ctx.h)
    assert embed(fresh._ctx.h, [32080, 32080], 32080, need) == -2
    assert lib.dex_ecapa_workspace_bytes(ctx.h, 1, 719) == 0 and lib.dex_ecapa_workspace_bytes(ctx.h, 1, 16000 * 90) == 0
    fr = np.asarray([5, 11], np.int32)
    xr = torch.zeros(2, 10, 256, device="cuda")
    assert lib.dex_ecapa_res2(ctx.h, 0, xr.data_ptr(), fr.ctypes.data_as(C.POINTER(C.c_int32)), 2, 10, out.data_ptr(), st) == -1
    assert lib.dex_ecapa_res2(ctx.h, 0, xr.data_ptr(), fr.ctypes.data_as(C.POINTER(C.c_int32)), 2, 10, xr.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                     # nothing was enqueued
    assert embed(ctx.h, [32080, 32080], 32080, need) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == 7.0).all()
