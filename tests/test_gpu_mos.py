"""GPU: the UTMOS path of dex_tts_amd/mos.py (csrc/mos.hip) against its float64 restatement (tests/mos_ref.py, itself held to
transformers' and torch.nn's modules by tests/test_mos_cpu.py).  Tolerances are not constants: each case measures, on its own inputs,
how far the torch fp32 CPU evaluation of the same graph lies from the float64 restatement, and allows the device ``NET_FACTOR`` = 8
times that distance, floored at 1e-6 of the largest magnitude (mos_ref.tolerance, which is wavlm_ref's).  Every case prints the device
error, the yardstick and the bound."""
import numpy as np
import pytest
import torch

from tests import mos_ref as R

pytestmark = pytest.mark.gpu

CFG = {"TINY": R.TINY, "TINY_H512": R.TINY_H512, "WIDE": R.WIDE}
RAGGED = [32080, 400, 20880]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SD, _MODEL, _CASE = {}, {}, {}


def weights(name):
    if name not in _SD:
        _SD[name] = R.make_weights(CFG[name], 0)
    return _SD[name]


def model(name):
    if name not in _MODEL:
        from dex_tts_amd import mos
        m = mos.UTMOS(R.library_config(CFG[name]), "cuda")
        _MODEL[name] = m.load_state_dict({k: torch.from_numpy(v) for k, v in weights(name).items()})
    return _MODEL[name]


def reference(name, wav, domain=R.DOMAIN, judge=R.JUDGE):
    """(wav, float64 (hidden, lstm_out, frames, score), fp32 CPU yardstick of the same) of one utterance."""
    return (wav, R.forward(CFG[name], weights(name), wav, domain, judge), R.torch_forward_fp32(CFG[name], weights(name), wav, domain, judge))


def case(name, n, seed, domain=R.DOMAIN, judge=R.JUDGE):
    """``reference`` of ``synth_wav(n, seed)``: computed once and shared, never changed."""
    key = (name, n, seed, domain, judge)
    if key not in _CASE:
        _CASE[key] = reference(name, R.synth_wav(n, seed), domain, judge)
    return _CASE[key]


def check(what, got, ref, yard):
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    tol, d = R.tolerance(yard, ref)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: device err {err:.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}, magnitude {np.abs(ref).max():.2f}")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert err <= tol, (what, err, tol)


def check_all(what, hid, frames, score, ref, yard):
    check(what + " hidden", hid, ref[0], yard[0])
    check(what + " frame scores", frames, ref[2], yard[2])
    check(what + " score", np.array([score]), np.array([ref[3]]), np.array([yard[3]]))


def run_single(name, n):
    wav, ref, yard = case(name, n, n)
    m = model(name)
    x = cuda(wav)
    hid, frames, score = m.hidden_states(x).cpu().numpy(), m.frame_scores(x).cpu().numpy(), m.forward(x)
    T = R.num_frames(CFG[name], n)
    assert hid.shape == (T, CFG[name].hidden_size) and frames.shape == (T,) and score.shape == ()
    check_all(f"{name} n={n}", hid, frames, float(score), ref, yard)


@pytest.mark.parametrize("n", [400, 720, 5200, 32080])
def test_single_rows_tiny(n):
    """400 samples are one frame: both directions of the recurrence are one step.  720 are two, 32080 a hundred."""
    run_single("TINY", n)


@pytest.mark.parametrize("n", [720, 32080])
def test_single_rows_production_recurrence(n):
    """lstm_hidden = 512 on the small trunk: the 2048-column recurrence (two columns per thread) for 2 and for 100 steps."""
    run_single("TINY_H512", n)


@pytest.mark.parametrize("T", [1, 2, 3, 100])
@pytest.mark.parametrize("name", ["TINY", "TINY_H512"])
def test_bilstm_alone(name, T):
    """The recurrence one launch at a time, H = 64 and H = 512, on seeded features: one row more than a workgroup owns, lengths that
    differ inside the group (length 1 next to length T), ids that differ per row.  Every row meets the restatement at its own length,
    is bitwise the row alone, and is 0 past its length."""
    from dex_tts_amd import mos
    cfg, sd, m = CFG[name], weights(name), model(name)
    B = mos.LSTM_ROWS + 1
    lens = [T, 1, max(1, T // 2), T, max(1, T - 1)][:B]
    dom, jud = [0, 1, 2, 1, 0][:B], [288, 0, 2999, 17, 1000][:B]
    feats = np.random.default_rng(100 + T).standard_normal((B, T, cfg.hidden_size)).astype(np.float32)
    out = m.bilstm(cuda(feats), lens, dom, jud).cpu().numpy()
    assert out.shape == (B, T, 2 * cfg.lstm_hidden)
    for b, L in enumerate(lens):
        ref = R.bilstm(cfg, sd, feats[b, :L], dom[b], jud[b])
        check(f"{name} bilstm T={T} row {b} (length {L})", out[b, :L], ref, R.torch_bilstm_fp32(cfg, sd, feats[b, :L], dom[b], jud[b]))
        assert not out[b, L:].any()
        alone = m.bilstm(cuda(feats[b, :L]), None, dom[b], jud[b]).cpu().numpy()
        assert np.array_equal(alone, out[b, :L]), f"row {b} differs from the row alone by {np.abs(alone - out[b, :L]).max():.3e}"


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_ragged_batch_rows_are_the_rows_alone(name):
    """[32080, 400, 20880] with garbage past each length: every row meets the restatement, is BITWISE the row alone (the group norm,
    the attention keys, the reverse direction and the mean end at the row's own frames), and its frame scores are 0 past its frames.
    WIDE runs the default widths: 48-channel positional groups, 12 heads, H = 512."""
    m = model(name)
    cases = [case(name, L, 20 + b) for b, L in enumerate(RAGGED)]
    x = (10.0 * np.random.default_rng(3).standard_normal((len(RAGGED), max(RAGGED)))).astype(np.float32)
    for b, L in enumerate(RAGGED):
        x[b, :L] = cases[b][0]
    hid = m.hidden_states(cuda(x), RAGGED).cpu().numpy()
    frames = m.frame_scores(cuda(x), RAGGED).cpu().numpy()
    score = m.forward(cuda(x), RAGGED).cpu().numpy()
    assert hid.shape == (3, 100, CFG[name].hidden_size) and frames.shape == (3, 100) and score.shape == (3,)
    for b, L in enumerate(RAGGED):
        T = R.num_frames(CFG[name], L)
        wav, ref, yard = cases[b]
        check_all(f"ragged {name} row {b}", hid[b, :T], frames[b, :T], float(score[b]), ref, yard)
        assert not hid[b, T:].any() and not frames[b, T:].any()
        xa = cuda(wav)
        assert np.array_equal(m.hidden_states(xa).cpu().numpy(), hid[b, :T]), f"row {b} hidden differs from the row alone"
        assert np.array_equal(m.frame_scores(xa).cpu().numpy(), frames[b, :T]), f"row {b} frame scores differ from the row alone"
        assert float(m.forward(xa)) == float(score[b]), f"row {b} score differs from the row alone"


def test_per_row_ids():
    """Two rows with the same wav and different (domain, judge): they differ, each meets the restatement, and an int for every row
    is bitwise the per-row form."""
    m = model("TINY")
    ids = [(0, 288), (2, 17)]
    wav = R.synth_wav(5200, 77)
    x = cuda(np.stack([wav, wav]))
    frames = m.frame_scores(x, None, [d for d, _ in ids], [j for _, j in ids]).cpu().numpy()
    score = m.forward(x, None, [d for d, _ in ids], [j for _, j in ids]).cpu().numpy()
    assert np.abs(frames[0] - frames[1]).max() > 1e-3 and abs(score[0] - score[1]) > 1e-4
    for b, (d, j) in enumerate(ids):
        _, ref, yard = case("TINY", 5200, 77, d, j)
        check(f"ids ({d}, {j}) frame scores", frames[b], ref[2], yard[2])
        check(f"ids ({d}, {j}) score", score[b: b + 1], np.array([ref[3]]), np.array([yard[3]]))
        assert np.array_equal(m.frame_scores(x, None, d, j).cpu().numpy()[b], frames[b])
        assert float(m.forward(x, None, d, j)[b]) == float(score[b])


def test_dc_offset_through_the_group_norm():
    """0.3 + a signal of amplitude 0.01: the group norm's 6415 frames per channel sit on a constant 30 times their deviation."""
    wav, ref, yard = reference("TINY", R.dc_wav(32080, 9))
    m = model("TINY")
    x = cuda(wav)
    check_all("TINY DC offset", m.hidden_states(x).cpu().numpy(), m.frame_scores(x).cpu().numpy(), float(m.forward(x)), ref, yard)


def test_refusals():
    from dex_tts_amd import mos
    m = model("TINY")
    with pytest.raises(ValueError, match="too short"):
        m.forward(torch.zeros(399, device="cuda"))
    with pytest.raises(ValueError, match="too short"):
        m.frame_scores(torch.zeros(2, 5200, device="cuda"), [5200, 399])
    with pytest.raises(ValueError, match="domain"):
        m.forward(torch.zeros(5200, device="cuda"), None, 3, 0)
    with pytest.raises(ValueError, match="judge"):
        m.forward(torch.zeros(2, 5200, device="cuda"), None, 0, [0, 3000])
    with pytest.raises(ValueError, match="judge"):
        m.bilstm(torch.zeros(4, 128, device="cuda"), None, 0, -1)
    fresh = mos.UTMOS(R.library_config(R.TINY), "cuda")
    with pytest.raises(ValueError, match="not loaded"):
        fresh.forward(torch.zeros(5200, device="cuda"))
    with pytest.raises(NotImplementedError, match="do_stable_layer_norm"):
        mos.UTMOS(R.library_config(R.variant(R.TINY, do_stable_layer_norm=True)), "cuda")
    with pytest.raises(NotImplementedError, match="lstm_hidden"):
        mos.UTMOS(R.library_config(R.variant(R.TINY, lstm_hidden=96)), "cuda")
    sd = {k: torch.from_numpy(v) for k, v in weights("TINY").items()}
    del sd["decoder_rnn.weight_hh_l0_reverse"]
    with pytest.raises(RuntimeError, match="decoder_rnn.weight_hh_l0_reverse"):
        fresh.load_state_dict(sd)
    # the C ABI refuses an id out of range on its own, before anything is enqueued
    import ctypes as C
    ctx, lib = m._ctx, m._ctx.lib
    x = torch.zeros(1, 5200, device="cuda")
    out = torch.full((1,), 7.0, device="cuda")
    ws = ctx.workspace(1, 5200)
    i32 = lambda v: np.asarray(v, np.int32).ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dex_mos_score(ctx.h, x.data_ptr(), i32([5200]), i32([0]), i32([3000]), 1, 5200, 0, out.data_ptr(), ws.data_ptr(), ws.numel(), st) == -1
    assert b"judge" in lib.dex_mos_last_error(ctx.h)
    assert lib.dex_mos_score(ctx.h, x.data_ptr(), i32([399]), i32([0]), i32([0]), 1, 5200, 0, out.data_ptr(), ws.data_ptr(), ws.numel(), st) == -1
    assert lib.dex_mos_workspace_bytes(ctx.h, 1, 399) == 0 and lib.dex_mos_workspace_bytes(ctx.h, 1, 16000 * 90) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_synthesize_mos_scores():
    """Two short int16 waveforms at 22050 Hz: ``synthesize.mos_scores`` is ``mos_score`` of the same data resampled by
    ``wavprep.resample``, and each row meets the restatement of what the resampler made of it."""
    from dex_tts_amd import mos, synthesize, wavprep
    m = model("TINY")
    audio = [np.round(R.synth_wav(n, 90 + i) * 32767.0).astype(np.int16) for i, n in enumerate((9000, 14000))]
    got, mean, err = synthesize.mos_scores(m, audio, sr=22050)
    got = got.cpu().numpy()
    assert got.shape == (2,) and (mean, err) == mos.mean_stderr(got)
    x = np.zeros((2, 14000), np.float32)
    for b, a in enumerate(audio):
        x[b, : len(a)] = a.astype(np.float32) / 32768.0
    y, ln = wavprep.resample(cuda(x), 22050, 16000, lengths=np.array([9000, 14000], np.int32))
    y = y.to(torch.float32)
    assert mos.mos_score(y, ln, source_sr=16000, model=m) == (mean, err)
    for b in range(2):
        wav = y[b, : int(ln[b])].cpu().numpy()
        _, ref, yard = reference("TINY", wav)
        check(f"mos_scores row {b}", got[b: b + 1], np.array([ref[3]]), np.array([yard[3]]))
