"""Windowed vocoding on the GPU (dex_vocode_window through ``Generator.forward(x, lengths, chunk_frames=N)`` and ``Generator.stream``):
a window of frames with ``halo_frames`` of context on each side reproduces the whole call's samples for that window, in fp32 bit for bit.

Geometries, weights, mel recipe and oracle bounds are those of tests/test_gpu_vocoder_ragged.py.  Cases:
(a) B = 2, T = 96 (208 for snakebeta_242, whose halo is 67 frames), lengths [T, 41], 16-frame windows: a first window on the true left
    edge, interior windows, a last one on the true right edge; the short utterance ends inside window 2, within the halo of its
    neighbours, and is pure silence for the later ones;
(b) B = 1, T = 37, 5-frame windows: odd sizes, a last window of 2 frames;
(c) both with ``chunk_frames >= T``: one window, no halo."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dex_tts_amd import synth, vocoder as V
from tests.test_bigvgan_22khz import mel_input, oracle
from tests.test_gpu_vocoder_ragged import GEOM, LOWP, gen_of, hop_of, weights_of

pytestmark = pytest.mark.gpu

DEX_ERR_ARG = -1


def case(name, key):
    """(B, T, lengths, chunk_frames)"""
    if key == "a":
        T = 208 if name == "snakebeta_242" else 96
        return 2, T, (T, 41), 16
    return 1, 37, (37,), 5


CHUNKED = [(g, k, big) for g in GEOM for k in "ab" for big in (False, True)]          # big: case (c), chunk_frames >= T


@functools.lru_cache(maxsize=None)
def mel_of(name, key):
    B, T, lengths, _ = case(name, key)
    mel = mel_input("window_mel", B, T, 93)
    for b, n in enumerate(lengths):
        mel[b, :, n:] = 0.0
    mel.setflags(write=False)
    return mel


def fp32_gen(name):
    gen = gen_of(name)
    gen.precision = "fp32"
    return gen


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def whole(name, key, ragged):
    """The whole call's result (dex_vocode_ragged with the lengths, dex_vocode without).  Computed once, shared, read-only."""
    lengths = case(name, key)[2]
    gen = fp32_gen(name)
    out = (gen(dev(mel_of(name, key)), list(lengths)) if ragged else gen(dev(mel_of(name, key)))).cpu().numpy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def alone_oracle(name, key, b):
    n = case(name, key)[2][b]
    ref = oracle(weights_of(name), GEOM[name][0], np.array(mel_of(name, key)[b:b + 1, :, :n]))[0, 0]
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("name,key,big", CHUNKED)
def test_chunked_forward_is_bitwise_the_whole_call(name, key, big):
    """fp32: fixed K order, ksplit = 1, no atomics - a window's interior runs the whole call's operations on the whole call's values."""
    B, T, lengths, N = case(name, key)
    N = T + 7 if big else N
    gen = fp32_gen(name)
    x = dev(mel_of(name, key))
    got = gen(x, list(lengths), chunk_frames=N).cpu().numpy()
    assert got.shape == (B, 1, T * hop_of(name)) and np.isfinite(got).all()
    assert np.array_equal(got, whole(name, key, True)), float(np.abs(got - whole(name, key, True)).max())
    got = gen(x, None, chunk_frames=N).cpu().numpy()
    assert np.array_equal(got, whole(name, key, False)), float(np.abs(got - whole(name, key, False)).max())
    for b, n in enumerate(lengths):
        assert not whole(name, key, True)[b, 0, n * hop_of(name):].any()


@pytest.mark.parametrize("name,key,big", CHUNKED)
def test_stream_yields_the_windows_in_order(name, key, big):
    B, T, lengths, N = case(name, key)
    N = T + 7 if big else N
    hop = hop_of(name)
    gen = fp32_gen(name)
    seen, chunks = [], []
    for t0, chunk, ev in gen.stream(dev(mel_of(name, key)), list(lengths), chunk_frames=N):
        assert isinstance(ev, torch.cuda.Event)
        ev.synchronize()                                           # the chunk is complete behind its event
        chunks.append(chunk.cpu().numpy())
        seen.append((t0, chunk.shape))
    want = [(t0, (B, 1, min(N, T - t0) * hop)) for t0 in range(0, T, N)]
    assert [(t, tuple(s)) for t, s in seen] == want
    if not big and key == "b":
        assert want[-1][1][2] == 2 * hop                           # the short last window
    assert np.array_equal(np.concatenate(chunks, axis=2), whole(name, key, True))


@pytest.mark.parametrize("name,key", [(g, k) for g in GEOM for k in "ab"])
def test_chunked_stays_within_the_oracle_bounds(name, key):
    from tests import gpu_util as U
    B, T, lengths, N = case(name, key)
    hop, bound = hop_of(name), GEOM[name][1]
    got = fp32_gen(name)(dev(mel_of(name, key)), list(lengths), chunk_frames=N).cpu().numpy()
    errs = []
    for b, n in enumerate(lengths):
        e = np.abs(got[b, 0, :n * hop] - alone_oracle(name, key, b))
        U.record(f"voc_window_{name}_T{T}_n{n}:fp32:call", max=e.max(), mean=e.mean())
        print(f"{name} T={T} n={n} chunk={N}: max|d| = {e.max():.3e}")
        errs.append(float(e.max()))
    assert max(errs) <= bound, errs


def window_call(gen, mel, ln, B, T, t0, n, out, bstride, ws_bytes=None):
    """dex_vocode_window itself, on the current stream; the workspace is the one (B = mel's, n) asks for unless ``ws_bytes`` is given."""
    lib, ctx = gen._lib, gen._ctx
    need = int(lib.dex_voc_window_workspace_bytes(ctx, mel.shape[0], max(n, 1)))
    base, nbytes = gen._workspace(need, mel.device)
    return lib.dex_vocode_window(ctx, C.c_void_p(mel.data_ptr()), C.c_void_p(ln.data_ptr()) if ln is not None else None, B, T, t0, n,
                                 C.c_void_p(out.data_ptr()), bstride, C.c_void_p(base), nbytes if ws_bytes is None else ws_bytes,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("name", list(GEOM))
def test_a_window_reads_nothing_outside_its_halo(name):
    """An interior window of case (a): NaN in every frame outside [t0 - H, t0 + n + H) and past every length does not reach the result."""
    B, T, lengths, n = case(name, "a")
    hop = hop_of(name)
    gen = fp32_gen(name)
    ref = whole(name, "a", True)                                   # (also brings the engine up)
    H = gen.halo_frames
    t0 = 80 if name == "snakebeta_242" else 32
    assert t0 - H > 0 and t0 + n + H < T                           # both edges of the window are artificial
    mel = np.array(mel_of(name, "a"))
    mel[:, :, :t0 - H] = np.nan
    mel[:, :, t0 + n + H:] = np.nan
    for b, m in enumerate(lengths):
        mel[b, :, m:] = np.nan
    x, ln = dev(mel), torch.tensor(lengths, dtype=torch.int32).cuda()
    out = torch.full((B, n * hop), 7.0, dtype=torch.float32).cuda()
    assert window_call(gen, x, ln, B, T, t0, n, out, n * hop) == 0, gen._lib.dex_voc_last_error(gen._ctx)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got, ref[:, 0, t0 * hop:(t0 + n) * hop])
    if name != "snakebeta_242":
        assert got[1, :(41 - t0) * hop].any() and not got[1, (41 - t0) * hop:].any()      # the short utterance ends inside this window


def test_bad_arguments_are_refused_before_anything_runs():
    name = "hifigan_v1"
    B, T, lengths, n = case(name, "a")
    hop = hop_of(name)
    gen = fp32_gen(name)
    whole(name, "a", True)
    x, ln = dev(mel_of(name, "a")), torch.tensor(lengths, dtype=torch.int32).cuda()
    out = torch.full((B, T * hop), 7.0, dtype=torch.float32).cuda()
    need = int(gen._lib.dex_voc_window_workspace_bytes(gen._ctx, B, n))
    bad = {"t0 < 0": dict(t0=-1, n=n), "n_frames < 1": dict(t0=0, n=0), "negative n_frames": dict(t0=8, n=-4),
           "t0 + n_frames > T": dict(t0=T - n + 1, n=n), "t0 past T": dict(t0=T, n=1), "B < 1": dict(t0=0, n=n, B=0),
           "workspace too small": dict(t0=0, n=n, ws_bytes=need - 256), "no workspace": dict(t0=0, n=n, ws_bytes=0)}
    for what, a in bad.items():
        rc = window_call(gen, x, ln, a.get("B", B), T, a["t0"], a["n"], out, T * hop, a.get("ws_bytes"))
        assert rc == DEX_ERR_ARG, (what, rc)
        assert gen._lib.dex_voc_last_error(gen._ctx), what
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                # nothing was enqueued
    assert window_call(gen, x, ln, B, T, 0, n, out, T * hop) == 0  # the same buffers are fine
    assert np.array_equal(out.cpu().numpy()[:, :n * hop], whole(name, "a", True)[:, 0, :n * hop]) and bool((out[:, n * hop:] == 7.0).all())


@pytest.mark.parametrize("name,prec,bounds", LOWP, ids=[f"{n}-{p}" for n, p, _ in LOWP])
def test_chunked_reduced_precision(name, prec, bounds):
    """bf16 / fp16 operands: case (a) chunked against the fp32 oracle alone, at the bounds of the ragged tests; bitwise repeatable.  (Not
    bitwise against the whole call: the reduced-precision GEMM chooses its tile form by problem size.)"""
    from tests import gpu_util as U
    B, T, lengths, N = case(name, "a")
    hop = hop_of(name)
    gen = gen_of(name)
    gen.precision = prec
    try:
        out = gen(dev(mel_of(name, "a")), list(lengths), chunk_frames=N).cpu().numpy()
        again = gen(dev(mel_of(name, "a")), list(lengths), chunk_frames=N).cpu().numpy()
    finally:
        gen.precision = "fp32"
    assert np.isfinite(out).all() and np.array_equal(out, again)
    bad = []
    for b, n in enumerate(lengths):
        assert not out[b, 0, n * hop:].any()
        e = out[b, 0, :n * hop] - alone_oracle(name, "a", b)
        mx, rms = float(np.abs(e).max()), float(np.sqrt((e * e).mean()))
        U.record(f"voc_window_{name}_T{T}_n{n}:{prec}:call", max=mx, mean=rms)
        print(f"{name} {prec} n={n}: max|d| = {mx:.3e}  rms = {rms:.3e}")
        if mx > bounds[0] or rms > bounds[1]:
            bad.append((n, mx, rms))
    assert not bad, bad
    assert not np.array_equal(out, whole(name, "a", True))


def test_synthesize_tokens_chunked():
    """The two-utterance case of test_synthesize_tokens_exact_lengths: ``chunk_frames=8`` returns the same int16 waveforms."""
    from dex_tts_amd import synthesize as SY, tts
    from tests.test_tts_module import full_state_dict, model_cfg
    m = tts.GeDEXTTS(model_cfg("gedex_lj"))
    m.load_state_dict(full_state_dict(m, "gedex_lj"))
    m = m.cuda().eval()
    voc = V.Generator()
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_vocoder_weights(V.param_shapes(V.HIFIGAN_V1)).items()})
    voc = voc.cuda().eval()
    tok, lengths = synth.make_text_inputs(2, 21, [21, 12], 149)
    args = (m, voc, torch.from_numpy(tok).cuda(), torch.from_numpy(lengths).cuda())
    SY.seed_init(100)
    audio, y_dec, _ = SY.synthesize_tokens(*args, n_timesteps=4, exact_lengths=True)
    SY.seed_init(100)
    chunked, y_dec2, _ = SY.synthesize_tokens(*args, n_timesteps=4, exact_lengths=True, chunk_frames=8)
    assert torch.equal(y_dec, y_dec2) and y_dec.shape[-1] > 8      # more than one window
    assert len(audio) == len(chunked) == 2
    for a, c in zip(audio, chunked):
        assert a.dtype == c.dtype == np.int16 and len(a) > 0 and np.array_equal(a, c)
    SY.seed_init(100)
    plain, _, _ = SY.synthesize_tokens(*args, n_timesteps=4)
    SY.seed_init(100)
    plain_chunked, _, _ = SY.synthesize_tokens(*args, n_timesteps=4, chunk_frames=8)
    for a, c in zip(plain, plain_chunked):
        assert np.array_equal(a, c)
