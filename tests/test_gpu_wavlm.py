"""GPU: the WavLM x-vector path of dex_tts_amd/wavlm.py (csrc/wavlm.hip) against its float64 restatement (tests/wavlm_ref.py, itself
held to transformers' model by tests/test_wavlm_cpu.py).  Tolerances are not constants: each case measures, on its own inputs, how
far the torch fp32 CPU evaluation of the same graph lies from the float64 restatement, and allows the device ``NET_FACTOR`` = 8 times
that distance, floored at 1e-6 of the largest magnitude (wavlm_ref.tolerance).  Every case prints the device error, the yardstick and
the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import wavlm_ref as R

pytestmark = pytest.mark.gpu

CFG = {"TINY": R.TINY, "WIDE": R.WIDE, "TINY_LAST": R.variant(R.TINY, use_weighted_layer_sum=False),
       "TINY_BIAS": R.variant(R.TINY, conv_bias=True)}
RAGGED = [32080, 5200, 20880]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SD, _MODEL, _CASE = {}, {}, {}


def weights(name):
    if name not in _SD:
        _SD[name] = R.make_weights(CFG[name], 0)
    return _SD[name]


def model(name, do_normalize=False):
    key = (name, do_normalize)
    if key not in _MODEL:
        from dex_tts_amd import wavlm
        m = wavlm.WavLMXVector(R.library_config(CFG[name]), "cuda", do_normalize=do_normalize)
        _MODEL[key] = m.load_state_dict({k: torch.from_numpy(v) for k, v in weights(name).items()})
    return _MODEL[key]


def reference(name, wav, do_normalize=False):
    """(wav, float64 (hidden, embeddings), fp32 CPU yardstick (hidden, embeddings)) of one utterance."""
    return (wav, R.forward(CFG[name], weights(name), wav, do_normalize), R.torch_forward_fp32(CFG[name], weights(name), wav, do_normalize))


def case(name, n, seed):
    """``reference`` of ``synth_wav(n, seed)``: computed once and shared, never changed."""
    key = (name, n, seed)
    if key not in _CASE:
        _CASE[key] = reference(name, R.synth_wav(n, seed))
    return _CASE[key]


def ragged(name):
    """The batch [32080, 5200, 20880] with garbage past each length, and its rows' cases."""
    cases = [case(name, L, 20 + b) for b, L in enumerate(RAGGED)]
    x = (10.0 * np.random.default_rng(3).standard_normal((len(RAGGED), max(RAGGED)))).astype(np.float32)
    for b, L in enumerate(RAGGED):
        x[b, :L] = cases[b][0]
    return x, cases


def check(what, got, ref, yard):
    tol, d = R.tolerance(yard, ref)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: device err {err:.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}, magnitude {np.abs(ref).max():.2f}")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert err <= tol, (what, err, tol)


def check_both(what, hid, emb, ref, yard):
    check(what + " hidden", hid, ref[0], yard[0])
    check(what + " embeddings", emb, ref[1], yard[1])


@pytest.mark.parametrize("n", [5200, 5520, 20880, 32080])
def test_single_rows_tiny(n):
    """5200 samples are 16 frames, the minimum: two frames reach statistics pooling.  32080 are 100: distances past
    max_bucket_distance = 40 take the clamped far bucket on both signs."""
    wav, ref, yard = case("TINY", n, n)
    m = model("TINY")
    hid, emb = m.hidden_states(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy()
    assert hid.shape == (R.num_frames(R.TINY, n), 128) and emb.shape == (32,)
    check_both(f"TINY n={n}", hid, emb, ref, yard)


def test_dc_offset_through_the_group_norm():
    """0.3 + a signal of amplitude 0.01: the group norm's 6415 frames per channel sit on a constant 30 times their deviation.  Its
    statistics are two-pass in fp64; E[x^2] - E[x]^2 in fp32 would cancel three of its seven digits here (mean^2 / var = 900)."""
    wav, ref, yard = reference("TINY", R.dc_wav(32080, 9))
    m = model("TINY")
    check_both("TINY DC offset", m.hidden_states(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy(), ref, yard)


@pytest.mark.parametrize("name", ["TINY", "WIDE"])
def test_ragged_batch_rows_are_the_rows_alone(name):
    """[32080, 5200, 20880] with garbage past each length: every row meets the restatement, is BITWISE the row alone (the group
    norm, the attention keys and the pooled statistics end at the row's own frames; every launch fixes its summation order from
    the config), its hidden states are 0 past its frames, and its embeddings are finite - dead ReLU channels included, whose
    deviation is exactly 0.  WIDE runs the default widths: 48-channel positional groups, 12 heads, a 1500-channel TDNN layer."""
    m = model(name)
    x, cases = ragged(name)
    hid = m.hidden_states(cuda(x), RAGGED).cpu().numpy()
    emb = m.forward(cuda(x), RAGGED).cpu().numpy()
    H = CFG[name].hidden_size
    assert hid.shape == (3, 100, H) and emb.shape == (3, CFG[name].xvector_output_dim) and np.isfinite(emb).all()
    for b, L in enumerate(RAGGED):
        T = R.num_frames(CFG[name], L)
        wav, ref, yard = cases[b]
        check_both(f"ragged {name} row {b}", hid[b, :T], emb[b], ref, yard)
        assert not hid[b, T:].any()
        alone_h, alone_e = m.hidden_states(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy()
        assert np.array_equal(alone_h, hid[b, :T]), f"row {b} hidden differs from the row alone by {np.abs(alone_h - hid[b, :T]).max():.3e}"
        assert np.array_equal(alone_e, emb[b]), f"row {b} embeddings differ from the row alone by {np.abs(alone_e - emb[b]).max():.3e}"


def test_wide_batch_of_16_takes_the_other_gemm_tile():
    """launch_igemm picks its 128 x 64 tile once a launch has 512 of them: at 16 utterances the strided convolutions (3207 frames,
    N = 512: 26 x 8 x 16 tiles) do, where the single rows run the 64 x 64 form.  Both walk K in the same order: the rows stay
    bitwise the rows alone."""
    m = model("WIDE")
    x3, cases = ragged("WIDE")
    x = np.concatenate([x3] * 6)[:16]
    lens = (RAGGED * 6)[:16]
    hid = m.hidden_states(cuda(x), lens).cpu().numpy()
    emb = m.forward(cuda(x), lens).cpu().numpy()
    for b in (0, 1, 2, 15):
        wav, ref, yard = cases[b % 3]
        T = ref[0].shape[0]
        check_both(f"WIDE B=16 row {b}", hid[b, :T], emb[b], ref, yard)
        assert np.array_equal(m.hidden_states(cuda(wav)).cpu().numpy(), hid[b, :T])
        assert np.array_equal(m.forward(cuda(wav)).cpu().numpy(), emb[b])


@pytest.mark.parametrize("name,norm", [("TINY_LAST", False), ("TINY_BIAS", False), ("TINY", True)])
def test_tiny_variants(name, norm):
    """use_weighted_layer_sum = False (the last hidden state), conv_bias = True, and do_normalize = True on a wav with a DC offset."""
    wav, ref, yard = reference(name, R.dc_wav(20880, 11, dc=0.05, amp=0.1) if norm else R.synth_wav(20880, 12), norm)
    m = model(name, norm)
    check_both(f"{name} do_normalize={norm}", m.hidden_states(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy(), ref, yard)


def cos_bound(what, got, embs_ref, embs_yard):
    """A pair's cosine against the restatement's, by the same x 8 fp32-yardstick rule (floor: 1e-6 of the largest cosine, 1)."""
    ref = R.cosine(*embs_ref)
    d = abs(R.cosine(*embs_yard) - ref)
    tol = max(R.NET_FACTOR * d, R.NET_FLOOR)
    print(f"{what}: device cos {got:.7f}, restatement {ref:.7f}, err {abs(got - ref):.3e}, cpu fp32 yardstick {d:.3e}, bound {tol:.3e}")
    assert abs(got - ref) <= tol, (what, got, ref, tol)


def test_similarity_and_sim_scores():
    """Three pairs; the third is at 22050 Hz, so the resampler is in the path: the restatement reads what wavprep.resample made of it."""
    from dex_tts_amd import synthesize, wavlm
    from dex_tts_amd._native import resample_to_16k
    m = model("TINY")
    syn = [R.synth_wav(20880, 50), R.synth_wav(12000, 51), R.synth_wav(30000, 52)]
    trg = [R.synth_wav(16000, 60), R.synth_wav(20880, 61), R.synth_wav(26000, 62)]

    def refs(wav):
        _, ref, yard = reference("TINY", wav)
        return ref[1], yard[1]

    def padded(wavs):
        x = np.zeros((len(wavs), max(len(w) for w in wavs)), np.float32)
        for b, w in enumerate(wavs):
            x[b, : len(w)] = w
        return cuda(x), [len(w) for w in wavs]

    s, sl = padded(syn[:2])
    t, tl = padded(trg[:2])
    cos = wavlm.similarity(s, t, sl, tl, source_sr=16000, model=m).cpu().numpy()
    assert cos.shape == (2,)
    for b in range(2):
        (es, ys), (et, yt) = refs(syn[b]), refs(trg[b])
        cos_bound(f"similarity pair {b} (16 kHz)", float(cos[b]), (es, et), (ys, yt))
    # the 22050 Hz pair: both sides resampled on the device
    cos3 = float(wavlm.similarity(cuda(syn[2]), cuda(trg[2]), source_sr=22050, model=m).cpu().numpy()[0])
    down = []
    for w in (syn[2], trg[2]):
        y, ln = resample_to_16k(cuda(w)[None], np.array([len(w)], np.int32), 22050)
        down.append(y[0, : int(ln[0])].cpu().numpy())
    assert abs(len(down[0]) - 30000 * 16000 / 22050) <= 1 and abs(len(down[1]) - 26000 * 16000 / 22050) <= 1
    (es, ys), (et, yt) = refs(down[0]), refs(down[1])
    cos_bound("similarity pair 2 (22050 Hz)", cos3, (es, et), (ys, yt))
    mean, err = wavlm.sim_score(s, t, sl, tl, source_sr=16000, model=m)
    assert abs(mean - float(np.mean(cos.astype(np.float64)))) < 1e-12 and abs(err - float(np.std(cos.astype(np.float64)) / np.sqrt(2))) < 1e-12
    # identical inputs
    same = float(wavlm.similarity(cuda(syn[0]), cuda(syn[0]), source_sr=16000, model=m).cpu().numpy()[0])
    e, y = refs(syn[0])
    cos_bound("similarity of a wav with itself", same, (e, e), (y, y))
    # synthesize.sim_scores: int16 audio at 16 kHz against float references at 22050 Hz
    audio = [np.round(w * 32767.0).astype(np.int16) for w in syn]
    cos, mean, err = synthesize.sim_scores(m, audio, trg, sr=16000, ref_sr=22050)
    cos = cos.cpu().numpy()
    assert cos.shape == (3,) and np.isfinite([mean, err]).all()
    assert (mean, err) == wavlm.mean_stderr(cos)
    for b in range(3):
        y, ln = resample_to_16k(cuda(trg[b])[None], np.array([len(trg[b])], np.int32), 22050)
        (es, ys), (et, yt) = refs(audio[b].astype(np.float32) / 32768.0), refs(y[0, : int(ln[0])].cpu().numpy())
        cos_bound(f"sim_scores pair {b}", float(cos[b]), (es, et), (ys, yt))


def test_refusals():
    """Refused before anything is enqueued: a CPU tensor, a short row, more frames than one call takes, weights that are not loaded -
    by the wrapper, and by the C ABI itself."""
    from dex_tts_amd import wavlm
    m = model("TINY")
    with pytest.raises(ValueError):
        m.forward(torch.zeros(32080))                             # a CPU tensor
    with pytest.raises(ValueError, match="too short"):
        m.forward(torch.zeros(5199, device="cuda"))
    with pytest.raises(ValueError, match="too short"):
        m.hidden_states(torch.zeros(2, 32080, device="cuda"), [32080, 4880])
    with pytest.raises(ValueError, match="at most"):
        m.forward(torch.zeros(16000 * 90, device="cuda"))         # 4499 frames > DEX_WAVLM_MAX_FRAMES
    fresh = wavlm.WavLMXVector(R.library_config(R.TINY), "cuda")
    with pytest.raises(ValueError, match="not loaded"):
        fresh.forward(torch.zeros(32080, device="cuda"))
    sd = {k: torch.from_numpy(v) for k, v in weights("TINY").items()}
    del sd["layer_weights"]
    fresh.load_state_dict(sd, strict=False)
    with pytest.raises(ValueError, match="layer_weights"):
        fresh.finalize()
    with pytest.raises(ValueError, match="not loaded"):
        fresh.forward(torch.zeros(32080, device="cuda"))
    # the C ABI refuses the same on its own: a short row, too many frames, a workspace that is too small, weights not finalized
    ctx, lib = m._ctx, m._ctx.lib
    x = torch.zeros(2, 32080, device="cuda")
    out = torch.full((2, 32), 7.0, device="cuda")
    ws = ctx.workspace(2, 32080)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def embed(handle, lens, n, nbytes):
        ln = np.asarray(lens, np.int32)
        return lib.dex_wavlm_embed(handle, x.data_ptr(), ln.ctypes.data_as(C.POINTER(C.c_int32)), len(lens), n, 0, out.data_ptr(), ws.data_ptr(), nbytes, st)

    assert embed(ctx.h, [32080, 4880], 32080, ws.numel()) == -1 and b"too short" in lib.dex_wavlm_last_error(ctx.h)
    assert embed(ctx.h, [32080, 32081], 32080, ws.numel()) == -1
    assert embed(ctx.h, [32080], 16000 * 90, ws.numel()) == -1 and b"at most" in lib.dex_wavlm_last_error(ctx.h)
    assert embed(ctx.h, [32080, 32080], 32080, 1024) != 0 and b"workspace" in lib.dex_wavlm_last_error(ctx.h)
    assert embed(fresh._ctx.h, [32080, 32080], 32080, ws.numel()) == -2
    assert lib.dex_wavlm_workspace_bytes(ctx.h, 1, 4880) == 0 and lib.dex_wavlm_workspace_bytes(ctx.h, 1, 16000 * 90) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                     # nothing was enqueued
    # HF's newer spelling of the weight norm, and the keys the embeddings never read
    sd = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): torch.from_numpy(v)
          for k, v in weights("TINY").items()}
    sd.update({"classifier.weight": torch.zeros(32, 32), "classifier.bias": torch.zeros(32), "objective.weight": torch.zeros(32, 2),
               "wavlm.masked_spec_embed": torch.zeros(128)})
    fresh.load_state_dict(sd)
    wav, _, _ = case("TINY", 5520, 5520)
    assert np.array_equal(fresh.forward(cuda(wav)).cpu().numpy(), m.forward(cuda(wav)).cpu().numpy())
