"""GPU: the Griffin-Lim mel inversion (dex_tts_amd.griffin_lim, csrc/griffin_lim.hip) against the reference's goldens
(tests/golden/griffin_lim.npz, written by tools/make_golden_griffin_lim.py from the reference's own STFT / griffin_lim) and the
float64 restatement (tests/griffin_lim.py); ragged batches, reproducibility, the wav writers and the C ABI's refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from dex_tts_amd import _lib
from dex_tts_amd import griffin_lim as G
from tests import griffin_lim as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "griffin_lim.npz")))


@pytest.fixture(scope="module")
def mels():
    d = np.load(os.path.join(GOLD, "audio_mel.npz"))
    return {"s1": d["sample1_1s_mel"], "chirp": d["chirp_mel"]}


def _record(**kw):
    """measured maxima, for DESIGN.md (GL_RECORD=<path> appends one JSON line per test)"""
    path = os.environ.get("GL_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({k: float(v) for k, v in kw.items()}) + "\n")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def test_transform_matches_reference(gold):
    mag, phase = G.STFT(1024, 256, 1024).transform(_cuda(gold["wav"])[None])
    mag, phase = mag[0].cpu().numpy(), phase[0].cpu().numpy()
    rm, rp = gold["wav_mag"], gold["wav_phase"]
    assert mag.shape == rm.shape
    peak = rm.max(axis=0, keepdims=True)
    em = (np.abs(mag - rm) / peak).max()
    live = rm > 1e-3 * peak
    ep = np.abs(np.angle(np.exp(1j * (phase.astype(np.float64) - rp))))[live].max()
    _record(transform_mag_rel=em, transform_phase=ep)
    assert em <= 2e-6            # measured 6.7e-7
    assert ep <= 1.5e-4          # measured 4.4e-5 rad


def test_round_trip_reconstructs(gold):
    wav = gold["wav"]
    out = G.STFT().forward(_cuda(wav)[None])[0, 0].cpu().numpy()
    n = 256 * (wav.size // 256)
    assert out.shape == (n,)
    e = np.abs(out - wav[:n]).max()
    _record(round_trip=e, round_trip_vs_ref=np.abs(out - gold["wav_inv"]).max())
    assert e <= 4e-7             # measured 1.2e-7 (the reference's own round trip: 3e-7)


def test_mel_to_linear_matches_reference(gold, mels):
    for name in ("s1", "chirp"):
        got = G.mel_to_linear(_cuda(mels[name])[None])[0].cpu().numpy()
        ref = gold[f"spec_{name}"][:, :-1]
        e = np.abs(got - ref).max() / np.abs(ref).max()
        _record(spec_from_mel_rel=e)
        assert e <= 1e-7         # measured 3.6e-8


@pytest.mark.parametrize("name,n,tol", [("s1", 0, 1e-6), ("chirp", 0, 3.5e-6), ("s1", 1, 3e-6), ("s1", 60, 2.5e-5)])
def test_griffin_lim_matches_reference(gold, name, n, tol):
    """bounds about 3x the measured maxima: 2.8e-7, 1.1e-6, 9.5e-7 and 7.1e-6 for 0 / 0 / 1 / 60 iterations"""
    S = gold[f"spec_{name}"][:, :-1]
    x = G.griffin_lim(_cuda(S)[None], G.STFT(), n, angles=_cuda(gold[f"angles_{name}"])[None])[0].cpu().numpy()
    ref = gold[f"gl{n}_{name}"]
    assert x.shape == ref.shape
    e = np.abs(x - ref).max()
    rec = {f"gl{n}_{name}": e}
    if n == 60:
        sc = R.spectral_convergence(S, x.astype(np.float64))
        rec["sc60"], rec["sc60_ref"] = sc, float(gold["sc60_s1"])
        assert abs(sc - float(gold["sc60_s1"])) <= 0.01 * float(gold["sc60_s1"])
    _record(**rec)
    assert e <= tol


def test_seeded_draw_is_the_references(gold):
    S = _cuda(gold["spec_s1"][:, :-1])[None]
    np.random.seed(int(gold["seed"]))
    x = G.griffin_lim(S, G.STFT(), 0)
    y = G.griffin_lim(S, G.STFT(), 0, angles=_cuda(gold["angles_s1"])[None])
    assert torch.equal(x, y)


def test_ragged_batch_rows_equal_rows_alone(mels):
    rows = [mels["s1"], mels["chirp"], mels["s1"][:, 20:60]]
    T = max(m.shape[1] for m in rows)
    batch = np.zeros((3, 80, T), np.float32)
    for b, m in enumerate(rows):
        batch[b, :, : m.shape[1]] = m
    lengths = [m.shape[1] for m in rows]
    np.random.seed(7)
    out = G.mel_to_wav(_cuda(batch), lengths, n_iters=8)
    assert out.shape == (3, 256 * (T - 2)) and out.dtype == torch.float32
    np.random.seed(7)                                             # consecutive single calls draw what the batch drew, row by row
    for b, m in enumerate(rows):
        alone = G.mel_to_wav(_cuda(m)[None], n_iters=8)[0]
        L = 256 * (m.shape[1] - 2)
        assert alone.shape == (L,)
        assert torch.equal(out[b, :L], alone), b
        assert not out[b, L:].any(), b
        assert torch.isfinite(alone).all()


def test_identical_calls_bitwise(mels):
    m = _cuda(mels["chirp"])[None]
    a = np.random.RandomState(3).rand(1, 513, m.shape[2] - 1)
    ang = _cuda(np.angle(np.exp(2j * np.pi * a)))
    x = G.mel_to_wav(m, n_iters=30, angles=ang)
    y = G.mel_to_wav(m, n_iters=30, angles=ang)
    assert torch.equal(x, y)


def test_inv_mel_spec_writes_mel_to_wav(tmp_path, mels):
    from scipy.io.wavfile import read
    from dex_tts_amd.audio import TacotronSTFT
    stft = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    assert stft._stft_fn is stft.stft_fn and isinstance(stft.stft_fn, G.STFT)
    m = _cuda(mels["chirp"])
    path = str(tmp_path / "gl.wav")
    np.random.seed(11)
    G.inv_mel_spec(m, path, stft, griffin_iters=5)
    np.random.seed(11)
    want = G.mel_to_wav(m[None], n_iters=5)[0].cpu().numpy()
    sr, got = read(path)
    assert sr == 22050 and got.dtype == np.float32
    np.testing.assert_array_equal(got, want)


def test_synthesize_wav_flag(tmp_path):
    import yaml
    from dex_tts_amd import synthesize as S
    sections = json.load(open(os.path.join(GOLD, "ref_model_sections.json")))
    cfg = tmp_path / "base.yaml"
    cfg.write_text(yaml.safe_dump({"model": sections["GeDEX-TTS/config/LJSpeech/base.yaml"]}))
    mu = np.random.RandomState(0).randn(1, 80, 40).astype(np.float32) * 0.5
    np.save(tmp_path / "mu.npy", mu)
    wav = tmp_path / "out.wav"
    S.main(["--config", str(cfg), "--mu", str(tmp_path / "mu.npy"), "--lengths", "36", "--n_timesteps", "2", "--out",
            str(tmp_path / "mel.npy"), "--wav", str(wav), "--griffin_iters", "3"])
    from scipy.io.wavfile import read
    sr, x = read(str(wav))
    assert sr == 22050 and x.shape == (256 * (36 - 2),)


def test_cabi_refusals_with_messages():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.dex_gl_create(C.byref(h)) == 0
    try:
        buf = torch.zeros(4 << 20, dtype=torch.uint8, device=DEV)
        p = buf.data_ptr()
        fr = lambda *v: (C.c_int32 * len(v))(*v)                      # noqa: E731
        ws = lib.dex_gl_workspace_bytes(2, 8)
        assert lib.dex_griffin_lim(h, p, p, fr(3, 3), 2, 3, 1, p, p, ws, None) == -1
        assert b"4 frames" in lib.dex_gl_last_error(h)
        assert lib.dex_griffin_lim(h, p, p, fr(8, 8), 2, 8, -1, p, p, ws, None) == -1
        assert b"n_iters" in lib.dex_gl_last_error(h)
        assert lib.dex_griffin_lim(h, p, p, fr(8, 9), 2, 8, 1, p, p, ws, None) == -1
        assert b"max_frames" in lib.dex_gl_last_error(h)
        assert lib.dex_griffin_lim(h, p, p, fr(8, 8), 2, 8, 1, p, p, ws - 1, None) == -4
        assert lib.dex_stft_transform(h, p, fr(3000), 1, 2048, p, p, None) == -1
        assert lib.dex_stft_transform(h, p, fr(400), 1, 2048, p, p, None) == -1
        assert lib.dex_stft_inverse(h, p, p, fr(9), 1, 8, p, p, ws, None) == -1
        assert lib.dex_mel_to_linear(h, p, fr(30), 1, 20, p, None) == -1
        torch.cuda.synchronize()
    finally:
        lib.dex_gl_destroy(h)
