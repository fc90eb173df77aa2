"""BigVGAN 22 kHz / 80 bands, the 112 M model (vocoder.BIGVGAN_22KHZ), and the narrow-stage kernels it needs (vocoder_narrow.hip:
widths that are multiples of 8, at most 64, not multiples of 32).  CPU: the parameter inventory and the oracle against fixtures from the
real reference (tests/golden/bigvgan_22khz.npz, manifest_bigvgan_22khz.json, written by tools/make_golden_bigvgan_22khz.py), and the
library's refusal of widths nothing handles.  GPU (-m gpu): dex_vocode against the golden, the oracle, small configurations that
isolate the narrow path (BigVGAN and HiFi-GAN V2 geometry), the reduced-precision modes, and the whole synthesize_tokens flow."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from dex_tts_amd import _lib, synth, vocoder as V

GOLD = os.path.join(os.path.dirname(__file__), "golden")
N_PARAMS = 112_199_473


def bvg22_weights():
    """The golden's weights: synth.make_vocoder_weights with conv_post halved (tools/make_golden_bigvgan_22khz.py), the reference's filter."""
    g = np.load(os.path.join(GOLD, "bigvgan_22khz.npz"))
    w = synth.make_vocoder_weights(V.param_shapes(V.BIGVGAN_22KHZ))
    w["conv_post.weight"] = w["conv_post.weight"] * np.float32(0.5)
    for k in w:
        if k.endswith(".filter"):
            w[k] = g["filter"].copy()
    return w


def small_weights(h):
    w = synth.make_vocoder_weights(V.param_shapes(h))
    if h.get("activation"):
        g = np.load(os.path.join(GOLD, "bigvgan_22khz.npz"))
        for k in w:
            if k.endswith(".filter"):
                w[k] = g["filter"].copy()
    return w


def mel_input(key, B, T, seed):
    return np.clip(synth.normalish(key, (B, 80, T), seed) * 1.5 - 5.0, -11.5, 2.5).astype(np.float32)


def oracle(w, h, mel):
    from oracle import bigvgan_oracle as BO, vocoder_oracle as VO
    W = {k: torch.from_numpy(v) for k, v in w.items()}
    with torch.no_grad():
        return (BO if h.get("activation") else VO).generator(W, h, torch.from_numpy(mel)).numpy()


def gpu_gen(h, w):
    m = V.Generator(V.AttrDict(h))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m.cuda().eval()


# ------------------------------------------------------------------------------------------------------------------------------- CPU
def test_param_shapes_match_reference_state_dict():
    man = json.load(open(os.path.join(GOLD, "manifest_bigvgan_22khz.json")))
    assert man["config"] == V.BIGVGAN_22KHZ
    assert {k: tuple(v) for k, v in man["keys"].items()} == {k: tuple(v) for k, v in V.param_shapes(V.BIGVGAN_22KHZ).items()}
    assert len(man["keys"]) == 668


def test_parameter_count():
    n = sum(int(np.prod(s)) for k, s in V.param_shapes(V.BIGVGAN_22KHZ).items() if not k.endswith(".filter"))
    assert n == N_PARAMS


def test_oracle_matches_reference_golden(golden_threads):
    g = np.load(os.path.join(GOLD, "bigvgan_22khz.npz"))
    wav = oracle(bvg22_weights(), V.BIGVGAN_22KHZ, g["mel"])
    assert wav.shape == g["wav"].shape == (2, 1, 9 * 256)
    assert np.abs(wav - g["wav"]).max() <= 1e-6
    assert np.abs(g["wav"]).max() < 0.98 and g["wav"].std() > 0.05          # neither saturated nor silent


def _create(h):
    lib = _lib.load()
    c = V.make_config(h)
    ctx = C.c_void_p()
    rc = lib.dex_voc_create(C.byref(c), C.byref(ctx))
    msg = lib.dex_voc_last_error(ctx).decode()
    n = lib.dex_voc_num_weights(ctx)
    lib.dex_voc_destroy(ctx)
    return rc, msg, n


def test_library_accepts_narrow_widths_and_names_unhandled_stage():
    """dex_voc_create (host logic only): the 112 M model and HiFi-GAN V2's 16 / 8-channel tail are accepted; 640 initial channels with the
    six 112 M rates (320/160/80/40/20/10) are refused at the 80-channel stage, which neither the implicit GEMM nor the narrow kernels take."""
    rc, msg, n = _create(V.BIGVGAN_22KHZ)
    shapes = V.param_shapes(V.BIGVGAN_22KHZ)
    n_filt = sum(k.endswith(".filter") for k in shapes)
    assert rc == 0 and n == len(shapes) - n_filt + 2, (rc, msg, n)          # the library keeps one copy of the resampling filter pair
    rc, msg, _ = _create(dict(V.HIFIGAN_V1, upsample_initial_channel=128))
    assert rc == 0, msg
    rc, msg, _ = _create(dict(V.BIGVGAN_22KHZ, upsample_initial_channel=640))
    assert rc == -1                                         # DEX_ERR_ARG (include/dex_amd.h)
    assert "stage 2 has 80 channels" in msg, msg


# ------------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_bigvgan_22khz_matches_reference_golden():
    """fp32 against the real reference's output: the 5e-5 bound of the other BigVGAN tests (measured 1.7e-6 on MI355X); two calls
    bitwise equal."""
    from tests import gpu_util as U
    g = np.load(os.path.join(GOLD, "bigvgan_22khz.npz"))
    m = V.BigVGAN(V.AttrDict(V.BIGVGAN_22KHZ))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in bvg22_weights().items()})
    m = m.cuda().eval()
    wav = m(torch.from_numpy(g["mel"]).cuda()).cpu().numpy()
    assert wav.shape == g["wav"].shape
    e = np.abs(wav - g["wav"])
    U.record("bigvgan22_golden:fp32:call", max=e.max(), mean=e.mean())
    assert np.isfinite(wav).all() and e.max() <= 5e-5, float(e.max())
    again = m(torch.from_numpy(g["mel"]).cuda()).cpu().numpy()
    assert np.array_equal(wav, again)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(1, 1), (1, 37), (3, 64)])
def test_bigvgan_22khz_matches_oracle(B, T):
    from tests import gpu_util as U
    w = bvg22_weights()
    m = gpu_gen(V.BIGVGAN_22KHZ, w)
    mel = mel_input("bvg22_mel2", B, T, 59)
    wav = m(torch.from_numpy(mel).cuda()).cpu().numpy()
    ref = oracle(w, V.BIGVGAN_22KHZ, mel)
    assert wav.shape == ref.shape == (B, 1, T * 256)
    e = np.abs(wav - ref)
    U.record(f"bigvgan22_oracle_B{B}_T{T}:fp32:call", max=e.max(), mean=e.mean())
    assert np.isfinite(wav).all() and e.max() <= 5e-5, float(e.max())


SMALL = {
    # widths 96 / 48 / 24: a wide stage, then two narrow ones (transposed convs 96 -> 48 with K = 96, 48 -> 24 with K = 48)
    "snakebeta_222": dict(V.BIGVGAN_22KHZ, upsample_initial_channel=192, upsample_rates=[2, 2, 2], upsample_kernel_sizes=[4, 4, 4]),
    "snake_222": dict(V.BIGVGAN_22KHZ, upsample_initial_channel=192, upsample_rates=[2, 2, 2], upsample_kernel_sizes=[4, 4, 4], activation="snake"),
    # a k = 8, u = 4 transposed conv (ups.1.0, 96 -> 48) into a narrow stage
    "snakebeta_242": dict(V.BIGVGAN_22KHZ, upsample_initial_channel=192, upsample_rates=[2, 4, 2], upsample_kernel_sizes=[4, 8, 4]),
    "snake_242": dict(V.BIGVGAN_22KHZ, upsample_initial_channel=192, upsample_rates=[2, 4, 2], upsample_kernel_sizes=[4, 8, 4], activation="snake"),
    # HiFi-GAN V2 geometry: 64 / 32 / 16 / 8 (leaky_relu on the narrow kernels' input gather)
    "hifigan_v2": dict(V.HIFIGAN_V1, upsample_initial_channel=128),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SMALL))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 5, 37, 300])
def test_narrow_stages_match_oracle(name, B, T):
    from tests import gpu_util as U
    h = SMALL[name]
    w = small_weights(h)
    m = gpu_gen(h, w)
    mel = mel_input("narrow_mel", B, T, 60 + T)
    wav = m(torch.from_numpy(mel).cuda()).cpu().numpy()
    ref = oracle(w, h, mel)
    assert wav.shape == ref.shape == (B, 1, T * int(np.prod(h["upsample_rates"])))
    e = np.abs(wav - ref)
    U.record(f"narrow_{name}_B{B}_T{T}:fp32:call", max=e.max(), mean=e.mean())
    assert np.isfinite(wav).all() and e.max() <= 5e-5, float(e.max())
    assert np.array_equal(wav, m(torch.from_numpy(mel).cuda()).cpu().numpy())


# (max|d|, RMS of d) against the reference golden (|wav| <= 0.81); bounds about 2x the values measured on MI355X
BVG22_LOWP = {"bf16": (1.7e-2, 3.3e-3), "fp16": (1.8e-3, 4.3e-4)}      # measured: bf16 8.4e-3 / 1.6e-3, fp16 9.1e-4 / 2.1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_bigvgan_22khz_reduced_precision_mode(prec):
    """bf16 / fp16 operands on the wide stages (the narrow stages and the anti-aliased activations stay fp32): against the golden,
    different from the fp32 output, bitwise repeatable; fp32 mode untouched afterwards."""
    from tests import gpu_util as U
    g = np.load(os.path.join(GOLD, "bigvgan_22khz.npz"))
    m = gpu_gen(V.BIGVGAN_22KHZ, bvg22_weights())
    mel = torch.from_numpy(g["mel"]).cuda()
    exact = m(mel).cpu().numpy()
    m.precision = prec
    wav = m(mel).cpu().numpy()
    e = wav - g["wav"]
    mx, rms = BVG22_LOWP[prec]
    U.record(f"bigvgan22_golden:{prec}:call", max=np.abs(e).max(), mean=np.sqrt((e * e).mean()), ref_absmax=np.abs(g["wav"]).max())
    assert np.isfinite(wav).all() and not np.array_equal(wav, exact)
    assert np.abs(e).max() <= mx and np.sqrt((e * e).mean()) <= rms, (float(np.abs(e).max()), float(np.sqrt((e * e).mean())))
    assert np.array_equal(wav, m(mel).cpu().numpy())
    m.precision = "fp32"
    assert np.array_equal(exact, m(mel).cpu().numpy())


@pytest.mark.gpu
def test_get_vocoder_config_json(tmp_path):
    """get_vocoder(<bigvgan_22khz_80band config.json>, ckpt) with a training-style checkpoint (weight_g / weight_v pairs)."""
    w = bvg22_weights()
    sd = {}
    for k, v in w.items():
        t = torch.from_numpy(v)
        if k.endswith(".weight"):
            sd[k[:-len("weight")] + "weight_v"] = t * 1.5
            sd[k[:-len("weight")] + "weight_g"] = t.flatten(1).norm(dim=1).reshape(-1, *([1] * (t.dim() - 1)))
        else:
            sd[k] = t
    cfg = dict(V.BIGVGAN_22KHZ, sampling_rate=22050, hop_size=256, n_fft=1024, win_size=1024, fmin=0, fmax=8000, resblock_initial_channel=0)
    p = tmp_path / "config.json"
    p.write_text(json.dumps(cfg))
    voc = V.get_vocoder(str(p), {"generator": sd})
    mel = mel_input("bvg22_mel3", 1, 12, 61)
    got = voc(torch.from_numpy(mel).cuda()).cpu().numpy()
    assert np.abs(got - oracle(w, V.BIGVGAN_22KHZ, mel)).max() <= 5e-5


@pytest.mark.gpu
def test_tokens_to_waveform_bigvgan_22khz():
    """synthesize.py:31-38 end to end with the 112 M vocoder: finite int16 audio of y_len * 256 samples per utterance."""
    from dex_tts_amd import synthesize as SY, tts
    from tests.test_tts_module import full_state_dict, model_cfg
    m = tts.GeDEXTTS(model_cfg("gedex_lj"))
    m.load_state_dict(full_state_dict(m, "gedex_lj"))
    m = m.cuda().eval()
    voc = gpu_gen(V.BIGVGAN_22KHZ, bvg22_weights())
    tok, lengths = synth.make_text_inputs(2, 21, [21, 12], 149)
    SY.seed_init(100)
    audio, y_dec, attn = SY.synthesize_tokens(m, voc, torch.from_numpy(tok).cuda(), torch.from_numpy(lengths).cuda(), n_timesteps=4)
    y_len = m.encoder._last["y_len"].cpu().numpy()
    assert len(audio) == 2 and all(a.dtype == np.int16 for a in audio)
    assert [len(a) for a in audio] == [int(n) * 256 for n in y_len]
    assert torch.isfinite(y_dec).all() and all(np.abs(a.astype(np.int32)).max() > 0 for a in audio)
