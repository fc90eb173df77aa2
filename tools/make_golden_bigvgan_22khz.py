"""Checker infrastructure (build container only): run the REAL reference BigVGAN generator (DEX-TTS/bigvgan/models.py) at the published
bigvgan_22khz_80band configuration (vocoder.BIGVGAN_22KHZ: 1536 initial channels, six up-sampling stages down to 24 channels, 112 M
parameters) on portable synthetic weights and a synthetic mel; commit tests/golden/bigvgan_22khz.npz (mel, waveform, the resampling
filter the reference registers) + manifest_bigvgan_22khz.json, and check oracle/bigvgan_oracle.py against it on the way.
The same recipe as oracle/make_golden_bigvgan.py (BigVGAN-base).

    python tools/make_golden_bigvgan_22khz.py [--reference DIR]      (DIR: the reference DEX-TTS tree)
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from dex_tts_amd import synth, vocoder as V  # noqa: E402
from oracle import bigvgan_oracle as BO  # noqa: E402
from oracle.make_golden_bigvgan import REF  # noqa: E402  (where the oracle's golden tools find the reference tree)


def weights(filt=None):
    """synth.make_vocoder_weights at this configuration (its output for the existing shapes is unchanged), conv_post scaled by 1/2:
    the six stages' periodic activations add more energy than BigVGAN-base's four, and unscaled the waveform peaks at 0.9797, at the
    edge of tanh's saturation.  The registered filters replaced by the reference's constant when given."""
    w = synth.make_vocoder_weights(V.param_shapes(V.BIGVGAN_22KHZ))
    w["conv_post.weight"] = w["conv_post.weight"] * np.float32(0.5)
    if filt is not None:
        for k in w:
            if k.endswith(".filter"):
                assert np.allclose(w[k], filt, atol=1e-7), k
                w[k] = filt.copy()
    return w


def mel_input(B=2, T=9):
    return np.clip(synth.normalish("bvg22_mel", (B, 80, T), 58) * 1.5 - 5.0, -11.5, 2.5).astype(np.float32)


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DEX_REFERENCE", REF))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, args.reference)
    import bigvgan                                      # the reference package
    torch.set_num_threads(8)
    h = bigvgan.AttrDict(dict(V.BIGVGAN_22KHZ))
    g = bigvgan.Generator(h).eval()
    with contextlib.redirect_stdout(io.StringIO()):
        g.remove_weight_norm()
    keys = {k: list(v.shape) for k, v in g.state_dict().items()}
    shapes = V.param_shapes(V.BIGVGAN_22KHZ)
    assert {k: tuple(v) for k, v in keys.items()} == {k: tuple(v) for k, v in shapes.items()}, "param_shapes disagrees with the reference"
    n = sum(int(np.prod(s)) for k, s in shapes.items() if not k.endswith(".filter"))
    assert n == 112_199_473, n
    filt = g.state_dict()["activation_post.upsample.filter"].numpy().copy()
    assert np.array_equal(BO.kaiser_sinc_filter1d(0.25, 0.3, 12).numpy(), filt.flatten())
    w = weights(filt)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    mel = mel_input()
    wav = g(torch.from_numpy(mel)).numpy()
    ow = BO.generator({k: torch.from_numpy(v) for k, v in w.items()}, V.BIGVGAN_22KHZ, torch.from_numpy(mel)).numpy()
    d = float(np.abs(ow - wav).max())
    sat = float((np.abs(wav) > 0.99).mean())
    print("oracle vs reference: max|d| =", d, " |wav|max =", float(np.abs(wav).max()), " saturated (|wav| > 0.99):", sat,
          " std:", float(wav.std()), wav.shape, " parameters:", n)
    assert d <= 1e-6, d
    assert np.abs(wav).max() < 0.98 and wav.std() > 0.05, "the synthetic weights saturate or silence this configuration"
    np.savez_compressed(os.path.join(OUT, "bigvgan_22khz.npz"), mel=mel, wav=wav, filter=filt)
    with open(os.path.join(OUT, "manifest_bigvgan_22khz.json"), "w") as f:
        json.dump({"config": dict(V.BIGVGAN_22KHZ), "keys": keys}, f, indent=0)
    print("wrote bigvgan_22khz.npz, manifest_bigvgan_22khz.json")


if __name__ == "__main__":
    main()
