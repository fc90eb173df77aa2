"""Write tests/golden/griffin_lim.npz from the reference's own STFT, griffin_lim and window_sumsquare (DEX-TTS audio/stft.py,
audio/audio_processing.py; GeDEX-TTS has the same files), run on the CPU.

The reference's inv_mel_spec (audio/tools.py:18-34) cannot run as it stands: it reads ``_stft._stft_fn``, which its TacotronSTFT never
defines (only ``stft_fn``, stft.py:137).  Its lines 19-29 are therefore restated here around the reference's griffin_lim, with the
reference's TacotronSTFT (mel_basis, spectral_de_normalize) and its STFT.

    python tools/make_golden_griffin_lim.py        (needs the reference tree; imported through oracle.ref_import)

Records, per mel (the real ``sample1_1s_mel`` of tests/golden/audio_mel.npz and its ``chirp_mel``):
    angles_<m>      the initial angles the seeded griffin_lim draws (np.random.seed(SEED), audio_processing.py:74-75)
    spec_<m>        spec_from_mel (tools.py:19-26), all T frames ([513, T]; griffin_lim gets the first T - 1)
    gl<n>_<m>       griffin_lim(spec_from_mel[:, :, :-1], stft_fn, n) under np.random.seed(SEED), n = 0, 1, 60 for sample1, 0 for chirp
    sc60_<m>        the spectral convergence |S - |STFT(x)|| / |S| of the 60-iteration output, with the reference's own transform
and for a slice of tests/golden/sample1_wav.npz:
    wav             the slice;  wav_mag / wav_phase  STFT.transform(wav);  wav_inv  STFT.inverse(transform(wav))
    wss_<F>         window_sumsquare('hann', F, 256, 1024, 1024, float32) for the frame counts used above
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference_audio  # noqa: E402

SEED = 1234
OUT = os.path.join(ROOT, "tests", "golden", "griffin_lim.npz")
WAV_SLICE = (22050, 22050 + 8192)            # 8192 samples of sample1 from 1 s on


def main():
    torch.set_num_threads(8)
    stft_mod, _ = import_reference_audio("DEX-TTS")
    ap = importlib.import_module("audio.audio_processing")
    tac = stft_mod.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    stft_fn = tac.stft_fn
    mels = np.load(os.path.join(ROOT, "tests", "golden", "audio_mel.npz"))
    out = {"seed": np.int64(SEED)}
    for name, key, iters in (("s1", "sample1_1s_mel", (0, 1, 60)), ("chirp", "chirp_mel", (0,))):
        mel = torch.from_numpy(mels[key].astype(np.float32))
        # tools.py:19-26
        m = torch.stack([mel])
        mel_decompress = tac.spectral_de_normalize(m).transpose(1, 2).data.cpu()
        spec_from_mel = torch.mm(mel_decompress[0], tac.mel_basis).transpose(0, 1).unsqueeze(0) * 1000
        S = spec_from_mel[:, :, :-1]
        out[f"spec_{name}"] = spec_from_mel[0].numpy().astype(np.float32)
        np.random.seed(SEED)
        out[f"angles_{name}"] = np.angle(np.exp(2j * np.pi * np.random.rand(*S.size()))).astype(np.float32)[0]
        for n in iters:
            np.random.seed(SEED)
            x = ap.griffin_lim(S, stft_fn, n)
            out[f"gl{n}_{name}"] = x[0].numpy().astype(np.float32)
            if n == 60:
                mag, _ = stft_fn.transform(x)
                out[f"sc60_{name}"] = np.float64(torch.linalg.norm(S - mag) / torch.linalg.norm(S))
        F = S.shape[-1]
        out[f"wss_{F}"] = ap.window_sumsquare("hann", F, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32)
    wav = np.load(os.path.join(ROOT, "tests", "golden", "sample1_wav.npz"))["wav"][WAV_SLICE[0]:WAV_SLICE[1]].astype(np.float32)
    y = torch.from_numpy(wav)[None]
    mag, phase = stft_fn.transform(y)
    out["wav"] = wav
    out["wav_mag"], out["wav_phase"] = mag[0].numpy(), phase[0].numpy()
    out["wav_inv"] = stft_fn.inverse(mag, phase)[0, 0].numpy()
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB, " + ", ".join(f"{k} {np.shape(v)}" for k, v in out.items()))


if __name__ == "__main__":
    main()
