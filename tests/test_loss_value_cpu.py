"""CPU: the golden of the reference's validation compute_loss (tests/golden/compute_loss.npz, tools/make_golden_compute_loss.py)
restated in numpy — the out_size cut, mu_y = attn^T mu_x on it, and the duration / prior / VQ commitment formulas — plus the offset
draws of align.segment_offsets and every refusal of loss_value that happens before a device is touched."""
import os
import random

import numpy as np
import pytest
import torch

from dex_tts_amd import align, style as S, synth, tts
from tests import mas_restatement as R
from tests.test_tts_module import model_cfg

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "compute_loss.npz"))
CASES = ["gedex_lj", "gedex_vctk", "dex_vctk"]


def g(case, k):
    return G[f"{case}__{k}"]


def cut(case):
    """tts.py:116-138 with the stored offsets: -> y_cut, mu_y (the 0/1 path product), mask, cut lengths."""
    y, mu, dur, yl, off, out_size = g(case, "y"), g(case, "mu_x"), g(case, "dur"), g(case, "y_lengths"), g(case, "offsets"), int(g(case, "out_size"))
    B, F, Ty = y.shape
    path = R.path_from_durations(dur, Ty).astype(np.float32)
    mu_y = np.einsum("bxt,bfx->bft", path, mu).astype(np.float32)
    if out_size and out_size < Ty:
        cl = np.minimum(yl, out_size)
        yc, mc = np.zeros((B, F, out_size), np.float32), np.zeros((B, F, out_size), np.float32)
        for b in range(B):
            yc[b, :, :cl[b]] = y[b, :, off[b]:off[b] + cl[b]]
            mc[b, :, :cl[b]] = mu_y[b, :, off[b]:off[b] + cl[b]]
        return yc, mc, (np.arange(out_size)[None] < cl[:, None]).astype(np.float32), cl
    return y, mu_y, (np.arange(Ty)[None] < yl[:, None]).astype(np.float32), yl


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_golden_losses(case):
    yc, mc, mask, cl = cut(case)
    assert np.array_equal(yc, g(case, "y_cut")) and np.array_equal(mc, g(case, "mu_y"))
    assert np.array_equal(mask, g(case, "y_mask")[:, 0])
    dur, xl, logw = g(case, "dur").astype(np.float64), g(case, "x_lengths"), g(case, "logw")[:, 0].astype(np.float64)
    xm = (np.arange(dur.shape[1])[None] < xl[:, None]).astype(np.float64)
    dur_loss = np.sum((logw - np.log(1e-8 + dur) * xm) ** 2) / xl.sum()
    F = yc.shape[1]
    prior = np.sum(0.5 * ((yc.astype(np.float64) - mc) ** 2 + np.log(2 * np.pi)) * mask[:, None]) / (mask.sum() * F)
    assert dur_loss == pytest.approx(float(g(case, "dur_loss")), rel=1e-6)
    assert prior == pytest.approx(float(g(case, "prior_loss")), rel=1e-6)
    if case.startswith("dex"):
        e = synth.make_style_weights(S.param_shapes(S.VCTK))["tv_encoder.vq.embedding"].astype(np.float64)
        x, m, idx = g(case, "vq_x").astype(np.float64), g(case, "vq_mask").transpose(0, 2, 1).astype(np.float64), g(case, "vq_idx")
        vq = 0.25 * np.sum((x * m - e[idx] * m) ** 2) / (m.sum() * x.shape[-1])
        assert vq == pytest.approx(float(g(case, "vq_loss")), rel=1e-6)


@pytest.mark.parametrize("case", ["gedex_lj", "dex_vctk"])
def test_segment_offsets_follow_random(case):
    random.seed(int(g(case, "seed")))
    off = align.segment_offsets(torch.from_numpy(g(case, "y_lengths")), int(g(case, "out_size")))
    assert off.tolist() == g(case, "offsets").tolist()
    assert random.random() == float(g(case, "random_after"))


def test_segment_offsets_draw_only_for_rows_with_range():
    random.seed(5)
    got = align.segment_offsets([40, 64, 65, 100], 64)      # max_offset 0, 0, 1, 36: two draws
    after = random.random()
    random.seed(5)
    assert got.tolist() == [0, 0, random.choice(range(0, 1)), random.choice(range(0, 36))]
    assert after == random.random()


def _gedex():
    return tts.GeDEXTTS(model_cfg("gedex_lj"))


def test_loss_value_refusals():
    m = _gedex()
    x, xl = torch.zeros(2, 10, dtype=torch.long), torch.tensor([10, 8])
    y, yl = torch.zeros(2, 80, 96), torch.tensor([96, 50])
    with pytest.raises(NotImplementedError):
        m.loss_value(x, xl, y, yl, mask_ratio=0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        m.loss_value(x, xl, y, yl)
    with pytest.raises(RuntimeError, match="forward-only"):
        m.loss_value(x, xl, y.clone().requires_grad_(True), yl)
    with pytest.raises(ValueError, match="more tokens than frames"):
        tts._TTSBase._loss_checks((), torch.tensor([10, 8]), y, torch.tensor([96, 7]), None, 0)
    with pytest.raises(ValueError, match="broadcast"):
        tts._TTSBase._loss_checks((), xl, y, torch.tensor([60, 50]), 64, 0)
    tts._TTSBase._loss_checks((), xl, y, torch.tensor([64, 50]), 64, 0)       # one row reaches out_size: the reference runs
    tts._TTSBase._loss_checks((), xl, y, torch.tensor([60, 50]), 96, 0)       # out_size >= Ty: no cut
    with pytest.raises(NotImplementedError):
        m.compute_loss(x, xl, y, yl)
    d = tts.DeXTTS(model_cfg("dex_vctk"))
    with pytest.raises(RuntimeError, match="CUDA"):
        d.loss_value(x, xl, y, yl, torch.zeros(2, 80, 40), torch.tensor([40, 30]), torch.zeros(2, 80, 40), torch.tensor([40, 30]),
                     torch.zeros(2, 40), torch.tensor([40, 30]), out_size=48)


def test_segment_refuses_cpu():
    with pytest.raises(RuntimeError):
        align.segment(torch.zeros(1, 80, 5), torch.ones(1, 5, dtype=torch.int32), torch.zeros(1, 80, 5), [5])
