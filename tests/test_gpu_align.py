"""GPU: the monotonic alignment search (csrc/mas.hip via dex_tts_amd.align) against the reference's Cython core
(tests/golden/align_mas.npz): bitwise paths and durations on the LDS and the global-memory bit matrices, in both value layouts,
batch independence, the device log-prior, forced alignment from mu_x / y, and the duration / prior loss reductions."""
import os

import numpy as np
import pytest
import torch

from dex_tts_amd import _lib, align
from tests import mas_restatement as R

pytestmark = pytest.mark.gpu
NAMES = ["random", "mel", "allequal", "zeros", "intties", "square", "tx1", "ragged", "wide", "global"]


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "align_mas.npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _value(g, name):
    if name == "global":
        return R.hashed_value(len(g["global__tx"]), 1100, 1200)
    return g[f"{name}__value"]


def _mask(tx, ty, Tx, Ty):
    m = np.zeros((len(tx), Tx, Ty), np.float32)
    for b in range(len(tx)):
        m[b, :tx[b], :ty[b]] = 1.0
    return m


@pytest.mark.parametrize("name", NAMES)
def test_maximum_path_bitwise(g, dev, name):
    v = _value(g, name)
    tx, ty = g[f"{name}__tx"], g[f"{name}__ty"]
    lds = _lib.load().dex_mas_workspace_bytes(*v.shape) == 256
    assert lds == (name != "global")                       # the global case is the one beyond LDS
    vt = torch.from_numpy(v).to(dev)
    mt = torch.from_numpy(_mask(tx, ty, *v.shape[1:])).to(dev)
    path = align.maximum_path(vt, mt)
    assert path.dtype == torch.float32 and path.device == vt.device
    want = R.path_from_durations(g[f"{name}__dur"], v.shape[2])
    np.testing.assert_array_equal(path.cpu().numpy().astype(np.int8), want)
    if f"{name}__path" in g.files:
        np.testing.assert_array_equal(path.cpu().numpy().astype(np.int8), g[f"{name}__path"])
    # frame-major layout (the one the log-prior kernel writes), durations only, no mask
    fm = vt.transpose(1, 2).contiguous().transpose(1, 2)
    dur, _ = align._search(fm, None, np.ascontiguousarray(tx), np.ascontiguousarray(ty), False)
    np.testing.assert_array_equal(dur.cpu().numpy(), g[f"{name}__dur"])
    again, _ = align._search(fm, None, np.ascontiguousarray(tx), np.ascontiguousarray(ty), False)
    assert torch.equal(dur, again)


def test_large_lds_bit_matrix(dev):
    """1000 rows x 38 words = 152 KB of bits: still in LDS (above the default 64 KB dynamic allocation); against the restatement."""
    v = R.hashed_value(2, 1000, 1200)
    tx, ty = np.array([1000, 900], np.int32), np.array([1200, 1111], np.int32)
    assert _lib.load().dex_mas_workspace_bytes(2, 1000, 1200) == 256
    dur, _ = align._search(torch.from_numpy(v).to(dev), None, tx, ty, False)
    np.testing.assert_array_equal(dur.cpu().numpy(), R.durations(v, tx, ty))


def test_maximum_path_keeps_dtype(g, dev):
    v = torch.from_numpy(g["intties__value"]).to(dev).double()
    tx, ty = g["intties__tx"], g["intties__ty"]
    m = torch.from_numpy(_mask(tx, ty, *v.shape[1:])).to(dev).double()
    p = align.maximum_path(v, m)
    assert p.dtype == torch.float64
    np.testing.assert_array_equal(p.cpu().numpy().astype(np.int8), g["intties__path"])


@pytest.mark.parametrize("name", ["ragged", "random", "global"])
def test_row_alone_equals_row_in_batch(g, dev, name):
    v = torch.from_numpy(_value(g, name)).to(dev)
    tx, ty = g[f"{name}__tx"], g[f"{name}__ty"]
    full, _ = align._search(v, None, np.ascontiguousarray(tx), np.ascontiguousarray(ty), False)
    for b in range(v.shape[0]):
        one, _ = align._search(v[b:b + 1], None, np.ascontiguousarray(tx[b:b + 1]), np.ascontiguousarray(ty[b:b + 1]), False)
        assert torch.equal(one[0], full[b]), b


def test_log_prior_and_forced_alignment(g, dev):
    mu, y = torch.from_numpy(g["mel__mu"]).to(dev), torch.from_numpy(g["mel__y"]).to(dev)
    want = g["mel__value"]
    lp = align.log_prior(mu, y).cpu().numpy()
    assert lp.shape == want.shape
    # the kernel sums in fp64 and rounds once: against fp64 it is within half an ulp of the largest value
    m64, y64 = g["mel__mu"].astype(np.float64), g["mel__y"].astype(np.float64)
    exact = (-0.5 * (y64 ** 2).sum(1)[:, None, :] + np.einsum("bfx,bfy->bxy", m64, y64) - 0.5 * (m64 ** 2).sum(1)[:, :, None]
             - 0.5 * np.log(2 * np.pi) * m64.shape[1])
    assert np.abs(lp - exact).max() <= 6e-8 * np.abs(exact).max()
    # the golden is torch's fp32 matmul, whose own rounding is ~1e-6 of max |log_prior| on these magnitudes
    assert np.abs(lp - want).max() <= 2e-6 * np.abs(want).max()
    tx, ty = g["mel__tx"], g["mel__ty"]
    dur, lp2 = align.mas_durations(mu, torch.from_numpy(tx), y, torch.from_numpy(ty), return_log_prior=True)
    assert torch.equal(lp2, align.log_prior(mu, y))
    np.testing.assert_array_equal(dur.cpu().numpy(), g["mel__dur"])


def test_refuses_grad_and_short_rows(dev):
    v = torch.zeros(1, 3, 6, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError):
        align.maximum_path(v, torch.ones(1, 3, 6, device=dev))
    m = torch.zeros(1, 4, 6, device=dev)
    m[0, :4, :3] = 1.0                                        # t_x = 4 > t_y = 3: no monotonic path
    with pytest.raises(ValueError):
        align.maximum_path(torch.zeros(1, 4, 6, device=dev), m)


def test_dur_prior_losses(dev):
    rng = np.random.default_rng(5)
    B, Tx, F, Ty = 3, 20, 80, 64
    tx, ty = np.array([20, 11, 7]), np.array([64, 40, 30])
    dur = np.zeros((B, Tx), np.int32)
    for b in range(B):
        dur[b, :tx[b]] = rng.multinomial(ty[b] - tx[b], np.ones(tx[b]) / tx[b]) + 1
    xm = (np.arange(Tx)[None] < tx[:, None]).astype(np.float32)
    ym = (np.arange(Ty)[None] < ty[:, None]).astype(np.float32)
    logw = (rng.standard_normal((B, 1, Tx)).astype(np.float32) + 1.0) * xm[:, None]
    y = rng.standard_normal((B, F, Ty)).astype(np.float32)
    mu_y = rng.standard_normal((B, F, Ty)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    d, p = align.dur_prior_losses(t(logw), t(dur), tx, t(y), t(mu_y), ty)
    assert d.dim() == 0 and p.dim() == 0 and d.device.type == "cuda"
    lw_ = np.log(1e-8 + dur.astype(np.float64)) * xm
    want_d = ((logw[:, 0].astype(np.float64) - lw_) ** 2).sum() / tx.sum()
    want_p = (0.5 * ((y.astype(np.float64) - mu_y) ** 2 + np.log(2 * np.pi)) * ym[:, None]).sum() / (ym.sum() * F)
    assert abs(float(d) - want_d) <= 1e-5 * abs(want_d)
    assert abs(float(p) - want_p) <= 1e-5 * abs(want_p)
    d2, p2 = align.dur_prior_losses(t(logw), t(dur), tx, t(y), t(mu_y), ty)
    assert torch.equal(d, d2) and torch.equal(p, p2)
