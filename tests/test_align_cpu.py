"""CPU: the MAS restatement (tests/mas_restatement.py) against the reference's Cython core (tests/golden/align_mas.npz, written by
tools/make_golden_align.py), the host-side argument checks of the MAS C ABI, and the refusals of dex_tts_amd.align."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from dex_tts_amd import _lib, align
from tests import mas_restatement as R


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "align_mas.npz"))


def _cases(g):
    return sorted({k.split("__")[0] for k in g.files})


def _value(g, name):
    if name == "global":
        return R.hashed_value(len(g["global__tx"]), 1100, 1200)
    return g[f"{name}__value"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dex_tts_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_golden_has_every_case(golden_dir):
    assert set(_cases(_golden(golden_dir))) == {"random", "mel", "allequal", "zeros", "intties", "square", "tx1", "ragged", "wide", "global"}


@pytest.mark.parametrize("name", ["random", "mel", "allequal", "zeros", "intties", "square", "tx1", "ragged", "wide", "global"])
def test_restatement_reproduces_reference_core(golden_dir, name):
    g = _golden(golden_dir)
    v = _value(g, name)
    dur = R.durations(v, g[f"{name}__tx"], g[f"{name}__ty"])
    np.testing.assert_array_equal(dur, g[f"{name}__dur"])
    if f"{name}__path" in g.files:
        np.testing.assert_array_equal(R.path_from_durations(dur, v.shape[2]), g[f"{name}__path"])


def test_tie_cases_hold_ties(golden_dir):
    """The all-equal and integer cases really exercise the strict comparison: their backtracks meet exact ties."""
    g = _golden(golden_dir)
    for name in ("allequal", "intties", "zeros"):
        v = g[f"{name}__value"]
        assert R.min_margin(v[0], int(g[f"{name}__tx"][0]), int(g[f"{name}__ty"][0])) == 0.0, name


def test_tie_stays_on_row():
    """An all-equal matrix: every comparison is a tie, so the path stays on the last row as long as it can and then walks the diagonal."""
    d = R.durations(np.zeros((3, 6), np.float32), 3, 6)
    np.testing.assert_array_equal(d, [1, 1, 4])


I32 = C.POINTER(C.c_int32)


def _arr(v):
    a = np.ascontiguousarray(np.asarray(v, np.int32))
    return a, a.ctypes.data_as(I32)


def test_cabi_rejects_bad_arguments(lib):
    fake = C.c_void_p(256)                        # never dereferenced: every case is refused before anything is enqueued
    ws = int(lib.dex_mas_workspace_bytes(2, 8, 16))
    assert ws > 0

    def call(B=2, Tx=8, Ty=16, tx=(8, 4), ty=(16, 4), value=fake, dur=fake, wsp=fake, strides=(128, 16, 1)):
        a, pa = _arr(tx) if tx is not None else (None, None)
        b, pb = _arr(ty) if ty is not None else (None, None)
        return lib.dex_mas_durations(value, None, B, Tx, Ty, *strides, pa, pb, dur, None, wsp, ws, None)

    assert call(tx=(8, 5), ty=(16, 4)) == -1                    # t_y < t_x: no monotonic path
    assert call(tx=(0, 4)) == -1                                # empty text
    assert call(tx=(9, 4)) == -1                                # t_x > Tx
    assert call(ty=(17, 4)) == -1                               # t_y > Ty
    assert call(tx=None) == -1 and call(ty=None) == -1          # null host lengths
    assert call(value=None) == -1 and call(dur=None) == -1 and call(wsp=None) == -1
    assert call(strides=(0, 16, 1)) == -1
    assert call(B=0) == -1
    assert call(Tx=2049, tx=(8, 4)) == -1                       # over DEX_MAS_MAX_TX
    assert call(Ty=8193) == -1                                  # over DEX_MAS_MAX_TY
    assert lib.dex_mas_workspace_bytes(1, 2049, 4096) == 0
    assert lib.dex_mas_workspace_bytes(1, 16, 8193) == 0
    assert lib.dex_mas_workspace_bytes(0, 16, 16) == 0
    # the split between LDS and global bit matrices: 160 KiB of packed bits
    assert lib.dex_mas_workspace_bytes(4, 256, 1024) == 256
    assert lib.dex_mas_workspace_bytes(2, 1100, 1200) == 2 * 1100 * 38 * 4
    assert lib.dex_mas_log_prior(fake, fake, 1, 129, 8, 8, fake, None) == -1
    assert lib.dex_mas_log_prior(None, fake, 1, 80, 8, 8, fake, None) == -1
    assert lib.dex_mas_log_prior(fake, fake, 1, 80, 2049, 8, fake, None) == -1
    assert lib.dex_mas_loss_workspace_bytes(0) == 0
    a, pa = _arr((3,)); b, pb = _arr((5,))
    assert lib.dex_mas_losses(fake, fake, pa, 1, 2, fake, fake, pb, 80, 8, fake, fake, 16, None) == -1     # x length 3 > Tx 2
    assert lib.dex_mas_losses(fake, fake, None, 1, 4, fake, fake, pb, 80, 8, fake, fake, 16, None) == -1


def test_align_refuses_cpu_and_grad_tensors():
    v = torch.zeros(1, 3, 6)
    with pytest.raises(RuntimeError):
        align.maximum_path(v, torch.ones_like(v))
    with pytest.raises(RuntimeError):
        align.log_prior(torch.zeros(1, 80, 3), torch.zeros(1, 80, 6))
    with pytest.raises(RuntimeError):
        align.mas_durations(torch.zeros(1, 80, 3, requires_grad=True), [3], torch.zeros(1, 80, 6), [6])
    with pytest.raises(RuntimeError):
        align.dur_prior_losses(torch.zeros(1, 3), torch.ones(1, 3, dtype=torch.int32), [3], torch.zeros(1, 80, 6), torch.zeros(1, 80, 6), [6])
