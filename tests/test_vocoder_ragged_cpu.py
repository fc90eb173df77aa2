"""Ragged vocoder batches (dex_vocode_ragged, Generator.forward(x, lengths)), the part that needs no GPU: the two entry points are declared,
exported and bound; the workspace query's host logic; the Python wrapper's argument checks.  The kernels are held to the oracle in
tests/test_gpu_vocoder_ragged.py."""
import ctypes as C
import os
import re

import pytest
import torch

from dex_tts_amd import _lib, vocoder as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dex_vocode_ragged", "dex_voc_ragged_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from dex_tts_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_ragged_entry_points_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "dex_amd.h")).read()
    declared = set(re.findall(r"\b(dex_[a-z_0-9]+)\s*\(", hdr))
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    # the same argument list as dex_vocode plus the device lengths behind the mel
    plain, ragged = bound["dex_vocode"][1], bound["dex_vocode_ragged"][1]
    assert ragged == plain[:2] + [C.c_void_p] + plain[2:]
    assert bound["dex_voc_ragged_workspace_bytes"] == bound["dex_voc_workspace_bytes"]


@pytest.mark.parametrize("h", [V.HIFIGAN_V1, V.BIGVGAN_BASE, V.BIGVGAN_22KHZ, dict(V.HIFIGAN_V1, upsample_initial_channel=128)],
                         ids=["hifigan_v1", "bigvgan_base", "bigvgan_22khz", "hifigan_v2"])
def test_ragged_workspace_query(lib, h):
    """Host logic only (no weights, no device): 0 for bad arguments; never less than the plain plan, and more by at most the 0 / 1 rows of
    the implicit GEMMs' output masks (one float per sample and rate, a 256-byte round-up each) - the activations are shared."""
    cfg = V.make_config(h)
    ctx = C.c_void_p()
    assert lib.dex_voc_create(C.byref(cfg), C.byref(ctx)) == 0, lib.dex_voc_last_error(ctx)
    try:
        for B, T in [(0, 8), (-1, 8), (2, 0), (2, -5)]:
            assert lib.dex_voc_ragged_workspace_bytes(ctx, B, T) == 0
        assert lib.dex_voc_ragged_workspace_bytes(None, 2, 8) == 0
        rates = [1]
        for u in h["upsample_rates"]:
            rates.append(rates[-1] * u)
        for B, T in [(1, 1), (3, 40), (32, 512)]:
            plain, ragged = lib.dex_voc_workspace_bytes(ctx, B, T), lib.dex_voc_ragged_workspace_bytes(ctx, B, T)
            assert plain > 0 and plain < ragged <= plain + sum(4 * B * T * r + 256 for r in rates), (B, T, plain, ragged)
    finally:
        lib.dex_voc_destroy(ctx)


def test_forward_checks_lengths_before_any_device_work():
    gen = V.Generator()
    mel = torch.zeros(3, 80, 4)
    for bad in ([4, 4], [4, 4, 4, 4], torch.tensor([[4, 4, 4], [4, 4, 4]]), []):
        with pytest.raises(ValueError):
            gen(mel, lengths=bad)                      # wrong count: ValueError, raised in front of the engine's device check
    with pytest.raises(ValueError):
        gen(mel, lengths=[4.0, 2.5, 1.0])              # frame counts are integers
    for ok in ([4, 2, 1], torch.tensor([4, 2, 1]), torch.tensor([4, 2, 1], dtype=torch.int32)):
        with pytest.raises(RuntimeError):
            gen(mel, lengths=ok)                       # CPU tensor: still no CPU path
    with pytest.raises(RuntimeError):
        gen(mel)
    assert gen._ctx is None                            # nothing was created on the way
