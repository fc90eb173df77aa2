"""GPU: ``_native.Handle`` (the owner of one C handle and its workspace), the per-device caches built on it, and a handle's life
cycle through ``VoiceEncoder``.  Small shapes, random weights."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_handle_workspace_and_check():
    from dex_tts_amd._native import Handle
    h = Handle("dex_gl")
    assert h.h and h.device == torch.device("cuda", torch.cuda.current_device())
    a = h.workspace(1024)
    assert a.dtype == torch.uint8 and a.device == h.device and a.numel() >= 1024
    assert h.workspace(512) is a and h.workspace(1024) is a                     # kept while it is large enough
    b = h.workspace(4096)
    assert b is not a and b.numel() >= 4096 and b.numel() > a.numel()
    assert h.workspace(1024) is b
    h.check(0, "nothing")
    with pytest.raises(ValueError, match="refused"):
        h.check(-1, "refused")
    with pytest.raises(ValueError):
        h.check(-2, "state")
    with pytest.raises(RuntimeError, match="hip"):
        h.check(-3, "hip")
    strict = Handle("dex_mel", "cuda", arg_errors=())                          # the owner names the codes: none here
    with pytest.raises(RuntimeError):
        strict.check(-1, "refused")
    h.__del__()
    assert h.h is None
    h.__del__()                                                                # a second destroy neither raises nor reaches the library


def test_one_context_per_device():
    from dex_tts_amd import griffin_lim, speaker
    here = torch.device("cuda", torch.cuda.current_device())
    for module in (speaker, griffin_lim):
        ctx = module._context(torch.device("cuda"))
        assert module._context(here) is ctx and module._context(torch.device("cuda")) is ctx
        assert ctx.device == here and ctx.h
    assert speaker._context(here) is not griffin_lim._context(here)


def test_a_fresh_encoder_works_after_one_was_deleted():
    from dex_tts_amd import speaker
    g = torch.Generator().manual_seed(0)
    sd = {k: 0.1 * torch.randn(shape, generator=g) for k, shape in speaker.state_dict_shapes().items()}
    wav = (0.1 * torch.randn(4000, generator=g)).cuda()
    enc = speaker.VoiceEncoder("cuda").load_state_dict(sd)
    first = enc.embed_utterance(wav)
    assert tuple(first.shape) == (256,) and abs(float(torch.linalg.vector_norm(first)) - 1.0) < 1e-5
    del enc
    gc.collect()
    again = speaker.VoiceEncoder("cuda").load_state_dict(sd).embed_utterance(wav)
    assert torch.equal(first, again)
