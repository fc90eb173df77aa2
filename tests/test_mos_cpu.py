"""CPU: the restatement tests/mos_ref.py (which the GPU tests hold the device to) against ``transformers.Wav2Vec2Model`` +
``nn.Embedding`` + ``nn.LSTM(bidirectional=True)`` + the projection, all in double precision; the reverse direction of a shorter row
against ``pack_padded_sequence``; the conditions ``make_weights`` must meet for the tests to see anything; the rename of the
upstream checkpoint's keys; and the host half of dex_tts_amd/mos.py (config refusals, too-short rows, the inventory, frame counts).

The bound on the restatement is tests/test_wavlm_cpu.py's: 1e-9 of the largest magnitude."""
import numpy as np
import pytest

from tests import mos_ref as R
from tests.test_wavlm_cpu import CAP

IDS = [(0, 288), (2, 17)]


def check_close(what, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{what}: |restatement - modules| = {err:.2e} at magnitude {scale:.2f}")
    assert got.shape == want.shape
    assert err <= CAP * scale, (what, err, scale)


@pytest.fixture(scope="module")
def tiny():
    pytest.importorskip("transformers")
    sd = R.make_weights(R.TINY, 0)
    return sd, R.hf_modules(R.TINY, sd)


@pytest.mark.parametrize("n", [400, 720, 5200, 32080])
def test_restatement_matches_transformers_and_torch_modules(tiny, n):
    """1, 2, 16 and 100 frames, two (domain, judge) pairs: hidden states, the LSTM's output, frame scores and the score."""
    import torch
    sd, mods = tiny
    wav = R.synth_wav(n, 40 + n % 7)
    for domain, judge in IDS:
        ref = R.forward(R.TINY, sd, wav, domain, judge)
        hf = R.hf_forward(mods, torch.from_numpy(wav.astype(np.float64))[None], domain, judge)
        assert ref[0].shape == (R.num_frames(R.TINY, n), 128)
        for name, a, b in zip(("hidden", "lstm_out", "frames"), ref[:3], hf[:3]):
            check_close(f"n={n} ids=({domain}, {judge}) {name}", a, b[0].numpy())
        check_close(f"n={n} ids=({domain}, {judge}) score", np.array([ref[3]]), hf[3].numpy())
    a, b = (R.forward(R.TINY, sd, wav, *ids)[3] for ids in IDS)
    assert abs(a - b) > 1e-3, "the ids must reach the score"


def test_torch_graph_is_the_same_graph(tiny):
    """The yardstick's graph (torch ops) in double meets the restatement as the modules do."""
    import torch
    sd, _ = tiny
    wav = R.synth_wav(5200, 3)
    w = {k: torch.from_numpy(v.astype(np.float64)) for k, v in sd.items()}
    got = R.torch_graph(R.TINY, w, torch.from_numpy(wav.astype(np.float64))[None], 1, 5)
    ref = R.forward(R.TINY, sd, wav, 1, 5)
    for name, a, b in zip(("hidden", "lstm_out", "frames"), ref[:3], got[:3]):
        check_close(f"torch_graph {name}", a, b[0].numpy())
    check_close("torch_graph score", np.array([ref[3]]), got[3].numpy())


def test_reverse_direction_of_a_shorter_row_is_pack_padded_sequence():
    """A batch [T = 9, L = 4] through ``nn.LSTM`` on a packed sequence: the shorter row's reverse direction starts at ITS last frame,
    and the row is the restatement of the row alone; past its frames the padded output is 0."""
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    cfg, sd = R.TINY, R.make_weights(R.TINY, 1)
    rng = np.random.default_rng(5)
    T, L = 9, 4
    feats = rng.standard_normal((2, T, cfg.hidden_size))
    w = {k: torch.from_numpy(v.astype(np.float64)) for k, v in sd.items() if not k.startswith("wav2vec2.")}
    cond = torch.cat([w["domain_embedding.weight"][1], w["judge_embedding.weight"][7]]).expand(2, T, -1)
    x = torch.cat([torch.from_numpy(feats), cond], dim=2)
    with torch.no_grad():
        out, _ = R.torch_lstm(cfg, w)(pack_padded_sequence(x, torch.tensor([T, L]), batch_first=True))
        out, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    out = out.numpy()
    check_close("long row", R.bilstm(cfg, sd, feats[0], 1, 7), out[0])
    check_close("short row", R.bilstm(cfg, sd, feats[1, :L], 1, 7), out[1, :L])
    assert not out[1, L:].any()
    # and it is NOT the padded row's: the reverse direction of the padded row has seen frames L .. T - 1 first
    padded = R.bilstm(cfg, sd, feats[1], 1, 7)[:L, cfg.lstm_hidden:]
    assert np.abs(padded - out[1, :L, cfg.lstm_hidden:]).max() > 1e-3


@pytest.mark.parametrize("name", ["TINY", "TINY_H512"])
def test_make_weights_leaves_the_linear_range(name):
    """At least a quarter of the gate pre-activations lie beyond +-1.5 (sigmoid below 0.18 / above 0.82) in both directions, and the
    frame scores move with the frame."""
    cfg = getattr(R, name)
    sd = R.make_weights(cfg, 0)
    hidden, lo, frames, score = R.forward(cfg, sd, R.synth_wav(5200, 2))
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    for rev in (False, True):
        pre = R.gate_preactivations(cfg, w, hidden, reverse=rev)
        share = float((np.abs(pre) > 1.5).mean())
        print(f"{name} reverse={rev}: {share:.2f} of the gate pre-activations beyond +-1.5, deviation {pre.std():.2f}")
        assert share >= 0.25
    assert frames.std() > 1e-2 and np.isfinite(score)


def test_from_utmos_checkpoint_is_the_inverse_rename():
    from dex_tts_amd import mos
    cfg, sd = R.TINY, R.make_weights(R.TINY, 0)
    up = R.to_utmos_checkpoint(sd)
    assert not set(up) & set(sd)
    assert "feature_extractors.0.ssl_model.feature_extractor.conv_layers.0.2.weight" in up
    assert "feature_extractors.0.ssl_model.encoder.layers.1.self_attn_layer_norm.bias" in up
    assert "feature_extractors.0.ssl_model.encoder.layers.0.fc2.weight" in up and "feature_extractors.0.ssl_model.layer_norm.weight" in up
    assert "feature_extractors.0.ssl_model.encoder.pos_conv.0.weight_g" in up and "output_layers.1.net.3.bias" in up
    z = np.zeros(3, np.float32)
    dropped = {"feature_extractors.0.ssl_model." + k: z for k in ("mask_emb", "quantizer.vars", "quantizer.weight_proj.weight", "project_q.weight",
                                                                 "final_proj.bias")}
    back = mos.from_utmos_checkpoint({**up, **dropped, "some.other.key": z})
    assert "some.other.key" in back                       # survives, for strict loading to report
    assert not any("quantizer" in k or "project_q" in k or "final_proj" in k or "mask_emb" in k for k in back)
    del back["some.other.key"]
    assert list(back) == list(sd) and all(np.array_equal(back[k], sd[k]) for k in sd)
    assert set(back) == set(R.state_dict_shapes(cfg))
    wav = R.synth_wav(720, 8)
    assert R.forward(cfg, back, wav)[3] == R.forward(cfg, sd, wav)[3]


# ---------------------------------------------------------------------------------------------------- host half of mos.py
def test_frame_counts_and_min_samples():
    from dex_tts_amd import mos
    assert mos.num_frames(400) == 1 and mos.num_frames(399) == 0 and mos.num_frames(720) == 2 and mos.num_frames(64000) == 199
    assert mos.min_samples() == 400 and mos.min_samples(R.library_config(R.TINY)) == 400
    for n in (400, 719, 720, 5200, 32080):
        assert mos.num_frames(n, R.library_config(R.TINY)) == R.num_frames(R.TINY, n)


def test_short_rows_are_refused():
    from dex_tts_amd import mos
    with pytest.raises(ValueError, match="too short"):
        mos.check_lengths([32080, 399], 32080)
    assert mos.check_lengths([32080, 400], 32080) == 100
    with pytest.raises(ValueError, match="at most"):
        mos.check_lengths([400], 16000 * 90)


@pytest.mark.parametrize("bad,field", [
    (dict(feat_extract_norm="layer"), "feat_extract_norm"), (dict(do_stable_layer_norm=True), "do_stable_layer_norm"),
    (dict(hidden_act="relu"), "hidden_act"), (dict(feat_extract_activation="gelu_new"), "feat_extract_activation"),
    (dict(num_attention_heads=4), "hidden_size"), (dict(lstm_hidden=96), "lstm_hidden"), (dict(lstm_hidden=576), "lstm_hidden"),
    (dict(proj_hidden=100), "proj_hidden"), (dict(num_judges=0), "num_judges")])
def test_unsupported_configs_name_the_field(bad, field):
    from dex_tts_amd import mos
    with pytest.raises(NotImplementedError, match=field):
        mos.state_dict_shapes(R.library_config(R.variant(R.TINY, **bad)))


def test_state_dict_inventory():
    from dex_tts_amd import mos
    for cfg in (R.TINY, R.TINY_H512, R.DEFAULT, R.variant(R.TINY, conv_bias=True)):
        got = mos.state_dict_shapes(R.library_config(cfg))
        assert got == R.state_dict_shapes(cfg) and list(got) == list(R.state_dict_shapes(cfg))
    shapes = mos.state_dict_shapes()
    assert shapes["decoder_rnn.weight_ih_l0_reverse"] == (2048, 1024) and shapes["judge_embedding.weight"] == (3000, 128)
    assert shapes["projection.3.weight"] == (1, 2048)
