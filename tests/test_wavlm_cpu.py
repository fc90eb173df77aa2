"""CPU: the restatement tests/wavlm_ref.py (which the GPU tests hold the device to) against HF's own ``WavLMForXVector`` in double
precision, the relative-position bucket table, the conditions ``make_weights`` must meet for the tests to see anything, and the
host half of dex_tts_amd/wavlm.py (config refusals, too-short rows, state-dict routing, frame counts, the score's mean and stderr).

tests/golden/wavlm_tiny.npz holds, for the four TINY variants (``use_weighted_layer_sum`` x ``conv_bias``) and the wav
``synth_wav(5520, 31)``, the float64 ``embeddings`` and the layer-mixed hidden states (the projector's input) of
``transformers.WavLMForXVector(config).double()`` (transformers 5.15, eval mode, ``attention_mask=None``, weights
``wavlm_ref.make_weights(variant, 0)``).  It was written by

    python -m tests.test_wavlm_cpu

and holds no weights: they come from the seed.  ``test_restatement_matches_fixture`` needs no transformers; where transformers is
installed ``test_restatement_matches_transformers`` rebuilds the models and checks the restatement against them at two lengths."""
import os

import numpy as np
import pytest

from tests import wavlm_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavlm_tiny.npz")
VARIANTS = [(True, False), (True, True), (False, False), (False, True)]            # (use_weighted_layer_sum, conv_bias)
FIXTURE_WAV = (5520, 31)
CAP = 1e-9                          # of the largest magnitude: catches semantic mistakes; rounding-level agreement is expected


def tiny(weighted, bias):
    return R.variant(R.TINY, use_weighted_layer_sum=weighted, conv_bias=bias)


def hf_outputs(cfg, sd, wav):
    """transformers' WavLMForXVector in double precision on one utterance without a mask -> float64 (mixed hidden [T, H], embeddings).
    The mixed hidden states are what the model itself hands its projector."""
    import torch
    import transformers
    hc = transformers.WavLMConfig(
        hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
        intermediate_size=cfg.intermediate_size, hidden_act="gelu", layer_norm_eps=cfg.layer_norm_eps, feat_extract_norm="group",
        feat_extract_activation="gelu", conv_dim=list(cfg.conv_dim), conv_stride=list(cfg.conv_stride), conv_kernel=list(cfg.conv_kernel),
        conv_bias=cfg.conv_bias, num_conv_pos_embeddings=cfg.num_conv_pos_embeddings,
        num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups, num_buckets=cfg.num_buckets,
        max_bucket_distance=cfg.max_bucket_distance, do_stable_layer_norm=False, apply_spec_augment=False,
        use_weighted_layer_sum=cfg.use_weighted_layer_sum, tdnn_dim=list(cfg.tdnn_dim), tdnn_kernel=list(cfg.tdnn_kernel),
        tdnn_dilation=list(cfg.tdnn_dilation), xvector_output_dim=cfg.xvector_output_dim)
    model = transformers.WavLMForXVector(hc).double().eval()
    own = model.state_dict()
    new = {}
    for k, v in sd.items():
        for a, b in (("weight_g", "parametrizations.weight.original0"), ("weight_v", "parametrizations.weight.original1")):
            if k.endswith(a) and k not in own:
                k = k[: -len(a)] + b
        new[k] = torch.from_numpy(np.asarray(v, np.float64))
    missing, unexpected = model.load_state_dict(new, strict=False)
    assert not unexpected, unexpected
    assert all(m.startswith("classifier.") or m in ("objective.weight", "wavlm.masked_spec_embed") for m in missing), missing
    seen = []
    model.projector.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    with torch.no_grad():
        emb = model(torch.from_numpy(np.asarray(wav, np.float64))[None]).embeddings
    return seen[0][0].numpy(), emb[0].numpy()


def check_close(what, got, want):
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{what}: |restatement - HF| = {err:.2e} at magnitude {scale:.2f}")
    assert got.shape == want.shape
    assert err <= CAP * scale, (what, err, scale)


@pytest.mark.parametrize("weighted,bias", VARIANTS)
def test_restatement_matches_fixture(weighted, bias):
    g = np.load(GOLDEN)
    cfg = tiny(weighted, bias)
    hid, emb = R.forward(cfg, R.make_weights(cfg, 0), R.synth_wav(*FIXTURE_WAV))
    tag = f"w{int(weighted)}b{int(bias)}"
    check_close(f"{tag} hidden", hid, g[tag + "_hidden"])
    check_close(f"{tag} embeddings", emb, g[tag + "_embeddings"])


@pytest.mark.parametrize("weighted,bias", VARIANTS)
def test_restatement_matches_transformers(weighted, bias):
    pytest.importorskip("transformers")
    cfg = tiny(weighted, bias)
    sd = R.make_weights(cfg, 0)
    for n, seed in (FIXTURE_WAV, (32080, 32)):              # 17 frames; 100 frames: the clamped far bucket on both signs
        wav = R.synth_wav(n, seed)
        hid, emb = R.forward(cfg, sd, wav)
        hf_hid, hf_emb = hf_outputs(cfg, sd, wav)
        check_close(f"weighted={weighted} conv_bias={bias} n={n} hidden", hid, hf_hid)
        check_close(f"weighted={weighted} conv_bias={bias} n={n} embeddings", emb, hf_emb)
    far = R.relative_position_buckets(cfg, 100)
    assert far[0] == cfg.num_buckets // 2 - 1 and far[-1] == cfg.num_buckets - 1 and (far == far[0]).sum() > 1 and (far == far[-1]).sum() > 1


def test_do_normalize_is_the_feature_extractors_step():
    """``forward(do_normalize=True)`` is ``forward`` of the normalised wav."""
    from tests import asr_ref
    wav = R.dc_wav(5520, 5)
    sd = R.make_weights(R.TINY, 0)
    a = R.forward(R.TINY, sd, wav, do_normalize=True)
    b = R.forward(R.TINY, sd, asr_ref.normalize_input(wav))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------- the weights the tests use
def test_make_weights_lets_the_tests_see_something():
    """Input sensitivity: in the float64 restatement the embeddings of the GPU tests' wavs differ pairwise by at least 10 % of their
    norm (default-initialised weights gave the same max |e| for every wav).  A non-trivial gate: ``gru_rel_pos_const`` differs per
    head and is not 1, ``rel_attn_embed`` has unit-scale entries, ``layer_weights`` is not uniform."""
    for cfg in (R.TINY, R.WIDE):
        sd = R.make_weights(cfg, 0)
        embs = [R.forward(cfg, sd, R.synth_wav(n, seed))[1] for n, seed in ((32080, 20), (5200, 21), (20880, 22))]
        for i in range(3):
            for j in range(i + 1, 3):
                rel = np.linalg.norm(embs[i] - embs[j]) / max(np.linalg.norm(embs[i]), np.linalg.norm(embs[j]))
                print(f"{cfg.hidden_size}: wavs {i}, {j}: |e_i - e_j| / max |e| = {rel:.3f}")
                assert rel >= 0.10
        for l in range(cfg.num_hidden_layers):
            c = sd[f"{R.ENC}layers.{l}.attention.gru_rel_pos_const"].reshape(-1)
            assert len(set(c.tolist())) == len(c) and (np.abs(c - 1.0) > 0.15).all()
        e = sd[f"{R.ENC}layers.0.attention.rel_attn_embed.weight"]
        assert 0.7 < e.std() < 1.3
        lw = np.exp(sd["layer_weights"].astype(np.float64))
        lw /= lw.sum()
        assert lw.max() / lw.min() > 1.5


def test_dead_relu_channels_exist():
    """Some TDNN channels are 0 on every frame (the device must give their deviation as exactly 0, not NaN); most are not."""
    cfg, sd = R.TINY, R.make_weights(R.TINY, 0)
    hid, emb = R.forward(cfg, sd, R.synth_wav(32080, 20))
    std = R.pooled_statistics(cfg, {k: np.asarray(v, np.float64) for k, v in sd.items()}, hid)[cfg.tdnn_dim[-1]:]
    print(f"TDNN channels: {int((std == 0).sum())} dead of {len(std)}")
    assert (std == 0).any() and (std > 0).sum() >= len(std) // 4 and np.isfinite(emb).all()


# ---------------------------------------------------------------------------------------------------- bucket table
def hf_buckets(cfg, lim):
    import torch
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    att = WavLMAttention(128, 2, num_buckets=cfg.num_buckets, max_distance=cfg.max_bucket_distance)
    return att._relative_positions_bucket(torch.arange(-lim, lim + 1)).numpy()


@pytest.mark.parametrize("name,lim", [("DEFAULT", 4095), ("TINY", 300)])
def test_bucket_table(name, lim):
    """The library's host table and the float64 restatement against the model's own ``_relative_positions_bucket`` (which evaluates
    the logarithm in fp32) at every distance: no mismatch for the defaults at -4095 .. 4095, none for TINY's at -300 .. 300."""
    pytest.importorskip("transformers")
    from dex_tts_amd import wavlm
    cfg = getattr(R, name)
    hf = hf_buckets(cfg, lim)
    lib = wavlm.relative_position_buckets(lim + 1, R.library_config(cfg))
    ref = R.relative_position_buckets(cfg, lim + 1)
    assert lib.dtype == np.int32 and lib.shape == (2 * lim + 1,)
    print(f"{name}: library vs HF {int((lib != hf).sum())} mismatches, float64 formula vs HF fp32 {int((ref != hf).sum())}")
    assert np.array_equal(ref, hf)
    assert np.array_equal(lib, hf)
    nb = cfg.num_buckets // 2
    assert hf[lim] == 0 and hf[lim + 1] == nb + 1 and hf[lim - 1] == 1 and hf[0] == nb - 1 and hf[-1] == 2 * nb - 1


def test_bucket_table_without_transformers():
    """The library's table against the restatement's (itself held to HF above)."""
    from dex_tts_amd import wavlm
    for cfg, n in ((R.DEFAULT, 4096), (R.TINY, 301), (R.TINY, 1)):
        assert np.array_equal(wavlm.relative_position_buckets(n, R.library_config(cfg)), R.relative_position_buckets(cfg, n))
    with pytest.raises(ValueError):
        wavlm.relative_position_buckets(0)


# ---------------------------------------------------------------------------------------------------- host half of wavlm.py
def test_frame_counts():
    from dex_tts_amd import wavlm
    assert wavlm.num_frames(5200) == 16 and wavlm.num_frames(4880) == 15 and wavlm.num_frames(64000) == 199 and wavlm.num_frames(399) == 0
    assert wavlm.min_samples() == 5200
    assert wavlm.min_samples(R.library_config(R.TINY)) == 5200
    short = R.library_config(R.variant(R.TINY, tdnn_kernel=(1, 1, 1, 1, 1)))
    assert wavlm.min_samples(short) == 720 and wavlm.num_frames(720, short) == 2
    for n in (400, 5199, 5200, 5519, 5520, 20880, 32080):
        assert wavlm.num_frames(n, R.library_config(R.TINY)) == R.num_frames(R.TINY, n)
    assert R.tdnn_frames(R.TINY, 16) == 2


def test_short_rows_are_refused():
    """4880 samples are 15 frames, one frame after the TDNN layers: torch's unbiased deviation over it is NaN.  5200 pass."""
    from dex_tts_amd import wavlm
    with pytest.raises(ValueError, match="too short"):
        wavlm.check_lengths([32080, 4880], 32080)
    with pytest.raises(ValueError, match="too short"):
        wavlm.check_lengths([5199], 5199, R.library_config(R.TINY))
    assert wavlm.check_lengths([32080, 5200], 32080) == 100
    with pytest.raises(ValueError, match="at most"):
        wavlm.check_lengths([5200], 16000 * 90)               # 4499 frames
    assert wavlm.check_lengths([16000 * 60], 16000 * 60) == 2999


@pytest.mark.parametrize("bad,field", [
    (dict(feat_extract_norm="layer"), "feat_extract_norm"), (dict(do_stable_layer_norm=True), "do_stable_layer_norm"),
    (dict(num_attention_heads=4), "hidden_size"), (dict(hidden_act="relu"), "hidden_act"),
    (dict(feat_extract_activation="gelu_new"), "feat_extract_activation"),
    (dict(conv_dim=(32,) * 9, conv_kernel=(2,) * 9, conv_stride=(2,) * 9), "conv_dim"),
    (dict(tdnn_dim=(64,) * 9, tdnn_kernel=(1,) * 9, tdnn_dilation=(1,) * 9), "tdnn_dim"),
    (dict(num_conv_pos_embeddings=129), "num_conv_pos_embeddings"), (dict(num_buckets=30), "num_buckets"),
    (dict(xvector_output_dim=40), "xvector_output_dim")])
def test_unsupported_configs_name_the_field(bad, field):
    from dex_tts_amd import wavlm
    with pytest.raises(NotImplementedError, match=field):
        wavlm.state_dict_shapes(R.library_config(R.variant(R.TINY, **bad)))


def test_state_dict_inventory_and_routing():
    import torch
    from dex_tts_amd import wavlm
    for cfg in (R.TINY, R.DEFAULT, tiny(False, True)):
        assert wavlm.state_dict_shapes(R.library_config(cfg)) == R.state_dict_shapes(cfg)
        assert list(wavlm.state_dict_shapes(R.library_config(cfg))) == list(R.state_dict_shapes(cfg))      # and in that order
    assert wavlm.state_dict_shapes() == R.state_dict_shapes(R.DEFAULT)
    want = wavlm.state_dict_shapes(R.library_config(R.TINY))
    sd = {k: torch.from_numpy(v) for k, v in R.make_weights(R.TINY, 0).items()}
    tensors, missing = wavlm.route_state_dict(sd, want)
    assert not missing and set(tensors) == set(want)
    # HF's newer spelling of the weight norm, and the keys the embeddings never read
    new = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): v for k, v in sd.items()}
    new.update({"classifier.weight": torch.zeros(32, 32), "classifier.bias": torch.zeros(32), "objective.weight": torch.zeros(32, 2),
                "wavlm.masked_spec_embed": torch.zeros(128)})
    tensors, missing = wavlm.route_state_dict(new, want)
    assert not missing and set(tensors) == set(want)
    assert torch.equal(tensors[R.ENC + "pos_conv_embed.conv.weight_g"], sd[R.ENC + "pos_conv_embed.conv.weight_g"])
    with pytest.raises(RuntimeError, match="unexpected keys .*lm_head"):
        wavlm.route_state_dict(dict(sd, **{"lm_head.weight": torch.zeros(2, 2)}), want)
    less = dict(sd)
    del less["layer_weights"]
    with pytest.raises(RuntimeError, match="layer_weights"):
        wavlm.route_state_dict(less, want)
    tensors, missing = wavlm.route_state_dict(less, want, strict=False)
    assert missing == ["layer_weights"] and "layer_weights" not in tensors
    with pytest.raises(RuntimeError, match="shape"):
        wavlm.route_state_dict(dict(sd, **{"projector.bias": torch.zeros(63)}), want)


def test_mean_and_stderr_of_given_cosines():
    """The error bar is speaker.asv_score's: numpy's population std over sqrt(n)."""
    import torch
    from dex_tts_amd import wavlm
    cos = [0.9, 0.5, 0.7, 0.1]
    mean, err = wavlm.mean_stderr(torch.tensor(cos))
    assert abs(mean - 0.55) < 1e-7 and abs(err - np.sqrt(np.mean((np.array(cos) - 0.55) ** 2)) / 2.0) < 1e-7
    assert wavlm.mean_stderr(np.array([0.25])) == (0.25, 0.0)


def write_fixture():
    out = {}
    for weighted, bias in VARIANTS:
        cfg = tiny(weighted, bias)
        hid, emb = hf_outputs(cfg, R.make_weights(cfg, 0), R.synth_wav(*FIXTURE_WAV))
        tag = f"w{int(weighted)}b{int(bias)}"
        out[tag + "_hidden"], out[tag + "_embeddings"] = hid, emb
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    write_fixture()
