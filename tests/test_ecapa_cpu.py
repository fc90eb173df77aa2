"""CPU: the restatement tests/ecapa_ref.py (which the GPU tests hold the device to) against ``transformers.WavLMModel`` (every hidden
state of the large family at TINY) and against a ``torch.nn`` transcription of the ECAPA-TDNN head (``Conv1d``, ``BatchNorm1d`` with
non-trivial running statistics, ``InstanceNorm1d``, both values of ``global_context_att``), both in double precision; and the host
half of dex_tts_amd/ecapa.py: the inventory and its order, state-dict routing, the rename of the fine-tuned checkpoint, config
refusals, frame counts, the C symbols.  The bound of a restatement against modules is the project's: 1e-9 of the largest magnitude."""
import re

import numpy as np
import pytest
import torch
from torch import nn

from tests import ecapa_ref as R

CAP = 1e-9
N_FIXTURE = (5520, 31)              # 17 frames


def check_close(what, got, want):
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{what}: |restatement - modules| = {err:.2e} at magnitude {scale:.2f}")
    assert got.shape == want.shape
    assert err <= CAP * scale, (what, err, scale)


def f64(sd):
    return {k: np.asarray(v, np.float64) for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------------- the trunk against transformers
def hf_hidden_states(cfg, sd, wav):
    pytest.importorskip("transformers")
    model = R.hf_wavlm_model(cfg, sd, torch.float64)
    with torch.no_grad():
        out = model(torch.from_numpy(np.asarray(wav, np.float64))[None], output_hidden_states=True)
    return [h[0].numpy() for h in out.hidden_states]


@pytest.mark.parametrize("n,seed", [N_FIXTURE, (32080, 32)])
def test_trunk_matches_transformers(n, seed):
    """Every one of the L + 1 hidden states of ``WavLMModel(output_hidden_states=True)`` at TINY; 100 frames reach the clamped far
    bucket on both signs."""
    cfg, sd = R.TINY, R.make_weights(R.TINY, 0)
    wav = R.normalize_wav(R.synth_wav(n, seed))
    ours = R.trunk_hidden_states(cfg, f64(sd), wav)
    hf = hf_hidden_states(cfg, sd, wav)
    assert len(ours) == len(hf) == cfg.num_hidden_layers + 1
    for l, (a, b) in enumerate(zip(ours, hf)):
        check_close(f"n={n} hidden state {l}", a, b)


# ---------------------------------------------------------------------------------------------------- the head against torch.nn modules
class Conv1dReluBn(nn.Module):
    def __init__(self, cin, cout, k=1, pad=0, dil=1):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, k, 1, pad, dil)
        self.bn = nn.BatchNorm1d(cout)

    def forward(self, x):
        return self.bn(torch.relu(self.conv(x)))


class Res2Conv1dReluBn(nn.Module):
    def __init__(self, channels, k, pad, dil, scale):
        super().__init__()
        self.scale, self.width = scale, channels // scale
        self.nums = scale - 1
        self.convs = nn.ModuleList([nn.Conv1d(self.width, self.width, k, 1, pad, dil) for _ in range(self.nums)])
        self.bns = nn.ModuleList([nn.BatchNorm1d(self.width) for _ in range(self.nums)])

    def forward(self, x):
        out, spx, sp = [], torch.split(x, self.width, 1), None
        for i in range(self.nums):
            sp = spx[i] if i == 0 else sp + spx[i]
            sp = self.bns[i](torch.relu(self.convs[i](sp)))
            out.append(sp)
        out.append(spx[self.nums])
        return torch.cat(out, dim=1)


class SE_Connect(nn.Module):
    def __init__(self, channels, s):
        super().__init__()
        self.linear1, self.linear2 = nn.Linear(channels, s), nn.Linear(s, channels)

    def forward(self, x):
        out = torch.sigmoid(self.linear2(torch.relu(self.linear1(x.mean(dim=2)))))
        return x * out.unsqueeze(2)


class SE_Res2Block(nn.Module):
    def __init__(self, channels, dil, scale, s):
        super().__init__()
        self.Conv1dReluBn1 = Conv1dReluBn(channels, channels)
        self.Res2Conv1dReluBn = Res2Conv1dReluBn(channels, 3, dil, dil, scale)
        self.Conv1dReluBn2 = Conv1dReluBn(channels, channels)
        self.SE_Connect = SE_Connect(channels, s)

    def forward(self, x):
        return self.SE_Connect(self.Conv1dReluBn2(self.Res2Conv1dReluBn(self.Conv1dReluBn1(x)))) + x


class AttentiveStatsPool(nn.Module):
    def __init__(self, dim, att, gc):
        super().__init__()
        self.gc = gc
        self.linear1 = nn.Conv1d(dim * 3 if gc else dim, att, 1)
        self.linear2 = nn.Conv1d(att, dim, 1)

    def forward(self, x):
        x_in = x
        if self.gc:
            cm = torch.mean(x, dim=-1, keepdim=True).expand_as(x)
            cs = torch.sqrt(torch.var(x, dim=-1, keepdim=True) + 1e-10).expand_as(x)
            x_in = torch.cat((x, cm, cs), dim=1)
        alpha = torch.softmax(self.linear2(torch.tanh(self.linear1(x_in))), dim=2)
        mean = torch.sum(alpha * x, dim=2)
        std = torch.sqrt((torch.sum(alpha * x ** 2, dim=2) - mean ** 2).clamp(min=1e-9))
        return torch.cat([mean, std], dim=1)


class EcapaTdnn(nn.Module):
    """The head as modules: the registration order of its parameters and buffers is the order of the library's inventory."""

    def __init__(self, cfg):
        super().__init__()
        C = cfg.channels
        self.feature_weight = nn.Parameter(torch.zeros(cfg.num_hidden_layers + 1))
        self.instance_norm = nn.InstanceNorm1d(cfg.hidden_size)
        self.layer1 = Conv1dReluBn(cfg.hidden_size, C, 5, 2)
        self.layer2 = SE_Res2Block(C, cfg.dilations[0], cfg.res2_scale, cfg.se_bottleneck_dim)
        self.layer3 = SE_Res2Block(C, cfg.dilations[1], cfg.res2_scale, cfg.se_bottleneck_dim)
        self.layer4 = SE_Res2Block(C, cfg.dilations[2], cfg.res2_scale, cfg.se_bottleneck_dim)
        self.conv = nn.Conv1d(3 * C, 3 * C, 1)
        self.pooling = AttentiveStatsPool(3 * C, cfg.attention_channels, cfg.global_context_att)
        self.bn = nn.BatchNorm1d(6 * C)
        self.linear = nn.Linear(6 * C, cfg.emb_dim)

    def forward(self, hidden):                              # [L + 1, B, T, H]
        w = torch.softmax(self.feature_weight, dim=-1)
        x = (w[:, None, None, None] * hidden).sum(dim=0).transpose(1, 2) + 1e-6
        x = self.instance_norm(x)
        out1 = self.layer1(x)
        out2 = self.layer2(out1)
        out3 = self.layer3(out2)
        out4 = self.layer4(out3)
        out = torch.relu(self.conv(torch.cat([out2, out3, out4], dim=1)))
        return x.transpose(1, 2), self.linear(self.bn(self.pooling(out)))


def head_keys(sd):
    return [k for k in sd if not k.startswith("wavlm.")]


@pytest.mark.parametrize("name", ["TINY", "TINY_GC", "WIDE"])
def test_head_matches_torch_modules(name):
    cfg = getattr(R, name)
    sd = R.make_weights(cfg, 0)
    model = EcapaTdnn(cfg).double().eval()
    own = [k for k in model.state_dict() if not k.endswith("num_batches_tracked")]
    assert own == head_keys(sd), "the modules' keys, in their order, are the head's inventory"
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.asarray(sd[k], np.float64)) for k in head_keys(sd)}, strict=False)
    assert not unexpected and all(m.endswith("num_batches_tracked") for m in missing)
    rng = np.random.default_rng(5)
    T = 37
    hidden = [rng.standard_normal((T, cfg.hidden_size)) * (1.0 + l) for l in range(cfg.num_hidden_layers + 1)]
    w = f64(sd)
    x = R.instance_normed_mix(cfg, w, hidden)
    emb = R.head(cfg, w, x)
    with torch.no_grad():
        tx, temb = model(torch.from_numpy(np.stack(hidden))[:, None])
    check_close(f"{name} instance-normed mix", x, tx[0].numpy())
    check_close(f"{name} embedding", emb, temb[0].numpy())
    # the same graph in functional ops (the GPU tests' yardstick, the bench) in double
    tw = {k: torch.from_numpy(v) for k, v in w.items()}
    with torch.no_grad():
        fx, femb = R.torch_head(cfg, tw, [torch.from_numpy(h)[None] for h in hidden])
    check_close(f"{name} torch_head mix", x, fx[0].numpy())
    check_close(f"{name} torch_head embedding", emb, femb[0].numpy())
    # the Res2 chain alone
    xr = rng.standard_normal((T, cfg.channels))
    blockm = model.layer3.Res2Conv1dReluBn
    with torch.no_grad():
        want = blockm(torch.from_numpy(xr).T[None])[0].T.numpy()
    check_close(f"{name} res2", R.res2(cfg, sd, 1, xr), want)
    assert np.array_equal(R.res2(cfg, sd, 1, xr)[:, -cfg.channels // 8:], xr[:, -cfg.channels // 8:])


def test_whole_restatement_is_its_parts_and_the_torch_graph():
    """``forward`` = trunk + mix + head; ``torch_graph`` in double agrees with it; ``do_normalize`` is the eps 1e-5 layer norm."""
    cfg, sd = R.TINY, R.make_weights(R.TINY, 0)
    wav = R.dc_wav(*N_FIXTURE, dc=0.05, amp=0.1)
    hid, emb = R.forward(cfg, sd, wav)
    tw = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in sd.items()}
    thid, temb = R.torch_graph(cfg, tw, torch.from_numpy(np.asarray(wav, np.float64))[None])
    check_close("torch_graph mix", hid, thid[0].numpy())
    check_close("torch_graph embedding", emb, temb[0].numpy())
    a = R.forward(cfg, sd, R.normalize_wav(wav), do_normalize=False)
    assert np.array_equal(a[0], hid) and np.array_equal(a[1], emb)
    x = np.asarray(wav, np.float64)
    assert np.array_equal(R.normalize_wav(wav), (x - x.mean()) / np.sqrt(x.var() + 1e-5))


def test_make_weights_lets_the_tests_see_something():
    """Embeddings move with the input; some channels before the pooling are dead on every frame (pooled deviation exactly
    sqrt(1e-9)), most are not; the pooling's softmax is far from uniform; the fp32 yardstick x 8 is no vacuous bound at TINY."""
    for cfg in (R.TINY, R.WIDE):
        sd = R.make_weights(cfg, 0)
        w = f64(sd)
        embs, devs = [], []
        for n, seed in ((32080, 20), (720, 21), (20880, 22)):
            hid, emb = R.forward(cfg, sd, R.synth_wav(n, seed))
            embs.append(emb)
            devs.append(R.pooled(cfg, w, hid)[3 * cfg.channels:])
        for i in range(3):
            for j in range(i + 1, 3):
                rel = np.linalg.norm(embs[i] - embs[j]) / max(np.linalg.norm(embs[i]), np.linalg.norm(embs[j]))
                print(f"{cfg.hidden_size}: wavs {i}, {j}: |e_i - e_j| / max |e| = {rel:.3f}")
                assert rel >= 0.10
        dead = devs[0] == np.sqrt(1e-9)
        print(f"{cfg.hidden_size}: {int(dead.sum())} dead channels of {dead.size} before the pooling")
        assert dead.any() and (~dead).sum() >= dead.size // 4
    cfg, sd = R.TINY, R.make_weights(R.TINY, 0)
    wav = R.synth_wav(32080, 20)
    ref, yard = R.forward(cfg, sd, wav), R.torch_forward_fp32(cfg, sd, wav)
    for what, a, b in (("mix", yard[0], ref[0]), ("embedding", yard[1], ref[1])):
        tol, d = R.tolerance(a, b)
        print(f"TINY {what}: fp32 yardstick {d:.3e}, bound {tol:.3e}, magnitude {np.abs(b).max():.2f}")
        assert tol < 1e-3 * np.abs(b).max()


# ---------------------------------------------------------------------------------------------------- host half of ecapa.py
def test_frame_counts():
    from dex_tts_amd import ecapa
    assert ecapa.num_frames(720) == 2 and ecapa.num_frames(719) == 1 and ecapa.num_frames(64000) == 199 and ecapa.num_frames(399) == 0
    assert ecapa.min_samples() == 720 == R.min_samples(R.DEFAULT)
    odd = R.variant(R.TINY, conv_kernel=(10, 3, 3, 3, 3, 2, 3), conv_stride=(5, 2, 2, 2, 2, 2, 1))
    assert ecapa.min_samples(R.library_config(odd)) == R.min_samples(odd)
    for n in (400, 719, 720, 1039, 1040, 20880, 32080):
        assert ecapa.num_frames(n, R.library_config(R.TINY)) == R.num_frames(R.TINY, n)
        assert ecapa.num_frames(n, R.library_config(odd)) == R.num_frames(odd, n)
    with pytest.raises(ValueError, match="too short"):
        ecapa.check_lengths([32080, 719], 32080)
    assert ecapa.check_lengths([32080, 720], 32080) == 100
    with pytest.raises(ValueError, match="at most"):
        ecapa.check_lengths([720], 16000 * 90)
    assert ecapa.RES2_TILE == 72 and ecapa.MAX_FRAMES == 4096


@pytest.mark.parametrize("bad,field", [
    (dict(feat_extract_norm="group"), "feat_extract_norm"), (dict(do_stable_layer_norm=False), "do_stable_layer_norm"),
    (dict(num_attention_heads=4), "hidden_size"), (dict(hidden_act="relu"), "hidden_act"),
    (dict(num_buckets=30), "num_buckets"), (dict(channels=384), "channels / scale"), (dict(channels=512, res2_scale=4), "channels / scale"),
    (dict(channels=128, res2_scale=4), "res2_scale"), (dict(emb_dim=40), "emb_dim"), (dict(se_bottleneck_dim=300), "se_bottleneck_dim"),
    (dict(attention_channels=48), "attention_channels"), (dict(dilations=(2, 3, 5)), "dilations"), (dict(dilations=(2, 3)), "dilations")])
def test_unsupported_configs_name_the_field(bad, field):
    from dex_tts_amd import ecapa
    with pytest.raises(NotImplementedError, match=re.escape(field)):
        ecapa.state_dict_shapes(R.library_config(R.variant(R.TINY, **bad)))


def test_wavlm_create_still_refuses_the_large_family():
    from dex_tts_amd import wavlm
    with pytest.raises(NotImplementedError, match="feat_extract_norm"):
        wavlm.state_dict_shapes(wavlm.WavLMConfig(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, hidden_size=1024,
                                                  num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096))


def test_state_dict_inventory_and_routing():
    from dex_tts_amd import ecapa
    for cfg in (R.TINY, R.DEFAULT, R.TINY_GC, R.variant(R.TINY, conv_bias=False)):
        assert ecapa.state_dict_shapes(R.library_config(cfg)) == R.state_dict_shapes(cfg)
        assert list(ecapa.state_dict_shapes(R.library_config(cfg))) == list(R.state_dict_shapes(cfg))      # and in that order
    assert ecapa.state_dict_shapes() == R.state_dict_shapes(R.DEFAULT)
    want = ecapa.state_dict_shapes(R.library_config(R.TINY))
    sd = {k: torch.from_numpy(v) for k, v in R.make_weights(R.TINY, 0).items()}
    tensors, missing = ecapa.route_state_dict(sd, want)
    assert not missing and set(tensors) == set(want)
    new = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): v for k, v in sd.items()}
    new.update({"wavlm.masked_spec_embed": torch.zeros(128), "layer1.bn.num_batches_tracked": torch.tensor(7),
                "layer3.Res2Conv1dReluBn.bns.4.num_batches_tracked": torch.tensor(7), "bn.num_batches_tracked": torch.tensor(7)})
    tensors, missing = ecapa.route_state_dict(new, want)
    assert not missing and set(tensors) == set(want)
    with pytest.raises(RuntimeError, match="unexpected keys .*loss_calculator"):
        ecapa.route_state_dict(dict(sd, **{"loss_calculator.projection.weight": torch.zeros(2, 2)}), want)
    less = dict(sd)
    del less["feature_weight"]
    with pytest.raises(RuntimeError, match="missing keys .*feature_weight"):
        ecapa.route_state_dict(less, want)
    tensors, missing = ecapa.route_state_dict(less, want, strict=False)
    assert missing == ["feature_weight"] and "feature_weight" not in tensors
    with pytest.raises(RuntimeError, match="layer2.SE_Connect.linear1.bias: expected shape"):
        ecapa.route_state_dict(dict(sd, **{"layer2.SE_Connect.linear1.bias": torch.zeros(33)}), want)


def hf_to_fairseq(k):
    """The inverse of the rename, written out independently: an HF ``WavLMModel`` key (without ``wavlm.``) -> fairseq's."""
    m = re.match(r"feature_extractor\.conv_layers\.(\d+)\.(conv|layer_norm)\.(\w+)$", k)
    if m:
        return f"feature_extractor.conv_layers.{m[1]}." + ("0." if m[2] == "conv" else "2.1.") + m[3]
    for a, b in (("feature_projection.layer_norm.", "layer_norm."), ("feature_projection.projection.", "post_extract_proj."),
                 ("encoder.pos_conv_embed.conv.", "encoder.pos_conv.0.")):
        if k.startswith(a):
            return b + k[len(a):]
    m = re.match(r"(encoder\.layers\.\d+\.)(.*)$", k)
    if m:
        rest = m[2]
        for a, b in (("attention.gru_rel_pos_linear.", "self_attn.grep_linear."), ("attention.gru_rel_pos_const", "self_attn.grep_a"),
                     ("attention.rel_attn_embed.", "self_attn.relative_attention_bias."), ("attention.", "self_attn."),
                     ("feed_forward.intermediate_dense.", "fc1."), ("feed_forward.output_dense.", "fc2.")):
            if rest.startswith(a):
                return m[1] + b + rest[len(a):]
        if rest.startswith("layer_norm."):
            return m[1] + "self_attn_layer_norm." + rest[len("layer_norm."):]
        return k
    return k


def test_from_unispeech_checkpoint_round_trip():
    """Rename back and forth: every key of the fine-tuned checkpoint's spelling is consumed, what comes out is the inventory with its
    shapes, and the keys the embeddings never read are dropped."""
    from dex_tts_amd import ecapa
    want = ecapa.state_dict_shapes(R.library_config(R.TINY))
    sd = R.make_weights(R.TINY, 0)
    up = {}
    for k, v in sd.items():
        up["feature_extract.model." + hf_to_fairseq(k[len("wavlm."):]) if k.startswith("wavlm.") else k] = v
    assert "feature_extract.model.encoder.layers.1.self_attn.grep_a" in up and "feature_extract.model.feature_extractor.conv_layers.3.2.1.weight" in up
    assert "feature_extract.model.encoder.layers.0.self_attn.relative_attention_bias.weight" in up and "feature_extract.model.layer_norm.bias" in up
    assert "feature_extract.model.encoder.layer_norm.weight" in up and "feature_extract.model.encoder.layers.0.final_layer_norm.bias" in up
    up.update({"feature_extract.model.mask_emb": np.zeros(128, np.float32), "feature_extract.model.label_embs_concat": np.zeros((4, 8), np.float32),
               "feature_extract.model.final_proj.weight": np.zeros((8, 128), np.float32), "layer1.bn.num_batches_tracked": np.int64(3)})
    for nested in (up, {"model": up}):
        back = ecapa.from_unispeech_checkpoint(nested)
        tensors, missing = ecapa.route_state_dict(back, want)
        assert not missing and list(tensors) == list(want)
        assert {k: tuple(v.shape) for k, v in tensors.items()} == want
        assert all(np.array_equal(tensors[k].numpy(), sd[k]) for k in want)
    # a key the rename does not know stays, for strict mode to report
    odd = ecapa.from_unispeech_checkpoint(dict(up, **{"feature_extract.model.encoder.layers.0.self_attn.bias_k": np.zeros(3, np.float32)}))
    with pytest.raises(RuntimeError, match="unexpected keys .*bias_k"):
        ecapa.route_state_dict(odd, want)


def test_new_symbols_load():
    import ctypes as C
    from dex_tts_amd import _lib, ecapa
    lib = _lib.load()
    for name in ("create", "destroy", "last_error", "load", "finalize", "num_weights", "weight_info", "num_frames", "min_samples",
                 "workspace_bytes", "hidden", "embed", "res2"):
        assert getattr(lib, "dex_ecapa_" + name) is not None
    assert lib.dex_ecapa_num_frames(None, 64000) == 199 and lib.dex_ecapa_min_samples(None) == 720
    h = C.c_void_p()
    bad = ecapa._c_config(ecapa.EcapaConfig())
    bad.channels = 384
    assert lib.dex_ecapa_create(C.byref(bad), C.byref(h)) == -1 and not h.value
    assert b"channels / scale" in lib.dex_ecapa_last_error(None)
    assert lib.dex_ecapa_workspace_bytes(None, 1, 16000) == 0
    with pytest.raises(ValueError, match="MI355X only"):
        ecapa.WavLMEcapa(device="cpu")
