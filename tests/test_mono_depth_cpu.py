"""splat_slam_amd.mono_depth and splat_slam_amd.vit without a GPU: the state-dict contract on meta tensors, the closed forms of the
backbone, the synthetic weights, the scratch size and the fp64 attention statement the GPU tests measure against."""
import math

import numpy as np
import pytest
import torch

import vit_ref as R


def full_meta():
    from splat_slam_amd import mono_depth as M
    cfg = M.MonoDepthConfig()
    return M, cfg, {k: torch.empty(s, device="meta") for k, s in M.state_shapes(cfg).items()}


def test_check_state_dict_on_meta_tensors_of_the_default_network():
    M, cfg, sd = full_meta()
    assert cfg.stage_chs == (256, 512, 1024) and cfg.stage_layers == (3, 4, 9) and cfg.net_size == (512, 512) and cfg.taps == (8, 11)
    for key in ("pretrained.model.patch_embed.backbone.stages.2.blocks.8.conv3.weight", "pretrained.model.patch_embed.proj.weight",
                "pretrained.model.blocks.11.mlp.fc2.bias", "pretrained.act_postprocess4.4.bias", "pretrained.act_postprocess3.0.project.0.weight",
                "scratch.layer4_rn.weight", "scratch.refinenet1.resConfUnit1.conv2.bias", "scratch.output_conv.4.weight"):
        assert key in sd, key
    assert tuple(sd["pretrained.model.pos_embed"].shape) == (1, 577, 768) and "scratch.layer1_rn.bias" not in sd
    M.check_state_dict(sd, cfg)
    M.check_state_dict({"state_dict": {"model." + k: v for k, v in sd.items()}}, cfg)      # the wrapper and its 6-character prefix
    extra = dict(sd)
    extra["pretrained.model.head.weight"] = torch.empty(1000, 768, device="meta")
    extra["pretrained.model.head.bias"] = torch.empty(1000, device="meta")
    extra["pretrained.model.norm.weight"] = torch.empty(768, device="meta")
    extra["scratch.refinenet4.resConfUnit1.conv1.weight"] = torch.empty(256, 256, 3, 3, device="meta")
    M.check_state_dict(extra, cfg)
    lacking = dict(sd)
    del lacking["scratch.refinenet4.resConfUnit2.conv1.bias"]
    with pytest.raises(ValueError, match="lacks"):
        M.check_state_dict(lacking, cfg)
    with pytest.raises(ValueError, match="unexpected"):
        M.check_state_dict(dict(sd, **{"scratch.refinenet5.out_conv.weight": torch.empty(1, device="meta")}), cfg)
    with pytest.raises(ValueError, match="shape"):
        M.check_state_dict(dict(sd, **{"pretrained.model.blocks.3.attn.qkv.weight": torch.empty(2304, 767, device="meta")}), cfg)


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("i", [1, 2, 7, 8])
def test_same_padding_amounts(i, k, s):
    from splat_slam_amd.mono_depth import same_pad
    total = max((math.ceil(i / s) - 1) * s + k - i, 0)
    before, after = same_pad(i, k, s)
    assert (before, after) == (total // 2, total - total // 2) and after - before in (0, 1)
    assert (i + before + after - k) // s + 1 == math.ceil(i / s)              # the output has ceil(i / s) elements


def test_weight_standardisation_against_numpy():
    from splat_slam_amd.mono_depth import standardize
    w = torch.randn(6, 5, 3, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 3 + 1
    a = w.numpy().reshape(6, -1)
    ref = ((a - a.mean(1, keepdims=True)) / np.sqrt(a.var(1, keepdims=True) + 1e-8)).reshape(w.shape)
    np.testing.assert_allclose(standardize(w).numpy(), ref, rtol=1e-12, atol=1e-12)
    flat = torch.full((2, 4, 1, 1), 0.5, dtype=torch.float64)
    assert (standardize(flat) == 0).all()                                      # eps keeps a constant kernel finite


def test_position_resize_is_the_identity_at_the_native_grid():
    from splat_slam_amd.vit import resize_pos_embed
    pos = torch.randn(1, 1 + 24 * 24, 16, generator=torch.Generator().manual_seed(2))
    assert torch.equal(resize_pos_embed(pos, 24, 24, 24), pos[0])
    out = resize_pos_embed(pos, 24, 32, 20)
    assert tuple(out.shape) == (1 + 32 * 20, 16) and torch.equal(out[0], pos[0, 0])
    assert torch.equal(out, R.resize_pos_ref(pos, 24, 32, 20))


def test_synthetic_weights_reproduce_from_seed_and_name():
    from splat_slam_amd import mono_depth as M
    from splat_slam_amd import vit as V
    from splat_slam_amd.update_op import _hash_uniform
    for name, n, seed in (("a.weight", 1000, 0), ("pretrained.model.pos_embed", 4097, 7), ("x", 3, 2 ** 31 + 5)):
        assert np.array_equal(V.hash_uniform(name, n, seed).numpy(), _hash_uniform(name, n, seed))
    cfg = M.MonoDepthConfig(stem_chs=32, stage_chs=(64, 128, 256), stage_layers=(1, 1, 2), gn_groups=8, dim=128, heads=2, depth=4, taps=(2, 3),
                            pos_grid=4, features=32, net_size=(64, 96))
    a, b, c = M.synthetic_state_dict(5, cfg), M.synthetic_state_dict(5, cfg), M.synthetic_state_dict(6, cfg)
    assert list(a) == list(M.state_shapes(cfg)) and all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["scratch.layer1_rn.weight"], c["scratch.layer1_rn.weight"])
    key = "pretrained.model.blocks.1.attn.qkv.weight"
    want = (_hash_uniform(key, 384 * 128, 5) / math.sqrt(128)).astype(np.float32).reshape(384, 128)
    assert np.array_equal(a[key].numpy(), want)
    assert torch.equal(V.synthetic_state_dict(5, cfg.vit())[key[len("pretrained."):]], V.synthetic_tensor(key[len("pretrained."):], (384, 128), 5, 1 / math.sqrt(128)))
    M.check_state_dict(a, cfg)
    assert set(M.normalize_state_dict(a, cfg)) == set(a)


def test_scratch_bytes_is_a_pure_monotone_function():
    from splat_slam_amd import _native as nat
    f = nat.lib().sgr_vit_scratch_bytes
    assert f(1, 1025, 0, 12) == 0 and f(1, 1025, 17, 12) == 0 and f(1, 1, 12, 12) == 0 and f(0, 5, 12, 12) == 0 and f(1, 5, 12, 0) == 0
    assert f(2 ** 21, 1025, 12, 12) == 0                                       # B * T beyond int32
    for B, T, heads in ((1, 2, 1), (1, 1025, 12), (3, 65, 2), (2, 577, 16)):
        n = f(B, T, heads, 12)
        assert n > 0 and n % 16 == 0 and f(B + 1, T, heads, 12) > n and f(B, T + 1, heads, 12) > n
        D = 64 * heads
        assert n >= B * T * D * (4 + 2 + 6 + 2 + 8 + 4)                       # stream, normalised row, qkv, attention, hidden, two taps


def test_attention_reference_against_explicit_loops():
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(2, 3, 3, 2, 64, generator=g, dtype=torch.float64)
    got = R.attention_ref(qkv)
    for b in range(2):
        for h in range(2):
            for i in range(3):
                s = [sum(float(qkv[b, i, 0, h, d] * qkv[b, j, 1, h, d]) for d in range(64)) / 8.0 for j in range(3)]
                e = [math.exp(v - max(s)) for v in s]
                for d in range(64):
                    want = sum(e[j] * float(qkv[b, j, 2, h, d]) for j in range(3)) / sum(e)
                    assert abs(float(got[b, i, h * 64 + d]) - want) < 1e-12
