"""splat_slam_amd.resnetv2 without a GPU: the weight packing against a numpy gather, the standardised fp16 kernels against
mono_depth_ref.prepare, the launch list, the scratch size, the state-dict contract, the backbone switch of MonoDepth and the build of the
kernels for gfx950."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mono_depth_ref as MR
from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def reduced_cfg(**kw):
    from splat_slam_amd.mono_depth import MonoDepthConfig
    base = dict(stem_chs=32, stage_chs=(64, 128, 256), stage_layers=(1, 1, 2), gn_groups=8, dim=128, heads=2, depth=4, taps=(2, 3), pos_grid=4,
                features=32, net_size=(64, 96))
    base.update(kw)
    return MonoDepthConfig(**base)


@pytest.mark.parametrize("cout,cin,k", [(16, 8, 1), (16, 16, 3), (32, 8, 7), (16, 3, 7)])
def test_weight_packing_against_a_numpy_gather(cout, cin, k):
    """[cout][round_up(k * k * cin_pad, 32)], column tap * cin_pad + c, tap = ky * k + kx, zeros elsewhere; 3 channels pad to 8"""
    from splat_slam_amd.resnetv2 import pack_conv
    w = torch.randn(cout, cin, k, k, generator=torch.Generator().manual_seed(cout + cin + k)).to(torch.float16)
    got = pack_conv(w).numpy()
    cin_pad = (cin + 7) // 8 * 8
    k_pad = (k * k * cin_pad + 31) // 32 * 32
    assert got.shape == (cout, k_pad) and got.dtype == np.float16
    assert {(16, 8, 1): 32, (16, 16, 3): 160, (32, 8, 7): 416, (16, 3, 7): 416}[(cout, cin, k)] == k_pad
    want = np.zeros((cout, k_pad), np.float16)
    wn = w.numpy()
    for o in range(cout):
        for ky in range(k):
            for kx in range(k):
                for c in range(cin):
                    want[o, (ky * k + kx) * cin_pad + c] = wn[o, c, ky, kx]
    assert np.array_equal(got, want)


def test_standardise_then_round_matches_the_prepared_reference_bit_for_bit():
    """the module standardises in fp32, the reference in fp64; after the one rounding to fp16 the kernels hold the same bits"""
    from splat_slam_amd import mono_depth as M
    from splat_slam_amd.resnetv2 import standardized_f16
    key = M._BACKBONE + "stages.0.blocks.0.conv2.weight"
    w = M.synthetic_state_dict(5, reduced_cfg())[key]
    assert tuple(w.shape) == (16, 16, 3, 3)
    got = standardized_f16(w)
    assert got.dtype == torch.float16
    assert torch.equal(got.float(), MR.prepare({key: w})[key])


def test_launch_names_have_the_stated_length_and_order():
    from splat_slam_amd.mono_depth import MonoDepthConfig
    from splat_slam_amd.resnetv2 import LAUNCH_NAMES, LAYER_NAMES
    for cfg, want in ((MonoDepthConfig(), 106), (reduced_cfg(), 34), (reduced_cfg(stage_layers=(2, 1, 1)), 34)):
        names = LAUNCH_NAMES(cfg)
        assert len(names) == 4 + sum(6 * n + 2 for n in cfg.stage_layers) == want and len(set(names)) == len(names)
        assert names[:4] == ("pack", "stem.conv", "stem.norm", "pool")
        want_names = []
        for s, n in enumerate(cfg.stage_layers):
            for b in range(n):
                p = f"stages.{s}.blocks.{b}."
                want_names += [p + "conv1", p + "norm1"] + ([p + "downsample.conv", p + "downsample.norm"] if b == 0 else [])
                want_names += [p + "conv2", p + "norm2", p + "conv3", p + "norm3"]
        assert list(names[4:]) == want_names
        layers = LAYER_NAMES(cfg)
        assert len(layers) == 1 + sum(3 * n + 1 for n in cfg.stage_layers)
        assert sorted(layers) == sorted(n for n in names if "conv" in n)           # every convolution is a layer, and nothing else is
    assert LAYER_NAMES(reduced_cfg())[:5] == ("stem.conv", "stages.0.blocks.0.conv1", "stages.0.blocks.0.conv2", "stages.0.blocks.0.conv3",
                                              "stages.0.blocks.0.downsample.conv")


def test_scratch_bytes_is_pure_and_grows_with_the_sizes():
    from splat_slam_amd import _native as nat
    f = nat.lib().sgr_resnet_scratch_bytes
    ok = (64, 256, 512, 1024)
    for bad in ((0, 32, 32) + ok, (1, 0, 32) + ok, (1, 40, 64) + ok, (1, 64, 48) + ok, (65536, 32, 32) + ok, (1, 32, 32, 8, 64, 128, 256),
                (1, 32, 32, 24, 64, 128, 256), (1, 32, 32, 32, 48, 128, 256), (1, 32, 32, 32, 64, 128, 2048), (1, -32, 32) + ok):
        assert f(*bad) == 0, bad
    for n, H, W, widths in ((1, 32, 32, (32, 64, 128, 256)), (2, 64, 96, (32, 64, 128, 256)), (1, 512, 512, ok), (3, 480, 640, ok)):
        size = f(n, H, W, *widths)
        assert size > 0 and size % 16 == 0 and f(n, H, W, *widths) == size
        assert f(n + 1, H, W, *widths) > size and f(n, H + 32, W, *widths) > size and f(n, H, W + 32, *widths) > size
        stem, c0 = widths[0], widths[1]
        # the packed image, four activation buffers and the fp32 sums of the largest map (the stem's, or stage 0's at a quarter of it)
        largest = n * max((H // 2) * (W // 2) * stem, (H // 4) * (W // 4) * max(stem, c0))
        assert size >= n * H * W * 8 * 2 + largest * (4 * 2 + 4)


def test_state_dict_validation():
    from splat_slam_amd import mono_depth as M
    from splat_slam_amd import resnetv2 as R
    cfg = M.MonoDepthConfig()
    shapes = R.backbone_shapes(cfg)
    assert len(shapes) == 52 * 3 and all(k.startswith(M._BACKBONE) for k in shapes)              # 52 kernels, 52 scales, 52 biases
    assert shapes == {k: v for k, v in M.state_shapes(cfg).items() if "patch_embed.backbone." in k}
    sd = {k: torch.empty(s, device="meta") for k, s in shapes.items()}
    assert list(R.normalize_state_dict(sd, cfg)) == list(shapes)
    lacking = dict(sd)
    del lacking[M._BACKBONE + "stages.2.blocks.8.norm3.bias"]
    with pytest.raises(ValueError, match="lacks"):
        R.normalize_state_dict(lacking, cfg)
    with pytest.raises(ValueError, match="unexpected"):
        R.normalize_state_dict(dict(sd, **{"pretrained.model.patch_embed.proj.weight": torch.empty(768, 1024, 1, 1, device="meta")}), cfg)
    with pytest.raises(ValueError, match="shape"):
        R.normalize_state_dict(dict(sd, **{M._BACKBONE + "stem.conv.weight": torch.empty(64, 3, 3, 3, device="meta")}), cfg)
    with pytest.raises(ValueError, match="per group"):                                          # 3 channels per group
        R.normalize_state_dict({}, reduced_cfg(stem_chs=48, stage_chs=(192, 384, 768), gn_groups=16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.ResNetV2({k: torch.zeros(s) for k, s in R.backbone_shapes(reduced_cfg()).items()}, reduced_cfg(), "cpu")


def test_an_unknown_backbone_raises_before_any_device_is_touched():
    from splat_slam_amd.mono_depth import MonoDepth
    with pytest.raises(ValueError, match="backbone"):
        MonoDepth({}, reduced_cfg(), "cuda", backbone="nonsense")
    with pytest.raises(ValueError, match="backbone"):
        MonoDepth.synthetic(1, reduced_cfg(), backbone="HIP")
    with pytest.raises(ValueError, match="backbone"):
        MonoDepth.from_state_dict({}, reduced_cfg(), backbone=None)


# kernel -> the VGPR count of its gfx950 code object when it was written, as a ceiling
VGPR_CEILING = {"resnet_conv_kernelILi1ELi16E": 52, "resnet_conv_kernelILi3ELi16E": 52, "resnet_conv_kernelILi7ELi16E": 52,
                "resnet_conv_kernelILi1ELi32E": 68, "resnet_conv_kernelILi3ELi32E": 64, "resnet_conv_kernelILi7ELi32E": 64,
                "resnet_conv_kernelILi1ELi64E": 88, "resnet_conv_kernelILi3ELi64E": 88, "resnet_conv_kernelILi7ELi64E": 88,
                "resnet_norm_kernel": 50, "resnet_stats_kernel": 12, "resnet_pool_kernel": 30}


def test_resnet_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """every kernel keeps its state in registers: no private segment, no spills (read from the code object's metadata)"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "resnet.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_resnet.hip")], check=True, capture_output=True)
    text = open(out).read()
    assert "v_mfma_f32_16x16x32_f16" in text
    seen = set()
    for block in text.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        key = next((k for k in VGPR_CEILING if name and k in name.group(1)), None)
        if key is None:
            continue
        seen.add(key)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        print(key, "vgpr", vgpr)
        assert scratch == 0 and spill == 0 and vgpr <= VGPR_CEILING[key], (key, vgpr, spill, scratch)
    assert seen == set(VGPR_CEILING)


def test_a_group_never_spans_two_channel_tiles():
    """The convolution folds the per-channel sums red[.][wave][0 .. BN) of its own channel tile into groups, so every group must lie
    inside one tile.  The launch takes the widest of 64 / 32 / 16 that divides cout; for every (cout, groups) the kernels accept (cout a
    multiple of 16 up to 1024, at most 256 groups, a power of two of at most 64 channels per group) the group size divides that tile."""
    checked = 0
    for cout in range(16, 1025, 16):
        bn = 64 if cout % 64 == 0 else 32 if cout % 32 == 0 else 16
        for groups in range(1, 257):
            cpg = cout // groups
            if cout % groups or cpg > 64 or cpg & (cpg - 1):
                continue
            checked += 1
            assert bn % cpg == 0, (cout, groups, bn)
            for g in range(groups):
                assert g * cpg // bn == ((g + 1) * cpg - 1) // bn, (cout, groups, g)
    assert checked >= 3 * 64                    # 4, 8 and 16 channels per group fit every one of the 64 widths
