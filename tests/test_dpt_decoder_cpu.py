"""splat_slam_amd.dpt_decoder without a GPU: the decoder switch of MonoDepth, the launch list, the scratch size, the build of the kernels
for gfx950 and the host-side restatement of the resampling tables against F.interpolate in fp64."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def reduced_cfg(**kw):
    from splat_slam_amd.mono_depth import MonoDepthConfig
    base = dict(stem_chs=32, stage_chs=(64, 128, 256), stage_layers=(1, 1, 2), gn_groups=8, dim=128, heads=2, depth=4, taps=(2, 3), pos_grid=4,
                features=32, net_size=(64, 96))
    base.update(kw)
    return MonoDepthConfig(**base)


def test_an_unknown_decoder_raises_before_any_device_is_touched():
    from splat_slam_amd.mono_depth import MonoDepth
    with pytest.raises(ValueError, match="decoder"):
        MonoDepth({}, reduced_cfg(), "cuda", decoder="nonsense")
    with pytest.raises(ValueError, match="decoder"):
        MonoDepth.synthetic(1, reduced_cfg(), backbone="hip", decoder="HIP")
    with pytest.raises(ValueError, match="decoder"):
        MonoDepth.from_state_dict({}, reduced_cfg(), decoder=None)


def test_cpu_tensors_raise():
    from splat_slam_amd import dpt_decoder as D
    from splat_slam_amd.mono_depth import state_shapes
    x = torch.zeros(1, 2, 2, 8, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.conv_cl_f16(x, torch.zeros(16, 8, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.up2_cl_f16(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.resize_in(torch.zeros(1, 3, 4, 4), (8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.resize_out(torch.zeros(4, 4), (8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.DPTDecoder({k: torch.zeros(s) for k, s in state_shapes(reduced_cfg()).items() if ".model." not in k}, reduced_cfg(), "cpu")


def test_launch_names_have_the_stated_length_and_order():
    from splat_slam_amd.dpt_decoder import LAUNCH_NAMES, LAYER_NAMES
    from splat_slam_amd.mono_depth import MonoDepthConfig, state_shapes
    want = ["pack3", "act_postprocess3.3", "pack4", "act_postprocess4.3", "act_postprocess4.4", "layer1_rn", "layer2_rn", "layer3_rn", "layer4_rn",
            "refinenet4.resConfUnit2.conv1", "refinenet4.resConfUnit2.conv2", "refinenet4.up2", "refinenet4.out_conv"]
    for i in (3, 2, 1):
        want += [f"refinenet{i}.resConfUnit1.conv1", f"refinenet{i}.resConfUnit1.conv2", f"refinenet{i}.resConfUnit2.conv1",
                 f"refinenet{i}.resConfUnit2.conv2", f"refinenet{i}.up2", f"refinenet{i}.out_conv"]
    want += ["output_conv.0", "head.up2", "output_conv.2", "output_conv.4"]
    for cfg in (MonoDepthConfig(), reduced_cfg()):
        names = LAUNCH_NAMES(cfg)
        assert len(names) == 35 and len(set(names)) == 35 and list(names) == want
        layers = LAYER_NAMES(cfg)
        shapes = state_shapes(cfg)
        assert len(layers) == 28 and all(n + ".weight" in shapes for n in layers)
        # every tensor of the state dict outside backbone and transformer (whose readouts are act_postprocessN.0.project) is a layer's
        rest = {k.rsplit(".", 1)[0] for k in shapes if not k.startswith("pretrained.model.") and ".project." not in k}
        assert rest == set(layers)


def test_scratch_bytes_is_pure_and_grows_with_the_sizes():
    from splat_slam_amd import _native as nat
    f = nat.lib().sgr_dpt_scratch_bytes
    for bad in ((0, 32, 32, 128, 32), (1, 0, 32, 128, 32), (1, 40, 64, 128, 32), (1, 64, 48, 128, 32), (-1, 32, 32, 128, 32), (1, -32, 32, 128, 32),
                (1, 32, -32, 128, 32), (1, 32, 32, 120, 32), (1, 32, 32, 128, 24), (1, 32, 32, 2048, 32), (65536, 32, 32, 128, 32)):
        assert f(*bad) == 0, bad
    for n, H, W, D, feat in ((1, 32, 32, 128, 32), (2, 64, 96, 128, 32), (1, 512, 512, 768, 256), (3, 480, 640, 768, 256)):
        size = f(n, H, W, D, feat)
        assert size > 0 and size % 16 == 0 and f(n, H, W, D, feat) == size
        assert f(n + 1, H, W, D, feat) > size and f(n, H + 32, W, D, feat) > size and f(n, H, W + 32, D, feat) > size
        # at least the two full-resolution maps of the head and one fusion map at half resolution, fp16
        assert size >= n * H * W * (feat // 2 + 32) * 2 + n * (H // 2) * (W // 2) * feat * 2


# kernel -> the VGPR count of its gfx950 code object when it was written, as a ceiling
VGPR_CEILING = {"dpt_conv_kernelILi1ELi16E": 48, "dpt_conv_kernelILi1ELi32E": 68, "dpt_conv_kernelILi1ELi64E": 92,
                "dpt_conv_kernelILi3ELi16E": 52, "dpt_conv_kernelILi3ELi32E": 68, "dpt_conv_kernelILi3ELi64E": 92,
                "dpt_up2_kernel": 38, "dpt_resize_in_kernel": 29, "dpt_resize_out_kernel": 47}


def test_dpt_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """every kernel keeps its state in registers: no private segment, no spills (read from the code object's metadata)"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "dpt.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_dpt.hip")], check=True, capture_output=True)
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


def _matrix(rows, n_in):
    """[(indices, weights)] per output -> the fp64 resampling matrix [n_out][n_in]; clamped indices that coincide add up"""
    m = torch.zeros(len(rows), n_in, dtype=torch.float64)
    for o, (idx, wts) in enumerate(rows):
        for i, w in zip(idx, wts):
            m[o, i] += float(w)
    return m


@pytest.mark.parametrize("src,dst", [((48, 80), (64, 96)), ((37, 130), (64, 96)), ((480, 640), (64, 96)), ((5, 3), (5, 7)), ((1, 9), (4, 2))])
def test_the_antialias_table_matches_interpolate_in_fp64(src, dst):
    from splat_slam_amd.dpt_decoder import aa_taps
    img = torch.rand(1, 3, *src, generator=torch.Generator().manual_seed(sum(src)), dtype=torch.float64)
    want = F.interpolate(img, size=dst, mode="bilinear", align_corners=False, antialias=True)
    mats = []
    for n_in, n_out in zip(src, dst):
        rows = []
        for o in range(n_out):
            first, w = aa_taps(o, n_in, n_out)
            assert sum(w) == 1 and all(v >= 0 for v in w) and first + len(w) <= n_in
            rows.append((range(first, first + len(w)), w))
        mats.append(_matrix(rows, n_in))
    got = mats[0] @ img @ mats[1].T
    assert float((got - want).abs().max()) < 1e-13


@pytest.mark.parametrize("src,dst", [((64, 96), (48, 80)), ((64, 96), (37, 130)), ((3, 2), (7, 9)), ((1, 1), (3, 2))])
def test_the_cubic_table_matches_interpolate_in_fp64(src, dst):
    from splat_slam_amd.dpt_decoder import cubic_taps
    img = torch.rand(1, 1, *src, generator=torch.Generator().manual_seed(sum(dst)), dtype=torch.float64)
    want = F.interpolate(img, size=dst, mode="bicubic", align_corners=False)
    mats = []
    for n_in, n_out in zip(src, dst):
        rows = [cubic_taps(o, n_in, n_out) for o in range(n_out)]
        for idx, w in rows:
            assert sum(w) == 1 and sum(abs(v) for v in w) <= 1.375 and 0 <= min(idx) and max(idx) < n_in
        mats.append(_matrix(rows, n_in))
    got = mats[0] @ img @ mats[1].T
    assert float((got - want).abs().max()) < 1e-13


@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (2, 5), (3, 2), (16, 24)])
def test_the_up2_table_matches_interpolate_in_fp64(h, w):
    from splat_slam_amd.dpt_decoder import up2_taps
    img = torch.rand(1, 2, h, w, generator=torch.Generator().manual_seed(h + w), dtype=torch.float64)
    want = F.interpolate(img, scale_factor=2, mode="bilinear", align_corners=True)
    mats = []
    for n in (h, w):
        rows = []
        for o in range(2 * n):
            i0, i1, t = up2_taps(o, n)
            assert 0 <= t < 1 and 0 <= i0 <= i1 < n
            rows.append(((i0, i1), (1 - t, t)))
        mats.append(_matrix(rows, n))
    got = mats[0] @ img @ mats[1].T
    assert float((got - want).abs().max()) < 1e-13
