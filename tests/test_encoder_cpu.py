"""The parts of splat_slam_amd.encoder, droid_net and motion_filter that need no GPU: the fp64 oracle tests/encoder_ref.py against the
recorded outputs of the reference's BasicEncoder, the state-dict handling, the synthetic weights, the argument checks and the build of
the kernels for gfx950."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import encoder_ref as R
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_encoders.npz")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WHICH = ("fnet", "cnet")


@pytest.mark.parametrize("which", WHICH)
def test_oracle_equals_the_recorded_outputs_of_the_reference_module(which):
    """both sides are fp64 sums of at most 1152 terms over 16 layers of order 1, with unrounded weights: held to 1e-10 of the largest
    output"""
    from splat_slam_amd import encoder as E
    g = np.load(GOLDEN)
    assert tuple(g["in_images"].shape) == (1, 2, 3, 40, 56) and g["in_images"].dtype == np.float16
    sd = E.synthetic_encoder_state_dict(which, int(g["seed"]))
    out = R.encoder_ref(sd, E.NORM[which], torch.from_numpy(g["in_images"].astype(np.float32)))
    ref = g["out_" + which]
    assert ref.dtype == np.float64 and tuple(out.shape) == ref.shape == (1, 2, E.OUT_DIM[which], 5, 7)
    assert np.abs(out.numpy() - ref).max() <= 1e-10 * np.abs(ref).max()
    assert np.sqrt((ref ** 2).mean()) > 0.3                                              # (not a comparison of zeros)


@pytest.mark.parametrize("which", WHICH)
def test_fixture_lists_exactly_the_keys_the_encoder_requires(which):
    from splat_slam_amd import encoder as E
    g = np.load(GOLDEN)
    recorded = {k: tuple(int(s) for s in sh.split(",")) for k, sh in zip(g["keys_" + which].tolist(), g["shapes_" + which].tolist())}
    assert recorded == E.LAYER_SHAPES(E.OUT_DIM[which]) and len(recorded) == 32
    assert os.path.getsize(GOLDEN) <= 300000


def test_launch_names_follow_the_layers():
    from splat_slam_amd import encoder as E
    from splat_slam_amd import _native as nat
    assert len(E.LAUNCH_NAMES["fnet"]) == nat.SGR_ENCODER_LAUNCHES[1] == 32 and len(E.LAUNCH_NAMES["cnet"]) == nat.SGR_ENCODER_LAUNCHES[0] == 17
    assert E.LAUNCH_NAMES["cnet"][0] == "pack" and sorted(E.LAUNCH_NAMES["cnet"][1:]) == sorted(E.ENCODER_LAYERS)
    assert len(E.ENCODER_LAYERS) == nat.SGR_ENCODER_LAYERS
    i = E.LAUNCH_NAMES["cnet"].index("layer2.0.downsample.0")
    assert E.LAUNCH_NAMES["cnet"][i - 1] == "layer2.0.conv1" and E.LAUNCH_NAMES["cnet"][i + 1] == "layer2.0.conv2"
    assert [n for n in E.LAUNCH_NAMES["fnet"] if n.endswith(":norm")] == [n + ":norm" for n in E.LAUNCH_NAMES["cnet"][1:-1]]


def test_state_dict_prefixes_and_errors():
    from splat_slam_amd import encoder as E
    from splat_slam_amd import update_op as U
    for which, other in (("fnet", "cnet"), ("cnet", "fnet")):
        sd = E.synthetic_encoder_state_dict(which, 1)
        shapes = E.LAYER_SHAPES(E.OUT_DIM[which])
        for prefix in ("", which + ".", "module." + which + ".", "module."):
            ck = {prefix + k: v for k, v in sd.items()}
            ck[("module." if prefix.startswith("module.") else "") + other + ".conv1.weight"] = torch.zeros(3)
            ck[("module." if prefix.startswith("module.") else "") + "update.gru.w.bias"] = torch.zeros(5)
            out = E.normalize_encoder_state_dict(ck, which)
            assert set(out) == set(shapes) and all(torch.equal(out[k], sd[k]) for k in sd)
        # errors come from the validation, before the device is looked at: these run on a machine without a GPU
        with pytest.raises(ValueError, match="layer2.0.downsample.0.bias"):
            E.Encoder.from_state_dict({k: v for k, v in sd.items() if k != "layer2.0.downsample.0.bias"}, which)
        with pytest.raises(ValueError, match="unexpected key 'norm1.weight'"):
            E.Encoder.from_state_dict({**sd, "norm1.weight": torch.zeros(32)}, which)
        with pytest.raises(ValueError, match="shape"):
            E.Encoder.from_state_dict({**sd, "conv1.weight": torch.zeros(32, 3, 3, 3)}, which)
        with pytest.raises(ValueError, match="shape"):
            E.Encoder.from_state_dict({**sd, "conv2.weight": torch.zeros(384 - E.OUT_DIM[which], 128, 1, 1)}, which)   # the other encoder's
        with pytest.raises(ValueError, match="twice"):
            E.normalize_encoder_state_dict({**sd, which + ".conv1.bias": torch.zeros(32)}, which)
    with pytest.raises(ValueError, match="fnet"):
        E.normalize_encoder_state_dict({}, "gnet")
    # the update operator goes on ignoring both encoders
    full = {"module.update." + k: v for k, v in U.synthetic_state_dict(1).items()}
    full.update({"module.fnet." + k: v for k, v in E.synthetic_encoder_state_dict("fnet", 1).items()})
    full.update({"module.cnet." + k: v for k, v in E.synthetic_encoder_state_dict("cnet", 1).items()})
    assert set(U.normalize_state_dict(full)) == set(U.LAYER_SHAPES)
    assert set(E.normalize_encoder_state_dict(full, "cnet")) == set(E.LAYER_SHAPES(256))


def test_synthetic_weights_follow_their_closed_form_rule():
    from splat_slam_amd import encoder as E
    a, b, c = E.synthetic_encoder_state_dict("fnet", 7), E.synthetic_encoder_state_dict("fnet", 7), E.synthetic_encoder_state_dict("fnet", 8)
    d = E.synthetic_encoder_state_dict("cnet", 7)
    for k, shape in E.LAYER_SHAPES(128).items():
        assert a[k].dtype == torch.float32 and tuple(a[k].shape) == shape and torch.equal(a[k], b[k]) and not torch.equal(a[k], c[k])
        if not k.startswith("conv2"):
            assert not torch.equal(a[k], d[k])                   # the name that is hashed carries the encoder's prefix
    w = a["layer3.1.conv1.weight"]
    bound = np.sqrt(3.0 / (128 * 9))
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.99 * bound and abs(float(w.mean())) < 0.01 * bound
    assert abs(float(w.std()) - bound / np.sqrt(3)) < 0.01 * bound                      # unit gain: variance 1 / fan_in
    assert float(a["layer3.1.conv1.bias"].abs().max()) <= 1 / np.sqrt(128 * 9)
    # one element by hand: the murmur3 finaliser of (index * 0x9E3779B1 + FNV-1a(name) + seed * 0x85EBCA77)
    name, idx = "cnet.conv1.bias", 3
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    x = (idx * 0x9E3779B1 + h + 7 * 0x85EBCA77) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    assert float(d["conv1.bias"][idx]) == np.float32((x / 2.0 ** 31 - 1.0) / np.sqrt(3 * 49))


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("n,H,W", [(2, 40, 56), (1, 13, 19), (3, 16, 24)])
def test_synthetic_encoders_neither_vanish_nor_saturate(which, n, H, W):
    """the accuracy tests run on these weights: on N(0, 1) images the fp64 output keeps an rms in [0.3, 5]"""
    from splat_slam_amd import encoder as E
    out = R.encoder_ref(E.synthetic_encoder_state_dict(which, 7), E.NORM[which], R.make_images(1, n, H, W, seed=5))
    rms = float(out.pow(2).mean().sqrt())
    print(which, (n, H, W), "rms", rms, "max", float(out.abs().max()))
    assert tuple(out.shape) == (1, n, E.OUT_DIM[which], (H + 7) // 8, (W + 7) // 8) and 0.3 <= rms <= 5.0


def test_oracle_instance_norm_and_block_tail_by_hand():
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(2, 4, 6, 5, generator=g), torch.randn(8, 4, 3, 3, generator=g), torch.randn(8, generator=g)
    res = torch.randn(2, 8, 3, 3, generator=g)
    y = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    assert tuple(y.shape) == (2, 8, 3, 3)
    want = torch.relu(res.double() + torch.relu(torch.nn.functional.instance_norm(y, eps=1e-5)))
    got, (mu, sd) = R.conv2d_ref(x, w, b, 2, "instance", "relu", res, return_stats=True)
    assert (got - want).abs().max() < 1e-12 and tuple(mu.shape) == (2, 8, 1, 1) == tuple(sd.shape)
    nobias = R.conv2d_ref(x, w, None, 2, "instance", "relu", res)
    assert (got - nobias).abs().max() < 1e-12                                         # the bias of a normalised convolution cancels


def test_argument_errors_raise_without_a_device():
    from splat_slam_amd import encoder as E
    from splat_slam_amd.droid_net import DroidNet, synthetic_state_dict
    sd = E.synthetic_encoder_state_dict("fnet", 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.Encoder(sd, "fnet", device="cpu")
    with pytest.raises(ValueError, match="which"):
        E.Encoder(sd, "enet")
    x, w = torch.zeros(1, 32, 4, 4), torch.zeros(32, 32, 3, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        E.conv2d_f16(x, w)
    full = synthetic_state_dict(2)
    assert len(full) == 38 + 32 + 32
    with pytest.raises(ValueError, match="outside"):
        DroidNet.from_state_dict({**full, "gnet.conv1.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="encoder cnet: the state dict lacks .'conv2.bias'"):
        DroidNet.from_state_dict({k: v for k, v in full.items() if k != "cnet.conv2.bias"})
    with pytest.raises(ValueError, match="agg.eta.0.bias"):
        DroidNet.from_state_dict({k: v for k, v in full.items() if k != "update.agg.eta.0.bias"})


# kernel -> the VGPR count of its gfx950 code object when it was written, as a ceiling
VGPR_CEILING = {"enc_conv_kernelILi1ELi32E": 68, "enc_conv_kernelILi1ELi64E": 92, "enc_conv_kernelILi3ELi32E": 64, "enc_conv_kernelILi3ELi64E": 92,
                "enc_conv_kernelILi7ELi32E": 64, "enc_conv_kernelILi7ELi64E": 92, "enc_apply_kernel": 34, "enc_pack_kernel": 10}


def test_encoder_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """every kernel keeps its state in registers: no private segment, no spills (read from the code object's metadata)"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "encoder.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_encoder.hip")], check=True, capture_output=True)
    text = open(out).read()
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
    from splat_slam_amd import _native as nat
    lib = nat.lib()
    assert lib.sgr_encoder_scratch_bytes(0, 40, 56, 128, 1) == 0 and lib.sgr_encoder_scratch_bytes(1, 40, 56, 64, 1) == 0
    assert lib.sgr_encoder_scratch_bytes(1, 8, 8, 128, 1) == 0 and lib.sgr_encoder_scratch_bytes(1, 8, 8, 256, 0) > 0     # layer3 is 1 x 1
    assert lib.sgr_encoder_scratch_bytes(1, 9, 8, 128, 1) > 0 and lib.sgr_encoder_scratch_bytes(1, 40, 56, 128, 2) == 0
    small, big = lib.sgr_encoder_scratch_bytes(2, 40, 56, 128, 1), lib.sgr_encoder_scratch_bytes(8, 384, 512, 128, 1)
    # the packed image, four fp16 maps and the fp32 sums of the largest level (20 x 28 x 32 per image)
    assert small >= 2 * (40 * 56 * 8 * 2 + 20 * 28 * 32 * (4 * 2 + 4)) and big > small and small % 16 == 0
    assert lib.sgr_encoder_scratch_bytes(2, 40, 56, 256, 0) < small
