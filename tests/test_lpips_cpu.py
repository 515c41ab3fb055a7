"""splat_slam_amd.lpips without a GPU: the two key layouts and every ValueError, the synthetic weights against a numpy recomputation,
the packed layout of conv1, the shape function, the properties of the fp64 restatement tests/lpips_ref.py itself, the unchanged
defaults of eval_rendering and the build of the kernels for gfx950."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lpips_ref as LR
from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SEED = 3


def _sd():
    from splat_slam_amd.lpips import synthetic_state_dict
    return synthetic_state_dict(SEED)


# ---- state dicts -----------------------------------------------------------------------------------------------------------------------
def test_module_keys_with_and_without_the_metric_prefix_give_the_same_tensors():
    from splat_slam_amd.lpips import CONV_SHAPES, SCALE, SHIFT, normalize_state_dict
    sd = _sd()
    assert len(sd) == 15
    canon = normalize_state_dict(sd)
    assert sorted(canon) == sorted([f"conv{i}.{p}" for i in range(1, 6) for p in ("weight", "bias")] + [f"lin{i}" for i in range(5)]
                                   + ["shift", "scale"])
    for i, (cout, cin, k, _, _) in enumerate(CONV_SHAPES):
        assert tuple(canon[f"conv{i + 1}.weight"].shape) == (cout, cin, k, k) and tuple(canon[f"lin{i}"].shape) == (1, cout, 1, 1)
    assert canon["shift"].tolist() == pytest.approx(SHIFT) and canon["scale"].tolist() == pytest.approx(SCALE)
    # as the metric object stores it: one more "net.", the scaling layer's buffers, and the lin layers a second time under lins.K
    full = {"net." + k: v for k, v in sd.items()}
    full["net.scaling_layer.shift"] = torch.tensor([-0.03, -0.088, -0.188]).reshape(1, 3, 1, 1) * 2
    full["net.scaling_layer.scale"] = torch.tensor([0.458, 0.448, 0.45]).reshape(1, 3, 1, 1) * 2
    for i in range(5):
        full[f"net.lins.{i}.model.1.weight"] = sd[f"lin{i}.model.1.weight"] + 1.0          # ignored
    again = normalize_state_dict(full)
    for k in canon:
        if k not in ("shift", "scale"):
            assert torch.equal(again[k], canon[k]), k
    assert again["shift"].tolist() == pytest.approx([2 * s for s in SHIFT]) and again["scale"].tolist() == pytest.approx([2 * s for s in SCALE])


def _parts(sd):
    alex = {}
    for s, f in (("net.slice1.0", "features.0"), ("net.slice2.3", "features.3"), ("net.slice3.6", "features.6"), ("net.slice4.8", "features.8"),
                 ("net.slice5.10", "features.10")):
        alex[f + ".weight"], alex[f + ".bias"] = sd[s + ".weight"], sd[s + ".bias"]
    alex["classifier.1.weight"] = torch.zeros(4, 4)                                  # the rest of torchvision's AlexNet is not read
    lin = {k: v for k, v in sd.items() if k.startswith("lin")}
    return alex, lin


def test_the_parts_layout_gives_the_same_tensors():
    from splat_slam_amd.lpips import normalize_state_dict, parts_state_dict
    sd = _sd()
    canon, parts = normalize_state_dict(sd), parts_state_dict(*_parts(sd))
    assert sorted(canon) == sorted(parts)
    for k in canon:
        assert torch.equal(canon[k], parts[k]), k


def test_every_value_error_names_its_key():
    from splat_slam_amd.lpips import LPIPS, normalize_state_dict, parts_state_dict
    sd = _sd()
    for key in sd:
        with pytest.raises(ValueError, match=re.escape(key)):
            normalize_state_dict({k: v for k, v in sd.items() if k != key})
        with pytest.raises(ValueError, match=re.escape(key)):
            normalize_state_dict({**sd, key: sd[key][..., None]})
        with pytest.raises(ValueError, match=re.escape(key)):
            normalize_state_dict({**sd, key: sd[key].numpy()})
    with pytest.raises(ValueError, match="net.slice1.1.weight"):
        normalize_state_dict({**sd, "net.slice1.1.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="scaling_layer.shift"):
        normalize_state_dict({**sd, "scaling_layer.shift": torch.zeros(4)})
    with pytest.raises(ValueError, match="scaling_layer.scale"):
        normalize_state_dict({**sd, "scaling_layer.scale": torch.tensor([0.458, 0.0, 0.45])})
    # a prefixed dict is named by its own keys
    with pytest.raises(ValueError, match=re.escape("net.lin2.model.1.weight")):
        normalize_state_dict({"net." + k: (v[:, :-1] if k == "lin2.model.1.weight" else v) for k, v in sd.items()})
    alex, lin = _parts(sd)
    for key in ("features.6.bias", "features.0.weight"):
        with pytest.raises(ValueError, match=re.escape(key)):
            parts_state_dict({k: v for k, v in alex.items() if k != key}, lin)
        with pytest.raises(ValueError, match=re.escape(key)):
            parts_state_dict({**alex, key: alex[key][1:]}, lin)
    with pytest.raises(ValueError, match=re.escape("lin4.model.1.weight")):
        parts_state_dict(alex, {k: v for k, v in lin.items() if k != "lin4.model.1.weight"})
    # the image checks come before anything touches a device or the object
    blank = object.__new__(LPIPS)
    for a, b in ((torch.zeros(1, 4, 40, 40), torch.zeros(1, 4, 40, 40)), (torch.zeros(1, 3, 30, 31), torch.zeros(1, 3, 30, 31)),
                 (torch.zeros(1, 3, 31, 30), torch.zeros(1, 3, 31, 30)), (torch.zeros(3, 40, 40), torch.zeros(3, 40, 40)),
                 (torch.zeros(1, 3, 40, 40), torch.zeros(2, 3, 40, 40))):
        with pytest.raises(ValueError, match="lpips"):
            LPIPS.lpips(blank, a, b)


# ---- synthetic weights -----------------------------------------------------------------------------------------------------------------
def _hash_uniform(name, n, seed):
    """FNV-1a of the name, the murmur3 finaliser of (index * 0x9E3779B1 + hash + seed * 0x85EBCA77) mod 2^32, to [-1, 1): the name in
    Python ints, the indices as uint64 masked to 32 bits after every product"""
    h = 2166136261
    for b in name.encode():
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    m = np.uint64(0xFFFFFFFF)
    x = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64((h + seed * 0x85EBCA77) & 0xFFFFFFFF)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.float64) / 2.0 ** 31 - 1.0


def test_the_hash_against_a_scalar_loop_in_python_ints():
    name, seed = "net.slice1.0.bias", SEED
    h = 2166136261
    for b in name.encode():
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    want = []
    for i in range(64):
        x = (i * 0x9E3779B1 + h + seed * 0x85EBCA77) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        x ^= x >> 16
        want.append(x / 2.0 ** 31 - 1.0)
    assert _hash_uniform(name, 64, seed).tolist() == want


def test_synthetic_weights_equal_a_numpy_recomputation():
    from splat_slam_amd.lpips import CONV_SHAPES, synthetic_state_dict
    sd = _sd()
    slices = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
    seen = set()
    for i, (s, (cout, cin, k, _, _)) in enumerate(zip(slices, CONV_SHAPES)):
        fan_in = cin * k * k
        for key in (s + ".weight", s + ".bias"):
            want = (_hash_uniform(key, sd[key].numel(), SEED) * fan_in ** -0.5).astype(np.float32).reshape(sd[key].shape)
            assert np.array_equal(sd[key].numpy(), want), key
            assert np.abs(want).max() <= fan_in ** -0.5
            seen.add(key)
        key = f"lin{i}.model.1.weight"
        want = (0.5 * (_hash_uniform(key, cout, SEED) + 1.0)).astype(np.float32).reshape(1, cout, 1, 1)
        assert np.array_equal(sd[key].numpy(), want) and want.min() >= 0.0
        seen.add(key)
    assert seen == set(sd)
    other = synthetic_state_dict(SEED + 1)
    assert not torch.equal(other["net.slice3.6.weight"], sd["net.slice3.6.weight"])
    w = sd["net.slice3.6.weight"]
    assert abs(float(w.mean())) < 1e-3 and float(w.std()) == pytest.approx((192 * 9) ** -0.5 / 3 ** 0.5, rel=0.02)


def test_conv1_is_packed_as_tap_times_8_plus_channel():
    from splat_slam_amd.lpips import pack_conv
    w = _sd()["net.slice1.0.weight"].to(torch.float16)
    got = pack_conv(w).numpy()
    assert got.shape == (64, 992) and got.dtype == np.float16
    want = np.zeros((64, 992), np.float16)
    wn = w.numpy()
    for ky in range(11):
        for kx in range(11):
            want[:, (ky * 11 + kx) * 8:(ky * 11 + kx) * 8 + 3] = wn[:, :, ky, kx]
    assert np.array_equal(got, want)
    assert np.count_nonzero(got[:, 968:]) == 0 and np.count_nonzero(got.reshape(64, 124, 8)[:, :, 3:]) == 0
    w2 = _sd()["net.slice2.3.weight"].to(torch.float16)
    got2 = pack_conv(w2).numpy()
    assert got2.shape == (192, 1600)
    assert np.array_equal(got2.reshape(192, 25, 64), w2.numpy().transpose(0, 2, 3, 1).reshape(192, 25, 64))


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
def test_tap_sizes_and_the_smallest_image():
    from splat_slam_amd import _native as nat
    from splat_slam_amd.lpips import tap_sizes
    assert tap_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert tap_sizes(480, 640) == [(119, 159), (59, 79), (29, 39), (29, 39), (29, 39)]
    assert tap_sizes(34, 31)[0] == (7, 7) and tap_sizes(35, 31)[0] == (8, 7)
    for h, w in ((30, 31), (31, 30), (24, 24), (6, 100), (0, 31)):
        with pytest.raises(ValueError, match="31 x 31"):
            tap_sizes(h, w)
    f = nat.lib().sgr_lpips_scratch_bytes
    assert f(1, 30, 31) == 0 and f(1, 31, 30) == 0 and f(0, 31, 31) == 0 and f(17, 31, 31) == 0
    assert f(1, 31, 31) > 0 and f(1, 31, 31) == f(1, 31, 31) and f(2, 31, 31) > f(1, 31, 31) and f(1, 35, 31) > f(1, 31, 31)
    # two alternating buffers, each as large as its largest map (the packed images, the pooled maps and tap 4 | taps 1, 2, 3 and 5), and
    # the partial sums of the five taps, each piece rounded up to 256 bytes
    sizes = tap_sizes(480, 640)
    tap = [2 * h * w * c * 2 for (h, w), c in zip(sizes, (64, 192, 384, 256, 256))]
    need = max(2 * 480 * 640 * 8 * 2, 2 * 59 * 79 * 64 * 2, 2 * 29 * 39 * 192 * 2, tap[3]) + max(tap[0], tap[1], tap[2], tap[4])
    assert need <= f(1, 480, 640) <= need + 2 * 256 + 5 * 4 * 256
    assert f(16, 480, 640) < 16 * f(1, 480, 640) + 4096 and f(16, 480, 640) < 250e6
    # the trunk of the restatement has these sizes
    P = _prepared()
    taps = LR.trunk(P, torch.zeros(1, 3, 33, 47, dtype=torch.float64))
    assert [tuple(t.shape[2:]) for t in taps] == tap_sizes(33, 47)


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
def _prepared():
    from splat_slam_amd.lpips import normalize_state_dict, prepare
    return prepare(normalize_state_dict(_sd()))


def test_prepare_rounds_the_convolutions_to_fp16_and_nothing_else():
    from splat_slam_amd.lpips import normalize_state_dict
    canon, P = normalize_state_dict(_sd()), _prepared()
    for k, v in P.items():
        assert v.dtype == torch.float32
        if k.startswith("conv"):
            assert torch.equal(v, canon[k].to(torch.float16).float()) and not torch.equal(v, canon[k])
        else:
            assert torch.equal(v, canon[k].float())


def test_hand_computed_distance_on_two_pixels_of_eight_channels():
    f0 = torch.tensor([[3.0, 4, 0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6, 7, 8]]).T.reshape(1, 8, 2)
    f1 = torch.tensor([[0.0, 0, 0, 0, 0, 0, 0, 5], [1, 2, 3, 4, 5, 6, 7, 8]]).T.reshape(1, 8, 2)
    w = torch.tensor([1.0, 2, 0, 0, 0, 0, 0, 3])
    d = LR.pixel_distance(f0, f1, w)
    # u = (0.6, 0.8, 0, ...), v = (0, ..., 1): 1 * 0.36 + 2 * 0.64 + 3 * 1; the 1e-8 under the root moves it by 4.64 * 1e-8 / 25
    assert d.shape == (1, 2) and abs(float(d[0, 0]) - 4.64) < 1e-8 and float(d[0, 1]) == 0.0
    assert abs(float(LR.pixel_bound_sum(f0, f1, w)[0, 0]) - 4.64) < 1e-8                    # disjoint supports: (|u| + |v|)^2 = (u - v)^2
    # a pixel that is all zero in one map is the weighted square norm of the other's unit vector; in both, 0
    z = torch.zeros_like(f0)
    assert abs(float(LR.pixel_distance(z, f1, w)[0, 0]) - 3.0) < 1e-8
    assert torch.count_nonzero(LR.pixel_distance(z, z, w)) == 0 and bool(torch.isfinite(LR.pixel_distance(z, z, w)).all())


def test_the_restatement_is_zero_on_equal_images_and_symmetric():
    P = _prepared()
    g = torch.Generator().manual_seed(1)
    x, y = torch.rand(2, 3, 31, 35, generator=g), torch.rand(2, 3, 31, 35, generator=g)
    total, levels = LR.lpips_ref(P, x, x.clone())
    assert total.dtype == torch.float64 and levels.shape == (2, 5) and torch.count_nonzero(total) == 0 and torch.count_nonzero(levels) == 0
    txy, lxy = LR.lpips_ref(P, x, y)
    tyx, lyx = LR.lpips_ref(P, y, x)
    assert torch.equal(txy, tyx) and torch.equal(lxy, lyx)
    assert bool((lxy > 0).all()) and torch.allclose(txy, lxy.sum(1), rtol=1e-15, atol=0)
    # normalize=False reads [-1, 1]
    t2, _ = LR.lpips_ref(P, 2 * x - 1, 2 * y - 1, normalize=False)
    assert torch.allclose(t2, txy, rtol=1e-12, atol=0)
    # the torch composition states the same function
    tt, lt = LR.lpips_torch(P, x.float(), y.float())
    assert torch.allclose(lt.double(), lxy, rtol=2e-2, atol=1e-6)


@pytest.mark.parametrize("layer,h,w", [(0, 31, 34), (0, 12, 9), (1, 7, 5), (2, 4, 3)])
def test_the_restatements_convolution_against_unfold_and_matmul(layer, h, w):
    from splat_slam_amd.lpips import CONV_SHAPES
    P = _prepared()
    cout, cin, k, stride, pad = CONV_SHAPES[layer]
    x = torch.randn(2, cin, h, w, generator=torch.Generator().manual_seed(h * w), dtype=torch.float64)
    wt, b = P[f"conv{layer + 1}.weight"], P[f"conv{layer + 1}.bias"]
    a, c = LR.conv_ref(x, wt, b, stride, pad), LR.conv_unfold(x, wt, b, stride, pad)
    assert a.shape == c.shape == (2, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1)
    assert float((a - c).abs().max()) <= 1e-13 * max(1.0, float(a.abs().max()))
    assert LR.GEOMETRY[layer] == (stride, pad)


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------
def test_eval_rendering_and_evaluate_keep_their_defaults():
    from splat_slam_amd.eval import eval_rendering
    from splat_slam_amd.session import MappingSession
    sig = inspect.signature(eval_rendering)
    assert list(sig.parameters) == ["frames", "gaussians", "pipe", "background", "gt_depths", "global_scale", "mesh", "mesh_path", "c2w",
                                    "voxel_length", "sdf_trunc", "eval_mesh", "gt_mesh_path", "distance_thresh", "icp_align", "mesh_samples",
                                    "lpips"]
    want = dict(gt_depths=None, global_scale=1.0, mesh=False, mesh_path=None, c2w=None, voxel_length=5.0 / 512.0, sdf_trunc=0.04,
                eval_mesh=True, gt_mesh_path=None, distance_thresh=0.05, icp_align=True, mesh_samples=200_000, lpips=None)
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == want
    ev = inspect.signature(MappingSession.evaluate)
    assert list(ev.parameters) == ["self", "gt_depths", "global_scale", "mesh", "mesh_path", "gt_mesh_path", "distance_thresh", "icp_align",
                                   "mesh_samples", "lpips"]
    assert ev.parameters["lpips"].default is None


# ---- the kernels' code object ----------------------------------------------------------------------------------------------------------
# kernel -> the VGPR count of its gfx950 code object when it was written, as a ceiling
VGPR_CEILING = {"lpips_pack_kernel": 18, "lpips_pool_kernel": 43, "lpips_final_kernel": 16, "lpips_conv_kernelILi11E": 84,
                "lpips_conv_kernelILi5E": 84, "lpips_conv_kernelILi3E": 84, "lpips_dist_kernelILi1E": 50, "lpips_dist_kernelILi3E": 94,
                "lpips_dist_kernelILi4E": 125, "lpips_dist_kernelILi6E": 163}


def test_lpips_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """every kernel keeps its state in registers (the distance a pixel's C <= 384 values of both maps): no private segment, no spills,
    read from the code object's metadata"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "lpips.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_lpips.hip")], check=True, capture_output=True)
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
