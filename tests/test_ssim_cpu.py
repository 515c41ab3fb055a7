"""The HIP SSIM and rendering metrics without a GPU: csrc/sgr_ssim.hip compiles for gfx950 with no scratch and no spills in any
kernel, ssim_native refuses what it does not implement (and CPU tensors: no fallback), and the derivative maps the kernels use
(include/splat_hip.h, sgr_ssim) are the gradient of the reference's SSIM in fp64."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("ssim_fwd_kernel", "ssim_final_kernel", "ssim_bwd_kernel", "metrics_kernel", "metrics_final_kernel")


@pytest.fixture(scope="module")
def ssim_meta(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "ssim.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_ssim.hip")], check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for block in text.split("\n  - ")[1:]:
        m = re.search(r"\.name:\s+(\S+)", block)
        if m and ".private_segment_fixed_size" in block:
            meta[m.group(1)] = block
    return meta


def test_every_ssim_kernel_has_no_scratch_and_no_spills(ssim_meta):
    for k in KERNELS:
        names = [n for n in ssim_meta if k in n and not any(o != k and o in n and len(o) > len(k) for o in KERNELS)]
        assert len(names) == 1, (k, sorted(ssim_meta))
        block = ssim_meta[names[0]]
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert scratch == 0 and spill == 0, (k, scratch, spill)
        assert lds <= 160 * 1024 // 6, (k, lds)           # six workgroups per CU fit in the 160 KiB of LDS


def test_ssim_native_refuses_what_it_does_not_implement():
    from splat_slam_amd.losses import ssim_native
    a, b = torch.rand(3, 16, 16), torch.rand(3, 16, 16)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ssim_native(a, b)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ssim_native(a[None].requires_grad_(True), b[None])
    with pytest.raises(ValueError, match="window_size"):
        ssim_native(a, b, window_size=7)
    with pytest.raises(ValueError, match="size_average"):
        ssim_native(a, b, size_average=False)
    with pytest.raises(TypeError, match="fp32"):
        ssim_native(a.double(), b.double())
    with pytest.raises(ValueError, match="img1 only"):
        ssim_native(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="shape"):
        ssim_native(a, b[:, :8])
    with pytest.raises(ValueError, match="shape"):
        ssim_native(a[0], b[0])


def test_new_entry_points_are_declared_bound_and_the_abi_is_unchanged():
    from splat_slam_amd import _native as nat
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert "#define SGR_ABI_VERSION 10" in hdr
    for name in ("sgr_ssim_scratch_bytes", "sgr_ssim", "sgr_ssim_backward", "sgr_render_metrics"):
        assert re.search(r"\b%s\(" % name, hdr) and name in nat.SIGNATURES, name
    import ctypes
    assert ctypes.sizeof(nat.SgrMetricFrame) == 6 * 8


def test_ssim_scratch_covers_one_partial_record_per_workgroup():
    from splat_slam_amd.build import build_native
    from splat_slam_amd import _native as nat
    build_native(verbose=False)
    lib = nat.lib()
    for (b, c, h, w) in [(1, 3, 7, 5), (1, 3, 480, 640), (12, 3, 481, 643), (40, 3, 480, 640)]:
        tiles = ((w + 31) // 32) * ((h + 15) // 16)
        assert lib.sgr_ssim_scratch_bytes(b, c, h, w) >= 5 * 4 * b * c * tiles
    assert lib.sgr_ssim_scratch_bytes(0, 3, 8, 8) == 0


def _gauss():
    x = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(x * x) / (2 * 1.5 ** 2))
    return g / g.sum()


def _blur(t):
    C, g = t.shape[-3], _gauss().to(t.dtype)
    t = F.conv2d(t, g.view(1, 1, 1, 11).expand(C, 1, 1, 11), padding=(0, 5), groups=C)
    return F.conv2d(t, g.view(1, 1, 11, 1).expand(C, 1, 11, 1), padding=(5, 0), groups=C)


def _moments(x, y):
    """the kernels' arrangement (csrc/sgr_ssim.hip ssim_pixel): the B's as A + (B - A)"""
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = _blur(x), _blur(y)
    dmu, mu12 = mu1 - mu2, mu1 * mu2
    A1, A2 = 2 * mu12 + c1, 2 * (_blur(x * y) - mu12) + c2
    D1 = dmu * dmu
    D2 = ((_blur(x * x) + _blur(y * y)) - 2 * _blur(x * y)) - D1
    return mu1, mu2, A1, A2, A1 + D1, A2 + D2, D1, D2


def _maps(x, y):
    mu1, mu2, A1, A2, B1, B2, D1, D2 = _moments(x, y)
    S = (A1 / B1) * (A2 / B2)
    t = (mu2 * (A2 - A1) * (1 - S) - mu2 * S * (D2 - D1)) - (mu1 - mu2) * S * (B2 - B1)
    return S, 2 * t / (B1 * B2), -S / B2, 2 * (A1 / B1) / B2


def _grad(x, y, dm, d11, d12):
    g1 = _blur(d11)
    return _blur(dm) + (y * (_blur(d12) + 2 * g1) + 2 * g1 * (x - y))


def test_derivative_maps_are_the_gradient_of_the_reference_ssim():
    """The kernels' backward in fp64: dL/dx = G*dm + 2x (G*d11) + y (G*d12) with the maps of sgr_ssim, against torch autograd of the
    reference's SSIM map with the separable window (the value agrees with losses.ssim, whose 2-D window is rounded to fp32), on a
    ragged image smaller than a tile and on a batch larger than the window."""
    from splat_slam_amd.losses import ssim
    gen = torch.Generator().manual_seed(3)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    for shape in [(1, 3, 7, 5), (2, 3, 37, 45)]:
        x = torch.rand(shape, generator=gen, dtype=torch.float64)
        y = (0.6 * x + 0.4 * torch.rand(shape, generator=gen, dtype=torch.float64)).clamp(0, 1)
        xr = x.clone().requires_grad_(True)
        mu1, mu2 = _blur(xr), _blur(y)
        s11, s22, s12 = _blur(xr * xr) - mu1 * mu1, _blur(y * y) - mu2 * mu2, _blur(xr * y) - mu1 * mu2
        ref = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))
        ref.mean().backward()
        n = x.numel()                      # the mean over B C H W: per-image maps / (C H W), times 1 / B
        S, dm, d11, d12 = _maps(x, y)
        g = _grad(x, y, dm / n, d11 / n, d12 / n)
        assert abs(S.mean().item() - ref.mean().item()) < 1e-14
        assert abs(S.mean().item() - ssim(x, y).item()) < 1e-7
        assert torch.allclose(g, xr.grad, rtol=0, atol=1e-13 * float(xr.grad.abs().max())), (g - xr.grad).abs().max()


def test_equal_images_give_one_and_an_exactly_zero_gradient_in_the_map_algebra():
    """The kernels' arrangement of the formulas cancels exactly for x == y (fp32, as in the kernels)."""
    for x in (torch.full((1, 3, 20, 30), 0.4), torch.rand(1, 3, 20, 30, generator=torch.Generator().manual_seed(1))):
        S, dm, d11, d12 = _maps(x, x.clone())
        assert S.dtype == torch.float32
        assert torch.equal(S, torch.ones_like(S)) and torch.count_nonzero(dm) == 0 and torch.equal(d12, -2 * d11)
        assert torch.count_nonzero(_grad(x, x.clone(), dm, d11, d12)) == 0
