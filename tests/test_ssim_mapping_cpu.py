"""The mapping loss with the SSIM term (`ssim_loss: True`) without a GPU: its kernels in csrc/sgr_ssim.hip compile for gfx950 with no
scratch, no spills and LDS within budget; sgr_ssim_term_bytes, sgr_mapping_loss_ssim, sgr_map_step_ssim and sgr_map_run_ssim are
declared, exported and bound with the ABI unchanged; and the per-pixel gradient the second kernel forms is, restated in fp64, the
gradient of the reference formulation (thirdparty/monogs/utils/slam_utils.py:80-105)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_KERNELS = ("ssimloss_moments_kernel", "ssimloss_grad_kernel")
OLD_KERNELS = ("ssim_fwd_kernel", "ssim_final_kernel", "ssim_bwd_kernel", "metrics_kernel", "metrics_final_kernel")
NEW_FUNCTIONS = ("sgr_ssim_term_bytes", "sgr_mapping_loss_ssim", "sgr_map_step_ssim", "sgr_map_run_ssim")


@pytest.fixture(scope="module")
def isa_meta(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "ssim.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_ssim.hip")], check=True, capture_output=True)
    meta = {}
    for block in open(out).read().split("\n  - ")[1:]:
        m = re.search(r"\.name:\s+(\S+)", block)
        if m and ".private_segment_fixed_size" in block:
            meta[m.group(1)] = block
    return meta


def test_ssim_loss_kernels_have_no_scratch_no_spills_and_fit_six_workgroups(isa_meta):
    for k in NEW_KERNELS:
        names = [n for n in isa_meta if k in n]
        assert len(names) == 1, (k, sorted(isa_meta))
        block = isa_meta[names[0]]
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert scratch == 0 and spill == 0, (k, scratch, spill)
        assert lds <= 160 * 1024 // 6, (k, lds)
    for n in isa_meta:            # (tests/test_ssim_cpu.py finds the older kernels by substring)
        if any(k in n for k in NEW_KERNELS):
            assert not any(o in n for o in OLD_KERNELS), n


def test_entry_points_are_declared_exported_and_bound_with_the_abi_unchanged():
    from splat_slam_amd.build import build_native
    from splat_slam_amd import _native as nat
    build_native(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert "#define SGR_ABI_VERSION 10" in hdr
    h = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\(" % name, hdr) and name in nat.SIGNATURES and hasattr(h, name), name
    assert "typedef struct SgrSsimTerm" in hdr
    assert ctypes.sizeof(nat.SgrSsimTerm) == 24
    assert [f[0] for f in nat.SgrSsimTerm._fields_] == ["lambda_dssim", "max_views", "arena", "arena_bytes"]
    assert nat.lib().sgr_abi_version() == 10


def test_term_bytes_is_a_host_function_monotone_in_its_arguments():
    from splat_slam_amd.build import build_native
    from splat_slam_amd import _native as nat
    build_native(verbose=False)
    f = nat.lib().sgr_ssim_term_bytes            # (no device: a pure host computation)
    assert f(0, 480, 640) == 0 and f(1, 0, 640) == 0 and f(1, 480, -1) == 0
    one = f(1, 480, 640)
    assert one >= 9 * 480 * 640 * 4 + 3 * 30 * 20 * 16       # three maps of three channels + one view's partial records
    for mv in (1, 2, 5, 12, 16):
        for H, W in ((7, 5), (37, 53), (480, 640), (481, 643)):
            b = f(mv, H, W)
            assert b > 0 and b % 256 == 0
            assert f(mv + 1, H, W) > b and f(mv, H + 1, W) >= b and f(mv, H, W + 1) >= b
            assert f(mv, H + 16, W) > b and f(mv, H, W + 32) > b


def _gauss_window():
    x = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(x * x) / (2 * 1.5 ** 2))
    return g / g.sum()


def _blur(t):          # [3,H,W] fp64, the 11x11 window with zero padding 5 (loss_utils.py:83), per channel
    g = _gauss_window()
    w = (g[:, None] @ g[None, :])[None, None].expand(3, 1, 11, 11).contiguous()
    return F.conv2d(t[None], w, padding=5, groups=3)[0]


def _reference_loss(image, depth, gt, gtd, a, b, alpha, thr, lam):
    """slam_utils.py:71-105 with ssim_loss: True, in fp64 (loss_utils.ssim restated)."""
    x = image if a is None else torch.exp(a) * image + b
    mu1, mu2 = _blur(x), _blur(gt)
    s11, s22, s12 = _blur(x * x) - mu1 * mu1, _blur(gt * gt) - mu2 * mu2, _blur(x * gt) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()
    m = (gt.sum(dim=0) > thr)[None]
    l1 = torch.abs(x * m - gt * m)
    rgb = (1 - lam) * l1 + lam * (1 - ssim)
    dm = gtd > 0.01
    return alpha * rgb.mean() + (1 - alpha) * torch.abs(depth * dm - gtd * dm).mean()


def _pass_b(image, depth, gt, gtd, a, b, alpha, thr, lam):
    """What ssimloss_moments_kernel / ssimloss_grad_kernel compute, per pixel, in fp64: the derivative maps of the SSIM mean, their
    blur, dL/d(image_ab) = w_l1 sign(m r) + u (G*dm + 2 x G*d11 + y G*d12), then the chain to image / exposure."""
    _, H, W = image.shape
    ea = torch.exp(a) if a is not None else torch.ones((), dtype=torch.float64)
    eb = b if b is not None else torch.zeros((), dtype=torch.float64)
    x, y = ea * image + eb, gt
    scale = 1.0 / (3 * H * W)
    mu1, mu2 = _blur(x), _blur(y)
    exx, eyy, exy = _blur(x * x), _blur(y * y), _blur(x * y)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    A1, A2 = 2 * mu1 * mu2 + c1, 2 * (exy - mu1 * mu2) + c2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + c1, (exx - mu1 * mu1) + (eyy - mu2 * mu2) + c2
    S = A1 * A2 / (B1 * B2)
    dm = scale * 2 * (mu2 * (A2 - A1) - mu1 * S * (B2 - B1)) / (B1 * B2)
    d11 = scale * (-S / B2)
    d12 = scale * 2 * A1 / (B1 * B2)
    w_l1, u, w_dep = alpha * (1 - lam) * scale, -alpha * lam, (1 - alpha) / (H * W)
    m = (gt.sum(dim=0) > thr)[None]
    r = torch.where(m, x - y, torch.zeros_like(x))
    dab = w_l1 * torch.sign(r) + u * (_blur(dm) + 2 * x * _blur(d11) + y * _blur(d12))
    rd = torch.where(gtd > 0.01, depth - gtd, torch.zeros_like(depth))
    return ea * dab, w_dep * torch.sign(rd), (dab * ea * image).sum(), dab.sum()


@pytest.mark.parametrize("exposure", [False, True])
@pytest.mark.parametrize("size", [(37, 53), (16, 32), (9, 70)])
def test_pass_b_gradient_is_the_gradient_of_the_reference_loss(exposure, size):
    H, W = size
    g = torch.Generator().manual_seed(H * 100 + W + exposure)
    gt = torch.rand(3, H, W, generator=g, dtype=torch.float64)
    gt[:, : H // 4] *= 0.002                                          # below the rgb boundary threshold: masked L1
    image = (0.6 * gt + 0.4 * torch.rand(3, H, W, generator=g, dtype=torch.float64)).requires_grad_(True)
    gtd = torch.rand(1, H, W, generator=g, dtype=torch.float64) * 3
    gtd[:, :, : W // 5] = 0.0
    depth = (gtd + 0.1 * torch.randn(1, H, W, generator=g, dtype=torch.float64)).requires_grad_(True)
    a = torch.tensor([0.07], dtype=torch.float64, requires_grad=True) if exposure else None
    b = torch.tensor([-0.03], dtype=torch.float64, requires_grad=True) if exposure else None
    alpha, thr, lam = 0.95, 0.01, 0.2
    _reference_loss(image, depth, gt, gtd, a, b, alpha, thr, lam).backward()
    d_img, d_dep, da, db = _pass_b(image.detach(), depth.detach(), gt, gtd, None if a is None else a.detach(),
                                   None if b is None else b.detach(), alpha, thr, lam)
    assert torch.allclose(d_img, image.grad, rtol=1e-9, atol=1e-15)
    assert torch.allclose(d_dep, depth.grad, rtol=1e-12, atol=1e-18)
    if exposure:
        assert abs(da.item() - a.grad.item()) <= 1e-9 * max(1.0, abs(a.grad.item()))
        assert abs(db.item() - b.grad.item()) <= 1e-9 * max(1.0, abs(b.grad.item()))


def test_native_loss_refuses_cpu_and_non_fp32_tensors():
    import types
    from splat_slam_amd.losses import get_loss_mapping_ssim_native
    cfg = {"Training": {"alpha": 0.95, "rgb_boundary_threshold": 0.01, "ssim_loss": True}, "opt_params": {"lambda_dssim": 0.2}}
    vp = types.SimpleNamespace(original_image=torch.rand(3, 8, 8), depth=torch.rand(1, 8, 8),
                               exposure_a=torch.zeros(1), exposure_b=torch.zeros(1))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        get_loss_mapping_ssim_native(cfg, torch.rand(3, 8, 8), torch.rand(1, 8, 8), vp, None)
    with pytest.raises(TypeError, match="fp32"):
        get_loss_mapping_ssim_native(cfg, torch.rand(3, 8, 8).double(), torch.rand(1, 8, 8), vp, None)
    with pytest.raises(TypeError, match="fp32"):
        get_loss_mapping_ssim_native(cfg, torch.rand(3, 8, 8), torch.rand(1, 8, 8).half(), vp, None)
