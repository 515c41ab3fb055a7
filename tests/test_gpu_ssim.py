"""-m gpu: the HIP SSIM (sgr_ssim / sgr_ssim_backward through losses.ssim_native) and the rendering evaluation (sgr_render_metrics
through eval.eval_rendering).

SSIM is held to the reference's own vectors (tests/golden/reference_ssim.npz, made by importing loss_utils.ssim and the
`ssim_loss: True` mapping loss) and to fp64 losses.ssim; the evaluation to a torch restatement of eval_utils.py:90-128 on the same
renders.  Tolerances come from an fp32 emulation of the separable kernels against fp64."""
import math
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.asarray(a)).float().to(DEV)


def _pairs(shape, seed):
    """independent, correlated, and smooth-with-noise image pairs (the last is where E[x^2] - mu^2 cancels most)"""
    g = torch.Generator().manual_seed(seed)
    x, y = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    out = [("independent", x, y), ("correlated", x, (0.7 * x + 0.3 * y).clamp(0, 1))]
    lead, (h, w) = shape[:-2], shape[-2:]
    low = torch.rand(lead + (max(h // 16, 2), max(w // 16, 2)), generator=g)
    smooth = torch.nn.functional.interpolate(low.reshape(-1, 1, *low.shape[-2:]), size=(h, w), mode="bilinear",
                                             align_corners=False).reshape(shape)
    out.append(("smooth", (0.2 + 0.6 * smooth + 0.01 * torch.randn(shape, generator=g)).clamp(0, 1),
                (0.2 + 0.6 * smooth + 0.01 * torch.randn(shape, generator=g)).clamp(0, 1)))
    return [(n, a.to(DEV).contiguous(), b.to(DEV).contiguous()) for n, a, b in out]


def _native_value_and_grad(x, y, up=0.37):
    from splat_slam_amd.losses import ssim_native
    xr = x.clone().requires_grad_(True)
    v = ssim_native(xr, y)
    (v * up).backward()
    return v.detach(), xr.grad


def test_reference_golden_ssim_and_the_ssim_mapping_loss():
    """`|ssim_native - loss_utils.ssim| <= 1e-6` on the reference's pair, and the whole `ssim_loss: True` mapping loss of
    slam_utils.py:80-105 with ssim_native in place of ssim meets the bounds the torch formulation meets
    (tests/test_golden_host.py::test_ssim_loss_branch_matches_reference)."""
    from splat_slam_amd.losses import ssim_native
    S = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_ssim.npz"))
    assert abs(ssim_native(_t(S["ssim_a"]), _t(S["ssim_b"])).item() - float(S["ssim"])) <= 1e-6
    alpha, thr, lam = 0.8, 0.01, 0.2
    image = _t(S["image"]).requires_grad_(True)
    depth = _t(S["depth"]).requires_grad_(True)
    gt, gtd = _t(S["gt"]), _t(S["gtd"])[None]
    exp_a = torch.tensor([0.05], device=DEV, requires_grad=True)
    exp_b = torch.tensor([-0.02], device=DEV, requires_grad=True)
    image_ab = torch.exp(exp_a) * image + exp_b                                   # slam_utils.py:80-83
    _, h, w = gt.shape
    rgb_mask = (gt.sum(dim=0) > thr).view(1, h, w)
    l1_rgb = torch.abs(image_ab * rgb_mask - gt * rgb_mask)
    l1_rgb = (1.0 - lam) * l1_rgb + lam * (1.0 - ssim_native(image_ab, gt))      # :89-98
    dmask = (gtd > 0.01).view(*depth.shape)
    l1_depth = torch.abs(depth * dmask - gtd * dmask)
    loss = alpha * l1_rgb.mean() + (1 - alpha) * l1_depth.mean()
    loss.backward()
    assert abs(loss.item() - float(S["loss"])) < 2e-7
    assert torch.allclose(image.grad.cpu(), torch.from_numpy(S["dimage"]), rtol=0, atol=2e-8)
    assert torch.allclose(depth.grad.cpu(), torch.from_numpy(S["ddepth"]), rtol=0, atol=1e-9)
    assert abs(exp_a.grad.item() - float(S["da"])) < 1e-6 and abs(exp_b.grad.item() - float(S["db"])) < 1e-6


@pytest.mark.parametrize("shape", [(3, 480, 640), (3, 481, 643), (3, 7, 5), (12, 3, 480, 640)])
def test_ssim_native_matches_fp64_value_and_gradient(shape):
    from splat_slam_amd.losses import ssim
    for i, (name, x, y) in enumerate(_pairs(shape, seed=11 + len(shape) + shape[-1])):
        v, g = _native_value_and_grad(x, y)
        xd = x.double().requires_grad_(True)
        r = ssim(xd, y.double())
        (r * 0.37).backward()
        assert v.dtype == torch.float32 and v.dim() == 0
        assert abs(v.item() - r.item()) <= 5e-6, (shape, name, v.item(), r.item())
        err = (g.double() - xd.grad).abs().max().item()
        assert err <= 2e-4 * xd.grad.abs().max().item(), (shape, name, err, xd.grad.abs().max().item())


@pytest.mark.parametrize("shape", [(3, 64, 96), (2, 3, 37, 45), (3, 7, 5)])
def test_equal_pairs_give_exactly_one_and_a_zero_gradient(shape):
    g = torch.Generator().manual_seed(5)
    for x in (torch.full(shape, 0.4), torch.rand(shape, generator=g)):
        x = x.to(DEV)
        v, grad = _native_value_and_grad(x, x.clone())
        assert v.item() == 1.0
        assert torch.count_nonzero(grad).item() == 0


def test_ssim_native_is_bitwise_reproducible():
    for shape in [(3, 481, 643), (12, 3, 480, 640)]:
        _, x, y = _pairs(shape, seed=3)[1]
        v1, g1 = _native_value_and_grad(x, y)
        v2, g2 = _native_value_and_grad(x, y)
        assert torch.equal(v1, v2) and torch.equal(g1, g2)


def test_ssim_native_without_grad_and_under_no_grad():
    from splat_slam_amd.losses import ssim, ssim_native
    _, x, y = _pairs((2, 3, 40, 50), seed=9)[1]
    with torch.no_grad():
        a = ssim_native(x.clone().requires_grad_(True), y)
    b = ssim_native(x, y)
    assert not a.requires_grad and not b.requires_grad and torch.equal(a, b)
    assert abs(a.item() - ssim(x.double(), y.double()).item()) <= 5e-6


# ---- eval_rendering

def _eval_scene(camera, views, n, seed):
    from splat_slam_amd import synthetic as syn
    intr = syn.INTRINSICS[camera]
    params = syn.room_parameters(n, seed=seed, device=DEV)
    params["scaling"] = params["scaling"] + 1.2
    cams = syn.make_views(params, views, intr, DEV, seed=seed)
    gm = syn.model_from_parameters(params, device=DEV)
    H, W = intr["H"], intr["W"]
    with torch.no_grad():
        for k, cam in enumerate(cams):
            if k > 0:                                          # optimised exposures: applied to every frame but the first
                cam.exposure_a.fill_(0.03 * ((k % 5) - 2))
                cam.exposure_b.fill_(0.01 * ((k % 3) - 1))
            cam.original_image[:, : H // 8, : W // 6] = 0.0     # masked out of the PSNR
            cam.original_image[1, H // 2:, W // 2:] = 0.0
            cam.depth[H // 3: H // 2, W // 4: W // 2] = 0.0      # masked out of the depth L1
    return cams, gm


def _torch_eval(frames, gm, gt_depths, global_scale):
    """eval_utils.py:90-128, restated in torch on the same renders"""
    from splat_slam_amd.eval import psnr
    from splat_slam_amd.losses import ssim
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.renderer import render
    bg = torch.zeros(3, device=DEV)
    out = {"psnr": [], "ssim": [], "depth_l1": []}
    with torch.no_grad():
        for k, frame in enumerate(frames):
            pkg = render(frame, gm, PipelineParams(), bg)
            rendering, depth = pkg["render"], pkg["depth"]
            image = torch.exp(frame.exposure_a) * rendering + frame.exposure_b if k > 0 else rendering
            image = torch.clamp(image, 0.0, 1.0)
            gt = frame.original_image
            mask = gt > 0
            gd = gt_depths[k]
            depth_mask = (depth > 0) * (gd > 0)
            l1 = (torch.abs(global_scale * depth - gd) * depth_mask).sum() / depth_mask.sum()
            out["psnr"].append(psnr(image[mask].unsqueeze(0), gt[mask].unsqueeze(0)).item())
            out["ssim"].append(ssim(image.double().unsqueeze(0), gt.double().unsqueeze(0)).item())
            out["depth_l1"].append(l1.item())
    return out


@pytest.mark.parametrize("camera,views,n", [("tiny", 18, 4000), ("metric", 3, 20000)])
def test_eval_rendering_matches_the_reference_evaluation(camera, views, n):
    from splat_slam_amd.eval import eval_rendering, eval_rendering_psnr
    from splat_slam_amd.mapper import PipelineParams
    cams, gm = _eval_scene(camera, views, n, seed=7)
    bg = torch.zeros(3, device=DEV)
    gt_depths = [c.depth.clone() for c in cams]
    gt_depths[1].zero_()                                         # no valid depth pixel: NaN, as the reference's 0/0
    scale = 1.07
    got = eval_rendering(cams, gm, PipelineParams(), bg, gt_depths=gt_depths, global_scale=scale)
    ref = _torch_eval(cams, gm, gt_depths, scale)
    assert len(got["psnr"]) == len(got["ssim"]) == len(got["depth_l1"]) == views
    for k in range(views):
        assert abs(got["psnr"][k] - ref["psnr"][k]) <= 1e-4, (k, got["psnr"][k], ref["psnr"][k])
        assert abs(got["ssim"][k] - ref["ssim"][k]) <= 5e-6, (k, got["ssim"][k], ref["ssim"][k])
        if k == 1:
            assert math.isnan(got["depth_l1"][k]) and math.isnan(ref["depth_l1"][k])
        else:
            assert abs(got["depth_l1"][k] - ref["depth_l1"][k]) <= 1e-5 * abs(ref["depth_l1"][k]), (k, got["depth_l1"][k])
    assert got["mean_psnr"] == pytest.approx(float(np.mean(got["psnr"])))
    assert got["mean_ssim"] == pytest.approx(float(np.mean(got["ssim"])))
    assert math.isnan(got["mean_depthl1"])
    for a, b in zip(got["psnr"], eval_rendering_psnr(cams, gm, PipelineParams(), bg)):
        assert abs(a - b) <= 1e-4
    # the default ground-truth depth is each frame's `depth`
    dflt = eval_rendering(cams, gm, PipelineParams(), bg)
    ref1 = _torch_eval(cams, gm, [c.depth for c in cams], 1.0)
    for k in range(views):
        assert abs(dflt["depth_l1"][k] - ref1["depth_l1"][k]) <= 1e-5 * abs(ref1["depth_l1"][k])
    assert math.isfinite(dflt["mean_depthl1"])


def test_eval_rendering_of_a_perfect_frame_and_the_session_entry_point():
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.eval import eval_rendering
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.renderer import render
    from splat_slam_amd.session import MappingSession
    cams, gm = _eval_scene("tiny", 3, 4000, seed=9)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        cams[0].original_image = render(cams[0], gm, PipelineParams(), bg)["render"].clamp(0, 1).contiguous()
    got = eval_rendering(cams, gm, PipelineParams(), bg)
    assert got["psnr"][0] == math.inf and got["ssim"][0] == 1.0
    assert all(math.isfinite(p) for p in got["psnr"][1:])
    loop = types.SimpleNamespace(config=syn.DEFAULT_CONFIG, device=DEV, viewpoints={2 * k: c for k, c in enumerate(cams)},
                                 gaussians=gm, background=bg)
    sess = MappingSession(loop, syn.INTRINSICS["tiny"])
    assert sess.evaluate() == got
