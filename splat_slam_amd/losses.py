"""Mapping loss -- mirror of /root/reference/thirdparty/monogs/utils/slam_utils.py:71-119 (SSIM branch off by default,
/root/reference/configs/splat_slam.yaml:36) plus a fused HIP variant (`sgr_mapping_loss`) with identical values, and
`ssim_native`, the HIP drop-in for loss_utils.ssim (`sgr_ssim` / `sgr_ssim_backward`)."""

import torch
from torch.autograd.function import once_differentiable

from splat_slam_amd import _native as nat


def _gt_depth(viewpoint, device):
    d = viewpoint.depth
    if not torch.is_tensor(d):
        d = torch.from_numpy(d)
    return d.to(dtype=torch.float32, device=device)[None]


_WINDOWS = {}


def ssim(img1, img2, window_size=11):
    """Mean structural similarity with an 11x11 Gaussian window of sigma 1.5, per channel, zero padding
    (/root/reference/thirdparty/gaussian_splatting/utils/loss_utils.py:36-101); C1 = 0.01^2, C2 = 0.03^2."""
    import torch.nn.functional as F
    ch = img1.size(-3)
    key = (window_size, ch, img1.device, img1.dtype)
    win = _WINDOWS.get(key)
    if win is None:
        x = torch.arange(window_size, dtype=torch.float32) - window_size // 2
        g1 = torch.exp(-(x * x) / (2 * 1.5 ** 2))
        g1 = (g1 / g1.sum()).unsqueeze(1)
        win = (g1 @ g1.t()).unsqueeze(0).unsqueeze(0).expand(ch, 1, window_size, window_size).contiguous().to(img1.device, img1.dtype)
        _WINDOWS[key] = win
    blur = lambda t: F.conv2d(t, win, padding=window_size // 2, groups=ch)
    mu1, mu2 = blur(img1), blur(img2)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = blur(img1 * img1) - mu1_sq, blur(img2 * img2) - mu2_sq, blur(img1 * img2) - mu12
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))).mean()


class _SsimNative(torch.autograd.Function):
    """The HIP SSIM (sgr_ssim / sgr_ssim_backward): per-image means, fixed-order sums; the forward keeps the three per-pixel
    derivative maps when img1 needs a gradient, the backward blurs them (no host sync: the upstream is read on the device)."""

    @staticmethod
    def forward(ctx, img1, img2):
        lib = nat.lib()
        x, y = img1.contiguous(), img2.contiguous()
        B, C, H, W = x.shape if x.dim() == 4 else (1,) + tuple(x.shape)
        dev = x.device
        n = B * C * H * W
        want = ctx.needs_input_grad[0]
        scratch_bytes = lib.sgr_ssim_scratch_bytes(B, C, H, W)
        # one arena per call: per-image SSIM | (3 derivative maps) | partials
        nmaps = 3 * n if want else 0
        arena = torch.empty(B + nmaps + scratch_bytes // 4, dtype=torch.float32, device=dev)
        out, maps, scratch = arena[:B], arena[B:B + nmaps], arena[B + nmaps:]
        if dev.index is not None and dev.index != torch.cuda.current_device():
            torch.cuda.set_device(dev)
        nat.check(lib.sgr_ssim(B, C, H, W, x.data_ptr(), y.data_ptr(), out.data_ptr(), maps.data_ptr() if want else None,
                               scratch.data_ptr(), scratch_bytes, torch.cuda.current_stream().cuda_stream), "sgr_ssim")
        if want:
            ctx.save_for_backward(x, y, maps)
        ctx.dims = (B, C, H, W)
        return out[0] if B == 1 else out.mean()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y, maps = ctx.saved_tensors
        B, C, H, W = ctx.dims
        g = g.to(dtype=torch.float32).contiguous()
        dx = torch.empty_like(x)
        nat.check(nat.lib().sgr_ssim_backward(B, C, H, W, x.data_ptr(), y.data_ptr(), maps.data_ptr(), g.data_ptr(), 0, 1.0 / B,
                                              dx.data_ptr(), torch.cuda.current_stream().cuda_stream), "sgr_ssim_backward")
        return dx, None


def ssim_native(img1, img2, window_size=11, size_average=True):
    """loss_utils.ssim (/root/reference/thirdparty/gaussian_splatting/utils/loss_utils.py:61-101) on the HIP kernels, for [C,H,W] and
    [B,C,H,W] fp32 GPU tensors: the mean of the SSIM map over B*C*H*W, differentiable in img1 (once).  Raises on what it does not
    implement (another window, size_average=False, non-fp32 input, a gradient for img2) and on CPU tensors: there is no fallback."""
    if window_size != 11:
        raise ValueError(f"ssim_native: window_size {window_size} (only 11 is implemented)")
    if not size_average:
        raise ValueError("ssim_native: size_average=False is not implemented")
    if img1.dtype != torch.float32 or img2.dtype != torch.float32:
        raise TypeError(f"ssim_native: fp32 inputs only ({img1.dtype}, {img2.dtype})")
    if img1.shape != img2.shape or img1.dim() not in (3, 4) or img1.numel() == 0:
        raise ValueError(f"ssim_native: [C,H,W] or [B,C,H,W] pairs of one shape ({tuple(img1.shape)}, {tuple(img2.shape)})")
    if img2.requires_grad:
        raise ValueError("ssim_native differentiates img1 only (ssim(image, gt_image)); img2 requires grad")
    if not (img1.is_cuda and img2.is_cuda) or img1.device != img2.device:
        raise RuntimeError("ssim_native needs GPU tensors on one device (HIP only, no CPU fallback)")
    return _SsimNative.apply(img1, img2)


def uses_ssim(mapping_config):
    """`ssim_loss: True` (slam_utils.py:89-98; off in configs/splat_slam.yaml:36): the loss is no longer a per-pixel L1, so the
    fused kernels (sign-code epilogue, sgr_mapping_loss) do not apply: the loops run the torch formulation through autograd."""
    return bool(mapping_config["Training"].get("ssim_loss", False))


def get_loss_mapping_rgbd(config, image, depth, viewpoint, initialization=False):
    alpha = config["Training"]["alpha"] if "alpha" in config["Training"] else 0.95
    rgb_boundary_threshold = config["Training"]["rgb_boundary_threshold"]
    gt_image = viewpoint.original_image.to(image.device)
    _, h, w = gt_image.shape
    gt_depth = _gt_depth(viewpoint, image.device)
    rgb_pixel_mask = (gt_image.sum(dim=0) > rgb_boundary_threshold).view(1, h, w)
    l1_rgb = torch.abs(image * rgb_pixel_mask - gt_image * rgb_pixel_mask)
    if uses_ssim(config):                      # slam_utils.py:89-98: (1 - lambda) |.| + lambda (1 - ssim), the scalar broadcast per pixel
        lam = config["opt_params"]["lambda_dssim"]
        l1_rgb = (1.0 - lam) * l1_rgb + lam * (1.0 - ssim(image, gt_image))
    depth_pixel_mask = (gt_depth > 0.01).view(*depth.shape)
    l1_depth = torch.abs(depth * depth_pixel_mask - gt_depth * depth_pixel_mask)
    return alpha * l1_rgb.mean() + (1 - alpha) * l1_depth.mean()


def get_loss_mapping(config, image, depth, viewpoint, opacity, initialization=False):
    if initialization:
        image_ab = image
    else:
        image_ab = (torch.exp(viewpoint.exposure_a)) * image + viewpoint.exposure_b
    return get_loss_mapping_rgbd(config, image_ab, depth, viewpoint)


def get_median_depth(depth, opacity=None, mask=None, return_std=False):
    """Median (and optionally std) of the rendered depth over pixels that are covered (depth > 0), nearly opaque
    (opacity > 0.95) and inside `mask` -- slam_utils.py:108-119; scales the keyframe baseline test (mapper.py:984)."""
    depth = depth.detach()
    use = depth > 0
    for extra in ((opacity.detach() > 0.95) if opacity is not None else None, mask):
        if extra is not None:
            use = use & extra
    picked = depth[use]
    return (picked.median(), picked.std(), use) if return_std else picked.median()


def _native_nodes():
    import diff_gaussian_rasterization as drg
    return getattr(drg, "native_extension", lambda: None)()       # (tests inject the oracle under this module name)


class _FusedMappingLoss(torch.autograd.Function):
    """One pass over the image: loss value + dL/dimage, dL/ddepth, dL/da, dL/db (fixed-order reduction)."""

    @staticmethod
    def forward(ctx, image, depth, exp_a, exp_b, gt_image, gt_depth, alpha, thr):
        lib = nat.lib()
        dev = image.device
        _, H, W = image.shape
        image, depth = image.contiguous(), depth.contiguous()
        # one arena per call: dL/dimage | dL/ddepth | d/da, d/db | loss | 16 KiB of reduction scratch
        hw = H * W
        arena = torch.empty(4 * hw + 4 + 4096, dtype=torch.float32, device=dev)
        d_img, d_dep = arena[:3 * hw].view(3, H, W), arena[3 * hw:4 * hw].view(depth.shape)
        d_a, d_b, loss = arena[4 * hw:4 * hw + 1], arena[4 * hw + 1:4 * hw + 2], arena[4 * hw + 2:4 * hw + 3]
        scratch = arena[4 * hw + 4:]
        if dev.index is not None and dev.index != torch.cuda.current_device():
            torch.cuda.set_device(dev)
        nat.check(lib.sgr_mapping_loss(H, W, image.data_ptr(), depth.data_ptr(), gt_image.data_ptr(), gt_depth.data_ptr(),
                                       nat.ptr(exp_a), nat.ptr(exp_b), alpha, thr, 1.0, loss.data_ptr(), d_img.data_ptr(),
                                       d_dep.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), scratch.data_ptr(), 4 * scratch.numel(),
                                       torch.cuda.current_stream().cuda_stream), "sgr_mapping_loss")
        ctx.save_for_backward(arena)
        ctx.has_exp, ctx.shape = exp_a is not None, (H, W, tuple(depth.shape))
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        arena, = ctx.saved_tensors
        H, W, dshape = ctx.shape
        hw = H * W
        s = arena[:4 * hw + 2] * g               # the four gradients are contiguous: ONE scaling launch
        return (s[:3 * hw].view(3, H, W), s[3 * hw:4 * hw].view(dshape), s[4 * hw:4 * hw + 1] if ctx.has_exp else None,
                s[4 * hw + 1:4 * hw + 2] if ctx.has_exp else None, None, None, None, None)


def get_loss_mapping_fused(config, image, depth, viewpoint, opacity, initialization=False):
    if uses_ssim(config):                      # not an L1 per pixel: the torch formulation
        return get_loss_mapping(config, image, depth, viewpoint, opacity, initialization)
    alpha = config["Training"]["alpha"] if "alpha" in config["Training"] else 0.95
    thr = config["Training"]["rgb_boundary_threshold"]
    gt_image = viewpoint.original_image
    gt_depth = getattr(viewpoint, "_depth_dev", None)
    if gt_depth is None:
        gt_depth = _gt_depth(viewpoint, image.device).contiguous()
        viewpoint._depth_dev = gt_depth     # keep the ground-truth depth resident instead of re-uploading per call
    a, b = (None, None) if initialization else (viewpoint.exposure_a, viewpoint.exposure_b)
    ext = _native_nodes()
    if ext is not None and image.is_cuda:        # the same launch, its autograd node in C++ (diff_gaussian_rasterization/csrc/dgr_native.cpp)
        import diff_gaussian_rasterization as drg
        return ext.mapping_loss(image, depth, a, b, gt_image, gt_depth, float(alpha), float(thr), bool(drg.DEFER_POSE_GRADS))
    return _FusedMappingLoss.apply(image, depth, a, b, gt_image.contiguous(), gt_depth, float(alpha), float(thr))


class _SsimMappingLoss(torch.autograd.Function):
    """The mapping loss with the SSIM term (sgr_mapping_loss_ssim): loss value + dL/dimage, dL/ddepth, dL/da, dL/db in one launch pair
    and a fixed-order reduction; the gradients are computed in the forward and scaled by the upstream in the backward."""

    @staticmethod
    def forward(ctx, image, depth, exp_a, exp_b, gt_image, gt_depth, alpha, thr, lam):
        lib = nat.lib()
        dev = image.device
        _, H, W = image.shape
        image, depth = image.contiguous(), depth.contiguous()
        hw = H * W
        # one arena per call: dL/dimage | dL/ddepth | d/da, d/db | loss | the SSIM term's maps and partial sums
        term_bytes = lib.sgr_ssim_term_bytes(1, H, W)
        arena = torch.empty(4 * hw + 4 + (term_bytes + 3) // 4, dtype=torch.float32, device=dev)
        d_img, d_dep = arena[:3 * hw].view(3, H, W), arena[3 * hw:4 * hw].view(depth.shape)
        d_a, d_b, loss = arena[4 * hw:4 * hw + 1], arena[4 * hw + 1:4 * hw + 2], arena[4 * hw + 2:4 * hw + 3]
        maps = arena[4 * hw + 4:]
        term = nat.SgrSsimTerm(float(lam), 1, maps.data_ptr(), term_bytes)
        if dev.index is not None and dev.index != torch.cuda.current_device():
            torch.cuda.set_device(dev)
        nat.check(lib.sgr_mapping_loss_ssim(H, W, image.data_ptr(), depth.data_ptr(), gt_image.data_ptr(), gt_depth.data_ptr(),
                                            nat.ptr(exp_a), nat.ptr(exp_b), alpha, thr, 1.0, term, loss.data_ptr(),
                                            d_img.data_ptr(), d_dep.data_ptr(), d_a.data_ptr(), d_b.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "sgr_mapping_loss_ssim")
        ctx.save_for_backward(arena[:4 * hw + 2])
        ctx.has_exp, ctx.shape = exp_a is not None, (H, W, tuple(depth.shape))
        return loss[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        grads, = ctx.saved_tensors
        H, W, dshape = ctx.shape
        hw = H * W
        s = grads * g                            # the four gradients are contiguous: ONE scaling launch
        return (s[:3 * hw].view(3, H, W), s[3 * hw:4 * hw].view(dshape), s[4 * hw:4 * hw + 1] if ctx.has_exp else None,
                s[4 * hw + 1:4 * hw + 2] if ctx.has_exp else None, None, None, None, None, None)


def get_loss_mapping_ssim_native(config, image, depth, viewpoint, opacity, initialization=False):
    """get_loss_mapping (slam_utils.py:71-105) with `ssim_loss: True` on the HIP kernels: (1 - lambda) |masked L1| + lambda (1 - ssim)
    of the exposure-compensated image, plus the depth L1, differentiable (once) in image, depth and the exposure parameters.  fp32
    GPU tensors only (no CPU fallback).  With `ssim_loss: False` it is get_loss_mapping_fused."""
    if not uses_ssim(config):
        return get_loss_mapping_fused(config, image, depth, viewpoint, opacity, initialization)
    if image.dtype != torch.float32 or depth.dtype != torch.float32:
        raise TypeError(f"get_loss_mapping_ssim_native: fp32 image and depth only ({image.dtype}, {depth.dtype})")
    if not (image.is_cuda and depth.is_cuda):
        raise RuntimeError("get_loss_mapping_ssim_native needs GPU tensors (HIP only, no CPU fallback)")
    if image.dim() != 3 or image.shape[0] != 3 or depth.numel() != image.shape[1] * image.shape[2]:
        raise ValueError(f"get_loss_mapping_ssim_native: image [3,H,W] and depth [1,H,W] ({tuple(image.shape)}, {tuple(depth.shape)})")
    alpha = config["Training"]["alpha"] if "alpha" in config["Training"] else 0.95
    thr = config["Training"]["rgb_boundary_threshold"]
    lam = config["opt_params"]["lambda_dssim"]
    gt_image = viewpoint.original_image.to(image.device, torch.float32).contiguous()
    gt_depth = _gt_depth(viewpoint, image.device).contiguous()
    a, b = (None, None) if initialization else (viewpoint.exposure_a, viewpoint.exposure_b)
    for t in (a, b):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise TypeError("get_loss_mapping_ssim_native: exposure parameters must be fp32 GPU tensors")
    return _SsimMappingLoss.apply(image, depth, a, b, gt_image, gt_depth, float(alpha), float(thr), float(lam))
