"""LPIPS v0.1 on the AlexNet trunk (the perceptual distance eval_rendering reports beside PSNR and SSIM; DESIGN.md section 3, "LPIPS",
states the definition) on the gfx950 kernels `sgr_lpips_*` (include/splat_hip.h, csrc/sgr_lpips.hip).  Inference only: no autograd, no
nn.Module.  No trained weights ship with the project: the metric loads any state dict with the key names below.

    LPIPS.from_state_dict(sd, device="cuda")       the keys of the LPIPS module: net.slice1.0, net.slice2.3, net.slice3.6, net.slice4.8,
                                                   net.slice5.10 (.weight, .bias), lin0 .. lin4 (.model.1.weight), optionally
                                                   scaling_layer.shift / .scale; one extra leading "net." on every key and duplicate
                                                   lins.K.* entries are accepted
    LPIPS.from_parts(alexnet_sd, lin_sd, device)   torchvision's features.{0,3,6,8,10}.{weight,bias} plus lin0 .. lin4
    LPIPS.synthetic(seed, device)                  synthetic_state_dict(seed): closed-form weights, the same values anywhere
    metric.lpips(img0, img1, normalize=True, return_levels=False) -> [N] fp32, or [N,5] (the five tap distances, whose sum it is)
    metric(img0, img1)                             the same
    normalize_state_dict(sd), parts_state_dict(alexnet_sd, lin_sd)    the validation alone (touches no device)
    prepare(canon)                                 the values as the kernels hold them: convolutions and biases rounded to fp16
    tap_sizes(H, W)                                the five (h, w) of the taps; ValueError below 31 x 31
    LAUNCH_NAMES                                   the launches of sgr_lpips_forward in order
    pack_pairs, pack_frames, conv_relu_f16, max_pool_f16, distance    the single kernels

Images are [N,3,H,W] in [0,1] (normalize=True) or [-1,1], H and W at least 31 (ValueError otherwise, before a device is touched).  All
work goes on the current torch stream in chunks of 16 pairs, nothing synchronises with the host, every output is bitwise reproducible,
a pair gives the bits it has alone inside any batch, lpips(x, x) is exactly 0 and lpips(x, y) has the bits of lpips(y, x).  Scratch
is one buffer per (image size, stream), grown to the largest batch seen, the four most recent kept.  A missing kernel or a CPU tensor
is an error: there is no eager fallback.
"""
import ctypes as C

import numpy as np
import torch

from splat_slam_amd import _native as nat
from splat_slam_amd._nn_common import (F16_F32, ScratchCache, gpu_tensor, hash_uniform, network_device, pack_bias, pack_weight, round_up,
                                       run_forward, stream)

__all__ = ["LPIPS", "LAUNCH_NAMES", "CHANNELS", "CONV_SHAPES", "SHIFT", "SCALE", "CHUNK", "normalize_state_dict", "parts_state_dict",
           "synthetic_state_dict", "prepare", "tap_sizes", "pack_conv", "pack_pairs", "pack_frames", "conv_relu_f16", "max_pool_f16",
           "distance"]

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
CHANNELS = (64, 192, 384, 256, 256)
# (cout, cin, kernel, stride, padding) of conv1 .. conv5
CONV_SHAPES = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))
CHUNK = nat.SGR_LPIPS_MAX_PAIRS
LAUNCH_NAMES = ("pack", "conv1", "distance1", "pool1", "conv2", "distance2", "pool2", "conv3", "distance3", "conv4", "distance4", "conv5",
                "distance5", "final")
_SLICES = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
_FEATURES = ("features.0", "features.3", "features.6", "features.8", "features.10")


def tap_sizes(H, W):
    """the (h, w) of the five taps of an H x W image: conv1 11x11 stride 4 padding 2, two 3x3 stride-2 pools without padding"""
    def axis(i):
        a = (i + 4 - 11) // 4 + 1 if i >= 7 else 0
        b = (a - 3) // 2 + 1 if a >= 3 else 0
        c = (b - 3) // 2 + 1 if b >= 3 else 0
        return a, b, c
    hs, ws = axis(int(H)), axis(int(W))
    if hs[2] < 1 or ws[2] < 1:
        raise ValueError(f"lpips: a {H} x {W} image leaves the second pool without output; the smallest image is 31 x 31")
    return [(hs[0], ws[0]), (hs[1], ws[1])] + [(hs[2], ws[2])] * 3


# ---- state dicts -----------------------------------------------------------------------------------------------------------------------
def _canon_shapes():
    shapes = {}
    for i, (cout, cin, k, _, _) in enumerate(CONV_SHAPES):
        shapes[f"conv{i + 1}.weight"] = (cout, cin, k, k)
        shapes[f"conv{i + 1}.bias"] = (cout,)
        shapes[f"lin{i}"] = (1, cout, 1, 1)
    return shapes


def _take(out, name, key, v, shape):
    if not isinstance(v, torch.Tensor) or tuple(v.shape) != shape:
        raise ValueError(f"lpips: {key!r} must be a tensor of shape {shape}, got {tuple(getattr(v, 'shape', ()))}")
    out[name] = v.detach()


def _finish(out, shapes, names):
    missing = [names[k] for k in shapes if k not in out]
    if missing:
        raise ValueError(f"lpips: the state dict lacks {missing}")
    for k, default in (("shift", SHIFT), ("scale", SCALE)):
        if k not in out:
            out[k] = torch.tensor(default, dtype=torch.float32)
    if not bool((out["scale"] > 0).all()):
        raise ValueError(f"lpips: 'scaling_layer.scale' must be positive, got {out['scale'].tolist()}")
    return out


def normalize_state_dict(sd):
    """The LPIPS module's keys -> conv1..5.weight / .bias, lin0..4 [1,C,1,1], shift, scale [3].  Raises ValueError naming the key for a
    missing key, an unexpected key or a wrong shape."""
    shapes = _canon_shapes()
    names, keys = {}, {}
    for i, s in enumerate(_SLICES):
        for part in ("weight", "bias"):
            keys[f"{s}.{part}"] = f"conv{i + 1}.{part}"
        keys[f"lin{i}.model.1.weight"] = f"lin{i}"
    names = {v: k for k, v in keys.items()}
    prefixed = any(k.startswith(("net.net.", "net.lin", "net.scaling_layer.")) for k in sd)
    out = {}
    for key, v in sd.items():
        k = key[4:] if prefixed and key.startswith("net.") else key
        if k.startswith("lins."):
            continue
        if k in ("scaling_layer.shift", "scaling_layer.scale"):
            if not isinstance(v, torch.Tensor) or v.numel() != 3:
                raise ValueError(f"lpips: {key!r} must be a tensor of 3 elements, got {tuple(getattr(v, 'shape', ()))}")
            out[k.split(".")[1]] = v.detach().reshape(3).to(torch.float32)
        elif k in keys:
            _take(out, keys[k], key, v, shapes[keys[k]])
        else:
            raise ValueError(f"lpips: unexpected key {key!r} in the state dict")
    return _finish(out, shapes, names)


def parts_state_dict(alexnet_sd, lin_sd):
    """torchvision's AlexNet (features.{0,3,6,8,10}.{weight,bias}; its other keys are not read) and the five lin weights
    (lin0..4.model.1.weight) -> the tensors of normalize_state_dict"""
    shapes = _canon_shapes()
    names, out = {}, {}
    for i, f in enumerate(_FEATURES):
        for part in ("weight", "bias"):
            names[f"conv{i + 1}.{part}"] = f"{f}.{part}"
            if f"{f}.{part}" in alexnet_sd:
                _take(out, f"conv{i + 1}.{part}", f"{f}.{part}", alexnet_sd[f"{f}.{part}"], shapes[f"conv{i + 1}.{part}"])
        key = f"lin{i}.model.1.weight"
        names[f"lin{i}"] = key
        if key in lin_sd:
            _take(out, f"lin{i}", key, lin_sd[key], shapes[f"lin{i}"])
    return _finish(out, shapes, names)


def synthetic_state_dict(seed):
    """closed-form weights under the LPIPS module's keys: convolutions and biases U(+-1 / sqrt(fan_in)), lin weights U[0, 1), each
    _nn_common.hash_uniform of the key, rounded once to fp32"""
    sd = {}
    for i, (s, (cout, cin, k, _, _)) in enumerate(zip(_SLICES, CONV_SHAPES)):
        bound = (cin * k * k) ** -0.5
        for part, shape in (("weight", (cout, cin, k, k)), ("bias", (cout,))):
            key = f"{s}.{part}"
            sd[key] = torch.from_numpy((hash_uniform(key, int(np.prod(shape)), seed) * bound).astype(np.float32).reshape(shape))
        key = f"lin{i}.model.1.weight"
        sd[key] = torch.from_numpy((0.5 * (hash_uniform(key, cout, seed) + 1.0)).astype(np.float32).reshape(1, cout, 1, 1))
    return sd


def prepare(canon):
    """the values as the kernels hold them, fp32 on the CPU: convolution weights and biases rounded to fp16, the rest as given"""
    out = {}
    for k, v in canon.items():
        v = v.detach().to("cpu", torch.float32)
        out[k] = v.to(torch.float16).to(torch.float32) if k.startswith("conv") else v
    return out


def pack_conv(w16):
    """[cout, cin, k, k] -> fp16 [cout][round_up(k * k * cin_pad, 32)], column tap * cin_pad + channel, cin_pad = round_up(cin, 8), zeros
    elsewhere: conv1 is [64][992] with k = tap * 8 + c"""
    return pack_weight(w16, round_up(w16.shape[1], 8))


# ---- the single kernels ----------------------------------------------------------------------------------------------------------------
def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def pack_pairs(img0, img1, normalize=True, shift=SHIFT, scale=SCALE):
    """sgr_lpips_pack_pairs: two fp32 [n,3,H,W] (n <= 16) -> fp16 [2n,H,W,8]"""
    for name, t in (("img0", img0), ("img1", img1)):
        gpu_tensor("lpips.pack_pairs", name, t, (torch.float32,))
    n, _, H, W = img0.shape
    a, b = img0.contiguous(), img1.contiguous()
    out = torch.empty((2 * n, H, W, 8), dtype=torch.float16, device=img0.device)
    with torch.cuda.device(img0.device):
        nat.check(nat.lib().sgr_lpips_pack_pairs(a.data_ptr(), b.data_ptr(), n, H, W, int(bool(normalize)), _f3(shift), _f3(scale),
                                                 out.data_ptr(), stream(img0.device)), "sgr_lpips_pack_pairs")
    return out


def pack_frames(renders, gts, exposure_a=None, exposure_b=None, shift=SHIFT, scale=SCALE):
    """sgr_lpips_pack: lists of n <= 16 fp32 [3,H,W] renders and ground truths, per-frame device scalars or None -> fp16 [2n,H,W,8]"""
    n = len(renders)
    _, H, W = renders[0].shape
    keep = [t.contiguous() for t in list(renders) + list(gts)]
    table = (nat.SgrMetricFrame * n)()
    for i in range(n):
        a = None if exposure_a is None else exposure_a[i]
        b = None if exposure_b is None else exposure_b[i]
        table[i] = nat.SgrMetricFrame(keep[i].data_ptr(), keep[n + i].data_ptr(), None, None, nat.ptr(a), nat.ptr(b))
    dev = renders[0].device
    out = torch.empty((2 * n, H, W, 8), dtype=torch.float16, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().sgr_lpips_pack(n, table, H, W, _f3(shift), _f3(scale), out.data_ptr(), stream(dev)), "sgr_lpips_pack")
    return out


def conv_relu_f16(x, w, bias, stride, pad):
    """relu(conv2d(x, w, bias, stride, pad)) on sgr_lpips_conv: x [B,cin,h,w], w [cout,cin,k,k] (k 11, 5 or 3; cout a multiple of 64) and
    bias are rounded to fp16, the sums are fp32; the result is fp16 [B,cout,ho,wo], a channels-last strided view"""
    for name, t in (("x", x), ("w", w), ("bias", bias)):
        gpu_tensor("lpips.conv_relu_f16", name, t, F16_F32)
    B, cin, h, wd = x.shape
    cout, k = w.shape[0], w.shape[2]
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    if min(h, wd) + 2 * pad < k:
        raise RuntimeError(f"lpips.conv_relu_f16: a {h} x {wd} map has no output under kernel {k}, padding {pad}")
    cin_pad = round_up(cin, 8)
    xs = torch.zeros((B, h, wd, cin_pad), dtype=torch.float16, device=x.device)
    xs[..., :cin] = x.permute(0, 2, 3, 1).to(torch.float16)
    wp, bp = pack_weight(w, cin_pad), pack_bias(bias, cout, x.device)
    out = torch.empty((B, ho, wo, cout), dtype=torch.float16, device=x.device)
    c = nat.SgrLpipsConv()
    c.src, c.n, c.h, c.w, c.cin, c.ksize, c.stride, c.pad = xs.data_ptr(), B, h, wd, cin_pad, k, stride, pad
    c.weight, c.weight_elems, c.bias, c.cout, c.out = wp.data_ptr(), wp.numel(), bp.data_ptr(), cout, out.data_ptr()
    with torch.cuda.device(x.device):
        nat.check(nat.lib().sgr_lpips_conv(C.byref(c), stream(x.device)), "sgr_lpips_conv")
    return out.permute(0, 3, 1, 2)


def max_pool_f16(x):
    """max_pool2d(x, 3, 2) without padding on sgr_lpips_maxpool: fp16 [B,C,h,w] (C a multiple of 8) -> fp16 [B,C,(h-3)//2+1,(w-3)//2+1], a
    channels-last strided view"""
    gpu_tensor("lpips.max_pool_f16", "x", x, (torch.float16,))
    B, ch, h, w = x.shape
    if min(h, w) < 3:
        raise RuntimeError(f"lpips.max_pool_f16: h and w >= 3, got {h} x {w}")
    src = x.permute(0, 2, 3, 1).contiguous()
    out = torch.empty((B, (h - 3) // 2 + 1, (w - 3) // 2 + 1, ch), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        nat.check(nat.lib().sgr_lpips_maxpool(src.data_ptr(), B, h, w, ch, out.data_ptr(), stream(x.device)), "sgr_lpips_maxpool")
    return out.permute(0, 3, 1, 2)


def distance(f0, f1, weight):
    """one tap on sgr_lpips_distance: f0, f1 fp16 [n,P,C] channels-last, weight fp32 [C] -> (partials fp32 [n, ceil(P / 128)], the sums of
    d_p over each workgroup's pixels; per_pixel fp32 [n,P]).  The tap's distance is partials.double().sum(1) / P."""
    for name, t in (("f0", f0), ("f1", f1)):
        gpu_tensor("lpips.distance", name, t, (torch.float16,))
    gpu_tensor("lpips.distance", "weight", weight, (torch.float32,))
    n, P, ch = f0.shape
    maps = torch.cat([f0, f1]).contiguous()
    w = weight.contiguous()
    blocks = (P + nat.SGR_LPIPS_DIST_PIXELS - 1) // nat.SGR_LPIPS_DIST_PIXELS
    partials = torch.empty((n, blocks), dtype=torch.float32, device=f0.device)
    per_pixel = torch.empty((n, P), dtype=torch.float32, device=f0.device)
    with torch.cuda.device(f0.device):
        nat.check(nat.lib().sgr_lpips_distance(maps.data_ptr(), n, P, ch, w.data_ptr(), partials.data_ptr(), per_pixel.data_ptr(),
                                               stream(f0.device)), "sgr_lpips_distance")
    return partials, per_pixel


# ---- the whole metric ------------------------------------------------------------------------------------------------------------------
class LPIPS:
    def __init__(self, canon, device="cuda"):
        """canon: the tensors of normalize_state_dict / parts_state_dict; weights are packed here, once"""
        self.device = network_device(device, "lpips", "metric")
        self._keep = []
        w = self._weights = nat.SgrLpipsWeights()
        for i in range(5):
            wp = pack_conv(canon[f"conv{i + 1}.weight"].to(self.device, torch.float32).to(torch.float16))
            bp = pack_bias(canon[f"conv{i + 1}.bias"].to(self.device, torch.float32), CHANNELS[i], self.device)
            lin = canon[f"lin{i}"].to(self.device, torch.float32).reshape(-1).contiguous()
            self._keep += [wp, bp, lin]
            w.conv[i].weight, w.conv[i].weight_elems, w.conv[i].bias, w.lin[i] = wp.data_ptr(), wp.numel(), bp.data_ptr(), lin.data_ptr()
        for c in range(3):
            w.shift[c], w.scale[c] = float(canon["shift"][c]), float(canon["scale"][c])
        self.launches = len(LAUNCH_NAMES)
        self._scratch = ScratchCache()

    @classmethod
    def from_state_dict(cls, sd, device="cuda"):
        return cls(normalize_state_dict(sd), device)

    @classmethod
    def from_parts(cls, alexnet_sd, lin_sd, device="cuda"):
        return cls(parts_state_dict(alexnet_sd, lin_sd), device)

    @classmethod
    def synthetic(cls, seed, device="cuda"):
        return cls(normalize_state_dict(synthetic_state_dict(seed)), device)

    def _run(self, call):
        """enqueues the launches first_launch..last_launch of the record on the current stream"""
        n, H, W = call.n, call.H, call.W                            # one buffer per (size, stream), grown to the largest n seen
        run_forward(self, call, (H, W), lambda: nat.lib().sgr_lpips_scratch_bytes(n, H, W), f"lpips: unsupported sizes (n={n} H={H} W={W})",
                    "sgr_lpips_forward", grow=True)

    def _call(self, n, H, W, out, levels):
        call = nat.SgrLpipsCall()
        call.n, call.H, call.W, call.out, call.levels = n, H, W, out.data_ptr(), nat.ptr(levels)
        call.first_launch, call.last_launch = 0, self.launches - 1
        return call

    def frames(self, table, H, W, out, levels=None):
        """the metric of a table of n <= 16 SgrMetricFrame (render against ground truth; the first image is clamp(exp(a) render + b, 0, 1),
        NULL exposure = identity) into out fp32 [n] and levels fp32 [n,5], both on the metric's device like the table's tensors, which
        the caller keeps alive"""
        if out.device != self.device or (levels is not None and levels.device != self.device):
            raise RuntimeError(f"lpips: the outputs are on {out.device}, the metric on {self.device}")
        call = self._call(len(table), H, W, out, levels)
        call.frames = table
        self._run(call)

    def lpips(self, img0, img1, normalize=True, return_levels=False):
        for name, t in (("img0", img0), ("img1", img1)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
                raise ValueError(f"lpips: {name} must be [N,3,H,W], got {tuple(getattr(t, 'shape', ()))}")
        if img0.shape != img1.shape:
            raise ValueError(f"lpips: img0 is {tuple(img0.shape)}, img1 {tuple(img1.shape)}")
        N, _, H, W = img0.shape
        tap_sizes(H, W)
        for name, t in (("img0", img0), ("img1", img1)):
            gpu_tensor("lpips", name, t, (torch.float16, torch.float32, torch.float64))
            if t.device != self.device:
                raise RuntimeError(f"lpips: {name} is on {t.device}, the metric on {self.device}")
        a, b = img0.detach().to(torch.float32).contiguous(), img1.detach().to(torch.float32).contiguous()
        out = torch.empty(N, dtype=torch.float32, device=self.device)
        levels = torch.empty((N, 5), dtype=torch.float32, device=self.device)
        for c0 in range(0, N, CHUNK):
            n = min(CHUNK, N - c0)
            call = self._call(n, H, W, out[c0:], levels[c0:])
            call.img0, call.img1, call.normalize = a[c0:].data_ptr(), b[c0:].data_ptr(), int(bool(normalize))
            self._run(call)
        return levels if return_levels else out

    __call__ = lpips
