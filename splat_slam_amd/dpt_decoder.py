"""The decoder of the mono-depth prior (reassemble, layerN_rn, the four fusion blocks and the head; DESIGN.md section 3, "Mono-depth
prior", states the equations) and the two resizes of MonoDepth.predict on the gfx950 kernels `sgr_dpt_*` (include/splat_hip.h,
csrc/sgr_dpt.hip; DESIGN.md section 3, "DPT decoder").  Inference only: no autograd, no nn.Module.

    DPTDecoder(sd, cfg=MonoDepthConfig(), device="cuda")  sd: the keys of mono_depth.state_shapes(cfg) outside backbone and transformer
    dec(tap3, tap4, l1, l2, H, W) -> [B,H,W] fp32         tap3, tap4 [B,dim,H/16,W/16] fp16 (the transformer's readouts, NCHW);
                                                          l1 [B, H/4 * W/4, C0], l2 [B, H/8 * W/8, C1] fp16 channels-last, contiguous
    LAUNCH_NAMES(cfg)                                     the 35 launches of sgr_dpt_forward in order; LAYER_NAMES(cfg) its 28 layers
    pack_nchw(x)                                          [B,C,h,w] -> [B, h * w, C] fp16 on sgr_update_pack (C a multiple of 8)
    conv_cl_f16(x, w, b=None, relu_in=False, relu=False, res0=None, res1=None, out_dtype=torch.float16)
    up2_cl_f16(x)                                         bilinear 2x, align_corners=True
    resize_in(image, size)                                fp32 [N,C,H,W] -> fp16 [N,C,h,w]: antialiased bilinear, then (x - 0.5) / 0.5
    resize_out(depth, size)                               fp32 [h,w] -> fp32 [H,W]: clamp, bicubic, clamp
    aa_taps(o, n_in, n_out), cubic_taps(o, n_in, n_out), up2_taps(o, n)
                                                          the host-side restatement of the kernels' index and weight tables, exact

A channels-last map is a tensor [B,h,w,C] fp16 whose last stride is 1 and whose pixels lie one row stride (a multiple of 8, at least
C) apart; a view [..., :C] of a wider buffer is one.  All work goes on the current torch stream, nothing synchronises with the host,
no input is modified, every output is bitwise reproducible and image i of a batch gives the bits of that image alone.  Scratch is
cached per (shape, stream), the four most recent kept.  A missing kernel or a CPU tensor is an error: there is no eager fallback.
"""
import ctypes as C
from fractions import Fraction

import torch

from splat_slam_amd import _native as nat
from splat_slam_amd._nn_common import (F16_F32, ScratchCache, gpu_tensor, network_device, pack_bias, pack_weight, round_up, run_forward, stream,
                                       tensor_desc)

__all__ = ["DPTDecoder", "LAUNCH_NAMES", "LAYER_NAMES", "pack_nchw", "conv_cl_f16", "up2_cl_f16", "resize_in", "resize_out", "aa_taps",
           "cubic_taps", "up2_taps"]


def _fusion_convs(i):
    return [f"refinenet{i}.resConfUnit{u}.conv{j}" for u in ((2,) if i == 4 else (1, 2)) for j in (1, 2)]


def LAUNCH_NAMES(cfg=None):
    """the launches of sgr_dpt_forward in order; their number does not depend on the widths"""
    names = ["pack3", "act_postprocess3.3", "pack4", "act_postprocess4.3", "act_postprocess4.4"] + [f"layer{i}_rn" for i in (1, 2, 3, 4)]
    for i in (4, 3, 2, 1):
        names += _fusion_convs(i) + [f"refinenet{i}.up2", f"refinenet{i}.out_conv"]
    return tuple(names + ["output_conv.0", "head.up2", "output_conv.2", "output_conv.4"])


def LAYER_NAMES(cfg=None):
    """the state-dict names of the convolutions in the order of SgrDptWeights.layer: the launches that are no pack and no up2"""
    return tuple(("pretrained." if n.startswith("act_") else "scratch.") + n for n in LAUNCH_NAMES(cfg)
                 if not n.startswith("pack") and not n.endswith("up2"))


def _cl(what, name, t):
    """the row stride of a channels-last map [B,h,w,C]"""
    gpu_tensor(what, name, t, (torch.float16,))
    if t.dim() != 4 or min(t.shape) < 1:
        raise RuntimeError(f"{what}: {name} must be a non-empty [B,h,w,C], got {tuple(t.shape)}")
    B, h, w, ch = t.shape
    s = t.stride(2) if w > 1 else t.stride(1) // w if h > 1 else t.stride(0) // (h * w) if B > 1 else round_up(ch, 8)
    ok = t.stride(3) == 1 or ch == 1
    ok = ok and (w == 1 or t.stride(2) == s) and (h == 1 or t.stride(1) == w * s) and (B == 1 or t.stride(0) == h * w * s)
    if not ok or s < ch or s % 8 or t.data_ptr() % 16:
        raise RuntimeError(f"{what}: {name} must be channels-last with a row stride that is a multiple of 8 and a 16-byte aligned base, got "
                           f"shape {tuple(t.shape)} strides {t.stride()}")
    return s


# ---- the single kernels ----------------------------------------------------------------------------------------------------------------
def pack_nchw(x):
    """[B,C,h,w] fp16 or fp32, any strides -> fp16 [B, h * w, C], C a multiple of 8 (sgr_update_pack)"""
    gpu_tensor("dpt_decoder.pack_nchw", "x", x, F16_F32)
    B, ch, h, w = x.shape
    if ch % 8:
        raise RuntimeError(f"dpt_decoder.pack_nchw: {ch} channels are no multiple of 8")
    out = torch.empty((B, h * w, ch), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        desc = tensor_desc(x)
        nat.check(nat.lib().sgr_update_pack(C.byref(desc), B, ch, h, w, out.data_ptr(), ch, ch, stream(x.device)), "sgr_update_pack")
    return out


def conv_cl_f16(x, w, b=None, relu_in=False, relu=False, res0=None, res1=None, out_dtype=torch.float16):
    """relu?(conv2d(relu_in?(x), w, b, padding=(k - 1) / 2)) + res0 + res1 on sgr_dpt_conv: x [B,h,w,cin] channels-last fp16 (cin a
    multiple of 8), w [cout,cin,k,k] (k = 1 or 3) and b [cout] rounded to fp16, fp32 sums, one rounding.  res0, res1: channels-last fp16
    [B,h,w,cout].  The result is [B,h,w,cout], fp16 or fp32."""
    what = "dpt_decoder.conv_cl_f16"
    sx = _cl(what, "x", x)
    gpu_tensor(what, "w", w, F16_F32)
    if b is not None:
        gpu_tensor(what, "b", b, F16_F32)
    if w.dim() != 4 or w.shape[1] != x.shape[3] or w.shape[2] != w.shape[3]:
        raise RuntimeError(f"{what}: x [B,h,w,cin] and w [cout,cin,k,k], got {tuple(x.shape)} and {tuple(w.shape)}")
    if out_dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"{what}: out_dtype must be fp16 or fp32, got {out_dtype}")
    B, h, wd, cin = x.shape
    cout, k = w.shape[0], w.shape[2]
    dev = x.device
    wp, bp = pack_weight(w, cin, 64), pack_bias(b, cout, dev, 64)
    so = round_up(cout, 8) if out_dtype == torch.float16 else cout
    out = (torch.zeros if so != cout else torch.empty)((B, h, wd, so), dtype=out_dtype, device=dev)
    c = nat.SgrDptConv()
    c.src, c.src_stride, c.cin, c.ksize, c.n, c.h, c.w = x.data_ptr(), sx, cin, k, B, h, wd
    c.weight, c.weight_elems, c.bias, c.cout, c.relu_in, c.relu = wp.data_ptr(), wp.numel(), bp.data_ptr(), cout, int(bool(relu_in)), int(bool(relu))
    for name, r in (("res0", res0), ("res1", res1)):
        if r is not None:
            s = _cl(what, name, r)
            if tuple(r.shape) != (B, h, wd, cout):
                raise RuntimeError(f"{what}: {name} must be {(B, h, wd, cout)}, got {tuple(r.shape)}")
            setattr(c, name, r.data_ptr()), setattr(c, name + "_stride", s)
    c.out, c.out_stride = out.data_ptr(), so
    c.out_kind = nat.SGR_UPDATE_OUT_CL_F16 if out_dtype == torch.float16 else nat.SGR_UPDATE_OUT_CL_F32
    with torch.cuda.device(dev):
        nat.check(nat.lib().sgr_dpt_conv(C.byref(c), stream(dev)), "sgr_dpt_conv")
    return out[..., :cout]


def up2_cl_f16(x):
    """F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) of a channels-last fp16 map [B,h,w,C] (C a multiple of 8) on
    sgr_dpt_up2 -> [B,2h,2w,C], contiguous"""
    sx = _cl("dpt_decoder.up2_cl_f16", "x", x)
    B, h, w, ch = x.shape
    out = torch.empty((B, 2 * h, 2 * w, ch), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        nat.check(nat.lib().sgr_dpt_up2(x.data_ptr(), B, h, w, ch, sx, out.data_ptr(), ch, stream(x.device)), "sgr_dpt_up2")
    return out


def _planes(what, t, size):
    gpu_tensor(what, "the input", t, (torch.float32,))
    if t.dim() < 2 or min(t.shape) < 1 or len(size) != 2 or min(size) < 1:
        raise RuntimeError(f"{what}: a non-empty [..., H, W] and a size (h, w), got {tuple(t.shape)} and {tuple(size)}")
    return t.contiguous(), int(t.numel() // (t.shape[-1] * t.shape[-2]))


def resize_in(image, size):
    """(F.interpolate(image, size, mode="bilinear", align_corners=False, antialias=True) - 0.5) / 0.5 as fp16, one launch of
    sgr_dpt_resize_in: image fp32 [..., H, W] -> fp16 [..., h, w]"""
    src, planes = _planes("dpt_decoder.resize_in", image, size)
    out = torch.empty(tuple(image.shape[:-2]) + tuple(size), dtype=torch.float16, device=image.device)
    with torch.cuda.device(image.device):
        nat.check(nat.lib().sgr_dpt_resize_in(src.data_ptr(), planes, image.shape[-2], image.shape[-1], out.data_ptr(), size[0], size[1],
                                              stream(image.device)), "sgr_dpt_resize_in")
    return out


def resize_out(depth, size):
    """clamp(F.interpolate(clamp(depth, 0, 1), size, mode="bicubic"), 0, 1), one launch of sgr_dpt_resize_out: fp32 [..., h, w] -> fp32
    [..., H, W]"""
    src, planes = _planes("dpt_decoder.resize_out", depth, size)
    out = torch.empty(tuple(depth.shape[:-2]) + tuple(size), dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        nat.check(nat.lib().sgr_dpt_resize_out(src.data_ptr(), planes, depth.shape[-2], depth.shape[-1], out.data_ptr(), size[0], size[1],
                                               stream(depth.device)), "sgr_dpt_resize_out")
    return out


# ---- the tables of the two resizes, as the kernels compute them, in exact arithmetic -----------------------------------------------------
def aa_taps(o, n_in, n_out):
    """(first tap, [weights]) of output o of the antialiased triangle filter: with S = max(n_in, n_out), tap x weighs
    max(0, 2S - |(2x + 1) n_out - (2o + 1) n_in|), divided by the sum over the taps"""
    S, c = max(n_in, n_out), (2 * o + 1) * n_in
    lo, hi = c - 2 * S + n_out, c + 2 * S + n_out
    first, last = (0 if lo <= 0 else lo // (2 * n_out)), min(n_in, hi // (2 * n_out))
    w = [max(0, 2 * S - abs((2 * x + 1) * n_out - c)) for x in range(first, last)]
    return first, [Fraction(v, sum(w)) for v in w]


def up2_taps(o, n):
    """(i0, i1, t) of output o of the 2x bilinear upsampling with align_corners=True: o (n - 1) / (2n - 1) = i0 + t, i1 = min(i0 + 1, n - 1)"""
    num, den = o * (n - 1), 2 * n - 1
    return num // den, min(num // den + 1, n - 1), Fraction(num % den, den)


def cubic_taps(o, n_in, n_out):
    """([4 clamped indices], [4 weights]) of output o of the cubic convolution, A = -3/4, align_corners=False"""
    num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
    i0 = num // den
    t, A = Fraction(num - i0 * den, den), Fraction(-3, 4)
    inner = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    outer = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return [min(max(i0 - 1 + d, 0), n_in - 1) for d in range(4)], [outer(t + 1), inner(t), inner(1 - t), outer(2 - t)]


# ---- the whole decoder -------------------------------------------------------------------------------------------------------------------
class DPTDecoder:
    def __init__(self, sd, cfg, device="cuda"):
        cfg.check()
        D, f = cfg.dim, cfg.features
        if D % 16 or f % 16 or D > 1024 or f > 1024 or any(c % 8 or c > 1024 for c in cfg.stage_chs[:2]):
            raise ValueError(f"dpt_decoder: dim and features are multiples of 16, the stage widths multiples of 8, all up to 1024; got {cfg}")
        self.cfg = cfg
        self.device = network_device(device, "dpt_decoder", "decoder")
        dev = self.device
        self._keep = []
        w = self._weights = nat.SgrDptWeights()
        w.dim, w.features, w.chs0, w.chs1 = D, f, cfg.stage_chs[0], cfg.stage_chs[1]
        for layer, name in zip(w.layer, LAYER_NAMES(cfg)):
            f32 = lambda k: sd[k].detach().to(dev, torch.float32).contiguous()
            wt, b = f32(name + ".weight"), (f32(name + ".bias") if name + ".bias" in sd else None)
            if name.endswith("act_postprocess4.4"):        # sgr_resnet_conv: rows and bias unpadded, the kernel rounded to fp16 first
                wp = pack_weight(wt.to(torch.float16), round_up(wt.shape[1], 8))
                bp = b.to(torch.float16).to(torch.float32).contiguous()
            else:                                           # the packing of mono_depth._Conv
                wp, bp = pack_weight(wt, round_up(wt.shape[1], 8), 64), pack_bias(b, wt.shape[0], dev, 64)
            self._keep += [wp, bp]
            layer.weight, layer.weight_elems, layer.bias = wp.data_ptr(), wp.numel(), bp.data_ptr()
        self.launches = len(LAUNCH_NAMES(cfg))
        self._scratch = ScratchCache()

    def _prepare(self, tap3, tap4, l1, l2, H, W):
        """checks the arguments, allocates the depth plane and fills the call record: (record, depth [B,H,W])"""
        cfg, what = self.cfg, "dpt_decoder"
        if H < 32 or H % 32 or W < 32 or W % 32:
            raise ValueError(f"dpt_decoder: H and W must be positive multiples of 32, got {H} x {W}")
        for name, t in (("tap3", tap3), ("tap4", tap4), ("l1", l1), ("l2", l2)):
            gpu_tensor(what, name, t, (torch.float16,))
            if t.device != self.device:
                raise RuntimeError(f"dpt_decoder: {name} is on {t.device}, the decoder on {self.device}")
        B = tap3.shape[0]
        if tuple(tap3.shape) != (B, cfg.dim, H // 16, W // 16) or tap4.shape != tap3.shape or B < 1:
            raise RuntimeError(f"dpt_decoder: the taps must be [B,{cfg.dim},{H // 16},{W // 16}], got {tuple(tap3.shape)} and {tuple(tap4.shape)}")
        for name, t, s, ch in (("l1", l1, 4, cfg.stage_chs[0]), ("l2", l2, 8, cfg.stage_chs[1])):
            if tuple(t.shape) != (B, (H // s) * (W // s), ch) or not t.is_contiguous():
                raise RuntimeError(f"dpt_decoder: {name} must be contiguous [{B},{(H // s) * (W // s)},{ch}], got {tuple(t.shape)}")
        depth = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
        call = nat.SgrDptCall()
        call._inputs = (tap3, tap4, l1, l2)                     # kept alive with the record
        call.tap3, call.tap4, call.l1, call.l2 = tensor_desc(tap3), tensor_desc(tap4), l1.data_ptr(), l2.data_ptr()
        call.n, call.H, call.W, call.depth = B, H, W, depth.data_ptr()
        call.first_launch, call.last_launch = 0, self.launches - 1
        return call, depth

    def _run(self, call):
        """enqueues the launches first_launch..last_launch of the record on the current stream"""
        n, H, W = call.n, call.H, call.W
        run_forward(self, call, (n, H, W), lambda: nat.lib().sgr_dpt_scratch_bytes(n, H, W, self.cfg.dim, self.cfg.features),
                    f"dpt_decoder: unsupported sizes (n={n} H={H} W={W})", "sgr_dpt_forward")

    def __call__(self, tap3, tap4, l1, l2, H, W):
        call, depth = self._prepare(tap3, tap4, l1, l2, H, W)
        self._run(call)
        return depth
