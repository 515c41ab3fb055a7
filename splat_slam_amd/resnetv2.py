"""The ResNet-V2 backbone of the mono-depth prior (the stem and the three bottleneck stages in front of the transformer; DESIGN.md
section 3, "Mono-depth prior", states the equations) on the gfx950 kernels `sgr_resnet_*` (include/splat_hip.h, csrc/sgr_resnet.hip).
Inference only: no autograd, no nn.Module.

    ResNetV2(sd, cfg=MonoDepthConfig(), device="cuda")    sd: the keys of mono_depth.state_shapes(cfg) below
    ResNetV2.from_state_dict(sd, cfg, device)             "pretrained.model.patch_embed.backbone." and nothing else
    ResNetV2.synthetic(seed, cfg, device)                 the backbone tensors of mono_depth.synthetic_state_dict(seed, cfg)
    net(x [B,3,H,W] fp16 / fp32) -> (l1, l2, l3)          fp16 [B,C0,H/4,W/4], [B,C1,H/8,W/8], [B,C2,H/16,W/16]: channels-last strided
                                                          views of the kernel's buffers, no copy
    net.channels_last(x) -> (l1, l2, l3)                  the buffers themselves, [B, h * w, C]; l3 is what VisionTransformer.tokens reads
    LAUNCH_NAMES(cfg)                                     the launches of sgr_resnet_forward in order; net.launches is their number
    normalize_state_dict(sd, cfg)                         the validation alone (touches no device); backbone_shapes(cfg) lists the keys
    standardized_f16(w), pack_conv(w)                     what the network holds of a kernel: standardised in fp32, rounded to fp16, packed
    conv2d_same_f16(x, w, stride=1, padding="same", bias=None, act="none")      the bare convolution on NCHW
    group_norm_f16(x, groups, gamma, beta, relu=False, residual=None)           the bare group norm on NCHW
    max_pool_same_f16(x)                                                        the bare 3x3 stride-2 pool on NCHW

H and W are positive multiples of 32 (ValueError otherwise).  The caller's normalisation is applied before the call, as MonoDepth.predict
does.  All work goes on the current torch stream, nothing synchronises with the host, the input is not modified, every output is
bitwise reproducible and image i of a batch gives the bits of that image alone.  Scratch is cached per (shape, stream), the four most
recent kept.  A missing kernel or a CPU tensor is an error: there is no eager fallback.
"""
import ctypes as C

import torch

from splat_slam_amd import _native as nat
from splat_slam_amd import mono_depth as M
from splat_slam_amd._nn_common import (F16_F32, ScratchCache, gpu_tensor, network_device, pack_weight, round_up, run_forward, stream,
                                       tensor_desc)

__all__ = ["ResNetV2", "LAUNCH_NAMES", "LAYER_NAMES", "backbone_shapes", "normalize_state_dict", "standardized_f16", "pack_conv",
           "conv2d_same_f16", "group_norm_f16", "max_pool_same_f16"]

_BACKBONE = M._BACKBONE


def _check_cfg(cfg):
    cfg.check()
    widths = (cfg.stem_chs,) + tuple(cfg.stage_chs) + tuple(c // 4 for c in cfg.stage_chs)
    if cfg.stem_chs % 16 or any(c % 64 or c > 1024 for c in cfg.stage_chs) or cfg.stem_chs > 1024 or cfg.gn_groups > 256:
        raise ValueError(f"resnetv2: the stem is a multiple of 16, the stages multiples of 64, all up to 1024, at most 256 groups; got {cfg}")
    for c in widths:
        per = c // cfg.gn_groups
        if per > 64 or per & (per - 1):
            raise ValueError(f"resnetv2: {c} channels in {cfg.gn_groups} groups is {per} per group; the kernels take a power of two up to 64")
    return cfg


def LAYER_NAMES(cfg):
    """the convolutions in the order of SgrResnetWeights.layers: stem.conv, then per block conv1, conv2, conv3 and, in a stage's first
    block, downsample.conv; the group norm of each is stem.norm, normN, downsample.norm"""
    names = ["stem.conv"]
    for p, _, _, _, _, down in M._blocks(cfg):
        p = p[len(_BACKBONE):]
        names += [p + "conv1", p + "conv2", p + "conv3"] + ([p + "downsample.conv"] if down else [])
    return tuple(names)


def _norm_of(name):
    return name[:-len("conv")] + "norm" if name.endswith(".conv") else name.replace("conv", "norm")


def LAUNCH_NAMES(cfg):
    """the launches of sgr_resnet_forward in order: 4 + sum over stages (6 blocks + 2)"""
    names = ["pack", "stem.conv", "stem.norm", "pool"]
    for p, _, _, _, _, down in M._blocks(cfg):
        p = p[len(_BACKBONE):]
        names += [p + "conv1", p + "norm1"]
        if down:
            names += [p + "downsample.conv", p + "downsample.norm"]
        names += [p + "conv2", p + "norm2", p + "conv3", p + "norm3"]
    return tuple(names)


def backbone_shapes(cfg):
    """key -> shape of every tensor the backbone reads: mono_depth.state_shapes restricted to the backbone"""
    return {k: v for k, v in M.state_shapes(cfg).items() if k.startswith(_BACKBONE)}


def normalize_state_dict(sd, cfg=M.MonoDepthConfig()):
    """Raises ValueError for a missing key, an unexpected key or a wrong shape; returns the tensors under the keys of backbone_shapes."""
    shapes = backbone_shapes(_check_cfg(cfg))
    for key, v in sd.items():
        if key not in shapes:
            raise ValueError(f"resnetv2: unexpected key {key!r} in the state dict")
        if not isinstance(v, torch.Tensor) or tuple(v.shape) != shapes[key]:
            raise ValueError(f"resnetv2: {key!r} must be a tensor of shape {shapes[key]}, got {tuple(getattr(v, 'shape', ()))}")
    missing = [k for k in shapes if k not in sd]
    if missing:
        raise ValueError(f"resnetv2: the state dict lacks {missing}")
    return {k: sd[k].detach() for k in shapes}


def standardized_f16(w):
    """a kernel as the network holds it: (w - mean) / sqrt(var + 1e-8) per output channel in fp32, rounded once to fp16"""
    return M.standardize(w.to(torch.float32)).to(torch.float16)


def pack_conv(w16):
    """[cout, cin, k, k] -> fp16 [cout][round_up(k * k * cin_pad, 32)], column tap * cin_pad + channel, cin_pad = round_up(cin, 8), zeros
    elsewhere"""
    return pack_weight(w16, round_up(w16.shape[1], 8))


# ---- the single kernels ----------------------------------------------------------------------------------------------------------------
def conv2d_same_f16(x, w, stride=1, padding="same", bias=None, act="none", out_dtype=torch.float16):
    """act(conv2d(x, w, bias)) on sgr_resnet_conv: x [B,cin,h,w] and w [cout,cin,k,k] (k = 1, 3 or 7; cout a multiple of 16) are rounded
    to fp16, the sums are fp32.  padding "same" is TF's (the smaller half in front, output ceil(h / stride)), an int is symmetric zero
    padding.  act: none, relu.  The result [B,cout,ho,wo] is out_dtype (fp16 or fp32)."""
    what = "resnetv2.conv2d_same_f16"
    for name, t in (("x", x), ("w", w)) + ((("bias", bias),) if bias is not None else ()):
        gpu_tensor(what, name, t, F16_F32)
    if act not in nat.SGR_RESNET_ACTS:
        raise RuntimeError(f"{what}: act must be one of {sorted(nat.SGR_RESNET_ACTS)}, got {act!r}")
    if x.dim() != 4 or w.dim() != 4 or w.shape[1] != x.shape[1] or w.shape[2] != w.shape[3] or min(x.shape) < 1:
        raise RuntimeError(f"{what}: x [B,cin,h,w] and w [cout,cin,k,k], got {tuple(x.shape)} and {tuple(w.shape)}")
    B, cin, h, wd = x.shape
    cout, k = w.shape[0], w.shape[2]
    if padding == "same":
        pt, pl = M.same_pad(h, k, stride)[0], M.same_pad(wd, k, stride)[0]
        ho, wo = -(-h // stride), -(-wd // stride)
    else:
        pt = pl = int(padding)
        ho, wo = (h + 2 * pt - k) // stride + 1, (wd + 2 * pl - k) // stride + 1
    dev = x.device
    cin_pad = round_up(cin, 8)
    wp = pack_weight(w, cin_pad)
    bp = None if bias is None else bias.to(torch.float16).to(torch.float32).contiguous()
    xs = torch.empty((B * h * wd, cin_pad), dtype=torch.float16, device=dev)
    out = torch.empty((B, cout, max(ho, 0), max(wo, 0)), dtype=out_dtype, device=dev)
    c = nat.SgrResnetConv()
    c.src, c.src_stride, c.cin, c.ksize, c.stride, c.n, c.h, c.w = xs.data_ptr(), cin_pad, cin_pad, k, stride, B, h, wd
    c.pad_top, c.pad_left, c.ho, c.wo = pt, pl, ho, wo
    c.weight, c.weight_elems, c.bias, c.cout, c.act = wp.data_ptr(), wp.numel(), nat.ptr(bp), cout, nat.SGR_RESNET_ACTS[act]
    c.out = out.data_ptr()
    c.out_kind = nat.SGR_UPDATE_OUT_NCHW_F16 if out_dtype == torch.float16 else nat.SGR_UPDATE_OUT_NCHW_F32
    lib = nat.lib()
    with torch.cuda.device(dev):
        desc = tensor_desc(x)
        if cin == 3:                        # the image pack of the encoders
            nat.check(lib.sgr_encoder_pack(C.byref(desc), B, h, wd, None, None, xs.data_ptr(), stream(dev)), "sgr_encoder_pack")
        else:
            nat.check(lib.sgr_update_pack(C.byref(desc), B, cin, h, wd, xs.data_ptr(), cin_pad, cin_pad, stream(dev)), "sgr_update_pack")
        nat.check(lib.sgr_resnet_conv(C.byref(c), stream(dev)), "sgr_resnet_conv")
    return out


def group_norm_f16(x, groups, gamma, beta, relu=False, residual=None):
    """relu?(residual + group_norm(x, groups, gamma, beta, eps=1e-5)) on sgr_resnet_stats and sgr_resnet_groupnorm: x [B,C,h,w] is taken
    as fp32 (the sums a convolution would hand over), gamma and beta [C] fp32, residual [B,C,h,w] rounded to fp16.  The result is fp16
    [B,C,h,w], a channels-last strided view."""
    what = "resnetv2.group_norm_f16"
    for name, t in (("x", x), ("gamma", gamma), ("beta", beta)) + ((("residual", residual),) if residual is not None else ()):
        gpu_tensor(what, name, t, F16_F32)
    if x.dim() != 4 or min(x.shape) < 1 or tuple(gamma.shape) != (x.shape[1],) or tuple(beta.shape) != (x.shape[1],):
        raise RuntimeError(f"{what}: x [B,C,h,w] with gamma and beta [C], got {tuple(x.shape)}, {tuple(gamma.shape)}, {tuple(beta.shape)}")
    if residual is not None and residual.shape != x.shape:
        raise RuntimeError(f"{what}: residual must be {tuple(x.shape)}, got {tuple(residual.shape)}")
    B, ch, h, w = x.shape
    dev = x.device
    raw = x.to(torch.float32).permute(0, 2, 3, 1).contiguous()
    stats = torch.empty((B, (h * w + 127) // 128, max(int(groups), 1), 4), dtype=torch.float32, device=dev)
    out = torch.empty((B, h, w, ch), dtype=torch.float16, device=dev)
    g32, b32 = gamma.to(torch.float32).contiguous(), beta.to(torch.float32).contiguous()
    res = None if residual is None else residual.to(torch.float16).permute(0, 2, 3, 1).contiguous()
    g = nat.SgrResnetNorm()
    g.raw, g.stats, g.n, g.hw, g.cout, g.groups, g.relu = raw.data_ptr(), stats.data_ptr(), B, h * w, ch, int(groups), int(bool(relu))
    g.gamma, g.beta, g.residual, g.residual_stride, g.out, g.out_stride = g32.data_ptr(), b32.data_ptr(), nat.ptr(res), ch, out.data_ptr(), ch
    lib = nat.lib()
    with torch.cuda.device(dev):
        nat.check(lib.sgr_resnet_stats(raw.data_ptr(), B, h * w, ch, int(groups), stats.data_ptr(), stream(dev)), "sgr_resnet_stats")
        nat.check(lib.sgr_resnet_groupnorm(C.byref(g), stream(dev)), "sgr_resnet_groupnorm")
    return out.permute(0, 3, 1, 2)


def max_pool_same_f16(x):
    """max_pool2d(x, 3, 2) with TF "same" padding filled with -inf on sgr_resnet_maxpool: fp16 [B,C,h,w] (C a multiple of 8) -> fp16
    [B,C,ceil(h/2),ceil(w/2)], a channels-last strided view"""
    what = "resnetv2.max_pool_same_f16"
    gpu_tensor(what, "x", x, (torch.float16,))
    if x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError(f"{what}: x must be a non-empty [B,C,h,w], got {tuple(x.shape)}")
    B, ch, h, w = x.shape
    src = x.permute(0, 2, 3, 1).contiguous()
    out = torch.empty((B, (h + 1) // 2, (w + 1) // 2, ch), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        nat.check(nat.lib().sgr_resnet_maxpool(src.data_ptr(), B, h, w, ch, out.data_ptr(), stream(x.device)), "sgr_resnet_maxpool")
    return out.permute(0, 3, 1, 2)


# ---- the whole backbone ----------------------------------------------------------------------------------------------------------------
class ResNetV2:
    def __init__(self, sd, cfg=M.MonoDepthConfig(), device="cuda"):
        sd = normalize_state_dict(sd, cfg)
        self.cfg = cfg
        self.device = network_device(device, "resnetv2", "backbone")
        self._keep = []
        names = LAYER_NAMES(cfg)
        self._layers = (nat.SgrResnetLayer * len(names))()
        for layer, name in zip(self._layers, names):
            f32 = lambda k: sd[_BACKBONE + k].to(self.device, torch.float32).contiguous()
            wp = pack_conv(standardized_f16(f32(name + ".weight")))
            gamma, beta = f32(_norm_of(name) + ".weight"), f32(_norm_of(name) + ".bias")
            self._keep += [wp, gamma, beta]
            layer.weight, layer.weight_elems, layer.gamma, layer.beta = wp.data_ptr(), wp.numel(), gamma.data_ptr(), beta.data_ptr()
        w = self._weights = nat.SgrResnetWeights()
        w.stem_chs, w.groups, w.num_layers, w.layers = cfg.stem_chs, cfg.gn_groups, len(names), self._layers
        for s in range(3):
            w.stage_chs[s], w.stage_blocks[s] = cfg.stage_chs[s], cfg.stage_layers[s]
        self.launches = len(LAUNCH_NAMES(cfg))
        self._scratch = ScratchCache()

    @classmethod
    def from_state_dict(cls, sd, cfg=M.MonoDepthConfig(), device="cuda"):
        return cls(sd, cfg, device)

    @classmethod
    def synthetic(cls, seed, cfg=M.MonoDepthConfig(), device="cuda"):
        shapes = backbone_shapes(_check_cfg(cfg))
        return cls({k: v for k, v in M.synthetic_state_dict(seed, cfg).items() if k in shapes}, cfg, device)

    def _prepare(self, x):
        """checks the argument, allocates the outputs and fills the call record: (record, the three [B, h * w, C] buffers)"""
        gpu_tensor("resnetv2", "x", x, F16_F32, "fp16 or fp32")
        if x.device != self.device:
            raise RuntimeError(f"resnetv2: x is on {x.device}, the backbone on {self.device}")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1 or x.shape[2] < 32 or x.shape[2] % 32 or x.shape[3] < 32 or x.shape[3] % 32:
            raise ValueError(f"resnetv2: x must be [B,3,H,W] with H and W positive multiples of 32, got {tuple(x.shape)}")
        B, _, H, W = x.shape
        outs = tuple(torch.empty((B, (H >> s) * (W >> s), c), dtype=torch.float16, device=self.device)
                     for s, c in zip((2, 3, 4), self.cfg.stage_chs))
        call = nat.SgrResnetCall()
        call._images = x                                        # kept alive with the record
        call.images = tensor_desc(x)
        call.n, call.H, call.W = B, H, W
        call.l1, call.l2, call.l3 = (t.data_ptr() for t in outs)
        call.first_launch, call.last_launch = 0, self.launches - 1
        return call, outs

    def _run(self, call):
        """enqueues the launches first_launch..last_launch of the record on the current stream"""
        n, H, W = call.n, call.H, call.W
        run_forward(self, call, (n, H, W), lambda: nat.lib().sgr_resnet_scratch_bytes(n, H, W, self.cfg.stem_chs, *self.cfg.stage_chs),
                    f"resnetv2: unsupported sizes (n={n} H={H} W={W})", "sgr_resnet_forward")

    def channels_last(self, x):
        call, outs = self._prepare(x)
        self._run(call)
        return outs

    def __call__(self, x):
        B, _, H, W = x.shape if isinstance(x, torch.Tensor) and x.dim() == 4 else (0, 0, 0, 0)
        outs = self.channels_last(x)
        return tuple(t.view(B, H >> s, W >> s, t.shape[2]).permute(0, 3, 1, 2) for s, t in zip((2, 3, 4), outs))
