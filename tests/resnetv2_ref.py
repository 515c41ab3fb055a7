"""fp64 statements of the ResNet-V2 backbone of the mono-depth prior (splat_slam_amd.resnetv2) and of its single operations, written from
their equations, and the torch compositions the GPU tests take as the scale of fp16 arithmetic: fp16 convolutions under the vendor
library's deterministic algorithm, fp32 F.group_norm, exactly what MonoDepth(backbone="torch") runs.

    conv_ref        zero padding (top, left, and whatever the output size needs after), then conv2d, + bias, relu?
    group_norm_ref  relu?(residual + group_norm(x) * gamma + beta), biased variance, eps = 1e-5
    pool_ref        3x3 stride-2 max over the map padded with -inf by TF "same" amounts
    backbone_ref    stem, pool and the three stages on prepared parameters (mono_depth_ref.prepare) -> (l1, l2, l3)
"""
import torch
import torch.nn.functional as F

from mono_depth_ref import BACKBONE, blocks, pad_same, prepare  # noqa: F401  (prepare is re-exported for the tests)


def out_size(i, k, s, before, after):
    return (i + before + after - k) // s + 1


def pad_explicit(x, k, s, padding):
    """x zero-padded for a convolution: padding "same" (TF: the smaller half in front) or an int (symmetric)"""
    if padding == "same":
        return pad_same(x, k, s)
    p = int(padding)
    return F.pad(x, (p, p, p, p)) if p else x


def conv_ref(x, w, stride=1, padding="same", bias=None, relu=False):
    """fp64 on the fp16-rounded x, w and bias"""
    r = lambda t: None if t is None else t.to(torch.float16).double()
    y = F.conv2d(pad_explicit(r(x), w.shape[-1], stride, padding), r(w), r(bias), stride=stride)
    return torch.relu(y) if relu else y


def conv_torch(x, w, stride=1, padding="same", bias=None, relu=False):
    """the fp16 convolution of the vendor library, held to its deterministic algorithm"""
    h = lambda t: None if t is None else t.to(torch.float16)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        y = F.conv2d(pad_explicit(h(x), w.shape[-1], stride, padding), h(w), h(bias), stride=stride)
    return torch.relu(y) if relu else y


def group_norm_ref(x, groups, gamma, beta, relu=False, residual=None):
    """fp64 from the sums: x as given (fp32 values), the residual rounded to fp16"""
    B, C, h, w = x.shape
    v = x.double().reshape(B, groups, -1)
    mean = v.mean(2, keepdim=True)
    var = ((v - mean) ** 2).mean(2, keepdim=True)
    y = ((v - mean) / torch.sqrt(var + 1e-5)).reshape(B, C, h, w) * gamma.double().reshape(1, C, 1, 1) + beta.double().reshape(1, C, 1, 1)
    if residual is not None:
        y = y + residual.to(torch.float16).double()
    return torch.relu(y) if relu else y


def group_norm_torch(x, groups, gamma, beta, relu=False, residual=None):
    """fp32 F.group_norm, rounded to fp16, then the residual and the ReLU in fp16, as the torch backbone composes them"""
    y = F.group_norm(x.float(), groups, gamma.float(), beta.float(), 1e-5).to(torch.float16)
    if residual is not None:
        y = y + residual.to(torch.float16)
    return torch.relu(y) if relu else y


def pool_ref(x):
    return F.max_pool2d(pad_same(x, 3, 2, float("-inf")), 3, 2)


def _backbone(P, cfg, x, cast):
    conv = lambda n, t, stride=1: F.conv2d(pad_same(t, P[n + ".weight"].shape[-1], stride), P[n + ".weight"], None, stride=stride)
    gn = lambda n, t: cast(F.group_norm(t, cfg.gn_groups, P[n + ".weight"], P[n + ".bias"], 1e-5))
    x = torch.relu(gn(BACKBONE + "stem.norm", conv(BACKBONE + "stem.conv", x, 2)))
    x = pool_ref(x)
    stages = []
    for p, s, b in blocks(cfg):
        stride = 2 if s > 0 and b == 0 else 1
        short = gn(p + "downsample.norm", conv(p + "downsample.conv", x, stride)) if b == 0 else x
        y = torch.relu(gn(p + "norm1", conv(p + "conv1", x)))
        y = torch.relu(gn(p + "norm2", conv(p + "conv2", y, stride)))
        x = torch.relu(gn(p + "norm3", conv(p + "conv3", y)) + short)
        if b == cfg.stage_layers[s] - 1:
            stages.append(x)
    return tuple(stages)


def backbone_ref(prepared, cfg, x):
    """the backbone in fp64 on the prepared parameters; x [B,3,H,W] (rounded to fp16 first, as the network reads it) -> (l1, l2, l3)"""
    P = {k: v.double().to(x.device) for k, v in prepared.items() if k.startswith(BACKBONE)}
    return _backbone(P, cfg, x.to(torch.float16).double(), lambda t: t)


def backbone_torch(prepared, cfg, x):
    """the same under torch.autocast: fp16 convolutions, fp32 group norms rounded to fp16"""
    P = {k: v.to(device=x.device, dtype=torch.float32) for k, v in prepared.items() if k.startswith(BACKBONE)}
    with torch.autocast("cuda", dtype=torch.float16), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        return tuple(t.float() for t in _backbone(P, cfg, x.to(torch.float16), lambda t: t.to(torch.float16)))
