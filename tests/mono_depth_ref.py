"""fp64 statement of the mono-depth prior (splat_slam_amd.mono_depth), written from its equations, and the torch composition of the same
weights under autocast that the GPU tests and scripts/mono_depth_times.py take as the scale of fp16 arithmetic.

    stem    relu(gn(conv7x7/2(x))), max-pool 3x3/2, both with TF "same" padding (-inf fill for the pool)
    block   relu(gn(conv1x1(relu(gn(conv3x3/s(relu(gn(conv1x1(x)))))))) + shortcut), shortcut = gn(conv1x1/s(x)) in the first block of a
            stage, else x; convolutions without bias, weights standardised per output channel, group norm with eps = 1e-5
    l1, l2  the outputs of stages 0 and 1; the patches of the transformer are the output of stage 2
    r3      conv1x1(tap3);  r4 = conv3x3/2 pad 1 (conv1x1(tap4))
    rcu(x)  conv2(relu(conv1(relu(x)))) + x
    fuse    out_conv(up2(rcu2(x [+ rcu1(skip)]))), up2 bilinear with align_corners=True
    head    relu(conv1x1(relu(conv3x3(up2(conv3x3(path1))))))
"""
import torch
import torch.nn.functional as F

import vit_ref as VR

BACKBONE = "pretrained.model.patch_embed.backbone."


def prepare(sd):
    """the values the network holds: backbone kernels standardised (in fp64) and then rounded to fp16, every other kernel and matrix
    and the decoder's biases rounded to fp16; group-norm parameters, the transformer's biases, norms, tokens and positions fp32"""
    out = {}
    for k, v in sd.items():
        r16 = lambda t: t.to(torch.float16).to(torch.float32)
        if k.startswith(BACKBONE):
            if v.dim() == 4:
                flat = v.double().reshape(v.shape[0], -1)
                mean = flat.mean(1, keepdim=True)
                var = ((flat - mean) ** 2).mean(1, keepdim=True)
                out[k] = r16(((flat - mean) / torch.sqrt(var + 1e-8)).reshape(v.shape))
            else:
                out[k] = v.float()
        elif k.startswith("pretrained.model.") or ".project." in k:
            out[k] = r16(v) if v.dim() >= 2 and not k.endswith(("cls_token", "pos_embed")) else v.float()
        else:
            out[k] = r16(v)
    return out


def pad_same(x, k, s, value=0.0):
    pads = []
    for i in (x.shape[3], x.shape[2]):
        total = max((-(-i // s) - 1) * s + k - i, 0)
        pads += [total // 2, total - total // 2]
    return F.pad(x, pads, value=value) if any(pads) else x


def blocks(cfg):
    for s, n in enumerate(cfg.stage_layers):
        for b in range(n):
            yield f"{BACKBONE}stages.{s}.blocks.{b}.", s, b


def network(P, cfg, x, vit, cast):
    """the data flow on parameters P; vit(patches) gives the two taps; cast(t) is applied to every map that leaves a norm or the ViT"""
    conv = lambda n, t, stride=1, padding=0: F.conv2d(t, P[n + ".weight"], P.get(n + ".bias"), stride=stride, padding=padding)
    gn = lambda n, t: cast(F.group_norm(t, cfg.gn_groups, P[n + ".weight"], P[n + ".bias"], 1e-5))
    same = lambda n, t, stride=1: conv(n, pad_same(t, P[n + ".weight"].shape[-1], stride), stride)
    up2 = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)
    x = torch.relu(gn(BACKBONE + "stem.norm", same(BACKBONE + "stem.conv", x, 2)))
    x = F.max_pool2d(pad_same(x, 3, 2, float("-inf")), 3, 2)
    stages = []
    for p, s, b in blocks(cfg):
        stride = 2 if s > 0 and b == 0 else 1
        short = gn(p + "downsample.norm", same(p + "downsample.conv", x, stride)) if b == 0 else x
        y = torch.relu(gn(p + "norm1", same(p + "conv1", x)))
        y = torch.relu(gn(p + "norm2", same(p + "conv2", y, stride)))
        x = torch.relu(gn(p + "norm3", same(p + "conv3", y)) + short)
        if b == cfg.stage_layers[s] - 1:
            stages.append(x)
    l1, l2, l3 = stages
    tap3, tap4 = (cast(t) for t in vit(l3))
    r3 = conv("pretrained.act_postprocess3.3", tap3)
    r4 = conv("pretrained.act_postprocess4.4", conv("pretrained.act_postprocess4.3", tap4), 2, 1)

    def rcu(n, t):
        return conv(n + ".conv2", torch.relu(conv(n + ".conv1", torch.relu(t), 1, 1)), 1, 1) + t

    def fuse(i, t, skip=None):
        n = f"scratch.refinenet{i}"
        if skip is not None:
            t = t + rcu(n + ".resConfUnit1", skip)
        return conv(n + ".out_conv", up2(rcu(n + ".resConfUnit2", t)))

    path = fuse(4, conv("scratch.layer4_rn", r4, 1, 1))
    path = fuse(3, path, conv("scratch.layer3_rn", r3, 1, 1))
    path = fuse(2, path, conv("scratch.layer2_rn", l2, 1, 1))
    path = fuse(1, path, conv("scratch.layer1_rn", l1, 1, 1))
    y = torch.relu(conv("scratch.output_conv.2", up2(conv("scratch.output_conv.0", path, 1, 1)), 1, 1))
    return torch.relu(conv("scratch.output_conv.4", y))[:, 0]


def vit_part(P):
    return {k[len("pretrained."):]: v for k, v in P.items() if (k.startswith("pretrained.model.") and not k.startswith(BACKBONE)) or ".project." in k}


def mono_depth_ref(prepared, cfg, x):
    """the network in fp64 on the prepared parameters; x [B,3,H,W] on any device -> [B,H,W]"""
    P = {k: v.double().to(x.device) for k, v in prepared.items()}
    vsd = vit_part(P)
    return network(P, cfg, x.double(), lambda t: VR.vit_ref(vsd, cfg.vit(), t), lambda t: t)


class TorchMonoDepth:
    """The same network as a composition of torch ops on fp32 parameters under torch.autocast: convolutions and linear maps in fp16
    through the vendor library, group norm, layer norm and softmax by autocast's rules, F.scaled_dot_product_attention."""

    def __init__(self, prepared, cfg, device):
        self.p = {k: v.to(device=device, dtype=torch.float32) for k, v in prepared.items()}
        self.cfg = cfg
        self.vit = VR.TorchVit(vit_part(self.p), cfg.vit(), device)

    def forward(self, x):
        with torch.autocast("cuda", dtype=torch.float16):
            return network(self.p, self.cfg, x.to(torch.float16), self.vit, lambda t: t.to(torch.float16)).float()

    __call__ = forward


def predict_by_hand(model, image):
    """predict_mono_depth of the reference around model.forward: resize to net_size (bilinear, align_corners=False, antialias), normalise
    with mean 0.5 and std 0.5, clamp to [0, 1], resize back bicubically, clamp"""
    x = F.interpolate(image.float(), size=tuple(model.cfg.net_size), mode="bilinear", align_corners=False, antialias=True)
    out = model.forward((x - 0.5) / 0.5).clamp(0, 1)
    return F.interpolate(out[None], size=tuple(image.shape[-2:]), mode="bicubic").clamp(0, 1)[0, 0]
