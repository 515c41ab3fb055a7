"""The mono-depth prior: Omnidata's DPTDepthModel(backbone="vitb_rn50_384") as the reference builds and calls it (src/mono_estimators.py,
thirdparty/mono_priors/omnidata/modules/midas/{dpt_depth,blocks,vit}.py), inference only, usable as Slam(..., mono_depth=MonoDepth...).

    MonoDepthConfig()                                     the reference's network; every width is a field
    MonoDepth.from_state_dict(sd, cfg=MonoDepthConfig(), device="cuda", backbone="torch", decoder="torch")
    MonoDepth.synthetic(seed, cfg=MonoDepthConfig(), device="cuda", backbone="torch", decoder="torch")
                                                          backbone, decoder: "torch" (the default) or "hip", independently
    m.forward(x [B,3,H,W]) -> [B,H,W] fp32                H and W multiples of 32; the network on a normalised image
    m.predict(image [1,3,H,W] in [0,1]) -> [H,W] fp32     the reference's predict_mono_depth without its file
    m(timestamp, image)                                   predict(image): the callable Slam, Tracker and MotionFilter take
    check_state_dict(sd, cfg)                             names and shapes only (works on meta tensors); state_shapes(cfg) lists them
    normalize_state_dict(sd, cfg)                         the tensors under the keys of state_shapes
    synthetic_state_dict(seed, cfg)                       the closed-form hash of update_op / vit
    same_pad(i, k, s), standardize(w)                     TF "same" padding amounts, weight standardisation

Data flow: backbone -> ViT -> reassemble -> layerN_rn -> refinenet4..1 -> head ("Mono-depth prior").  The
transformer is splat_slam_amd.vit on the sgr_vit_* kernels.  Every stride-1 convolution with symmetric zero padding (the two 1x1
reassemble maps, the four layerN_rn, the residual units, out_conv, the head) is the MFMA convolution sgr_update_conv with weights packed
once.  With backbone="torch" the ResNet-V2 backbone, the one 3x3 stride-2 reassemble convolution and the max-pool are torch ops in
fp16 with fp32 group norms; those convolutions run the vendor library's deterministic algorithm, so forward and predict repeat bit
for bit.  With backbone="hip" self.backbone is a splat_slam_amd.resnetv2.ResNetV2 on the sgr_resnet_* kernels: its stage maps stay
channels-last (the transformer and layer1_rn / layer2_rn read them without a copy or a pack launch), the stride-2 reassemble
convolution runs on sgr_resnet_conv, and an image inside a batch gives the bits of the image alone.  With decoder="torch" the adds,
ReLU and all resampling of the decoder and the two resizes of predict are torch ops, and every decoder convolution converts NCHW to
channels-last and back.  With decoder="hip" self.dpt is a
splat_slam_amd.dpt_decoder.DPTDecoder on the sgr_dpt_* kernels: every map from the stage maps to the depth plane stays channels-last
fp16, the decoder is one host call of 35 launches without a torch op in between (the adds and ReLUs sit in the convolutions' gathers
and epilogues), and predict runs each of its two resizes as one launch.  A CPU tensor or a missing kernel is an error: there is no
eager fallback.

Both state-dict functions accept the checkpoint's {"state_dict": ...} wrapper, whose keys lose their first 6 characters as in the
reference, and accept and ignore timm's classifier pretrained.model.head.*, the final pretrained.model.norm.* and
scratch.refinenet4.resConfUnit1.* (never run).
"""
import ctypes as C
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from splat_slam_amd import _native as nat
from splat_slam_amd import vit as V
from splat_slam_amd._nn_common import pack_bias, pack_weight, round_up, stream, tensor_desc

__all__ = ["MonoDepthConfig", "MonoDepth", "check_state_dict", "normalize_state_dict", "synthetic_state_dict", "state_shapes", "same_pad",
           "standardize"]

_BACKBONE = "pretrained.model.patch_embed.backbone."
_IGNORED = ("pretrained.model.head.", "pretrained.model.norm.", "scratch.refinenet4.resConfUnit1.")
HEAD_MID = 32


@dataclass(frozen=True)
class MonoDepthConfig:
    stem_chs: int = 64
    stage_chs: tuple = (256, 512, 1024)
    stage_layers: tuple = (3, 4, 9)
    gn_groups: int = 32
    dim: int = 768
    heads: int = 12
    depth: int = 12
    taps: tuple = (8, 11)
    pos_grid: int = 24
    features: int = 256
    net_size: tuple = (512, 512)

    def vit(self):
        return V.VitConfig(self.dim, self.heads, self.depth, tuple(self.taps), self.pos_grid, self.stage_chs[-1]).check()

    def check(self):
        self.vit()
        if len(self.stage_chs) != 3 or len(self.stage_layers) != 3 or min(self.stage_layers) < 1:
            raise ValueError("mono_depth: three stages with at least one block each")
        for c in (self.stem_chs,) + tuple(self.stage_chs) + tuple(c // 4 for c in self.stage_chs):
            if c < self.gn_groups or c % self.gn_groups:
                raise ValueError(f"mono_depth: {c} channels do not split into {self.gn_groups} groups")
        if self.features < 2 or self.features % 2 or self.net_size[0] % 32 or self.net_size[1] % 32 or min(self.net_size) < 32:
            raise ValueError("mono_depth: features is even, net_size a pair of multiples of 32")
        return self


def same_pad(i, k, s):
    """(before, after) of TF "same" padding for input size i, kernel k, stride s"""
    total = max((math.ceil(i / s) - 1) * s + k - i, 0)
    return total // 2, total - total // 2


def standardize(w, eps=1e-8):
    """(w - mean) / sqrt(biased variance + eps) per output channel, in the dtype of w"""
    flat = w.reshape(w.shape[0], -1)
    mean = flat.mean(1, keepdim=True)
    var = ((flat - mean) ** 2).mean(1, keepdim=True)
    return ((flat - mean) / torch.sqrt(var + eps)).reshape(w.shape)


def _blocks(cfg):
    """(key prefix, in, mid, out, stride, has downsample) of every bottleneck, in order"""
    cin = cfg.stem_chs
    for s, (out, n) in enumerate(zip(cfg.stage_chs, cfg.stage_layers)):
        for b in range(n):
            yield f"{_BACKBONE}stages.{s}.blocks.{b}.", cin, out // 4, out, (2 if s > 0 and b == 0 else 1), b == 0
            cin = out


def state_shapes(cfg):
    """key -> shape of every tensor the network reads"""
    cfg.check()
    s, f, D = {}, cfg.features, cfg.dim

    def conv(name, cout, cin, k, bias=True):
        s[name + ".weight"] = (cout, cin, k, k)
        if bias:
            s[name + ".bias"] = (cout,)

    def norm(name, c):
        s[name + ".weight"], s[name + ".bias"] = (c,), (c,)

    conv(_BACKBONE + "stem.conv", cfg.stem_chs, 3, 7, False)
    norm(_BACKBONE + "stem.norm", cfg.stem_chs)
    for p, cin, mid, out, _, down in _blocks(cfg):
        conv(p + "conv1", mid, cin, 1, False), norm(p + "norm1", mid)
        conv(p + "conv2", mid, mid, 3, False), norm(p + "norm2", mid)
        conv(p + "conv3", out, mid, 1, False), norm(p + "norm3", out)
        if down:
            conv(p + "downsample.conv", out, cin, 1, False), norm(p + "downsample.norm", out)
    for k, shape in V.state_shapes(cfg.vit()).items():
        s["pretrained." + k] = shape
    conv("pretrained.act_postprocess3.3", D, D, 1)
    conv("pretrained.act_postprocess4.3", D, D, 1)
    conv("pretrained.act_postprocess4.4", D, D, 3)
    for i, cin in enumerate((cfg.stage_chs[0], cfg.stage_chs[1], D, D)):
        conv(f"scratch.layer{i + 1}_rn", f, cin, 3, False)
    for i in (1, 2, 3, 4):
        conv(f"scratch.refinenet{i}.out_conv", f, f, 1)
        for u in ((2,) if i == 4 else (1, 2)):
            conv(f"scratch.refinenet{i}.resConfUnit{u}.conv1", f, f, 3)
            conv(f"scratch.refinenet{i}.resConfUnit{u}.conv2", f, f, 3)
    conv("scratch.output_conv.0", f // 2, f, 3)
    conv("scratch.output_conv.2", HEAD_MID, f // 2, 3)
    conv("scratch.output_conv.4", 1, HEAD_MID, 1)
    return s


def _select(sd, cfg):
    if "state_dict" in sd and not isinstance(sd["state_dict"], torch.Tensor):
        sd = {k[6:]: v for k, v in sd["state_dict"].items()}
    shapes = state_shapes(cfg)
    out = {}
    for key, v in sd.items():
        if key.startswith(_IGNORED):
            continue
        if key not in shapes:
            raise ValueError(f"mono_depth: unexpected key {key!r} in the state dict")
        if not isinstance(v, torch.Tensor) or tuple(v.shape) != shapes[key]:
            raise ValueError(f"mono_depth: {key!r} must be a tensor of shape {shapes[key]}, got {tuple(getattr(v, 'shape', ()))}")
        out[key] = v
    missing = [k for k in shapes if k not in out]
    if missing:
        raise ValueError(f"mono_depth: the state dict lacks {missing}")
    return out


def check_state_dict(sd, cfg=MonoDepthConfig()):
    """Raises ValueError for a missing key, an unexpected key or a wrong shape.  Reads no values."""
    _select(sd, cfg)


def normalize_state_dict(sd, cfg=MonoDepthConfig()):
    """The network's tensors out of a checkpoint, detached, under the keys of state_shapes(cfg)."""
    return {k: v.detach() for k, v in _select(sd, cfg).items()}


def synthetic_state_dict(seed, cfg=MonoDepthConfig()):
    """matrices and kernels from U(-1, 1) / sqrt(fan_in), biases and norm biases 0.1 U, norm scales 1 + 0.1 U, tokens and positions
    0.5 U, each tensor hashed under its own key as vit.synthetic_state_dict does"""
    sd = {}
    for key, shape in state_shapes(cfg).items():
        if key.endswith(("cls_token", "pos_embed")):
            sd[key] = V.synthetic_tensor(key, shape, seed, 0.5)
        elif len(shape) == 1:
            sd[key] = V.synthetic_tensor(key, shape, seed, 0.1, 1.0 if "norm" in key.rsplit(".", 2)[-2] and key.endswith("weight") else 0.0)
        else:
            sd[key] = V.synthetic_tensor(key, shape, seed, 1.0 / math.sqrt(math.prod(shape[1:])))
    return sd


class _Conv:
    """a stride-1 convolution with zero padding (k - 1) / 2 on sgr_update_conv, its weights packed once"""

    def __init__(self, w, b, device):
        self.cout, self.cin, self.k = w.shape[0], w.shape[1], w.shape[2]
        self.cin_pad = round_up(self.cin, 8)
        self.w = pack_weight(w.to(device), self.cin_pad, 64)
        self.b = pack_bias(None if b is None else b.to(device), self.cout, device, 64)

    def __call__(self, x, act="none", out_dtype=torch.float16):
        B, cin, h, w = x.shape
        dev = x.device
        xs = torch.empty((B * h * w, self.cin_pad), dtype=torch.float16, device=dev)
        with torch.cuda.device(dev):
            desc = tensor_desc(x)
            nat.check(nat.lib().sgr_update_pack(C.byref(desc), B, cin, h, w, xs.data_ptr(), self.cin_pad, self.cin_pad, stream(dev)),
                      "sgr_update_pack")
        return self.packed(xs, B, h, w, act, out_dtype)

    def packed(self, xs, B, h, w, act="none", out_dtype=torch.float16):
        """the convolution of a map that is already channels-last fp16 [B * h * w][cin_pad]: no pack launch"""
        dev = xs.device
        if xs.dtype != torch.float16 or not xs.is_contiguous() or xs.numel() != B * h * w * self.cin_pad:
            raise RuntimeError(f"mono_depth: a packed map must be contiguous fp16 [{B * h * w}][{self.cin_pad}], got {tuple(xs.shape)} {xs.dtype}")
        out = torch.empty((B, self.cout, h, w), dtype=out_dtype, device=dev)
        c = nat.SgrUpdateConv()
        c.src0, c.stride0, c.cin, c.ksize, c.E, c.h, c.w = xs.data_ptr(), self.cin_pad, self.cin_pad, self.k, B, h, w
        c.weight, c.weight_elems, c.bias, c.cout, c.act = self.w.data_ptr(), self.w.numel(), self.b.data_ptr(), self.cout, nat.SGR_UPDATE_ACTS[act]
        c.out = out.data_ptr()
        c.out_kind = nat.SGR_UPDATE_OUT_NCHW_F16 if out_dtype == torch.float16 else nat.SGR_UPDATE_OUT_NCHW_F32
        with torch.cuda.device(dev):
            nat.check(nat.lib().sgr_update_conv(C.byref(c), stream(dev)), "sgr_update_conv")
        return out


class _DownConv:
    """the 3x3 stride-2 reassemble convolution (zero padding 1, with bias) on sgr_resnet_conv, its weights packed once"""

    def __init__(self, w16, b16, device):
        from splat_slam_amd.resnetv2 import pack_conv
        self.cout, self.cin = w16.shape[0], w16.shape[1]
        self.cin_pad = round_up(self.cin, 8)
        self.w = pack_conv(w16.to(device))
        self.b = b16.to(device, torch.float32).contiguous()

    def __call__(self, x):
        B, cin, h, w = x.shape
        dev = x.device
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        xs = torch.empty((B * h * w, self.cin_pad), dtype=torch.float16, device=dev)
        out = torch.empty((B, self.cout, ho, wo), dtype=torch.float16, device=dev)
        c = nat.SgrResnetConv()
        c.src, c.src_stride, c.cin, c.ksize, c.stride, c.n, c.h, c.w = xs.data_ptr(), self.cin_pad, self.cin_pad, 3, 2, B, h, w
        c.pad_top, c.pad_left, c.ho, c.wo = 1, 1, ho, wo
        c.weight, c.weight_elems, c.bias, c.cout = self.w.data_ptr(), self.w.numel(), self.b.data_ptr(), self.cout
        c.out, c.out_kind = out.data_ptr(), nat.SGR_UPDATE_OUT_NCHW_F16
        lib = nat.lib()
        with torch.cuda.device(dev):
            desc = tensor_desc(x)
            nat.check(lib.sgr_update_pack(C.byref(desc), B, cin, h, w, xs.data_ptr(), self.cin_pad, self.cin_pad, stream(dev)), "sgr_update_pack")
            nat.check(lib.sgr_resnet_conv(C.byref(c), stream(dev)), "sgr_resnet_conv")
        return out


def _conv2d(x, w, b=None, stride=1, padding=0):
    """F.conv2d with the vendor library held to its deterministic algorithm: its default choice does not repeat bit for bit from call
    to call, and predict is stated to be reproducible"""
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        return F.conv2d(x, w, b, stride=stride, padding=padding)


def _conv_same(x, w, stride):
    """fp16 convolution with TF "same" padding"""
    (t, b), (l, r) = same_pad(x.shape[2], w.shape[2], stride), same_pad(x.shape[3], w.shape[3], stride)
    if t or b or l or r:
        x = F.pad(x, (l, r, t, b))
    return _conv2d(x, w, None, stride)


def _up2(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


BACKBONES = ("torch", "hip")
DECODERS = ("torch", "hip")


class MonoDepth:
    def __init__(self, sd, cfg=MonoDepthConfig(), device="cuda", backbone="torch", decoder="torch"):
        if backbone not in BACKBONES:
            raise ValueError(f"mono_depth: backbone must be one of {BACKBONES}, got {backbone!r}")
        if decoder not in DECODERS:
            raise ValueError(f"mono_depth: decoder must be one of {DECODERS}, got {decoder!r}")
        sd = normalize_state_dict(sd, cfg)
        self.backbone_kind = backbone
        self.decoder_kind = decoder
        self.cfg = cfg
        self.device = dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("mono_depth (MI355X build): the network lives on a GPU; there is no CPU path")
        if dev.index is None:
            self.device = dev = torch.device("cuda", torch.cuda.current_device())
        f32 = lambda k: sd[k].to(dev, torch.float32).contiguous()
        # backbone: weights standardised once in fp32, then rounded to fp16; group-norm parameters fp32
        self._std = {k[:-len(".weight")]: standardize(f32(k)).to(torch.float16) for k in sd if k.startswith(_BACKBONE) and sd[k].dim() == 4}
        self._gn = {k[:-len(".weight")]: (f32(k), f32(k[:-len("weight")] + "bias")) for k in sd
                    if k.startswith(_BACKBONE) and sd[k].dim() == 1 and k.endswith(".weight")}
        vit_keys = V.state_shapes(cfg.vit())
        self.vit = V.VisionTransformer({k: sd["pretrained." + k] for k in vit_keys}, cfg.vit(), dev)
        conv = lambda name, bias=True: _Conv(f32(name + ".weight"), f32(name + ".bias") if bias else None, dev)
        self._c = {n: conv(n) for n in ("pretrained.act_postprocess3.3", "pretrained.act_postprocess4.3", "scratch.output_conv.0",
                                        "scratch.output_conv.2", "scratch.output_conv.4")}
        for i in (1, 2, 3, 4):
            self._c[f"scratch.layer{i}_rn"] = conv(f"scratch.layer{i}_rn", False)
            self._c[f"scratch.refinenet{i}.out_conv"] = conv(f"scratch.refinenet{i}.out_conv")
            for u in ((2,) if i == 4 else (1, 2)):
                for j in (1, 2):
                    n = f"scratch.refinenet{i}.resConfUnit{u}.conv{j}"
                    self._c[n] = conv(n)
        self._down_w = f32("pretrained.act_postprocess4.4.weight").to(torch.float16)       # the 3x3 stride-2 convolution: torch, or
        self._down_b = f32("pretrained.act_postprocess4.4.bias").to(torch.float16)          # sgr_resnet_conv with backbone="hip"
        if backbone == "hip":
            from splat_slam_amd.resnetv2 import ResNetV2
            self.backbone = ResNetV2({k: v for k, v in sd.items() if k.startswith(_BACKBONE)}, cfg, dev)
            self._down = _DownConv(self._down_w, self._down_b, dev)
        if decoder == "hip":
            from splat_slam_amd.dpt_decoder import DPTDecoder
            self.dpt = DPTDecoder(sd, cfg, dev)

    @classmethod
    def from_state_dict(cls, sd, cfg=MonoDepthConfig(), device="cuda", backbone="torch", decoder="torch"):
        return cls(sd, cfg, device, backbone, decoder)

    @classmethod
    def synthetic(cls, seed, cfg=MonoDepthConfig(), device="cuda", backbone="torch", decoder="torch"):
        return cls(synthetic_state_dict(seed, cfg), cfg, device, backbone, decoder)

    # ---- the torch part: ResNet-V2 stem and stages in fp16, group norms in fp32 ----
    def _norm(self, name, x, relu):
        w, b = self._gn[name]
        y = F.group_norm(x.float(), self.cfg.gn_groups, w, b, 1e-5)
        return (torch.relu(y) if relu else y).to(torch.float16)

    def backbone(self, x):
        """x [B,3,H,W] fp16 -> (stage 0, stage 1, stage 2) at 1/4, 1/8 and 1/16 (backbone="hip" replaces this method by a ResNetV2)"""
        x = self._norm(_BACKBONE + "stem.norm", _conv_same(x, self._std[_BACKBONE + "stem.conv"], 2), True)
        (t, b), (l, r) = same_pad(x.shape[2], 3, 2), same_pad(x.shape[3], 3, 2)
        x = F.max_pool2d(F.pad(x, (l, r, t, b), value=float("-inf")), 3, 2)
        outs, blocks, first = [], list(_blocks(self.cfg)), 0
        for n in self.cfg.stage_layers:
            for p, _, _, _, stride, down in blocks[first:first + n]:
                short = x
                if down:
                    short = self._norm(p + "downsample.norm", _conv_same(x, self._std[p + "downsample.conv"], stride), False)
                y = self._norm(p + "norm1", _conv_same(x, self._std[p + "conv1"], 1), True)
                y = self._norm(p + "norm2", _conv_same(y, self._std[p + "conv2"], stride), True)
                y = self._norm(p + "norm3", _conv_same(y, self._std[p + "conv3"], 1), False)
                x = torch.relu(y + short)
            first += n
            outs.append(x)
        return outs

    # ---- the decoder on the MFMA convolution ----
    def _rcu(self, name, x):
        return self._c[name + ".conv2"](self._c[name + ".conv1"](torch.relu(x), "relu")) + x

    def _fusion(self, i, x, skip=None):
        n = f"scratch.refinenet{i}"
        if skip is not None:
            x = x + self._rcu(n + ".resConfUnit1", skip)
        return self._c[n + ".out_conv"](_up2(self._rcu(n + ".resConfUnit2", x)))

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("mono_depth (MI355X build): x must be a GPU tensor; there is no CPU path")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1 or x.shape[2] < 32 or x.shape[2] % 32 or x.shape[3] < 32 or x.shape[3] % 32:
            raise ValueError(f"mono_depth: x must be [B,3,H,W] with H and W positive multiples of 32, got {tuple(x.shape)}")
        if self.decoder_kind == "hip":
            return self._forward_hip_decoder(x)
        c = self._c
        if self.backbone_kind == "hip":
            # the stage maps stay channels-last: l3 is the transformer's patches, l1 and l2 are packed inputs of layer1_rn and layer2_rn
            B, _, H, W = x.shape
            l1, l2, l3 = self.backbone.channels_last(x.to(self.device, torch.float16))
            tap3, tap4 = self.vit.tokens(l3, H // 16, W // 16)
            r4 = self._down(c["pretrained.act_postprocess4.3"](tap4))
            skip2 = c["scratch.layer2_rn"].packed(l2, B, H // 8, W // 8)
            skip1 = c["scratch.layer1_rn"].packed(l1, B, H // 4, W // 4)
        else:
            l1, l2, l3 = self.backbone(x.to(self.device, torch.float16))
            tap3, tap4 = self.vit(l3)
            r4 = _conv2d(c["pretrained.act_postprocess4.3"](tap4), self._down_w, self._down_b, 2, 1)
            skip2, skip1 = c["scratch.layer2_rn"](l2), c["scratch.layer1_rn"](l1)
        r3 = c["pretrained.act_postprocess3.3"](tap3)
        path = self._fusion(4, c["scratch.layer4_rn"](r4))
        path = self._fusion(3, path, c["scratch.layer3_rn"](r3))
        path = self._fusion(2, path, skip2)
        path = self._fusion(1, path, skip1)
        y = c["scratch.output_conv.2"](_up2(c["scratch.output_conv.0"](path)), "relu")
        return c["scratch.output_conv.4"](y, "relu", torch.float32)[:, 0]

    def _forward_hip_decoder(self, x):
        """every map channels-last fp16 from the stage maps to the depth plane: the decoder is one call of sgr_dpt_forward"""
        from splat_slam_amd.dpt_decoder import pack_nchw
        B, _, H, W = x.shape
        x = x.to(self.device, torch.float16)
        if self.backbone_kind == "hip":
            l1, l2, l3 = self.backbone.channels_last(x)
            tap3, tap4 = self.vit.tokens(l3, H // 16, W // 16)
        else:
            l1, l2, l3 = self.backbone(x)
            tap3, tap4 = self.vit(l3)
            l1, l2 = pack_nchw(l1), pack_nchw(l2)
        return self.dpt(tap3, tap4, l1, l2, H, W)

    def predict(self, image):
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise RuntimeError("mono_depth (MI355X build): image must be a GPU tensor; there is no CPU path")
        if image.dim() != 4 or image.shape[0] != 1 or image.shape[1] != 3:
            raise ValueError(f"mono_depth: image must be [1,3,H,W], got {tuple(image.shape)}")
        if self.decoder_kind == "hip":
            from splat_slam_amd.dpt_decoder import resize_in, resize_out
            depth = self.forward(resize_in(image.float(), tuple(self.cfg.net_size)))
            return resize_out(depth[0], tuple(image.shape[-2:]))
        x = F.interpolate(image.float(), size=tuple(self.cfg.net_size), mode="bilinear", align_corners=False, antialias=True)
        out = self.forward((x - 0.5) / 0.5).clamp(0, 1)
        return F.interpolate(out[None], size=tuple(image.shape[-2:]), mode="bicubic").clamp(0, 1)[0, 0]

    def __call__(self, timestamp, image):
        return self.predict(image)
