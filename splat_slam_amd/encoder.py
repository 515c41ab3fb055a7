"""The tracker's feature and context encoders (BasicEncoder of the reference's thirdparty/glorie_slam/modules/droid_net/extractor.py) on
the gfx950 kernels `sgr_encoder_*` (include/splat_hip.h, csrc/sgr_encoder.hip).  Inference only: no autograd, no nn.Module.

    Encoder(sd, which, device="cuda")                     which = "fnet" (out_dim 128, InstanceNorm2d) or "cnet" (out_dim 256, no norm);
    Encoder.from_state_dict(sd, which, device="cuda")     the reference's 32 keys (LAYER_SHAPES(out_dim)), optional "module." and
                                                          "fnet." / "cnet." prefixes, the other encoder and update.* ignored
    Encoder.synthetic(which, seed, device="cuda")         weights of synthetic_encoder_state_dict(which, seed)
    enc(images, mean=None, std=None)                      [b,n,3,H,W] -> [b,n,out_dim,h,w] fp16, h = ceil(H / 8)
    cnet.context(images, mean=None, std=None)             -> (tanh(net), relu(inp)), each [b,n,128,h,w] fp16, from the split epilogue
    synthetic_encoder_state_dict(which, seed)             fp32 CPU tensors by the update operator's hash of ("fnet." + key, index, seed)
    normalize_encoder_state_dict(sd, which)               the validation of from_state_dict alone (touches no device)
    conv2d_f16(x, w, b=None, stride=1, norm=None, act="none", residual=None, out_dtype=torch.float16)     the bare convolution on NCHW

images are fp16 or fp32 GPU tensors of any strides; mean and std (3 numbers each) make the pack launch store (x - mean[c]) / std[c].
All work goes on the current torch stream, nothing synchronises with the host, the input is not modified, every output is bitwise
reproducible and image i of a batch gives the bits of that image encoded alone.  With the instance norm every normalised map must hold
more than one element (the smallest is layer3's, ceil(H / 8) x ceil(W / 8)); torch raises there as well.  A missing kernel or a CPU
tensor is an error: there is no eager fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from splat_slam_amd import _native as nat
from splat_slam_amd._nn_common import (F16_F32, ScratchCache, gpu_tensor, hash_uniform, network_device, pack_bias, pack_weight, round_up,
                                       run_forward, stream, tensor_desc)

__all__ = ["Encoder", "synthetic_encoder_state_dict", "normalize_encoder_state_dict", "conv2d_f16", "ENCODER_LAYERS", "LAYER_SHAPES",
           "LAUNCH_NAMES", "OUT_DIM", "NORM"]

OUT_DIM = {"fnet": 128, "cnet": 256}
NORM = {"fnet": "instance", "cnet": "none"}
# name: (cout, cin, kernel size, stride), in the order of SgrEncoderWeights.layer; cout None = out_dim
ENCODER_LAYERS = {
    "conv1": (32, 3, 7, 2),
    "layer1.0.conv1": (32, 32, 3, 1), "layer1.0.conv2": (32, 32, 3, 1), "layer1.1.conv1": (32, 32, 3, 1), "layer1.1.conv2": (32, 32, 3, 1),
    "layer2.0.conv1": (64, 32, 3, 2), "layer2.0.conv2": (64, 64, 3, 1), "layer2.0.downsample.0": (64, 32, 1, 2),
    "layer2.1.conv1": (64, 64, 3, 1), "layer2.1.conv2": (64, 64, 3, 1),
    "layer3.0.conv1": (128, 64, 3, 2), "layer3.0.conv2": (128, 128, 3, 1), "layer3.0.downsample.0": (128, 64, 1, 2),
    "layer3.1.conv1": (128, 128, 3, 1), "layer3.1.conv2": (128, 128, 3, 1),
    "conv2": (None, 128, 1, 1),
}


def LAYER_SHAPES(out_dim):
    """the 32 state-dict keys of BasicEncoder(out_dim) and their shapes (the instance-norm variant has no further keys)"""
    shapes = {}
    for name, (cout, cin, k, _) in ENCODER_LAYERS.items():
        cout = out_dim if cout is None else cout
        shapes[name + ".weight"] = (cout, cin, k, k)
        shapes[name + ".bias"] = (cout,)
    return shapes


def _launch_names(norm):
    """the launches of sgr_encoder_forward in order: a strided block runs conv1, downsample, conv2"""
    order = list(ENCODER_LAYERS)
    for blk in ("layer2.0", "layer3.0"):
        i = order.index(blk + ".conv2")
        order[i], order[i + 1] = order[i + 1], order[i]
    names = ["pack"]
    for name in order:
        names.append(name)
        if norm and name != "conv2":
            names.append(name + ":norm")
    return tuple(names)


LAUNCH_NAMES = {"fnet": _launch_names(True), "cnet": _launch_names(False)}


def _which(which):
    if which not in OUT_DIM:
        raise ValueError(f"encoder: which must be 'fnet' or 'cnet', got {which!r}")
    return which


def synthetic_encoder_state_dict(which, seed):
    """Every tensor of LAYER_SHAPES(out_dim) from the closed-form hash of update_op on the full key name (e.g. "fnet.conv1.weight"):
    weights U(-sqrt(3 / fan_in), sqrt(3 / fan_in)) (unit gain, so that the no-norm cnet neither decays nor saturates over its 16 layers),
    biases U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), fan_in = cin * k * k."""
    sd = {}
    for key, shape in LAYER_SHAPES(OUT_DIM[_which(which)]).items():
        _, cin, k, _ = ENCODER_LAYERS[key.rsplit(".", 1)[0]]
        fan_in = cin * k * k
        scale = math.sqrt(3.0 / fan_in) if key.endswith(".weight") else 1.0 / math.sqrt(fan_in)
        v = hash_uniform(which + "." + key, int(np.prod(shape)), seed) * scale
        sd[key] = torch.from_numpy(v.astype(np.float32).reshape(shape))
    return sd


def normalize_encoder_state_dict(sd, which):
    """One encoder's tensors out of a checkpoint, as fp32 CPU tensors under the keys of LAYER_SHAPES(out_dim).  Keys may carry "module."
    and the encoder's own prefix; the other encoder's keys and update.* are ignored.  Raises ValueError for a missing key, an
    unexpected key or a wrong shape."""
    shapes = LAYER_SHAPES(OUT_DIM[_which(which)])
    other = "cnet." if which == "fnet" else "fnet."
    out = {}
    for key, v in sd.items():
        k = key[len("module."):] if key.startswith("module.") else key
        if k.startswith((other, "update.")):
            continue
        k = k[len(which) + 1:] if k.startswith(which + ".") else k
        if k not in shapes:
            raise ValueError(f"encoder {which}: unexpected key {key!r} in the state dict")
        if k in out:
            raise ValueError(f"encoder {which}: key {key!r} appears twice once its prefixes are stripped")
        if not isinstance(v, torch.Tensor):
            raise ValueError(f"encoder {which}: {key!r} must be a torch.Tensor")
        if tuple(v.shape) != shapes[k]:
            raise ValueError(f"encoder {which}: {key!r} must have shape {shapes[k]}, got {tuple(v.shape)}")
        out[k] = v.detach().to("cpu", torch.float32)
    missing = [k for k in shapes if k not in out]
    if missing:
        raise ValueError(f"encoder {which}: the state dict lacks {missing}")
    return out


def _out_size(v, stride):
    return (v - 1) // stride + 1


def _three(what, name, v):
    v = [float(x) for x in (v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else v)]
    if len(v) != 3:
        raise RuntimeError(f"{what}: {name} must hold 3 numbers, got {len(v)}")
    return v


def conv2d_f16(x, w, b=None, stride=1, norm=None, act="none", residual=None, out_dtype=torch.float16):
    """conv2d(x, w, b) with zero padding (k - 1) / 2 and stride 1 or 2 on the encoder's kernel: x [B,cin,h,w] and w [cout,cin,k,k] (k = 1, 3
    or 7; cout = 32, 64, 128 or 256) are rounded to fp16, the sums are fp32.  norm None: v = act(sum + b); norm "instance" (cout <= 128):
    v = act(InstanceNorm2d(sum)), the bias cancelling.  act: none, relu.  With residual [B,cout,ho,wo] (rounded to fp16) the result is
    relu(residual + v).  act "split" (cout = 256, no norm, no residual) returns (tanh(v[:, :128]), relu(v[:, 128:])) in fp16.  The
    result [B,cout,ho,wo] is out_dtype (fp16 or fp32), ho = (h - 1) // stride + 1."""
    what = "encoder.conv2d_f16"
    for name, t in (("x", x), ("w", w)) + ((("b", b),) if b is not None else ()) + ((("residual", residual),) if residual is not None else ()):
        gpu_tensor(what, name, t, F16_F32, "fp16 or fp32")
    if act not in nat.SGR_ENCODER_ACTS:
        raise RuntimeError(f"{what}: act must be one of {sorted(nat.SGR_ENCODER_ACTS)}, got {act!r}")
    if norm not in (None, "none", "instance"):
        raise RuntimeError(f"{what}: norm must be None or 'instance', got {norm!r}")
    normed = norm == "instance"
    if out_dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"{what}: out_dtype must be fp16 or fp32, got {out_dtype}")
    if stride not in (1, 2):
        raise RuntimeError(f"{what}: stride must be 1 or 2, got {stride}")
    if x.dim() != 4 or w.dim() != 4 or w.shape[1] != x.shape[1] or w.shape[2] != w.shape[3] or w.shape[2] not in (1, 3, 7):
        raise RuntimeError(f"{what}: x [B,cin,h,w] and w [cout,cin,k,k] with k in (1, 3, 7), got {tuple(x.shape)} and {tuple(w.shape)}")
    B, cin, h, wd = x.shape
    cout, k = w.shape[0], w.shape[2]
    if min(B, cin, h, wd) < 1 or cout not in (32, 64, 128, 256) or (b is not None and tuple(b.shape) != (cout,)):
        raise RuntimeError(f"{what}: empty tensor, cout {cout} not in (32, 64, 128, 256) or a bias that is not [{cout}]")
    ho, wo = _out_size(h, stride), _out_size(wd, stride)
    if residual is not None and tuple(residual.shape) != (B, cout, ho, wo):
        raise RuntimeError(f"{what}: residual must be [{B},{cout},{ho},{wo}], got {tuple(residual.shape)}")
    if act == "split" and (cout != 256 or normed or residual is not None):
        raise RuntimeError(f"{what}: act 'split' needs cout = 256, no norm and no residual")
    if normed and cout > 128:
        raise RuntimeError(f"{what}: a normalised convolution has cout <= 128, got {cout}")
    dev = x.device
    cin_pad = round_up(cin, 8)
    lib = nat.lib()
    c = nat.SgrEncoderConv()
    wp, bp = pack_weight(w, cin_pad), pack_bias(b, cout, dev)
    keep = [wp, bp]
    xs = torch.empty((B * h * wd, cin_pad), dtype=torch.float16, device=dev)
    c.src, c.src_stride, c.cin, c.ksize, c.stride, c.n, c.h, c.w = xs.data_ptr(), cin_pad, cin_pad, k, stride, B, h, wd
    c.weight, c.weight_elems, c.bias, c.cout = wp.data_ptr(), wp.numel(), bp.data_ptr(), cout
    c.norm = nat.SGR_ENCODER_NORM_INSTANCE if normed else nat.SGR_ENCODER_NORM_NONE
    c.act = nat.SGR_ENCODER_ACTS[act]
    if residual is not None:
        res = residual.to(torch.float16).permute(0, 2, 3, 1).contiguous()
        keep.append(res)
        c.residual, c.residual_stride = res.data_ptr(), cout
    if act == "split":
        out = tuple(torch.empty((B, 128, ho, wo), dtype=torch.float16, device=dev) for _ in range(2))
        c.out, c.out2 = out[0].data_ptr(), out[1].data_ptr()
    elif normed:
        cl = torch.empty((B, ho, wo, cout), dtype=out_dtype, device=dev)            # the apply launch writes channels-last
        raw = torch.empty((B * ho * wo, cout), dtype=torch.float32, device=dev)
        stats = torch.empty((B, (ho * wo + 127) // 128, cout, 4), dtype=torch.float32, device=dev)
        keep += [raw, stats]
        c.out, c.out_stride = cl.data_ptr(), cout
        c.out_kind = nat.SGR_UPDATE_OUT_CL_F16 if out_dtype == torch.float16 else nat.SGR_UPDATE_OUT_CL_F32
        c.raw, c.raw_elems, c.stats, c.stats_elems = raw.data_ptr(), raw.numel(), stats.data_ptr(), stats.numel()
        out = cl.permute(0, 3, 1, 2)
    else:
        out = torch.empty((B, cout, ho, wo), dtype=out_dtype, device=dev)
        c.out = out.data_ptr()
        c.out_kind = nat.SGR_UPDATE_OUT_NCHW_F16 if out_dtype == torch.float16 else nat.SGR_UPDATE_OUT_NCHW_F32
    with torch.cuda.device(dev):
        desc = tensor_desc(x)
        if cin == 3:                        # the image pack of the encoders
            nat.check(lib.sgr_encoder_pack(C.byref(desc), B, h, wd, None, None, xs.data_ptr(), stream(dev)), "sgr_encoder_pack")
        else:
            nat.check(lib.sgr_update_pack(C.byref(desc), B, cin, h, wd, xs.data_ptr(), cin_pad, cin_pad, stream(dev)), "sgr_update_pack")
        nat.check(lib.sgr_encoder_conv(C.byref(c), stream(dev)), "sgr_encoder_conv")
    return out.contiguous() if normed else out


class Encoder:
    def __init__(self, sd, which, device="cuda"):
        self.which = _which(which)
        sd = normalize_encoder_state_dict(sd, which)
        self.out_dim, self.norm = OUT_DIM[which], NORM[which]
        self.device = network_device(device, "encoder", "encoder")
        self._keep = []
        self._weights = nat.SgrEncoderWeights()
        self._weights.out_dim = self.out_dim
        self._weights.norm = nat.SGR_ENCODER_NORM_INSTANCE if self.norm == "instance" else nat.SGR_ENCODER_NORM_NONE
        for i, (name, (_, cin, _, _)) in enumerate(ENCODER_LAYERS.items()):
            w, b = sd[name + ".weight"], sd[name + ".bias"]
            wp = pack_weight(w, round_up(cin, 8)).to(self.device)
            bp = pack_bias(b, w.shape[0], "cpu").to(self.device)
            self._keep += [wp, bp]
            self._weights.layer[i].weight, self._weights.layer[i].weight_elems = wp.data_ptr(), wp.numel()
            self._weights.layer[i].bias = bp.data_ptr()
        self.launches = len(LAUNCH_NAMES[which])
        self._scratch = ScratchCache()

    @classmethod
    def from_state_dict(cls, sd, which, device="cuda"):
        return cls(sd, which, device)

    @classmethod
    def synthetic(cls, which, seed, device="cuda"):
        return cls(synthetic_encoder_state_dict(which, seed), which, device)

    def _prepare(self, images, mean, std, split):
        """checks the arguments, allocates the outputs and fills the call record: (record, outputs)"""
        what = f"encoder {self.which}"
        gpu_tensor(what, "images", images, F16_F32, "fp16 or fp32")
        if images.device != self.device:
            raise RuntimeError(f"{what}: images is on {images.device}, the encoder on {self.device}")
        if images.dim() != 5 or images.shape[2] != 3:
            raise RuntimeError(f"{what}: images must be [b,n,3,H,W], got {tuple(images.shape)}")
        b, n, _, H, W = images.shape
        if min(b, n, H, W) < 1:
            raise RuntimeError(f"{what}: images is empty, shape {tuple(images.shape)}")
        if (mean is None) != (std is None):
            raise RuntimeError(f"{what}: mean and std come together")
        if split and self.which != "cnet":
            raise RuntimeError(f"{what}: context() is the context encoder's")
        h, w = H, W
        for _ in range(3):
            h, w = _out_size(h, 2), _out_size(w, 2)
        if self.norm == "instance" and h * w < 2:
            raise RuntimeError(f"{what}: the {H} x {W} image leaves layer3 a {h} x {w} map; an instance norm needs more than one element")
        call = nat.SgrEncoderCall()
        call._images = images.reshape(b * n, 3, H, W)           # a view wherever the strides allow one; kept alive with the record
        call.images = tensor_desc(call._images)
        call.n, call.H, call.W = b * n, H, W
        if mean is not None:
            call.normalize = 1
            call.mean, call.std_ = (C.c_float * 3)(*_three(what, "mean", mean)), (C.c_float * 3)(*_three(what, "std", std))
            if min(abs(s) for s in call.std_) == 0.0:
                raise RuntimeError(f"{what}: std must not be zero")
        if split:
            outs = tuple(torch.empty((b, n, 128, h, w), dtype=torch.float16, device=self.device) for _ in range(2))
            call.out, call.out2, call.split = outs[0].data_ptr(), outs[1].data_ptr(), 1
        else:
            outs = torch.empty((b, n, self.out_dim, h, w), dtype=torch.float16, device=self.device)
            call.out = outs.data_ptr()
        call.first_launch, call.last_launch = 0, self.launches - 1
        return call, outs

    def _run(self, call):
        """enqueues the launches first_launch..last_launch of the record on the current stream"""
        n, H, W = call.n, call.H, call.W
        run_forward(self, call, (n, H, W), lambda: nat.lib().sgr_encoder_scratch_bytes(n, H, W, self.out_dim, self._weights.norm),
                    f"encoder {self.which}: unsupported sizes (n={n} H={H} W={W})", "sgr_encoder_forward")

    def __call__(self, images, mean=None, std=None):
        call, out = self._prepare(images, mean, std, False)
        self._run(call)
        return out

    def context(self, images, mean=None, std=None):
        call, outs = self._prepare(images, mean, std, True)
        self._run(call)
        return outs
