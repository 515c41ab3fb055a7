"""The tracker's update operator (UpdateModule of the reference's thirdparty/glorie_slam/modules/droid_net/droid_net.py:83-153, with the
ConvGRU of gru.py and GraphAgg of droid_net.py:48-80) on the gfx950 kernels `sgr_update_*` (include/splat_hip.h, csrc/sgr_update.hip).
Inference only: no autograd, no nn.Module.

    UpdateOperator.from_state_dict(sd, device="cuda")     the reference's keys (LAYER_SHAPES), optional "module." / "update." prefixes,
                                                          fnet.* / cnet.* ignored, 3-row weight.2 / delta.2 cut to their first 2 rows
    UpdateOperator.synthetic(seed, device="cuda")         weights of synthetic_state_dict(seed)
    op(net, inp, corr, flow=None, ii=None, jj=None)       -> (net, delta, weight) or, with ii, (net, delta, weight, eta, upmask)
    synthetic_state_dict(seed)                            fp32 CPU tensors by a closed-form integer hash of (name, flat index, seed)
    normalize_state_dict(sd)                              the validation and slicing of from_state_dict alone (touches no device)
    conv2d_f16(x, w, b=None, act="none", out_dtype=torch.float16)   the bare convolution on NCHW tensors (1x1, 3x3, 7x7, zero padding)

net, inp [1,E,128,h,w], corr [1,E,196,h,w], flow [1,E,4,h,w] (None: zeros) are fp16 or fp32 GPU tensors of any strides; ii is int64 [E].
Outputs: net [1,E,128,h,w] fp16, delta and weight [1,E,h,w,2] fp16, eta [1,K,h,w] fp32, upmask [1,K,576,h,w] fp16, K the number of
distinct ii and group k its k-th smallest value.  These are the dtypes the reference gives under the autocast FactorGraph.update runs
it in when net is fp16, as DepthVideo stores it; with an fp32 net the reference's blend (1 - z) * net + z * q promotes its result to
fp32, this operator still returns fp16.  All work goes on the current torch stream.  Nothing synchronises with the host except the
torch.unique(ii) whose length sizes eta and upmask, as in the reference.  The input net is not modified.  Every output is bitwise
reproducible.  A missing kernel or a CPU tensor is an error: there is no eager fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from splat_slam_amd import _native as nat
from splat_slam_amd._nn_common import (F16_F32, ScratchCache, gpu_tensor, network_device, pack_bias, pack_weight, round_up, run_forward, stream,
                                       tensor_desc)
from splat_slam_amd._nn_common import hash_uniform as _hash_uniform      # its name here before the networks shared it

__all__ = ["UpdateOperator", "synthetic_state_dict", "normalize_state_dict", "conv2d_f16", "LAYER_SHAPES"]

HIDDEN, CORR_PLANES, FLOW_PLANES, UPMASK = 128, 196, 4, 576
_CONVS = {  # name: (cout, cin, kernel size)
    "corr_encoder.0": (128, 196, 1), "corr_encoder.2": (128, 128, 3), "flow_encoder.0": (128, 4, 7), "flow_encoder.2": (64, 128, 3),
    "weight.0": (128, 128, 3), "weight.2": (2, 128, 3), "delta.0": (128, 128, 3), "delta.2": (2, 128, 3),
    "gru.convz": (128, 448, 3), "gru.convr": (128, 448, 3), "gru.convq": (128, 448, 3), "gru.w": (128, 128, 1),
    "gru.convz_glo": (128, 128, 1), "gru.convr_glo": (128, 128, 1), "gru.convq_glo": (128, 128, 1),
    "agg.conv1": (128, 128, 3), "agg.conv2": (128, 128, 3), "agg.eta.0": (1, 128, 3), "agg.upmask.0": (576, 128, 1),
}
LAYER_SHAPES = {}
for _n, (_o, _i, _k) in _CONVS.items():
    LAYER_SHAPES[_n + ".weight"] = (_o, _i, _k, _k)
    LAYER_SHAPES[_n + ".bias"] = (_o,)
_SLICED = ("weight.2", "delta.2")        # checkpoints carry 3 output rows here; the first 2 are used


def synthetic_state_dict(seed):
    """Every tensor of LAYER_SHAPES drawn from U(-1/sqrt(fan_in), 1/sqrt(fan_in)), fan_in = cin * k * k of its layer."""
    sd = {}
    for key, shape in LAYER_SHAPES.items():
        _, cin, k = _CONVS[key.rsplit(".", 1)[0]]
        n = int(np.prod(shape))
        v = _hash_uniform(key, n, seed) / math.sqrt(cin * k * k)
        sd[key] = torch.from_numpy(v.astype(np.float32).reshape(shape))
    return sd


def normalize_state_dict(sd):
    """The operator's tensors out of a checkpoint, as fp32 CPU tensors under the keys of LAYER_SHAPES.  Raises ValueError for a missing
    key, an unexpected key or a wrong shape."""
    out = {}
    for key, v in sd.items():
        k = key[len("module."):] if key.startswith("module.") else key
        if k.startswith(("fnet.", "cnet.")):
            continue
        k = k[len("update."):] if k.startswith("update.") else k
        if k not in LAYER_SHAPES:
            raise ValueError(f"update_op: unexpected key {key!r} in the state dict")
        if k in out:
            raise ValueError(f"update_op: key {key!r} appears twice once its prefixes are stripped")
        if not isinstance(v, torch.Tensor):
            raise ValueError(f"update_op: {key!r} must be a torch.Tensor")
        shape = LAYER_SHAPES[k]
        if k.rsplit(".", 1)[0] in _SLICED and v.dim() == len(shape) and v.shape[0] == 3 and tuple(v.shape[1:]) == shape[1:]:
            v = v[:2]
        if tuple(v.shape) != shape:
            raise ValueError(f"update_op: {key!r} must have shape {shape}, got {tuple(v.shape)}")
        out[k] = v.detach().to("cpu", torch.float32)
    missing = [k for k in LAYER_SHAPES if k not in out]
    if missing:
        raise ValueError(f"update_op: the state dict lacks {missing}")
    return out


def conv2d_f16(x, w, b=None, act="none", out_dtype=torch.float16):
    """act(conv2d(x, w, b)) with zero padding (k - 1) / 2 and stride 1: x [B,cin,h,w] and w [cout,cin,k,k] (k = 1, 3 or 7) are rounded to
    fp16, the sums are fp32, the result [B,cout,h,w] is out_dtype (fp16 or fp32).  act: none, relu, sigmoid, tanh."""
    for name, t in (("x", x), ("w", w)) + ((("b", b),) if b is not None else ()):
        gpu_tensor("update_op.conv2d_f16", name, t, F16_F32, "fp16 or fp32")
    if act not in nat.SGR_UPDATE_ACTS:
        raise RuntimeError(f"update_op.conv2d_f16: act must be one of {sorted(nat.SGR_UPDATE_ACTS)}, got {act!r}")
    if out_dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"update_op.conv2d_f16: out_dtype must be fp16 or fp32, got {out_dtype}")
    if x.dim() != 4 or w.dim() != 4 or w.shape[1] != x.shape[1] or w.shape[2] != w.shape[3] or w.shape[2] not in (1, 3, 7):
        raise RuntimeError(f"update_op.conv2d_f16: x [B,cin,h,w] and w [cout,cin,k,k] with k in (1, 3, 7), got {tuple(x.shape)} and "
                           f"{tuple(w.shape)}")
    B, cin, h, wd = x.shape
    cout, k = w.shape[0], w.shape[2]
    if min(B, cin, h, wd, cout) < 1 or (b is not None and tuple(b.shape) != (cout,)):
        raise RuntimeError(f"update_op.conv2d_f16: empty tensor or a bias that is not [{cout}]")
    dev = x.device
    cin_pad = round_up(cin, 8)
    lib = nat.lib()
    xs = torch.empty((B * h * wd, cin_pad), dtype=torch.float16, device=dev)
    wp, bp = pack_weight(w, cin_pad, 64), pack_bias(b, cout, dev, 64)
    out = torch.empty((B, cout, h, wd), dtype=out_dtype, device=dev)
    c = nat.SgrUpdateConv()
    c.src0, c.stride0, c.cin, c.ksize, c.E, c.h, c.w = xs.data_ptr(), cin_pad, cin_pad, k, B, h, wd
    c.weight, c.weight_elems, c.bias, c.cout, c.act = wp.data_ptr(), wp.numel(), bp.data_ptr(), cout, nat.SGR_UPDATE_ACTS[act]
    c.out = out.data_ptr()
    c.out_kind = nat.SGR_UPDATE_OUT_NCHW_F16 if out_dtype == torch.float16 else nat.SGR_UPDATE_OUT_NCHW_F32
    with torch.cuda.device(dev):
        desc = tensor_desc(x)
        nat.check(lib.sgr_update_pack(C.byref(desc), B, cin, h, wd, xs.data_ptr(), cin_pad, cin_pad, stream(dev)), "sgr_update_pack")
        nat.check(lib.sgr_update_conv(C.byref(c), stream(dev)), "sgr_update_conv")
    return out


# the layers of SgrUpdateWeights in order: (state-dict names whose rows are stacked, padded input channels)
_PACKED = ((("corr_encoder.0",), 200), (("corr_encoder.2",), 128), (("flow_encoder.0",), 8), (("flow_encoder.2",), 128), (("gru.w",), 128),
           (("gru.convz", "gru.convr"), 448), (("gru.convq",), 448), (("delta.0", "weight.0"), 128), (("delta.2",), 128),
           (("weight.2",), 128), (("agg.conv1",), 128), (("agg.conv2",), 128), (("agg.eta.0",), 128), (("agg.upmask.0",), 128))
_GLO = ("gru.convz_glo", "gru.convr_glo", "gru.convq_glo")
LAUNCH_NAMES = ("pack", "corr_encoder.0", "corr_encoder.2", "flow_encoder.0", "flow_encoder.2", "gru.w+gate", "gru.glo", "gru.convz|convr",
                "gru.convq+blend", "delta.0|weight.0", "delta.2", "weight.2", "agg.conv1", "agg.segmented_mean", "agg.conv2", "agg.eta",
                "agg.upmask")


class UpdateOperator:
    def __init__(self, sd, device="cuda"):
        sd = normalize_state_dict(sd)
        self.device = network_device(device, "update_op", "operator")
        self._keep = []
        self._weights = nat.SgrUpdateWeights()
        for i, (names, cin_pad) in enumerate(_PACKED):
            w = torch.cat([sd[n + ".weight"] for n in names])
            b = torch.cat([sd[n + ".bias"] for n in names])
            wp = pack_weight(w, cin_pad, 64).to(self.device)
            bp = pack_bias(b, w.shape[0], "cpu", 64).to(self.device)
            self._keep += [wp, bp]
            self._weights.layer[i].weight, self._weights.layer[i].weight_elems = wp.data_ptr(), wp.numel()
            self._weights.layer[i].bias = bp.data_ptr()
        gw = torch.cat([sd[n + ".weight"].reshape(HIDDEN, HIDDEN) for n in _GLO]).to(torch.float16).to(torch.float32).contiguous()
        gb = torch.cat([sd[n + ".bias"] for n in _GLO]).to(torch.float16).to(torch.float32).contiguous()
        gw, gb = gw.to(self.device), gb.to(self.device)
        self._keep += [gw, gb]
        self._weights.glo_weight, self._weights.glo_bias = gw.data_ptr(), gb.data_ptr()
        self._scratch = ScratchCache()

    @classmethod
    def from_state_dict(cls, sd, device="cuda"):
        return cls(sd, device)

    @classmethod
    def synthetic(cls, seed, device="cuda"):
        return cls(synthetic_state_dict(seed), device)

    def _check(self, net, inp, corr, flow, ii):
        for name, t, ch in (("net", net, HIDDEN), ("inp", inp, HIDDEN), ("corr", corr, CORR_PLANES), ("flow", flow, FLOW_PLANES)):
            if t is None and name == "flow":
                continue
            gpu_tensor("update_op", name, t, F16_F32, "fp16 or fp32")
            if t.device != self.device:
                raise RuntimeError(f"update_op: {name} is on {t.device}, the operator on {self.device}")
            if t.dim() != 5 or t.shape[0] != 1 or t.shape[2] != ch:
                raise RuntimeError(f"update_op: {name} must be [1,E,{ch},h,w], got {tuple(t.shape)}")
            if t.shape[1] < 1 or t.shape[3] < 1 or t.shape[4] < 1:
                raise RuntimeError(f"update_op: {name} is empty, shape {tuple(t.shape)}")
            if (t.shape[1], t.shape[3], t.shape[4]) != (net.shape[1], net.shape[3], net.shape[4]):
                raise RuntimeError(f"update_op: {name} {tuple(t.shape)} does not match net {tuple(net.shape)}")
        if ii is not None:
            if not isinstance(ii, torch.Tensor) or ii.dtype != torch.int64 or ii.dim() != 1 or ii.shape[0] != net.shape[1]:
                raise RuntimeError(f"update_op: ii must be int64 [E] = ({net.shape[1]},)")

    def _prepare(self, net, inp, corr, flow, ii):
        """checks the arguments, allocates the outputs and fills the call record: (record, outputs, tensors the record points into)"""
        self._check(net, inp, corr, flow, ii)
        dev = self.device
        _, E, _, h, w = net.shape
        K, ix = 0, None
        if ii is not None:
            uniq, ix = torch.unique(ii.to(dev), sorted=True, return_inverse=True)
            K, ix = uniq.shape[0], ix.contiguous()
        call = nat.SgrUpdateCall()
        call.net, call.inp, call.corr = tensor_desc(net[0]), tensor_desc(inp[0]), tensor_desc(corr[0])
        call.flow = tensor_desc(None if flow is None else flow[0])
        call.E, call.h, call.w, call.K = E, h, w, K
        net_out = torch.empty((1, E, HIDDEN, h, w), dtype=torch.float16, device=dev)
        delta = torch.empty((1, E, h, w, 2), dtype=torch.float16, device=dev)
        weight = torch.empty((1, E, h, w, 2), dtype=torch.float16, device=dev)
        call.net_out, call.delta, call.weight = net_out.data_ptr(), delta.data_ptr(), weight.data_ptr()
        outs = (net_out, delta, weight)
        if K:
            eta = torch.empty((1, K, h, w), dtype=torch.float32, device=dev)
            upmask = torch.empty((1, K, UPMASK, h, w), dtype=torch.float16, device=dev)
            call.ix, call.eta, call.upmask = ix.data_ptr(), eta.data_ptr(), upmask.data_ptr()
            outs += (eta, upmask)
        call.first_launch, call.last_launch = 0, nat.SGR_UPDATE_LAUNCHES - 1
        return call, outs, (net, inp, corr, flow, ix)

    def _run(self, call):
        """enqueues the launches first_launch..last_launch of the record on the current stream"""
        E, K, h, w = call.E, call.K, call.h, call.w
        run_forward(self, call, (E, K, h, w), lambda: nat.lib().sgr_update_scratch_bytes(E, K, h, w),
                    f"update_op: unsupported sizes (E={E} K={K} h={h} w={w})", "sgr_update_forward")

    def __call__(self, net, inp, corr, flow=None, ii=None, jj=None):
        call, outs, _ = self._prepare(net, inp, corr, flow, ii)
        self._run(call)
        return outs
