"""The vision transformer of the mono-depth prior (timm's ViT blocks as the DPT of the reference's
thirdparty/mono_priors/omnidata/modules/midas/vit.py reads them: forward_flex, the hooks on two blocks, the "project" readout) on the
gfx950 kernels `sgr_vit_*` (include/splat_hip.h, csrc/sgr_vit.hip).  Inference only: no autograd, no nn.Module.

    VitConfig(dim=768, heads=12, depth=12, taps=(8, 11), pos_grid=24, cin=1024)
    VisionTransformer.from_state_dict(sd, cfg=VitConfig(), device="cuda")
    VisionTransformer.synthetic(seed, cfg=VitConfig(), device="cuda")      weights of synthetic_state_dict(seed, cfg)
    vit(patch_features [B,cin,gh,gw]) -> (tap_a, tap_b)                     each fp16 [B,dim,gh,gw]
    vit.tokens(patches [B,gh*gw,cin] fp16, gh, gw) -> (tap_a, tap_b)        the same on channels-last features, without the copy
    synthetic_state_dict(seed, cfg)      fp32 CPU tensors by the update operator's closed-form integer hash of (name, flat index, seed)
    normalize_state_dict(sd, cfg)        validation alone (touches no device); state_shapes(cfg) lists the keys
    resize_pos_embed(pos, g0, gh, gw)    the reference's _resize_pos_embed: bilinear, align_corners=False, the class row kept
    layernorm, gemm, attention           the single kernels on torch tensors (what the tests and the timing script call)

The keys are the checkpoint's below "pretrained.": model.patch_embed.proj, model.cls_token, model.pos_embed, model.blocks.I.{norm1,
attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2} and act_postprocess{3,4}.0.project.0 (the two readouts, [dim, 2 dim]).  The taps are
the outputs of blocks taps[0] and taps[1] before any final norm, which the DPT never reads.  Weights are rounded to fp16 once at
construction; biases, norm scales and the position table stay fp32.  The position table is resized per (gh, gw) and cached.  All work
goes on the current torch stream, nothing synchronises with the host, every output is bitwise reproducible and image i of a batch
gives the bits of that image alone.  A missing kernel or a CPU tensor is an error: there is no eager fallback.
"""
import ctypes as C
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from splat_slam_amd import _native as nat
from splat_slam_amd import _nn_common
from splat_slam_amd._nn_common import ScratchCache, gpu_tensor, network_device, run_forward, stream

__all__ = ["VitConfig", "VisionTransformer", "synthetic_state_dict", "normalize_state_dict", "state_shapes", "resize_pos_embed",
           "hash_uniform", "layernorm", "gemm", "attention", "launch_names"]

READOUTS = ("act_postprocess3.0.project.0", "act_postprocess4.0.project.0")
_BLOCK = ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2")


@dataclass(frozen=True)
class VitConfig:
    dim: int = 768
    heads: int = 12
    depth: int = 12
    taps: tuple = (8, 11)
    pos_grid: int = 24
    cin: int = 1024

    def check(self):
        if not (1 <= self.heads <= 16 and self.dim == 64 * self.heads):
            raise ValueError(f"vit: dim = 64 * heads with heads 1..16, got dim={self.dim} heads={self.heads}")
        if self.depth < 1 or len(self.taps) != 2 or self.taps[0] == self.taps[1] or not all(0 <= t < self.depth for t in self.taps):
            raise ValueError(f"vit: taps must be two distinct blocks below depth={self.depth}, got {self.taps}")
        if self.cin < 64 or self.cin % 64 or self.pos_grid < 1:
            raise ValueError(f"vit: cin is a positive multiple of 64 and pos_grid >= 1, got cin={self.cin} pos_grid={self.pos_grid}")
        return self


def state_shapes(cfg):
    """key -> shape of every tensor the transformer reads"""
    D = cfg.dim
    s = {"model.patch_embed.proj.weight": (D, cfg.cin, 1, 1), "model.patch_embed.proj.bias": (D,), "model.cls_token": (1, 1, D),
         "model.pos_embed": (1, 1 + cfg.pos_grid ** 2, D)}
    lin = {"attn.qkv": (3 * D, D), "attn.proj": (D, D), "mlp.fc1": (4 * D, D), "mlp.fc2": (D, 4 * D)}
    for i in range(cfg.depth):
        for n in _BLOCK:
            w = lin.get(n, (D,))
            s[f"model.blocks.{i}.{n}.weight"] = w
            s[f"model.blocks.{i}.{n}.bias"] = (w[0],)
    for n in READOUTS:
        s[n + ".weight"], s[n + ".bias"] = (D, 2 * D), (D,)
    return s


def hash_uniform(name, n, seed):
    """n values of U[-1, 1) as a float64 tensor: the closed-form integer hash every synthetic network here draws its weights from"""
    return torch.from_numpy(_nn_common.hash_uniform(name, n, seed))


def synthetic_tensor(key, shape, seed, scale, offset=0.0):
    n = int(math.prod(shape))
    return (offset + scale * hash_uniform(key, n, seed)).to(torch.float32).reshape(shape)


def synthetic_state_dict(seed, cfg=VitConfig()):
    """matrices from U(-1, 1) / sqrt(fan_in), their biases and the norm biases 0.1 U, norm scales 1 + 0.1 U, tokens and positions 0.5 U"""
    sd = {}
    for key, shape in state_shapes(cfg.check()).items():
        if key.endswith(("cls_token", "pos_embed")):
            sd[key] = synthetic_tensor(key, shape, seed, 0.5)
        elif len(shape) == 1:
            sd[key] = synthetic_tensor(key, shape, seed, 0.1, 1.0 if ".norm" in key and key.endswith("weight") else 0.0)
        else:
            sd[key] = synthetic_tensor(key, shape, seed, 1.0 / math.sqrt(shape[1]))
    return sd


def normalize_state_dict(sd, cfg=VitConfig()):
    """Raises ValueError for a missing key, an unexpected key or a wrong shape; returns the tensors under the keys of state_shapes."""
    shapes = state_shapes(cfg.check())
    for key, v in sd.items():
        if key not in shapes:
            raise ValueError(f"vit: unexpected key {key!r} in the state dict")
        if not isinstance(v, torch.Tensor) or tuple(v.shape) != shapes[key]:
            raise ValueError(f"vit: {key!r} must be a tensor of shape {shapes[key]}, got {tuple(getattr(v, 'shape', ()))}")
    missing = [k for k in shapes if k not in sd]
    if missing:
        raise ValueError(f"vit: the state dict lacks {missing}")
    return {k: sd[k].detach() for k in shapes}


def resize_pos_embed(pos, g0, gh, gw):
    """pos [1, 1 + g0 * g0, D] -> [1 + gh * gw, D]: the grid rows resized bilinearly (align_corners=False), the class row kept"""
    D = pos.shape[-1]
    grid = pos[0, 1:].reshape(1, g0, g0, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(gh, gw), mode="bilinear", align_corners=False)
    return torch.cat([pos[0, :1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)], 0)


def launch_names(depth):
    names = ["embed"]
    for i in range(depth):
        names += [f"blocks.{i}.{n}" for n in ("norm1", "qkv", "attention", "proj", "norm2", "fc1", "fc2")]
    return names + ["readout3.cls", "readout3", "readout4.cls", "readout4"]


def _gpu(name, t, dtype):
    """gpu_tensor for the one dtype a kernel takes, and contiguous"""
    if not gpu_tensor("vit", name, t, (dtype,), f"contiguous {dtype}").is_contiguous():
        raise RuntimeError(f"vit: {name} must be contiguous {dtype}, got {t.dtype}")
    return t


# ---- the single kernels ----------------------------------------------------------------------------------------------------------------
def layernorm(x, gamma, beta):
    """fp32 [M,D] -> fp16 [M,D], eps = 1e-6"""
    x, gamma, beta = _gpu("x", x, torch.float32), _gpu("gamma", gamma, torch.float32), _gpu("beta", beta, torch.float32)
    M, D = x.shape
    out = torch.empty((M, D), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        nat.check(nat.lib().sgr_vit_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), M, D, out.data_ptr(), stream(x.device)),
                  "sgr_vit_layernorm")
    return out


def gemm(a, w, bias=None, epi="store_f16", out=None, tap=False, aux=None, T=0):
    """epi(a [M,K] w [N,K]^T + bias) with fp16 a and w, fp32 bias.  store_f16, gelu_f16: fp16 [M,N]; store_f32: fp32 [M,N]; residual:
    adds into the fp32 out [M,N] in place and returns (out, its fp16 copy or None); readout (aux fp32 [B,N], M = B T): fp16 [B,N,T-1];
    embed (aux fp32 [T,N], M = B (T-1)): fp32 [B T,N] whose class rows are zero."""
    a, w = _gpu("a", a, torch.float16), _gpu("w", w, torch.float16)
    (M, K), N, dev = a.shape, w.shape[0], a.device
    g = nat.SgrVitGemm()
    g.a, g.w, g.lda, g.ldw, g.M, g.N, g.K, g.epi, g.T, g.ldo = a.data_ptr(), w.data_ptr(), K, w.shape[1], M, N, K, nat.SGR_VIT_EPI[epi], T, N
    if bias is not None:
        g.bias = _gpu("bias", bias, torch.float32).data_ptr()
    if aux is not None:
        g.aux = _gpu("aux", aux, torch.float32).data_ptr()
    ret = None
    if epi in ("store_f16", "gelu_f16"):
        out = torch.empty((M, N), dtype=torch.float16, device=dev)
    elif epi == "store_f32":
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    elif epi == "residual":
        _gpu("out", out, torch.float32)
        t16 = torch.empty((M, N), dtype=torch.float16, device=dev) if tap else None
        g.tap = nat.ptr(t16)
        ret = (out, t16)
    elif epi == "readout":
        out = torch.empty((M // max(T, 1), N, T - 1), dtype=torch.float16, device=dev)
    elif epi == "embed":
        out = torch.zeros((M // max(T - 1, 1) * T, N), dtype=torch.float32, device=dev)
    else:
        raise RuntimeError(f"vit.gemm: unknown epilogue {epi!r}")
    g.out = out.data_ptr()
    with torch.cuda.device(dev):
        nat.check(nat.lib().sgr_vit_gemm(C.byref(g), stream(dev)), "sgr_vit_gemm")
    return out if ret is None else ret


def attention(qkv):
    """fp16 [B,T,3,heads,64] -> fp16 [B,T,heads * 64]"""
    qkv = _gpu("qkv", qkv, torch.float16)
    if qkv.dim() != 5 or qkv.shape[2] != 3 or qkv.shape[4] != 64:
        raise RuntimeError(f"vit.attention: qkv must be [B,T,3,heads,64], got {tuple(qkv.shape)}")
    B, T, _, heads, _ = qkv.shape
    out = torch.empty((B, T, heads * 64), dtype=torch.float16, device=qkv.device)
    with torch.cuda.device(qkv.device):
        nat.check(nat.lib().sgr_vit_attention(qkv.data_ptr(), B, T, heads, out.data_ptr(), stream(qkv.device)), "sgr_vit_attention")
    return out


# ---- the whole stack -------------------------------------------------------------------------------------------------------------------
class VisionTransformer:
    def __init__(self, sd, cfg=VitConfig(), device="cuda"):
        sd = normalize_state_dict(sd, cfg)
        self.cfg = cfg
        self.device = network_device(device, "vit", "transformer")
        self._keep = []

        def f16(key):
            t = sd[key].to(self.device, torch.float16).reshape(sd[key].shape[0], -1).contiguous()
            self._keep.append(t)
            return t.data_ptr()

        def f32(key):
            t = sd[key].to(self.device, torch.float32).contiguous()
            self._keep.append(t)
            return t.data_ptr()

        w = self._weights = nat.SgrVitWeights()
        w.dim, w.heads, w.depth, w.cin = cfg.dim, cfg.heads, cfg.depth, cfg.cin
        w.tap[0], w.tap[1] = cfg.taps
        w.embed_w, w.embed_b = f16("model.patch_embed.proj.weight"), f32("model.patch_embed.proj.bias")
        self._blocks = (nat.SgrVitBlock * cfg.depth)()
        for i, b in enumerate(self._blocks):
            p = f"model.blocks.{i}."
            b.ln1_g, b.ln1_b, b.ln2_g, b.ln2_b = f32(p + "norm1.weight"), f32(p + "norm1.bias"), f32(p + "norm2.weight"), f32(p + "norm2.bias")
            b.qkv_w, b.qkv_b, b.proj_w, b.proj_b = f16(p + "attn.qkv.weight"), f32(p + "attn.qkv.bias"), f16(p + "attn.proj.weight"), f32(p + "attn.proj.bias")
            b.fc1_w, b.fc1_b, b.fc2_w, b.fc2_b = f16(p + "mlp.fc1.weight"), f32(p + "mlp.fc1.bias"), f16(p + "mlp.fc2.weight"), f32(p + "mlp.fc2.bias")
        w.blocks = self._blocks
        for j, n in enumerate(READOUTS):
            w.readout_w[j], w.readout_b[j] = f16(n + ".weight"), f32(n + ".bias")
        self._pos_embed = sd["model.pos_embed"].to(self.device, torch.float32)
        self._cls = sd["model.cls_token"].to(self.device, torch.float32).reshape(1, cfg.dim)
        self._pos, self._scratch = {}, ScratchCache()
        self.launches = 5 + 7 * cfg.depth

    @classmethod
    def from_state_dict(cls, sd, cfg=VitConfig(), device="cuda"):
        return cls(sd, cfg, device)

    @classmethod
    def synthetic(cls, seed, cfg=VitConfig(), device="cuda"):
        return cls(synthetic_state_dict(seed, cfg), cfg, device)

    def pos_table(self, gh, gw):
        """fp32 [1 + gh * gw, dim]: row 0 the class token plus its position row, then the resized position rows"""
        t = self._pos.get((gh, gw))
        if t is None:
            t = resize_pos_embed(self._pos_embed, self.cfg.pos_grid, gh, gw)
            t[0] += self._cls[0]
            t = self._pos[(gh, gw)] = t.contiguous()
        return t

    def _prepare(self, x):
        """checks the argument, allocates the outputs and fills the call record: (record, outputs, tensors the record points into)"""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("vit (MI355X build): patch_features must be a GPU tensor; there is no CPU path")
        if x.device != self.device:
            raise RuntimeError(f"vit: patch_features is on {x.device}, the transformer on {self.device}")
        if x.dim() != 4 or x.shape[1] != self.cfg.cin or min(x.shape) < 1 or x.dtype not in (torch.float16, torch.float32):
            raise RuntimeError(f"vit: patch_features must be a non-empty fp16 or fp32 [B,{self.cfg.cin},gh,gw], got {tuple(x.shape)} {x.dtype}")
        B, _, gh, gw = x.shape
        return self._record(x.permute(0, 2, 3, 1).to(torch.float16).contiguous(), B, gh, gw)

    def _record(self, patches, B, gh, gw):
        pos = self.pos_table(gh, gw)
        outs = tuple(torch.empty((B, self.cfg.dim, gh, gw), dtype=torch.float16, device=self.device) for _ in range(2))
        call = nat.SgrVitCall()
        call.patches, call.B, call.gh, call.gw, call.pos = patches.data_ptr(), B, gh, gw, pos.data_ptr()
        call.out[0], call.out[1] = outs[0].data_ptr(), outs[1].data_ptr()
        call.first_launch, call.last_launch = 0, self.launches - 1
        return call, outs, (patches, pos)

    def _run(self, call):
        """enqueues the launches first_launch..last_launch of the record on the current stream"""
        B, T = call.B, 1 + call.gh * call.gw
        run_forward(self, call, (B, T), lambda: nat.lib().sgr_vit_scratch_bytes(B, T, self.cfg.heads, self.cfg.depth),
                    f"vit: unsupported sizes (B={B} T={T})", "sgr_vit_forward")

    def __call__(self, patch_features):
        call, outs, _ = self._prepare(patch_features)
        self._run(call)
        return outs

    def tokens(self, patches, gh, gw):
        """the transformer on patch features that are already channels-last: patches fp16 [B, gh * gw, cin], contiguous, as a backbone
        on this library's kernels leaves them -> (tap_a, tap_b); no copy is made"""
        _gpu("patches", patches, torch.float16)
        if patches.device != self.device:
            raise RuntimeError(f"vit: patches is on {patches.device}, the transformer on {self.device}")
        if patches.dim() != 3 or gh < 1 or gw < 1 or patches.shape[0] < 1 or tuple(patches.shape[1:]) != (gh * gw, self.cfg.cin):
            raise RuntimeError(f"vit: patches must be [B,{gh * gw},{self.cfg.cin}], got {tuple(patches.shape)}")
        call, outs, _ = self._record(patches, patches.shape[0], gh, gw)
        self._run(call)
        return outs
