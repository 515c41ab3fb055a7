"""fp64 statement of the vision transformer of the mono-depth prior (splat_slam_amd.vit), written from its equations, and the torch
composition of the same weights under autocast that the GPU tests and scripts/mono_depth_times.py take as the scale of fp16 arithmetic.

    x      = [cls | proj(patches)] + pos                         pos resized bilinearly (align_corners=False) to the patch grid
    x      = x + proj(attention(qkv(norm1(x))))                   attention = softmax(q k^T / 8) v per head of 64
    x      = x + fc2(gelu(fc1(norm2(x))))                         exact erf GELU; norms with biased variance and eps = 1e-6
    tap_j  = gelu(W_j [x_tokens | x_cls] + b_j) of block taps[j]  the "project" readout, reshaped to [B,D,gh,gw]
"""
import math

import torch
import torch.nn.functional as F

READOUTS = ("act_postprocess3.0.project.0", "act_postprocess4.0.project.0")


def round_fp16(sd):
    """the values the transformer holds: matrices rounded to fp16; biases, norm parameters, tokens and positions stay fp32"""
    return {k: (v.to(torch.float16).to(torch.float32) if v.dim() >= 2 and not k.endswith(("cls_token", "pos_embed")) else v.float())
            for k, v in sd.items()}


def gelu_ref(v):
    return 0.5 * v * torch.special.erfc(-v / math.sqrt(2.0))


def layernorm_ref(x, g, b, eps=1e-6):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g.double() + b.double()


def attention_ref(qkv):
    """qkv [B,T,3,heads,64] -> [B,T,heads * 64] in fp64"""
    B, T, _, H, d = qkv.shape
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4)                  # [B,H,T,64]
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, T, H * d)


def resize_pos_ref(pos, g0, gh, gw):
    D = pos.shape[-1]
    grid = pos[0, 1:].reshape(1, g0, g0, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(gh, gw), mode="bilinear", align_corners=False)
    return torch.cat([pos[0, :1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)], 0)


def vit_ref(sd, cfg, x):
    """the transformer in fp64 on the weights sd exactly as given; x [B,cin,gh,gw]; returns the two taps [B,D,gh,gw]"""
    dev = x.device
    P = {k: v.double().to(dev) for k, v in sd.items()}
    lin = lambda n, t: t @ P[n + ".weight"].reshape(P[n + ".weight"].shape[0], -1).T + P[n + ".bias"]
    B, _, gh, gw = x.shape
    D = cfg.dim
    t = lin("model.patch_embed.proj", x.double().permute(0, 2, 3, 1).reshape(B, gh * gw, -1))
    t = torch.cat([P["model.cls_token"].expand(B, -1, -1), t], 1) + resize_pos_ref(P["model.pos_embed"], cfg.pos_grid, gh, gw)[None]
    taps = {}
    for i in range(cfg.depth):
        p = f"model.blocks.{i}."
        qkv = lin(p + "attn.qkv", layernorm_ref(t, P[p + "norm1.weight"], P[p + "norm1.bias"]))
        t = t + lin(p + "attn.proj", attention_ref(qkv.reshape(B, -1, 3, cfg.heads, 64)))
        t = t + lin(p + "mlp.fc2", gelu_ref(lin(p + "mlp.fc1", layernorm_ref(t, P[p + "norm2.weight"], P[p + "norm2.bias"]))))
        taps[i] = t
    outs = []
    for n, blk in zip(READOUTS, cfg.taps):
        y = taps[blk]
        y = gelu_ref(lin(n, torch.cat([y[:, 1:], y[:, :1].expand(-1, gh * gw, -1)], -1)))
        outs.append(y.transpose(1, 2).reshape(B, D, gh, gw))
    return tuple(outs)


class TorchVit:
    """The same transformer as a composition of torch ops on fp32 parameters under torch.autocast: every linear map runs in fp16
    through the vendor library, layer norm and softmax follow autocast's rules, attention is F.scaled_dot_product_attention."""

    def __init__(self, sd, cfg, device):
        self.p = {k: v.to(device=device, dtype=torch.float32) for k, v in sd.items()}
        self.cfg = cfg

    def lin(self, n, t):
        w = self.p[n + ".weight"]
        return F.linear(t, w.reshape(w.shape[0], -1), self.p[n + ".bias"])

    def __call__(self, x):
        cfg, P = self.cfg, self.p
        B, _, gh, gw = x.shape
        D = cfg.dim
        with torch.autocast("cuda", dtype=torch.float16):
            t = self.lin("model.patch_embed.proj", x.permute(0, 2, 3, 1).reshape(B, gh * gw, -1))
            t = torch.cat([P["model.cls_token"].expand(B, -1, -1), t], 1) + resize_pos_ref(P["model.pos_embed"], cfg.pos_grid, gh, gw)[None]
            taps = {}
            for i in range(cfg.depth):
                p = f"model.blocks.{i}."
                qkv = self.lin(p + "attn.qkv", F.layer_norm(t, (D,), P[p + "norm1.weight"], P[p + "norm1.bias"], 1e-6))
                q, k, v = qkv.reshape(B, -1, 3, cfg.heads, 64).permute(2, 0, 3, 1, 4)
                a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, -1, D)
                t = t + self.lin(p + "attn.proj", a)
                t = t + self.lin(p + "mlp.fc2", F.gelu(self.lin(p + "mlp.fc1", F.layer_norm(t, (D,), P[p + "norm2.weight"], P[p + "norm2.bias"], 1e-6))))
                taps[i] = t
            outs = []
            for n, blk in zip(READOUTS, cfg.taps):
                y = taps[blk]
                y = F.gelu(self.lin(n, torch.cat([y[:, 1:], y[:, :1].expand(-1, gh * gw, -1)], -1)))
                outs.append(y.transpose(1, 2).reshape(B, D, gh, gw))
        return tuple(outs)


def err(got, ref):
    d = (got.detach().double().cpu() - ref.detach().double().cpu()).abs()
    return float(d.max()), float(d.pow(2).mean().sqrt())


def check_against_oracle(name, names, hip, torch_out, oracle):
    """the criterion of tests/test_gpu_update_op.py: max |hip - oracle| <= 2 max |torch - oracle| and rms <= 1.5 rms, per output"""
    bad = []
    for n, a, b, o in zip(names, hip, torch_out, oracle):
        (e_hip, r_hip), (e_ref, r_ref) = err(a, o), err(b, o)
        print(f"{name} {n}: max {e_hip:.3e} (torch {e_ref:.3e})  rms {r_hip:.3e} (torch {r_ref:.3e})")
        if not (e_hip <= 2 * e_ref and r_hip <= 1.5 * r_ref):
            bad.append((n, e_hip, e_ref, r_hip, r_ref))
    assert not bad, bad
