"""GPU box: times of the correlation lookups of droid_backends (csrc/sgr_corr.hip) at the tracker's sizes, each next to a plain-torch
formulation of the same result on the same GPU in the same process: HIP-event medians (one warm-up, --reps timed calls).
  (a) the 4-level corr_index_forward lookup, fp16 volumes, radius 3, 60 edges, 48x64 and 40x80 feature maps
      torch: grid_sample over the planes (grid built and output permuted inside the timed region: they are part of that formulation)
  (b) the 4-level altcorr_forward, C = 128, 80 edges, 48x64
      torch: gather of the (rd+1)^2 channel rows per pixel, contraction over the channels, bilinear spread (in chunks of edges)
  (c) the two backwards at the same sizes; torch: autograd through (a) and (b)
Next to each HIP time: the bytes the call must move at least (every input element it needs and every output element once) and the
bandwidth that time amounts to.  Writes one JSON file.

    python scripts/corr_times.py [--out profiles/corr_times.json] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
R = 3
RD = 2 * R + 1
LEVELS = 4


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4), "reps": reps}


def flow_coords(g, E, ht, wd):
    """pixel grid plus a flow of a few pixels: what the update operator looks up"""
    ys, xs = torch.meshgrid(torch.arange(ht, dtype=torch.float32), torch.arange(wd, dtype=torch.float32), indexing="ij")
    flow = torch.randn(E, 2, ht, wd, generator=g) * 4.0
    return (torch.stack([xs, ys], 0)[None] + flow).to(DEV).contiguous()        # [E,2,ht,wd]


# ---- (a) corr_index
def torch_index_lookup(volume, coords):
    """volume [E,h1,w1,h2,w2], coords [E,2,h1,w1] -> [E,rd,rd,h1,w1] with grid_sample (align_corners, zero padding)"""
    E, h1, w1, h2, w2 = volume.shape
    P = E * h1 * w1
    off = torch.arange(RD, device=volume.device, dtype=torch.float32) - R
    x0 = coords[:, 0].reshape(P, 1, 1)
    y0 = coords[:, 1].reshape(P, 1, 1)
    gx = (2 * (x0 + off.view(1, 1, RD)) / (w2 - 1) - 1).expand(P, RD, RD)         # output [y offset, x offset]
    gy = (2 * (y0 + off.view(1, RD, 1)) / (h2 - 1) - 1).expand(P, RD, RD)
    grid = torch.stack([gx, gy], -1).to(volume.dtype)
    out = F.grid_sample(volume.view(P, 1, h2, w2), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return out.view(E, h1, w1, RD, RD).permute(0, 4, 3, 1, 2).contiguous()


def index_workload(E, ht, wd, reps):
    import droid_backends as db
    g = torch.Generator().manual_seed(0)
    coords = flow_coords(g, E, ht, wd)
    pyr = [(torch.randn(E * ht * wd, (ht >> i) * (wd >> i), generator=g) * 0.5).half().to(DEV).view(E, ht, wd, ht >> i, wd >> i)
           for i in range(LEVELS)]
    cs = [(coords / 2 ** i).contiguous() for i in range(LEVELS)]
    grads = [torch.randn(E, RD, RD, ht, wd, generator=g).half().to(DEV) for _ in range(LEVELS)]
    P = E * ht * wd
    res = {"edges": E, "ht": ht, "wd": wd, "radius": R, "levels": LEVELS, "dtype": "float16"}
    hip = lambda: [db.corr_index_forward(pyr[i], cs[i], R)[0] for i in range(LEVELS)]
    ref = lambda: [torch_index_lookup(pyr[i], cs[i]) for i in range(LEVELS)]
    a, b = hip(), ref()
    res["max_abs_difference_hip_vs_torch"] = max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b))
    del a, b
    fwd_bytes = LEVELS * P * ((RD + 1) ** 2 * 2 + 8 + RD * RD * 2)
    res["forward"] = {"hip": timed(hip, reps), "torch": timed(ref, reps), "min_bytes": fwd_bytes,
                      "per_level_hip": [timed(lambda i=i: db.corr_index_forward(pyr[i], cs[i], R), reps)["ms_median"] for i in range(LEVELS)],
                      "per_level_torch": [timed(lambda i=i: torch_index_lookup(pyr[i], cs[i]), reps)["ms_median"] for i in range(LEVELS)]}
    hipb = lambda: [db.corr_index_backward(pyr[i], cs[i], grads[i], R)[0] for i in range(LEVELS)]

    def refb():
        out = []
        for i in range(LEVELS):
            v = pyr[i].detach().requires_grad_(True)
            torch_index_lookup(v, cs[i]).backward(grads[i])
            out.append(v.grad)
        return out
    bwd_bytes = sum(pyr[i].numel() * 2 for i in range(LEVELS)) + LEVELS * P * (8 + RD * RD * 2)
    res["backward"] = {"hip": timed(hipb, reps), "torch": timed(refb, reps), "min_bytes": bwd_bytes}
    return res


# ---- (b) altcorr
def torch_alt_lookup(fmap1, fmap2, coords, chunk=8):
    """fmap1 [B,H1,W1,C], fmap2 [B,H2,W2,C], coords [B,1,H1,W1,2] -> [B,1,rd*rd,H1,W1]: gather + channel contraction"""
    B, H1, W1, C = fmap1.shape
    H2, W2 = fmap2.shape[1:3]
    rc = RD + 1
    off = torch.arange(rc, device=fmap1.device) - R
    outs = []
    for s in range(0, B, chunk):
        f1, f2, c = fmap1[s:s + chunk].reshape(-1, H1 * W1, C), fmap2[s:s + chunk].reshape(-1, H2 * W2, C), coords[s:s + chunk, 0]
        b = f1.shape[0]
        x0, y0 = c[..., 0].reshape(b, -1), c[..., 1].reshape(b, -1)
        fx, fy = torch.floor(x0), torch.floor(y0)
        dx, dy = (x0 - fx)[..., None, None], (y0 - fy)[..., None, None]
        x2 = (fx.long()[..., None, None] + off.view(1, 1, rc, 1)).expand(b, -1, rc, rc)          # [b,P,ix,iy]
        y2 = (fy.long()[..., None, None] + off.view(1, 1, 1, rc)).expand(b, -1, rc, rc)
        inb = (x2 >= 0) & (x2 < W2) & (y2 >= 0) & (y2 < H2)
        lin = torch.where(inb, y2 * W2 + x2, torch.zeros_like(x2)).reshape(b, -1)                 # [b, P*rc*rc]
        rows = torch.gather(f2, 1, lin[..., None].expand(-1, -1, C)).view(b, H1 * W1, rc * rc, C)
        dots = (torch.einsum("bpkc,bpc->bpk", rows, f1) * inb.reshape(b, -1, rc * rc)).view(b, -1, rc, rc)
        out = ((1 - dx) * (1 - dy) * dots[:, :, :RD, :RD] + dx * (1 - dy) * dots[:, :, 1:, :RD]
               + (1 - dx) * dy * dots[:, :, :RD, 1:] + dx * dy * dots[:, :, 1:, 1:])
        outs.append(out.reshape(b, H1, W1, RD * RD).permute(0, 3, 1, 2))
    return torch.cat(outs, 0)[:, None].contiguous()


def alt_workload(E, ht, wd, C, reps):
    import droid_backends as db
    g = torch.Generator().manual_seed(1)
    coords = flow_coords(g, E, ht, wd).permute(0, 2, 3, 1)[:, None].contiguous()              # [E,1,ht,wd,2]
    fmap1 = (torch.randn(E, ht, wd, C, generator=g) * 0.25).to(DEV)
    pyr = [(torch.randn(E, ht >> i, wd >> i, C, generator=g) * 0.25).to(DEV) for i in range(LEVELS)]
    cs = [(coords / 2 ** i).contiguous() for i in range(LEVELS)]
    grads = [torch.randn(E, 1, RD * RD, ht, wd, generator=g).to(DEV) for _ in range(LEVELS)]
    P = E * ht * wd
    res = {"edges": E, "ht": ht, "wd": wd, "radius": R, "levels": LEVELS, "channels": C, "dtype": "float32"}
    hip = lambda: [db.altcorr_forward(fmap1, pyr[i], cs[i], R)[0] for i in range(LEVELS)]
    ref = lambda: [torch_alt_lookup(fmap1, pyr[i], cs[i]) for i in range(LEVELS)]
    a, b = hip(), ref()
    res["max_abs_difference_hip_vs_torch"] = max(float((x - y).abs().max()) for x, y in zip(a, b))
    del a, b
    fwd_bytes = sum(fmap1.numel() * 4 + pyr[i].numel() * 4 for i in range(LEVELS)) + LEVELS * P * (8 + RD * RD * 4)
    res["forward"] = {"hip": timed(hip, reps), "torch": timed(ref, reps), "min_bytes": fwd_bytes,
                      "gathered_bytes_through_the_caches": LEVELS * P * (RD + 1) ** 2 * C * 4,
                      "per_level_hip": [timed(lambda i=i: db.altcorr_forward(fmap1, pyr[i], cs[i], R), reps)["ms_median"] for i in range(LEVELS)]}
    hipb = lambda: [db.altcorr_backward(fmap1, pyr[i], cs[i], grads[i], R) for i in range(LEVELS)]

    def refb():
        out = []
        for i in range(LEVELS):
            f1, f2 = fmap1.detach().requires_grad_(True), pyr[i].detach().requires_grad_(True)
            torch_alt_lookup(f1, f2, cs[i]).backward(grads[i])
            out.append((f1.grad, f2.grad))
        return out
    bwd_bytes = sum(2 * fmap1.numel() * 4 + 2 * pyr[i].numel() * 4 for i in range(LEVELS)) + LEVELS * P * (16 + RD * RD * 4)
    res["backward"] = {"hip": timed(hipb, reps), "torch": timed(refb, max(3, reps // 4)), "min_bytes": bwd_bytes,
                       "atomic_bytes": LEVELS * P * (RD + 1) ** 2 * C * 4}
    return res


def finish(block):
    for k in ("forward", "backward"):
        d = block[k]
        d["hip_over_torch"] = round(d["hip"]["ms_median"] / d["torch"]["ms_median"], 4)
        d["achieved_GBps_over_min_bytes"] = round(d["min_bytes"] / (d["hip"]["ms_median"] * 1e-3) / 1e9, 1)
    return block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_times.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "warmup_calls": 1, "workloads": {}}
    for name, fn in (("corr_index_48x64", lambda: index_workload(60, 48, 64, a.reps)), ("corr_index_40x80", lambda: index_workload(60, 40, 80, a.reps)),
                     ("altcorr_48x64", lambda: alt_workload(80, 48, 64, 128, a.reps))):
        res["workloads"][name] = finish(fn())
        w = res["workloads"][name]
        print(name, "forward", w["forward"]["hip"]["ms_median"], "ms (torch", w["forward"]["torch"]["ms_median"], ") backward",
              w["backward"]["hip"]["ms_median"], "ms (torch", w["backward"]["torch"]["ms_median"], ")", flush=True)
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: {"fwd_ms": v["forward"]["hip"]["ms_median"], "fwd_hip_over_torch": v["forward"]["hip_over_torch"]}
                      for k, v in res["workloads"].items()}))


if __name__ == "__main__":
    main()
