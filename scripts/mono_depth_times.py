"""GPU box: times of the mono-depth prior (splat_slam_amd.mono_depth, splat_slam_amd.vit, csrc/sgr_vit.hip) next to the torch composition
of the same weights in fp16 (tests/vit_ref.TorchVit and tests/mono_depth_ref.TorchMonoDepth: F.linear and F.conv2d under torch.autocast,
i.e. the vendor libraries, and F.scaled_dot_product_attention): the whole transformer at dim 768, depth 12, 1025 tokens, one image, whole
and launch by launch, and a whole predict of a 480 x 640 image through the default network.  HIP-event medians after a warm-up, the
two sides alternating in this one process on the same card.  A single launch is timed on the buffers a whole call has left in scratch.
Writes one JSON file (rewritten after every section, so a run that is cut short leaves what it measured).

    timeout 900 python scripts/mono_depth_times.py [--out profiles/mono_depth_times.json] [--reps 10]"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
SEED = 7
PEAK_F16_TFLOPS = 2500.0         # MI355X dense fp16 matrix peak


def one_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(times):
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4), "reps": len(times)}


def alternating(hip, ref, reps):
    """warm both, then hip, torch, hip, torch, ...: a drift of the card's clock falls on both sides alike"""
    hip(), ref(), hip(), ref()
    th, tr = [], []
    for _ in range(reps):
        th.append(one_time(hip))
        tr.append(one_time(ref))
    r = {"hip": summary(th), "torch": summary(tr)}
    r["ratio_hip_over_torch"] = round(r["hip"]["ms_median"] / r["torch"]["ms_median"], 4)
    r["hip_not_slower"] = r["hip"]["ms_median"] <= r["torch"]["ms_median"]
    return r


def hold_fp16(params):
    """the torch side keeps its matrices and kernels in fp16, so that autocast casts no weight inside the timed call"""
    for k, v in params.items():
        if v.dim() >= 2 and not k.endswith(("cls_token", "pos_embed")):
            params[k] = v.to(torch.float16)


def launch_gflop(name, B, T, D, cin):
    """the matrix work of one launch of sgr_vit_forward"""
    M, kind = B * T, name.rsplit(".", 1)[-1]
    if name == "embed":
        return 2.0 * B * (T - 1) * D * cin / 1e9
    if kind in ("qkv", "fc1", "fc2", "proj"):
        return 2.0 * M * D * D * {"qkv": 3, "fc1": 4, "fc2": 4, "proj": 1}[kind] / 1e9
    if kind == "attention":
        return 4.0 * B * T * T * D / 1e9
    if name.startswith("readout"):
        return 2.0 * (B if kind == "cls" else M) * D * D / 1e9
    return 0.0


def main():
    import mono_depth_ref as MR
    import vit_ref as VR
    from splat_slam_amd import mono_depth as MD
    from splat_slam_amd import vit as V
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mono_depth_times.json"))
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "peak_f16_tflops": PEAK_F16_TFLOPS}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    # ---- the whole transformer ----
    cfg = V.VitConfig()
    sd = V.synthetic_state_dict(SEED, cfg)
    vit, torch_vit = V.VisionTransformer.from_state_dict(sd, cfg, DEV), VR.TorchVit(VR.round_fp16(sd), cfg, DEV)
    hold_fp16(torch_vit.p)
    B, gh, gw = 1, 32, 32
    T = 1 + gh * gw
    x = torch.relu(torch.randn(B, cfg.cin, gh, gw, generator=torch.Generator().manual_seed(1))).half().to(DEV)
    r = {"B": B, "T": T, "dim": cfg.dim, "depth": cfg.depth, "heads": cfg.heads}
    r.update(alternating(lambda: vit(x), lambda: torch_vit(x), a.reps))
    print("vit", r["hip"]["ms_median"], "ms; torch", r["torch"]["ms_median"], "ms; ratio", r["ratio_hip_over_torch"], flush=True)
    res["vit_768x12_T1025_B1"] = r
    save()
    call, outs, keep = vit._prepare(x)
    vit._run(call)
    launches, by_kind, total = {}, {}, 0.0
    for i, name in enumerate(V.launch_names(cfg.depth)):
        call.first_launch = call.last_launch = i
        vit._run(call)
        t = summary([one_time(lambda: vit._run(call)) for _ in range(a.reps)])
        gf = launch_gflop(name, B, T, cfg.dim, cfg.cin)
        if gf:
            t["gflop"], t["tflops"] = round(gf, 3), round(gf / t["ms_median"], 1)
            t["fraction_of_f16_peak"] = round(t["tflops"] / PEAK_F16_TFLOPS, 4)
        total += gf
        launches[name] = t
        kind = name.rsplit(".", 1)[-1] if name.startswith("blocks.") else name
        by_kind[kind] = round(by_kind.get(kind, 0.0) + t["ms_median"], 4)
    r["launches"], r["ms_by_kind_of_launch"] = launches, by_kind
    r["gflop"], r["sum_of_launches_ms"] = round(total, 1), round(sum(t["ms_median"] for t in launches.values()), 4)
    r["hip_tflops"] = round(total / r["hip"]["ms_median"], 1)
    save()
    print("by kind", by_kind, flush=True)
    del vit, torch_vit, call, outs, keep, sd
    torch.cuda.empty_cache()

    # ---- a whole predict ----
    mcfg = MD.MonoDepthConfig()
    sd = MD.synthetic_state_dict(SEED, mcfg)
    model, torch_model = MD.MonoDepth.from_state_dict(sd, mcfg, DEV), MR.TorchMonoDepth(MR.prepare(sd), mcfg, DEV)
    del sd
    hold_fp16(torch_model.p), hold_fp16(torch_model.vit.p)
    image = torch.rand(1, 3, 480, 640, generator=torch.Generator().manual_seed(2)).to(DEV)
    p = {"image": [480, 640], "net_size": list(mcfg.net_size)}
    p.update(alternating(lambda: model.predict(image), lambda: MR.predict_by_hand(torch_model, image), a.reps))
    xn = torch.rand(1, 3, *mcfg.net_size, generator=torch.Generator().manual_seed(3)).half().to(DEV)
    p["backbone_torch_fp16"] = summary([one_time(lambda: model.backbone(xn)) for _ in range(a.reps + 1)][1:])
    d = (model.predict(image) - MR.predict_by_hand(torch_model, image)).abs()
    p["max_abs_difference_hip_torch"] = float(d.max())
    res["predict_480x640"] = p
    save()
    print("predict", p["hip"]["ms_median"], "ms; torch", p["torch"]["ms_median"], "ms; ratio", p["ratio_hip_over_torch"], flush=True)
    print(json.dumps({k: v.get("ratio_hip_over_torch") for k, v in res.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
