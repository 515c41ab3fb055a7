"""GPU box: HIP-event times of one mapping iteration (10 window keyframes + 2 random views, 640x480, 300k Gaussians: bench.py's light
scene) for three loops, and the kernels they launch ("SSIM in the fused loop"):

  fused_l1     FusedMappingLoop, ssim_loss: False (the L1 loss rides in the tile kernel's epilogue)
  fused_ssim   FusedMappingLoop(native_ssim=True), ssim_loss: True (sgr_map_run_ssim: plain compositing, the SSIM loss launch pair,
               the float-gradient backward)
  fallback     FusedMappingLoop, ssim_loss: True without native_ssim: the autograd MappingLoop (drop-in rasterizer + torch SSIM)

Per-kernel device times come from the torch profiler over a few iterations of each loop.  The JSON goes to
profiles/ssim_loop_times.json (and stdout).

    python scripts/ssim_loop_times.py [--iters 40] [--gaussians 300000]"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def build(kind, n, views=16):
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.fused import FusedMappingLoop
    cfg = copy.deepcopy(syn.DEFAULT_CONFIG)
    cfg["mapping"]["Training"]["ssim_loss"] = kind != "fused_l1"
    cfg["mapping"].setdefault("opt_params", {}).setdefault("lambda_dssim", 0.2)
    torch.manual_seed(43)
    np.random.seed(43)
    params = syn.room_parameters(n, seed=43, device=DEV)
    cams = syn.make_views(params, views, syn.INTRINSICS["metric"], DEV, seed=43)
    loop = FusedMappingLoop(cfg, device=DEV, native_ssim=(kind == "fused_ssim"))
    loop.gaussians = syn.model_from_parameters(params, config=cfg, device=DEV)
    loop.viewpoints = {c.uid: c for c in cams}
    loop.current_window = list(range(10))
    loop.build_keyframe_optimizers()
    loop.iteration_count = 50
    assert loop.autograd_fallback == (kind == "fallback")
    return loop


def run(loop, k):
    loop.iteration_count = 50            # (clear of the densification points: 149 regular iterations follow)
    loop.map(loop.current_window, iters=k)


def time_loop(loop, iters, reps=3):
    run(loop, 4)                          # warm-up: capacities, workspaces, launch structs
    torch.cuda.synchronize()
    per = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run(loop, iters)
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / iters)
    per.sort()
    return round(per[len(per) // 2], 4), round(per[0], 4)


def kernel_times(loop, iters):
    """device milliseconds per iteration of every kernel, largest first (torch profiler, HIP activity)"""
    from torch.profiler import ProfilerActivity, profile
    run(loop, 2)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        run(loop, iters)
        torch.cuda.synchronize()
    rows = []
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        if t is None:
            t = getattr(e, "cuda_time_total", 0.0)
        if t and e.device_type.name in ("CUDA", "HIP"):
            rows.append({"kernel": e.key[:120], "ms_per_iteration": round(t / 1e3 / iters, 4), "launches_per_iteration": round(e.count / iters, 2)})
    rows.sort(key=lambda r: -r["ms_per_iteration"])
    return rows[:25]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--fallback-iters", type=int, default=10)
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_loop_times.json"))
    args = ap.parse_args()
    out = {"scene": "room, %d Gaussians, 640x480, 10 window + 2 random views per iteration" % args.gaussians, "loops": {}}
    for kind in ("fused_l1", "fused_ssim", "fallback"):
        loop = build(kind, args.gaussians)
        it = args.fallback_iters if kind == "fallback" else args.iters
        med, best = time_loop(loop, it)
        rec = {"ms_per_iteration_median": med, "ms_per_iteration_min": best, "iterations_timed": it}
        try:
            rec["kernels"] = kernel_times(loop, min(it, 10))
        except Exception as e:                # (the timing above stands on its own)
            rec["kernels_error"] = repr(e)[:200]
        out["loops"][kind] = rec
        print(json.dumps({kind: {k: v for k, v in rec.items() if k != "kernels"}}), flush=True)
        del loop
        torch.cuda.empty_cache()
    L = out["loops"]
    out["fused_ssim_over_fused_l1"] = round(L["fused_ssim"]["ms_per_iteration_median"] / L["fused_l1"]["ms_per_iteration_median"], 3)
    out["fallback_over_fused_ssim"] = round(L["fallback"]["ms_per_iteration_median"] / L["fused_ssim"]["ms_per_iteration_median"], 2)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "loops"}))


if __name__ == "__main__":
    main()
