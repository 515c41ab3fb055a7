"""GPU box: times of DSPO stage 2 (splat_slam_amd.dspo, csrc/sgr_dspo.hip) on a frontend-sized window (12 frames, ~60 edges, at 48x64 and
40x80) and a backend-sized graph (100 frames, ~1000 edges, at 48x64): HIP-event medians of depth_scale_step with itrs=2 and of the
alignment alone, the per-kernel split of one depth_scale_step from torch.profiler, and the rate at which the edge pass (system_kernel)
reads the targets and weights it must read (16 bytes per edge and pixel and iteration).  Writes one JSON file.

    python scripts/dspo_times.py [--out profiles/dspo_times.json] [--reps 20]"""
import argparse
import datetime
import json
import os
import re
import sys
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
INTR = {(48, 64): [50.0, 52.0, 31.5, 23.5], (40, 80): [60.0, 58.0, 39.5, 19.5]}
ITRS = 2


def workload(n, radius, ht, wd, seed=0):
    import dba_ref as R
    rng = np.random.default_rng(seed)
    poses = []
    for f in range(n):
        t, q = R.exp_se3(np.concatenate([[0.03 * f, 0.01 * np.sin(f), 0.02 * f], rng.normal(0, 0.02, 3)]))
        poses.append(np.concatenate([t, q]))
    ii, jj = [], []
    for i in range(n):
        for j in range(max(0, i - radius), min(n, i + radius + 1)):
            if i != j:
                ii.append(i)
                jj.append(j)
    E = len(ii)
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()
    disps = rng.uniform(0.3, 1.0, (n, ht, wd))
    return dict(poses=f(np.stack(poses)), disps=f(disps), intr=f(INTR[(ht, wd)]), mono=f(1.7 * disps + 0.05 + rng.normal(0, 0.01, disps.shape)),
                vmask=torch.tensor(rng.uniform(size=disps.shape) < 0.6, device=DEV), scales=torch.ones(n, device=DEV),
                shifts=torch.zeros(n, device=DEV), tgt=f(rng.uniform(0, wd, (E, ht, wd, 2))), wgt=f(rng.uniform(0, 1, (E, ht, wd, 2))),
                eta=f(rng.uniform(1e-3, 1e-2, (n, ht, wd))), ii=torch.tensor(ii, device=DEV), jj=torch.tensor(jj, device=DEV), frames=n,
                edges=E)


def step(w, disps):
    from splat_slam_amd import dspo
    return dspo.depth_scale_step(w["poses"], disps, w["intr"], w["mono"], w["vmask"], w["scales"], w["shifts"], w["frames"], w["tgt"],
                                 w["wgt"], w["eta"], w["ii"], w["jj"], itrs=ITRS)


def align(w, disps):
    from splat_slam_amd import dspo
    return dspo.align_scale_and_shift(w["mono"], disps, w["vmask"])


def event_times(fn, w, reps):
    disps = w["disps"].clone()
    fn(w, disps)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        disps.copy_(w["disps"])
        torch.cuda.synchronize()
        a.record()
        fn(w, disps)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4), "reps": reps}


def kernel_split(w):
    disps = w["disps"].clone()
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step(w, disps)
            torch.cuda.synchronize()
        acc, cnt = defaultdict(float), defaultdict(int)
        for ev in prof.events():
            dt = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
            m = re.search(r"sgr::\(anonymous namespace\)::(\w+_kernel)", ev.name)
            short = m.group(1) if m else "torch"
            if not dt:
                continue
            acc[short] += dt / 1000.0
            cnt[short] += 1
        return {k: {"ms": round(acc[k], 4), "launches": cnt[k]} for k in sorted(acc, key=lambda k: -acc[k])}
    except Exception as e:          # noqa: BLE001
        return {"error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dspo_times.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "iterations_per_call": ITRS, "workloads": {}}
    for name, (n, radius, ht, wd) in {"frontend_48x64": (12, 3, 48, 64), "frontend_40x80": (12, 3, 40, 80),
                                      "backend_48x64": (100, 5, 48, 64)}.items():
        w = workload(n, radius, ht, wd)
        r = {"depth_scale_step": event_times(step, w, a.reps), "align_scale_and_shift": event_times(align, w, a.reps),
             "per_kernel_one_step": kernel_split(w), "frames": n, "edges": w["edges"], "ht": ht, "wd": wd}
        edge = r["per_kernel_one_step"].get("system_kernel")
        if edge and edge["launches"]:
            must_read = w["edges"] * ht * wd * 16               # targets + weights, once per iteration
            per_launch_s = edge["ms"] / edge["launches"] * 1e-3
            r["edge_pass"] = {"bytes_per_iteration": must_read, "ms_per_iteration": round(edge["ms"] / edge["launches"], 4),
                              "gb_per_s": round(must_read / per_launch_s / 1e9, 1)}
        res["workloads"][name] = r
        print(name, r["depth_scale_step"]["ms_median"], "ms", r.get("edge_pass"), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["depth_scale_step"]["ms_median"] for k, v in res["workloads"].items()}))


if __name__ == "__main__":
    main()
