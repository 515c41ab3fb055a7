"""GPU box: times of droid_backends.ba (2 Gauss-Newton iterations, csrc/sgr_dba.hip) on a frontend-sized window (12 frames, ~60
edges, at 48x64 and 40x80) and a backend-sized graph (100 frames, ~1000 edges, at 48x64): HIP-event medians of the whole call and the
per-kernel split of one call from torch.profiler.  Writes one JSON file.

    python scripts/dba_times.py [--out profiles/dba_times.json] [--reps 20]"""
import argparse
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
    return dict(poses=f(np.stack(poses)), disps=f(rng.uniform(0.3, 1.0, (n, ht, wd))), intr=f(INTR[(ht, wd)]),
                sens=torch.zeros(n, ht, wd, device=DEV), tgt=f(rng.uniform(0, wd, (E, 2, ht, wd))),
                wgt=f(rng.uniform(0, 1, (E, 2, ht, wd))), eta=f(rng.uniform(1e-3, 1e-2, (n, ht, wd))),
                ii=torch.tensor(ii, device=DEV), jj=torch.tensor(jj, device=DEV), t0=1, t1=n, edges=E)


def call(w, poses, disps):
    import droid_backends
    return droid_backends.ba(poses, disps, w["intr"], w["sens"], w["tgt"], w["wgt"], w["eta"], w["ii"], w["jj"], w["t0"], w["t1"], 2,
                             1e-4, 0.1, False, False)


def measure(w, reps):
    poses, disps = w["poses"].clone(), w["disps"].clone()
    run = lambda: call(w, poses.copy_(w["poses"]), disps.copy_(w["disps"]))
    run()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        poses.copy_(w["poses"])
        disps.copy_(w["disps"])
        torch.cuda.synchronize()
        a.record()
        call(w, poses, disps)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    split = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call(w, poses, disps)
            torch.cuda.synchronize()
        acc, cnt = defaultdict(float), defaultdict(int)
        for ev in prof.events():
            name = ev.name
            dt = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
            m = re.search(r"(\w+_kernel)", name)
            if not m:
                continue
            short = m.group(1)
            acc[short] += dt / 1000.0
            cnt[short] += 1
        split = {k: {"ms": round(acc[k], 4), "launches": cnt[k]} for k in sorted(acc, key=lambda k: -acc[k])}
    except Exception as e:          # noqa: BLE001
        split = {"error": repr(e)}
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4), "reps": reps,
            "per_kernel_one_call": split}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dba_times.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "iterations_per_call": 2, "workloads": {}}
    for name, (n, radius, ht, wd) in {"frontend_48x64": (12, 3, 48, 64), "frontend_40x80": (12, 3, 40, 80),
                                      "backend_48x64": (100, 5, 48, 64)}.items():
        w = workload(n, radius, ht, wd)
        r = measure(w, a.reps)
        r.update(frames=n, window=w["t1"] - w["t0"], edges=w["edges"], ht=ht, wd=wd)
        res["workloads"][name] = r
        print(name, r["ms_median"], "ms", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["ms_median"] for k, v in res["workloads"].items()}))


if __name__ == "__main__":
    main()
