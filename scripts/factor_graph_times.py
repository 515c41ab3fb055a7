"""GPU box: times of the factor-graph kernels (splat_slam_amd.factor_graph, csrc/sgr_graph.hip), each next to the same result composed
in the same process the way the reference composes it: the reprojection with motion features from plain torch ops (40 x 80 maps, 24
and 96 edges), the frontend's edge selection (25 frames, max_factors 75) and the backend's (128 x 128 and 512 x 512) from a device
argsort followed by a host loop that reads one device scalar per candidate.  HIP-event medians after one warm-up (the selections
include their one host read of the edge count).  Writes one JSON file.

    python scripts/factor_graph_times.py [--out profiles/factor_graph_times.json] [--reps 20]"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


# ---- (a) the reference's reprojection and motion features, op by op
def qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                        aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def qrot(q, X):
    uv = 2 * torch.cross(q[..., :3].expand_as(X), X, dim=-1)
    return X + q[..., 3:] * uv + torch.cross(q[..., :3].expand_as(X), uv, dim=-1)


def torch_reproject(poses, disps, intr, ii, jj, target, grid):
    ti, qi, tj, qj = poses[ii, :3], poses[ii, 3:], poses[jj, :3], poses[jj, 3:]
    qinv = qi * torch.tensor([-1.0, -1.0, -1.0, 1.0], device=DEV)
    q = qmul(qj, qinv)
    t = tj - qrot(q, ti)
    stereo = ii == jj
    t[stereo] = torch.tensor([-0.1, 0.0, 0.0], device=DEV)
    q[stereo] = torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV)
    fx, fy, cx, cy = intr[ii][:, None, None, :].unbind(-1)
    d = disps[ii]
    X0 = torch.stack([(grid[..., 0] - cx) / fx, (grid[..., 1] - cy) / fy, torch.ones_like(d)], -1)
    X1 = qrot(q[:, None, None], X0) + t[:, None, None] * d[..., None]
    fx, fy, cx, cy = intr[jj][:, None, None, :].unbind(-1)
    Z = torch.where(X1[..., 2] < 0.1, torch.ones_like(d), X1[..., 2])
    z = 1.0 / Z
    coords = torch.stack([fx * (X1[..., 0] * z) + cx, fy * (X1[..., 1] * z) + cy], -1)
    valid = (X1[..., 2] > 0.2).float().unsqueeze(-1)
    motn = torch.cat([coords - grid, target - coords], -1).permute(0, 3, 1, 2).clamp(-64.0, 64.0)
    return coords, valid, motn


# ---- (b), (c) the reference's selections: sorted on the device, visited on the host
def host_proximity(d, t0, t1, t, ii_old, jj_old, rad, nms, thresh, max_factors):
    rows, cols = t - t0, t - t1
    ii, jj = torch.meshgrid(torch.arange(t0, t), torch.arange(t1, t), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    d = d.clone()
    d[(ii - rad < jj).to(DEV)] = np.inf
    d[~(d <= 100)] = np.inf

    def suppress(i, j):
        r = max(min(abs(i - j) - 2, nms), 0)
        for di in range(-r, r + 1):
            for dj in range(-r, r + 1):
                if abs(di) + abs(dj) <= r and t0 <= i + di < t and t1 <= j + dj < t:
                    d[(i + di - t0) * cols + (j + dj - t1)] = np.inf

    for i, j in zip(ii_old.tolist(), jj_old.tolist()):
        suppress(i, j)
    es = []
    for i in range(t0, t):
        for j in range(max(i - rad - 1, 0), i):
            es += [(i, j), (j, i)]
            if t1 <= j:
                d[(i - t0) * cols + (j - t1)] = np.inf
    for k in torch.argsort(d, stable=True).tolist():
        if not d[k].item() <= thresh:
            continue
        if len(es) > max_factors:
            break
        i, j = ii[k].item(), jj[k].item()
        es += [(i, j), (j, i)]
        suppress(i, j)
    return es


def host_backend(d, t_start, t_end, nms, radius, thresh, max_factors):
    n = t_end - t_start
    ii, jj = torch.meshgrid(torch.arange(t_start, t_end), torch.arange(t_start, t_end), indexing="ij")
    d = d.clone().view(n, n)
    d[(ii - radius < jj).to(DEV)] = np.inf
    d[~(d <= thresh)] = np.inf
    es = []
    for i in range(t_start, t_end):
        for j in range(max(i - radius - 1, 0), i):
            es += [(i, j), (j, i)]
            if t_start <= j:
                d[i - t_start, j - t_start] = np.inf
    vals, ix = torch.sort(d.reshape(-1), stable=True)
    for k in ix[vals <= thresh].tolist():
        r, c = k // n, k % n
        if d[r, c].item() > thresh:
            continue
        if len(es) > max_factors:
            break
        es += [(t_start + r, t_start + c), (t_start + c, t_start + r)]
        d[max(0, r - nms):r + nms + 1, max(0, c - nms):c + nms + 1] = np.inf
    return es


def event_times(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4), "reps": reps}


def pair(hip, ref, reps):
    r = {"hip": event_times(hip, reps), "torch": event_times(ref, reps)}
    r["ratio_hip_over_torch"] = round(r["hip"]["ms_median"] / r["torch"]["ms_median"], 4)
    r["hip_not_slower"] = r["hip"]["ms_median"] <= r["torch"]["ms_median"]
    return r


def main():
    from splat_slam_amd import factor_graph as fg
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_graph_times.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "hbm_peak_gb_per_s": 8000,
           "reproject": {}, "select_proximity": {}, "select_backend": {}}
    rng = np.random.default_rng(0)
    f = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32, device=DEV)
    h, w, n = 40, 80, 25
    poses = np.zeros((n, 7), np.float32)
    for k in range(n):
        ang = 0.01 * k
        poses[k] = [0.03 * k, 0.01 * np.sin(k), 0.02 * k, 0.0, np.sin(ang / 2), 0.0, np.cos(ang / 2)]
    poses, disps = f(poses), f(rng.uniform(0.45, 0.55, (n, h, w)))
    intr = f(np.tile([50.0, 50.0, 39.5, 19.5], (n, 1)) + rng.uniform(0, 0.5, (n, 4)))
    grid = torch.stack(torch.meshgrid(torch.arange(w, device=DEV).float(), torch.arange(h, device=DEV).float(), indexing="xy"), -1)
    for E in (24, 96):
        ii = torch.tensor(rng.integers(0, n, E), device=DEV)
        jj = (ii + torch.tensor(rng.integers(1, 4, E), device=DEV)) % n
        target = grid[None] + f(rng.normal(0, 3.0, (E, h, w, 2)))
        got, want = fg.reproject(poses, disps, intr, ii, jj, target), torch_reproject(poses, disps, intr, ii, jj, target, grid)
        r = pair(lambda: fg.reproject(poses, disps, intr, ii, jj, target), lambda: torch_reproject(poses, disps, intr, ii, jj, target, grid),
                 a.reps)
        r["floor_bytes"] = E * h * w * (4 + 8 + 28)                 # disparity and target read, coords, valid and motn written
        r["hip_gb_per_s_of_floor"] = round(r["floor_bytes"] / (r["hip"]["ms_median"] * 1e-3) / 1e9, 1)
        r["max_abs_difference_coords"] = float((got[0] - want[0]).abs().max())
        res["reproject"][f"40x80_{E}_edges"] = r
        print("reproject", E, "edges:", r["hip"]["ms_median"], "ms vs torch", r["torch"]["ms_median"], "ms", flush=True)
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    t = 25
    d = f(rng.uniform(0, 40, t * t))
    old = torch.tensor(rng.integers(0, t, (40, 2)), device=DEV)
    io, jo = old[:, 0].contiguous(), old[:, 1].contiguous()
    hip = lambda: fg.select_proximity_edges(d, 0, 0, t, io, jo, 2, 2, 16.0, 75)
    ref = lambda: host_proximity(d, 0, 0, t, io, jo, 2, 2, 16.0, 75)
    r = pair(hip, ref, a.reps)
    r["equal"] = list(zip(hip()[0].tolist(), hip()[1].tolist())) == ref()
    r["edges"] = len(ref())
    res["select_proximity"]["25_frames_max_factors_75"] = r
    print("select_proximity 25 frames:", r["hip"]["ms_median"], "ms vs host loop", r["torch"]["ms_median"], "ms; equal", r["equal"], flush=True)
    for n in (128, 512):
        # about 2 % of the entries lie under the threshold: the host loop reads one device scalar for each of them
        d = f(rng.uniform(0, 800, n * n))
        hip = lambda: fg.select_backend_edges(d, 0, n, None, False, 2, 1, 16.0, 100000)
        ref = lambda: host_backend(d, 0, n, 2, 1, 16.0, 100000)
        r = pair(hip, ref, a.reps)
        r["equal"] = list(zip(hip()[0].tolist(), hip()[1].tolist())) == ref()
        r["edges"] = len(ref())
        res["select_backend"][f"{n}x{n}"] = r
        print(f"select_backend {n} x {n}:", r["hip"]["ms_median"], "ms vs host loop", r["torch"]["ms_median"], "ms; equal", r["equal"],
              flush=True)
    groups = ("reproject", "select_proximity", "select_backend")
    res["hip_not_slower_everywhere"] = all(r["hip_not_slower"] for g in groups for r in res[g].values())
    res["selections_equal_everywhere"] = all(r["equal"] for g in groups[1:] for r in res[g].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"hip_not_slower_everywhere": res["hip_not_slower_everywhere"],
                      "selections_equal_everywhere": res["selections_equal_everywhere"]}))


if __name__ == "__main__":
    main()
