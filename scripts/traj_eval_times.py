"""GPU box: times of the trajectory scoring (csrc/sgr_traj.hip, splat_slam_amd.traj_eval) at n = 512 keyframes and n = 2 000 frames:
the two entry points (HIP events around a batch of calls on one stream: the per-call time with the launches back to back), one
kf_traj_eval (host clock around work that ends in a device synchronise: two read-backs), and the obvious alternative, alternating
with it in the same process: download video.poses, then the numpy fp64 restatement (centres, Umeyama, errors, statistics).  No claim
is made in advance: at these sizes both are dominated by fixed costs, and the file says what was measured.  Writes one JSON file.

    python scripts/traj_eval_times.py [--out profiles/traj_eval_times.json] [--reps 30] [--batch 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"


def batch_us(fn, batch, reps):
    """median and spread over reps of (event time of `batch` back-to-back calls) / batch, microseconds"""
    fn()
    vals = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        vals.append(a.elapsed_time(b) * 1e3 / batch)
    return {"median_us": float(np.median(vals)), "min_us": float(np.min(vals)), "max_us": float(np.max(vals))}


def host_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def numpy_kf_traj_eval(video, gt):
    """the alternative: one download of the poses, then numpy fp64"""
    n = video.counter.value
    p = video.poses[:n].cpu().numpy().astype(np.float64)
    ts = video.timestamp[:n].cpu().numpy().astype(np.int64)
    ref = gt[ts]
    ok = np.isfinite(ref.reshape(n, 16).sum(1))
    t, q = p[:, :3], p[:, 3:]
    u, w = -q[:, :3], q[:, 3:4]
    c = np.cross(u, t)
    x, y = -(t + 2.0 * (w * c + np.cross(u, c)))[ok], ref[ok, :3, 3].astype(np.float64)
    xm, ym = x.mean(0), y.mean(0)
    dx, dy = x - xm, y - ym
    var = (dx * dx).sum() / len(x)
    U, d, Vt = np.linalg.svd(dy.T @ dx / len(x))
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    r = U @ S @ Vt
    s = np.trace(np.diag(d) @ S) / var
    e = np.linalg.norm(s * x @ r.T + (ym - s * r @ xm) - y, axis=1)
    return {"rmse": float(np.sqrt((e * e).mean())), "mean": float(e.mean()), "median": float(np.median(e)), "std": float(e.std()),
            "min": float(e.min()), "max": float(e.max()), "sse": float((e * e).sum())}, float(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_eval_times.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=200)
    args = ap.parse_args()
    import traj_eval_ref as R
    from splat_slam_amd import _native as nat
    from splat_slam_amd import traj_eval as te
    from splat_slam_amd.depth_video import DepthVideo
    lib = nat.lib()
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, batch=args.batch, launches=te.LAUNCHES, sizes={})
    for n in (512, 2000):
        rng = np.random.default_rng(n)
        x = np.cumsum(rng.normal(scale=0.02, size=(n, 3)), 0)
        video = DepthVideo(8, 8, buffer=n, device=DEV)
        video.poses[:] = torch.tensor(R.w2c_from_centres(x, rng), device=DEV)
        video.timestamp[:] = torch.arange(n, device=DEV, dtype=torch.float32)
        video.counter.value = n
        gt = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
        gt[:, :3, 3] = 1.3 * x + 0.01 * rng.normal(size=(n, 3))
        gt[7, 0, 0] = np.nan
        ref = torch.tensor(gt, device=DEV)
        pairs = te.pair_centres(video.poses[:n], ref)
        r, t, s = te.umeyama(pairs.sums)
        sim3 = (nat.C.c_double * 13)(s, *r.reshape(-1).tolist(), *t.tolist())
        sums = torch.empty(17, dtype=torch.float64, device=DEV)
        err = torch.empty(n, dtype=torch.float64, device=DEV)
        stats = torch.empty(8, dtype=torch.float64, device=DEV)
        scratch, nbytes = pairs._scratch, pairs._scratch.numel()
        acc = lambda: nat.check(lib.sgr_traj_accumulate(te.POSE7_W2C, video.poses.data_ptr(), n, None, n, ref.data_ptr(), pairs.pos.data_ptr(),
                                                        pairs.valid.data_ptr(), sums.data_ptr(), scratch.data_ptr(), nbytes, stream), "acc")
        errs = lambda: nat.check(lib.sgr_traj_errors(n, pairs.pos.data_ptr(), pairs.valid.data_ptr(), sim3, err.data_ptr(), stats.data_ptr(),
                                                     scratch.data_ptr(), nbytes, stream), "err")
        row = {"sgr_traj_accumulate": batch_us(acc, args.batch, args.reps), "sgr_traj_errors": batch_us(errs, args.batch, args.reps)}
        hip, alt = [], []
        te.kf_traj_eval(video, gt)
        numpy_kf_traj_eval(video, gt)
        for _ in range(args.reps):                       # alternating, same process
            us, got = host_us(lambda: te.kf_traj_eval(video, gt))
            hip.append(us)
            us, want = host_us(lambda: numpy_kf_traj_eval(video, gt))
            alt.append(us)
        row["kf_traj_eval_host_us"] = {"median_us": float(np.median(hip)), "min_us": float(np.min(hip)), "max_us": float(np.max(hip))}
        row["numpy_after_download_host_us"] = {"median_us": float(np.median(alt)), "min_us": float(np.min(alt)), "max_us": float(np.max(alt))}
        row["rmse"] = {"hip": got[0]["rmse"], "numpy": want[0]["rmse"]}
        row["scale"] = {"hip": got[1], "numpy": want[1]}
        out["sizes"][str(n)] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
