"""GPU box: times of the trajectory scoring (csrc/sgr_traj.hip, splat_slam_amd.traj_eval) at n = 512 keyframes and n = 2 000 frames:
the two entry points (HIP events around a batch of calls on one stream: the per-call time with the launches back to back), one
kf_traj_eval (host clock around work that ends in a device synchronise: two read-backs), and the obvious alternative, alternating
with it in the same process: download video.poses, then the numpy fp64 restatement (centres, Umeyama, errors, statistics); the same for sgr_traj_associate, sgr_traj_pose_errors and one rpe().  No claim
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


def numpy_rpe(video, gt, sim3, delta):
    """the alternative to rpe(): one download of the poses, then the relative translation error in numpy fp64"""
    n = video.counter.value
    p = video.poses[:n].cpu().numpy().astype(np.float64)
    ok = np.isfinite(gt.reshape(n, 16).sum(1))
    s, r_a, t_a = sim3
    q = p[:, 3:] / np.linalg.norm(p[:, 3:], axis=1, keepdims=True)
    x, y, z, w = q.T
    rot = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w), 2 * (x * y - z * w), 1 - 2 * (x * x + z * z),
                    2 * (y * z + x * w), 2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)
    P = np.tile(np.eye(4), (n, 1, 1))
    P[:, :3, :3] = r_a @ rot
    P[:, :3, 3] = s * np.einsum("ij,nj->ni", r_a, -np.einsum("nij,nj->ni", rot, p[:, :3])) + t_a
    P, Q = P[ok], gt[ok].astype(np.float64)
    i = np.arange(0, len(P) - delta, delta)[:(len(P) - 1) // delta]
    E = np.linalg.inv(np.linalg.inv(Q[i]) @ Q[i + delta]) @ (np.linalg.inv(P[i]) @ P[i + delta])
    e = np.linalg.norm(E[:, :3, 3], axis=1)
    return {"rmse": float(np.sqrt((e * e).mean())), "mean": float(e.mean()), "median": float(np.median(e))}


def pose_error_times(n, video, gt, ref, sim3, args, nat, te, lib, stream):
    """sgr_traj_associate (n stamps into a clock five times as dense) and sgr_traj_pose_errors (relative, delta 1, translation part) per
    call, and one rpe() against numpy_rpe(), alternating"""
    rng = np.random.default_rng(n + 1)
    stamps_b = torch.tensor(np.arange(5 * n) * 0.01, device=DEV)
    stamps_a = torch.tensor(np.sort(rng.choice(5 * n, n, replace=False)) * 0.01 + rng.uniform(-0.002, 0.002, n), device=DEV)
    out = torch.empty(3, n, dtype=torch.int32, device=DEV)
    header = torch.empty(nat.SGR_TRAJ_HEADER_WORDS, dtype=torch.int32, device=DEV)
    a_bytes = lib.sgr_traj_associate_scratch_bytes(n, 5 * n)
    a_scratch = torch.empty(a_bytes, dtype=torch.uint8, device=DEV)
    assoc = lambda: nat.check(lib.sgr_traj_associate(stamps_a.data_ptr(), n, stamps_b.data_ptr(), 5 * n, 0.0, 0.005, out[0].data_ptr(),
                                                     out[1].data_ptr(), out[2].data_ptr(), header.data_ptr(), a_scratch.data_ptr(), a_bytes,
                                                     stream), "associate")
    s, r, t = sim3
    c_sim3 = (nat.C.c_double * 13)(s, *r.reshape(-1).tolist(), *t.tolist())
    p_bytes = lib.sgr_traj_pose_errors_scratch_bytes(n)
    p_scratch = torch.empty(p_bytes, dtype=torch.uint8, device=DEV)
    err = torch.empty(n, dtype=torch.float64, device=DEV)
    pair_rows = torch.empty(n, 2, dtype=torch.int32, device=DEV)
    stats = torch.empty(8, dtype=torch.float64, device=DEV)
    flat = ref.reshape(n, 16)
    pose = lambda: nat.check(lib.sgr_traj_pose_errors(te.POSE7_W2C, video.poses.data_ptr(), n, flat.data_ptr(), n, None, None, n, c_sim3,
                                                      nat.SGR_TRAJ_RELATIVE, 1, 0, nat.SGR_TRAJ_TRANSLATION_PART, err.data_ptr(),
                                                      pair_rows.data_ptr(), stats.data_ptr(), header.data_ptr(), p_scratch.data_ptr(), p_bytes,
                                                      stream), "pose_errors")
    row = {"sgr_traj_associate": batch_us(assoc, args.batch, args.reps), "sgr_traj_pose_errors": batch_us(pose, args.batch, args.reps)}
    al = te.Alignment(r, t, s, 0, 0)
    hip, alt = [], []
    te.rpe(video.poses[:n], ref, al, delta=1)
    numpy_rpe(video, gt, sim3, 1)
    for _ in range(args.reps):                           # alternating, same process
        us, got = host_us(lambda: te.rpe(video.poses[:n], ref, al, delta=1).stats)
        hip.append(us)
        us, want = host_us(lambda: numpy_rpe(video, gt, sim3, 1))
        alt.append(us)
    spread = lambda v: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}
    row["rpe_host_us"] = spread(hip)
    row["numpy_rpe_after_download_host_us"] = spread(alt)
    row["rpe_rmse"] = {"hip": got["rmse"], "numpy": want["rmse"]}
    return row


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
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, batch=args.batch, launches={**te.LAUNCHES, **te.POSE_LAUNCHES}, sizes={})
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
        row.update(pose_error_times(n, video, gt, ref, (s, r, t), args, nat, te, lib, stream))
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
