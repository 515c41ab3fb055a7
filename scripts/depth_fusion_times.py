"""GPU box: times of the keyframe depth fusion (splat_slam_amd.depth_fusion, csrc/sgr_fuse.hip) at the metric's 480 x 640: HIP-event
medians of prepare_mono for one map and of fuse_depth for m = 1, 16 and 64 frames read out of a 64-frame buffer, each next to a torch
composition of the same equations on the GPU, the two alternating in one process.  The torch side of prepare_mono is the mean, the
threshold and the erosion (max_pool2d of the negated flags over 11 x 11, zero padding = the reference's padding with ones); the FILL IS
LEFT OUT of it, so the ratio understates what the kernel saves.  The torch side of fuse_depth gathers the m frames, fits with fp64 sums
and composes the depth.  Also: the bytes each call must move (computed from the shapes) over its time.  Writes one JSON file.

    python scripts/depth_fusion_times.py [--out profiles/depth_fusion_times.json] [--reps 30]"""
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
H, W, N = 480, 640, 64


def mono_map(seed):
    """a smooth surface with noise, 2 % of the pixels in outlier blobs of 25 x the surface and a few pixels without a value"""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    m = 2.0 + 0.4 * torch.sin(0.02 * x + seed) * torch.cos(0.03 * y) + 0.02 * torch.rand(H, W, generator=g)
    for _ in range(12):
        cy, cx = int(torch.randint(20, H - 20, (1,), generator=g)), int(torch.randint(20, W - 20, (1,), generator=g))
        m[cy - 11:cy + 11, cx - 11:cx + 11] *= 25.0
    m.view(-1)[torch.randint(0, H * W, (40,), generator=g)] = 0.0
    return m


def torch_prepare(mono):
    """mean, threshold and erosion of one [H,W] map; no fill"""
    m = torch.where(mono > 4 * mono.mean(), torch.zeros_like(mono), mono)
    holes = (m <= 0).float()[None, None]
    eroded = torch.nn.functional.max_pool2d(holes, 11, stride=1, padding=5)[0, 0] == 0
    return torch.where(eroded, m, torch.zeros_like(m)), eroded


def torch_fuse(disps_up, valid, filled, eroded, ix, min_valid=100):
    d, v, x = disps_up[ix], valid[ix], filled[ix]
    w = (v & (eroded[ix] != 0)).double()
    y = torch.where(v, 1.0 / d, torch.zeros_like(d))
    xd, yd = x.double(), y.double()
    a00, a01, a11 = (w * xd * xd).sum((1, 2)), (w * xd).sum((1, 2)), w.sum((1, 2))
    b0, b1 = (w * xd * yd).sum((1, 2)), (w * yd).sum((1, 2))
    det = a00 * a11 - a01 * a01
    s, q = ((a11 * b0 - a01 * b1) / det).float(), ((-a01 * b0 + a00 * b1) / det).float()
    invalid = v.sum((1, 2)) < min_valid
    fill = torch.where(invalid[:, None, None], torch.zeros_like(x), x * s[:, None, None] + q[:, None, None])
    return torch.where(v, y, fill), s, q, invalid


def alternate(fns, reps):
    """HIP-event times of the callables, alternating, after a warm-up of each"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(np.min(t)), 4), "reps": reps} for k, t in times.items()}


def main():
    from splat_slam_amd import depth_fusion as df
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_fusion_times.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_fusion_times: needs the GPU; a CPU run says nothing about these kernels")
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "ht": H, "wd": W, "buffer_frames": N,
           "torch_side": "prepare: mean, threshold, max_pool2d erosion, NO fill; fuse: gather, fp64 sums, 2x2 solve, compose"}
    g = torch.Generator().manual_seed(0)
    monos = torch.stack([mono_map(s % 8) for s in range(N)]).to(DEV)
    disps_up = (0.3 + 0.7 * torch.rand(N, H, W, generator=g)).to(DEV)
    valid = (torch.rand(N, H, W, generator=g) < 0.6).to(DEV)

    filled1, eroded1 = df.prepare_mono(monos[0])
    ref_filled, ref_eroded = torch_prepare(monos[0])
    assert torch.equal(eroded1 != 0, ref_eroded) and torch.equal(filled1[ref_eroded], ref_filled[ref_eroded])
    holes = int((eroded1 == 0).sum())
    r = alternate({"hip": lambda: df.prepare_mono(monos[0]), "torch_without_fill": lambda: torch_prepare(monos[0])}, a.reps)
    r["hole_pixels"] = holes
    r["torch_over_hip"] = round(r["torch_without_fill"]["ms_median"] / r["hip"]["ms_median"], 2)
    res["prepare_mono_1x480x640"] = r
    print("prepare_mono", r, flush=True)

    filled, eroded = df.prepare_mono(monos)
    for m in (1, 16, 64):
        ix = torch.arange(N - 1, N - 1 - m, -1, device=DEV)
        d, s, q, inv = df.fuse_depth(disps_up, valid, filled, eroded, ix)
        d2, s2, q2, inv2 = torch_fuse(disps_up, valid, filled, eroded, ix)
        assert not inv.any() and not inv2.any() and torch.allclose(s, s2, rtol=1e-5) and torch.allclose(q, q2, rtol=1e-5)
        assert torch.equal(d[valid[ix]], d2[valid[ix]]) and torch.allclose(d, d2, rtol=1e-4)
        r = alternate({"hip": lambda: df.fuse_depth(disps_up, valid, filled, eroded, ix),
                       "torch": lambda: torch_fuse(disps_up, valid, filled, eroded, ix)}, a.reps)
        must_move = m * H * W * (2 * (4 + 1 + 4) + 1 + 4)      # both passes read disp, mask and mono; the first the erosion; one write
        r["bytes_moved"] = must_move
        r["hip_gb_per_s"] = round(must_move / (r["hip"]["ms_median"] * 1e-3) / 1e9, 1)
        r["torch_over_hip"] = round(r["torch"]["ms_median"] / r["hip"]["ms_median"], 2)
        res[f"fuse_depth_m{m}"] = r
        print(f"fuse_depth m={m}", r, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["hip"]["ms_median"] for k, v in res.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
