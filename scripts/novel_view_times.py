"""GPU box: what the novel-view evaluation costs (splat_slam_amd.novel_view, csrc/sgr_novel.hip), at 3 x 480 x 640 and 3 x 344 x 600.
  - exposure fit, n = 1 and n = 16 frames per call: HIP-event time per call of sgr_exposure_fit (its two launches) and of a torch
    composition of the same six masked fp64 sums on the device (mask, two casts, three products, six reductions), the two
    alternating in one process after a warm-up of each; a sample is the event time of `inner` calls back to back, divided by
    `inner`, so it holds the launch gaps a caller sees.  Median, minimum and maximum over the samples.  The two sides' (a, b)
    are compared, so that the time is the time of the same result;
  - a whole chunk: the host-clock time of eval_novel_views over 16 held-out frames of the synthetic room (it ends in its copy to the
    host, so the device is done), per exposure mode: 16 renders, the table, the fit, the metrics.
No threshold: the numbers are a record.  Writes one JSON file.

    python scripts/novel_view_times.py [--out profiles/novel_view_times.json] [--samples 30] [--inner 10]"""
import argparse
import datetime
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
SHAPES = {"3x480x640": (3, 480, 640), "3x344x600": (3, 344, 600)}


def summary(t, unit_scale, digits):
    return {"median": round(float(np.median(t)) * unit_scale, digits), "min": round(float(np.min(t)) * unit_scale, digits),
            "max": round(float(np.max(t)) * unit_scale, digits), "samples": len(t)}


def event_times(fns, samples, inner):
    """HIP-event time per call in microseconds of the callables, alternating, after a warm-up of each"""
    for fn in fns.values():
        for _ in range(5):
            fn()
    times = {k: [] for k in fns}
    for _ in range(samples):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / inner)
    return {k: {**summary(t, 1e3, 2), "unit": "us per call", "calls_per_sample": inner} for k, t in times.items()}


def make_images(n, C, H, W):
    g = torch.Generator(device=DEV).manual_seed(3)
    render = torch.rand((n, C, H, W), device=DEV, generator=g) * 0.8 + 0.1
    gt = (1.3 * render - 0.05 + 1e-3 * torch.randn((n, C, H, W), device=DEV, generator=g)).clamp(0, 1)
    gt[torch.rand((n, C, H, W), device=DEV, generator=g) < 0.2] = 0
    return render.contiguous(), gt.contiguous()


def torch_fit(render, gt):
    """the six masked fp64 sums and the solve with torch ops on the device: [n,2]"""
    mask = gt > 0
    r = torch.where(mask, render.double(), 0.0).flatten(1)
    t = torch.where(mask, gt.double(), 0.0).flatten(1)
    m, sr, st, srr, srt, stt = mask.flatten(1).sum(1).double(), r.sum(1), t.sum(1), (r * r).sum(1), (r * t).sum(1), (t * t).sum(1)
    gain = (m * srt - sr * st) / (m * srr - sr * sr)
    return torch.stack([gain.log(), (st - gain * sr) / m], dim=1).float(), stt


def fit_times(nat, lib, n, shape, samples, inner):
    C, H, W = shape
    render, gt = make_images(n, C, H, W)
    ab = torch.zeros((n, 2), dtype=torch.float32, device=DEV)
    flags = torch.zeros(n, dtype=torch.int32, device=DEV)
    table = (nat.SgrMetricFrame * n)()
    for f in range(n):
        table[f] = nat.SgrMetricFrame(render[f].data_ptr(), gt[f].data_ptr(), None, None, ab[f, 0:].data_ptr(), ab[f, 1:].data_ptr())
    nbytes = lib.sgr_exposure_fit_bytes(n, C, H, W)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def hip():
        nat.check(lib.sgr_exposure_fit(n, table, C, H, W, ab.data_ptr(), flags.data_ptr(), scratch.data_ptr(), nbytes, stream), "sgr_exposure_fit")

    entry = event_times({"hip": hip, "torch": lambda: torch_fit(render, gt)}, samples, inner)
    hip()
    entry["max_abs_difference_of_ab"] = float((ab - torch_fit(render, gt)[0]).abs().max())
    entry["flags"] = int(flags.sum())
    entry["bytes_read"] = 2 * n * C * H * W * 4
    entry["hip_read_GB_per_s_at_median"] = round(entry["bytes_read"] / (entry["hip"]["median"] * 1e-6) / 1e9, 1)
    entry["torch_over_hip"] = round(entry["torch"]["median"] / entry["hip"]["median"], 2)
    return entry


def chunk_times(shape, reps):
    """eval_novel_views over 16 held-out frames between six mapped orbit views of the synthetic room, per exposure mode"""
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.novel_view import EXPOSURE_MODES, eval_novel_views
    from splat_slam_amd.renderer import render
    from splat_slam_amd.session import MappingSession
    C, H, W = shape
    f = 400.0 * W / 640.0
    intr = dict(W=W, H=H, fx=f, fy=f, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0)
    world = syn.room_parameters(60000, seed=43, device=DEV)
    world["scaling"] = world["scaling"] * 0 + world["scaling"].mean(dim=1, keepdim=True) + 1.6
    world["opacity"] = torch.full_like(world["opacity"], 4.0)
    gm = syn.model_from_parameters(world, device=DEV, knn_fn=lambda p: torch.ones(p.shape[0], device=p.device))
    cams = syn.make_views(world, 6, intr, DEV, seed=5, perturb=False)
    bg = torch.zeros(3, device=DEV)
    loop = types.SimpleNamespace(config=syn.DEFAULT_CONFIG, device=DEV, viewpoints={6 * k: c for k, c in enumerate(cams)}, gaussians=gm,
                                 background=bg)
    sess = MappingSession(loop, intr)
    T = 36
    w2c = torch.stack([syn.orbit_w2c(k / 6.0, 6) for k in range(T)])
    c2w = torch.linalg.inv(w2c.double()).float().to(DEV)
    ids = [k for k in range(T) if k % 6][:16]
    frames = [(None, None)] * T
    with torch.no_grad():
        for k in ids:
            cam = syn.make_camera(k, w2c[k], intr, torch.zeros(3, H, W, device=DEV), torch.zeros(H, W, device=DEV), DEV)
            pkg = render(cam, gm, PipelineParams(), bg)
            frames[k] = ((0.7 * pkg["render"].detach() + 0.1).clamp(0, 1).contiguous(), pkg["depth"][0].detach().contiguous())

    class Stream:
        def __getitem__(self, i):
            return float(i), frames[i][0], frames[i][1], None

    stream = Stream()
    out = {"frames": len(ids), "gaussians": 60000}
    for mode in EXPOSURE_MODES:
        for _ in range(2):
            res = eval_novel_views(sess, stream, c2w, ids, exposure=mode)
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eval_novel_views(sess, stream, c2w, ids, exposure=mode)
            t.append(time.perf_counter() - t0)
        out[mode] = {**summary(t, 1e3, 3), "unit": "ms per 16-frame call", "clock": "host", "mean_psnr": res["mean_psnr"]}
    return out


def main():
    from splat_slam_amd import _native as nat
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "novel_view_times.json"))
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--chunk-reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "novel_view_times.py measures on the GPU"
    lib = nat.lib()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "hip_side": "sgr_exposure_fit: two launches, six fp64 sums per frame in fixed order, the solve on the device",
           "torch_side": "mask, casts to fp64, where, three products, six sums over dim 1, the solve; no fixed order of additions"}
    for name, shape in SHAPES.items():
        entry = {"exposure_fit": {f"n={n}": fit_times(nat, lib, n, shape, args.samples, args.inner) for n in (1, 16)}}
        entry["chunk_of_16"] = chunk_times(shape, args.chunk_reps)
        res[name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
