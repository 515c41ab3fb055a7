"""GPU box: what the per-keyframe figures cost (splat_slam_amd.plots, csrc/sgr_plot.hip), at the two image sizes the reference's configs
use, 680 x 1200 (s = 2) and 480 x 640 (s = 1), for 16 frames per call.  Per size,
  - HIP-event medians of compose_panels (the table copy and the two launches of sgr_plot_panels) and of a torch composition of the
    same six cells on the device (clamp, jet lookups by index, the two maxima, an average pool, pasted into a white canvas; no text),
    the two alternating in one process after a warm-up of each;
  - by the host clock, per panel: the copy of a chunk's panels to the host, and the PNG encoding by Pillow;
  - where matplotlib imports, the host time of one matplotlib figure of the same six images (2 x 3 imshow, savefig), labelled as such:
    the reference's way, after its four full images went to the host.
The torch composition is a time yardstick: float division where the kernel rounds in integers, so its values differ in places.
Writes one JSON file.

    python scripts/plots_times.py [--out profiles/plots_times.json] [--reps 20] [--frames 16]"""
import argparse
import datetime
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
SHAPES = {"680x1200": (680, 1200), "480x640": (480, 640)}


def event_times(fns, reps):
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


def host_times(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(np.min(t)), 3), "reps": reps, "clock": "host"}


def make_frames(n, H, W):
    g = torch.Generator(device=DEV).manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    out = []
    for k in range(n):
        gt = torch.stack([0.5 + 0.5 * torch.sin(0.01 * xx + k), 0.5 + 0.5 * torch.cos(0.013 * yy - k), (0.001 * (xx + yy)) % 1.0])
        render = (gt + 0.03 * torch.randn(3, H, W, device=DEV, generator=g)).contiguous()
        gd = (1.5 + 0.001 * xx + 0.002 * yy + 0.05 * k).contiguous()
        d = (gd + 0.05 * torch.randn(H, W, device=DEV, generator=g)).contiguous()
        out.append((render, gt.contiguous(), d, gd))
    return out


def torch_composition(frames, s, jet, size, global_scale=1.0, depth_max=5.0):
    """the six cells with torch ops on the device; no text"""
    import torch.nn.functional as F
    PH, PW = size
    render = torch.stack([f[0] for f in frames])
    gt = torch.stack([f[1] for f in frames])
    d = torch.stack([f[2] for f in frames]) * global_scale
    gd = torch.stack([f[3] for f in frames])
    lg, lp = (255.0 * gt.clamp(0, 1)).to(torch.int64), (255.0 * render.clamp(0, 1)).to(torch.int64)
    e = (lg - lp).abs().sum(1)
    ed = torch.where((d > 0) & (gd > 0), (d - gd).abs(), torch.zeros_like(d))
    idx = lambda t: (256.0 * t).floor().clamp(0, 255).to(torch.int64)
    as_chw = lambda lut: jet[lut].permute(0, 3, 1, 2).float()
    cells = [lg.float(), as_chw(idx(gd / depth_max)), as_chw((256 * e // e.amax((1, 2), keepdim=True).clamp_min(1)).clamp_max(255)),
             lp.float(), as_chw(idx(d / depth_max)), as_chw(idx(ed / ed.amax((1, 2), keepdim=True).clamp_min(1e-30)))]
    canvas = torch.full((len(frames), 3, PH, PW), 255, dtype=torch.uint8, device=DEV)
    for k, c in enumerate(cells):
        small = F.avg_pool2d(c, s, ceil_mode=True, count_include_pad=False).round().to(torch.uint8)
        ch, cw = small.shape[-2:]
        y0, x0 = 32 + (k // 3) * (28 + ch) + 20, 8 + (k % 3) * (cw + 8)
        canvas[:, :, y0:y0 + ch, x0:x0 + cw] = small
    return canvas.permute(0, 2, 3, 1).contiguous()


def matplotlib_figure(images):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, axs = plt.subplots(2, 3, figsize=(12, 6))
    for ax, (img, cmap) in zip(axs.reshape(-1), images):
        ax.imshow(img, cmap=cmap)
        ax.set_title("title")
        ax.axis("off")
    fig.savefig(io.BytesIO(), format="png", bbox_inches="tight")
    plt.close(fig)


def main():
    from PIL import Image
    from splat_slam_amd import plots
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plots_times.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "plots_times.py measures on the GPU"
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "frames_per_call": args.frames,
           "torch_side": "clamp, jet by index, amax, avg_pool2d, paste into a white canvas; float arithmetic, no text",
           "hip_side": "plots.compose_panels: the host table, its copy, the two launches of sgr_plot_panels"}
    jet = torch.from_numpy(plots.jet_table()).to(DEV)
    n = args.frames
    for name, (H, W) in SHAPES.items():
        frames = make_frames(n, H, W)
        s = plots.reduction_factor(W)
        size = plots.panel_size(H, W, s)
        lists = [[f[i] for f in frames] for i in range(4)]
        headings, titles = ["frame: video_idx_%d_kf_idx_%d" % (k, 5 * k) for k in range(n)], [plots.frame_titles(25.0 + k, 0.1) for k in range(n)]
        hip = lambda: plots.compose_panels(*lists, headings, titles, s=s)
        entry = {"s": s, "panel": list(size), "panel_bytes": size[0] * size[1] * 3}
        entry["compose_16_frames"] = event_times({"hip": hip, "torch": lambda: torch_composition(frames, s, jet, size)}, args.reps)
        entry["torch_over_hip"] = round(entry["compose_16_frames"]["torch"]["ms_median"] / entry["compose_16_frames"]["hip"]["ms_median"], 2)
        panels = hip()
        torch.cuda.synchronize()
        copy = host_times(lambda: panels.cpu(), 10)
        entry["copy_to_host_per_panel"] = {**copy, "ms_median": round(copy["ms_median"] / n, 3), "ms_min": round(copy["ms_min"] / n, 3)}
        host = panels.cpu().numpy()
        entry["png_encode_per_panel"] = host_times(lambda: Image.fromarray(host[0]).save(io.BytesIO(), format="png"), 5)
        try:
            imgs = [(frames[0][1].permute(1, 2, 0).clamp(0, 1).cpu().numpy(), None), (frames[0][3].cpu().numpy(), "jet"),
                    ((frames[0][1] - frames[0][0]).abs().sum(0).cpu().numpy(), "jet"), (frames[0][0].permute(1, 2, 0).clamp(0, 1).cpu().numpy(), None),
                    (frames[0][2].cpu().numpy(), "jet"), ((frames[0][2] - frames[0][3]).abs().cpu().numpy(), "jet")]
            matplotlib_figure(imgs)
            entry["matplotlib_figure_per_frame_host"] = host_times(lambda: matplotlib_figure(imgs), 3)
        except ImportError:
            entry["matplotlib_figure_per_frame_host"] = "matplotlib is not importable here"
        res[name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
