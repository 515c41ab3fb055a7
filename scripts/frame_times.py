"""GPU box: times of the frame preparation (splat_slam_amd.datasets, csrc/sgr_frame.hip) at the two shapes the reference's configs use:
Replica-like 680 x 1200 -> 344 x 600 without an undistortion map, and TUM 480 x 640 -> 384 x 512 with edges 8 and the freiburg1
distortion.  Per shape, HIP-event medians of
  - the sgr_frame_prepare launch on bytes that are already on the device (RGBX u8 + u16 depth -> fp32 colour and depth),
  - a torch composition of the same work on the device (grid_sample for the map, bilinear interpolate, / 255, nearest depth, crop),
    the two alternating in one process,
  - a whole stream[i] (Pillow decode, copy, launch) over a sequence written to a temporary directory, with prefetch 0 and 1 and
    prepare="hip", and with prepare="host" (numpy on the CPU, then one copy); read back to back, and with a host pause between reads
    that stands for the consumer's work (the pause is outside the timed window: it is what lets the prefetch thread run ahead),
and, by the host clock, the numpy host path alone.  Also the bytes the launch must move (from the shapes) over its time.  The torch
composition is float bilinear, not the integer arithmetic: it is a time yardstick, its values differ in the last bits.  Writes one JSON
file.

    python scripts/frame_times.py [--out profiles/frame_times.json] [--reps 30] [--frames 12] [--pause-ms 20]"""
import argparse
import datetime
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
TUM_DISTORTION = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
SHAPES = {
    "replica_680x1200_to_344x600": dict(dataset="replica", H=680, W=1200, fx=600.0, fy=600.0, cx=599.5, cy=339.5, H_out=344, W_out=600,
                                        H_edge=0, W_edge=0, png_depth_scale=6553.5),
    "tum_480x640_to_384x512_edge8_map": dict(dataset="tumrgbd", H=480, W=640, fx=517.3, fy=516.5, cx=318.6, cy=255.3, H_out=384, W_out=512,
                                             H_edge=8, W_edge=8, png_depth_scale=5000.0, distortion=TUM_DISTORTION),
}


def frame(k, H, W):
    """a smooth image with some texture (what a JPEG encoder sees in a room) and a depth ramp"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    rng = np.random.default_rng(k)
    rgb = np.stack([127 + 100 * np.sin(0.01 * xx + 0.3 * k), 127 + 100 * np.cos(0.013 * yy - 0.2 * k), 0.1 * (xx + yy) % 256], -1)
    rgb = np.clip(rgb + rng.normal(0, 6, rgb.shape), 0, 255).astype(np.uint8)
    depth = np.clip(6553.5 * (1.5 + 0.001 * xx + 0.002 * yy + 0.05 * k), 0, 65535).astype(np.uint16)
    return rgb, depth


def write_sequence(root, name, cam, frames):
    from PIL import Image
    cam = dict(cam)
    dataset = cam.pop("dataset")
    base = os.path.join(root, name)
    if dataset == "replica":
        os.makedirs(os.path.join(base, "results"))
        with open(os.path.join(base, "traj.txt"), "w") as f:
            for k in range(frames):
                rgb, depth = frame(k, cam["H"], cam["W"])
                Image.fromarray(rgb).save(os.path.join(base, "results", f"frame{k:06d}.jpg"), quality=90)
                Image.fromarray(depth).save(os.path.join(base, "results", f"depth{k:06d}.png"))
                f.write(" ".join(str(v) for v in np.eye(4).reshape(-1)) + "\n")
    else:
        os.makedirs(os.path.join(base, "rgb"))
        os.makedirs(os.path.join(base, "depth"))
        with open(os.path.join(base, "rgb.txt"), "w") as fc, open(os.path.join(base, "depth.txt"), "w") as fd, \
                open(os.path.join(base, "groundtruth.txt"), "w") as fp:
            for k in range(frames):
                t = 100.0 + 0.1 * k
                rgb, depth = frame(k, cam["H"], cam["W"])
                Image.fromarray(rgb).save(os.path.join(base, "rgb", f"{t:.6f}.png"))          # TUM colour is PNG
                Image.fromarray(depth).save(os.path.join(base, "depth", f"{t:.6f}.png"))
                fc.write(f"{t:.6f} rgb/{t:.6f}.png\n")
                fd.write(f"{t:.6f} depth/{t:.6f}.png\n")
                fp.write(f"{t:.6f} {0.01 * k} 0 0 0 0 0 1\n")
    return {"dataset": dataset, "stride": 1, "max_frames": -1, "cam": cam, "data": {"dataset_root": root, "input_folder": name}}


def event_times(fns, reps, between=None):
    """HIP-event times of the callables, alternating, after a warm-up of each"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            if between is not None:
                between()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(np.min(t)), 4), "reps": reps} for k, t in times.items()}


def torch_composition(color_u8, depth_i16, grid, H_oe, W_oe, H_edge, W_edge, scale):
    """the reference's per-frame work with torch ops on the device"""
    import torch.nn.functional as F
    img = color_u8[..., :3].permute(0, 3, 1, 2).float()
    if grid is not None:
        img = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    img = F.interpolate(img, (H_oe, W_oe), mode="bilinear", align_corners=False) / 255.0
    depth = (depth_i16.to(torch.int32) & 0xFFFF).float() / scale
    depth = F.interpolate(depth[:, None], (H_oe, W_oe), mode="nearest")[:, 0]
    return (img[:, :, H_edge:H_oe - H_edge, W_edge:W_oe - W_edge].contiguous(),
            depth[:, H_edge:H_oe - H_edge, W_edge:W_oe - W_edge].contiguous())


def main():
    from splat_slam_amd import datasets as D
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_times.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--pause-ms", type=float, default=20.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "frame_times.py measures on the GPU"
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "frames": args.frames,
           "pause_ms": args.pause_ms,
           "torch_side": "u8 -> float, grid_sample (map only), bilinear interpolate, / 255, nearest depth, crop; float arithmetic",
           "stream_item": "Pillow decode + copy + launch of one stream[i], read in order and cyclically; HIP events around the call"}
    with tempfile.TemporaryDirectory() as root:
        for name, cam in SHAPES.items():
            cfg = write_sequence(root, name, cam, args.frames)
            H, W, H_edge, W_edge = cam["H"], cam["W"], cam["H_edge"], cam["W_edge"]
            H_oe, W_oe, scale = cam["H_out"] + 2 * H_edge, cam["W_out"] + 2 * W_edge, cam["png_depth_scale"]
            rgb, depth = frame(0, H, W)
            rgbx = np.concatenate([rgb, np.zeros((H, W, 1), np.uint8)], -1)[None]
            map_host = D.undistortion_map(H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["distortion"]) if "distortion" in cam else None
            color_d = torch.from_numpy(rgbx).to(DEV)
            depth_d = torch.from_numpy(depth.view(np.int16)[None].copy()).to(DEV)
            map_d = None if map_host is None else torch.from_numpy(map_host).to(DEV)
            grid = None
            if map_host is not None:          # the same positions as a normalised grid_sample grid (align_corners=True)
                q = torch.from_numpy(map_host).to(DEV).float() / 32.0
                grid = torch.stack([2.0 * q[..., 0] / (W - 1) - 1.0, 2.0 * q[..., 1] / (H - 1) - 1.0], -1)[None]
            entry = {"map": map_host is not None}
            entry["launch"] = event_times({
                "hip": lambda: D.frame_prepare(color_d, depth_d, map_d, H_oe, W_oe, H_edge, W_edge, scale),
                "torch": lambda: torch_composition(color_d, depth_d, grid, H_oe, W_oe, H_edge, W_edge, scale)}, args.reps)
            a = D.frame_prepare(color_d, depth_d, map_d, H_oe, W_oe, H_edge, W_edge, scale)
            b = torch_composition(color_d, depth_d, grid, H_oe, W_oe, H_edge, W_edge, scale)
            entry["max_abs_colour_difference_hip_torch_in_levels"] = round(float((a[0] - b[0]).abs().max()) * 255.0, 3)
            # (the kernel's depth is CPU torch's bit for bit, tests/test_gpu_datasets.py; what torch computes on the device may differ)
            entry["depth_equal_hip_torch"] = bool(torch.equal(a[1], b[1]))
            entry["max_rel_depth_difference_hip_torch"] = float(((a[1] - b[1]).abs() / a[1].abs().clamp_min(1e-30)).max())
            out_px = cam["H_out"] * cam["W_out"]
            moved = H * W * 6 + (H * W * 8 if map_host is not None else 0) + out_px * 16      # inputs read at most once + outputs
            entry["bytes_moved_upper"] = moved
            entry["hip_gb_per_s"] = round(moved / (entry["launch"]["hip"]["ms_median"] * 1e-3) / 1e9, 1)
            entry["torch_over_hip"] = round(entry["launch"]["torch"]["ms_median"] / entry["launch"]["hip"]["ms_median"], 2)
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                D.frame_prepare_host(rgbx, depth[None], map_host, H_oe, W_oe, H_edge, W_edge, scale)
                t.append(1e3 * (time.perf_counter() - t0))
            entry["host_path_numpy"] = {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(np.min(t)), 3), "reps": 5,
                                        "clock": "host"}
            streams = {"hip_prefetch0": D.get_dataset(cfg, DEV, "hip", 0), "hip_prefetch1": D.get_dataset(cfg, DEV, "hip", 1),
                       "host_prefetch0": D.get_dataset(cfg, DEV, "host", 0), "host_prefetch1": D.get_dataset(cfg, DEV, "host", 1)}
            cursor = {k: 0 for k in streams}

            def reader(key):
                def read():
                    i = cursor[key] % len(streams[key])
                    cursor[key] += 1
                    return streams[key][i]
                return read

            fns = {k: reader(k) for k in streams}
            stream_reps = max(args.reps, 2 * args.frames)
            entry["stream_item_back_to_back"], entry["stream_item_after_pause"] = {}, {}
            for k, fn in fns.items():           # one stream at a time: nothing else gives its prefetch thread a head start
                entry["stream_item_back_to_back"].update(event_times({k: fn}, stream_reps))
                entry["stream_item_after_pause"].update(event_times({k: fn}, stream_reps, between=lambda: time.sleep(args.pause_ms * 1e-3)))
            for s in streams.values():
                s.close()
            res[name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
