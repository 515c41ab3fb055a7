"""GPU box: times of the depth-video kernels (splat_slam_amd.depth_video, csrc/sgr_video.hip), each next to the same operation written
with plain torch ops in the same process: DepthVideo.upsample for 1, 12 and 25 frames at 60x80 -> 480x640 with fp16 and fp32 masks,
update_valid_depth_mask(up=True) on 12 frames at 480x640 and update_valid_depth_mask(up=False) on 100 frames at 60x80.  HIP-event
medians after one warm-up; the effective bandwidth is the traffic floor of DESIGN.md section 3 ("Depth video") over the median time.
Writes one JSON file.

    python scripts/depth_video_times.py [--out profiles/depth_video_times.json] [--reps 20]"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
HT, WD = 480, 640
REL, VISIBLE = 0.01, 2


def video(n, buffer, seed=0):
    import dba_ref as R
    from splat_slam_amd.depth_video import DepthVideo
    rng = np.random.default_rng(seed)
    v = DepthVideo(HT, WD, buffer=buffer, device=DEV, filter_thresh=REL, filter_visible_num=VISIBLE)
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)
    for k in range(n):
        t, q = R.exp_se3(np.concatenate([[0.03 * k, 0.01 * np.sin(k), 0.02 * k], rng.normal(0, 0.01, 3)]))
        v.append(float(k), torch.zeros(3, HT, WD, dtype=torch.uint8, device=DEV), f(np.concatenate([t, q])),
                 f(rng.uniform(0.45, 0.55, (HT // 8, WD // 8))), None, f([75.0, 75.0, 39.5, 29.5]))
    v.disps_up[:n] = F.interpolate(v.disps[:n, None], scale_factor=8, mode="bilinear")[:, 0]
    return v, rng


def torch_upsample(v, ix, mask):
    """cvx_upsample of the reference (modules/droid_net/droid_net.py:23-37) on disps[ix], written back as DepthVideo.upsample does"""
    data = v.disps[ix].unsqueeze(1)
    n, _, h, w = data.shape
    m = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(data, kernel_size=(3, 3), padding=(1, 1)).view(n, 1, 9, 1, 1, h, w)
    up = torch.sum(m * up, dim=2).permute(0, 4, 2, 5, 3, 1).contiguous()
    v.disps_up[ix] = up.reshape(n, 8 * h, 8 * w).float()


def torch_valid_mask(v, index, up):
    """update_valid_depth_mask of the reference (depth_video.py:340-375) with droid_backends.depth_filter for the counts"""
    import droid_backends
    if index is None:
        index, = torch.where(v.dirty)
    src = v.disps_up if up else v.disps
    disps = torch.index_select(src, 0, index)
    intr = v.intrinsics[0] * (8.0 if up else 1.0)
    depths = 1.0 / disps
    thresh = REL * depths.mean(dim=[1, 2])
    count = droid_backends.depth_filter(v.poses, src, intr, index, thresh)
    depths[~(count >= VISIBLE)] = torch.nan
    med = depths.view(depths.shape[0], -1).nanmedian(dim=1).values
    masks = depths < 3 * med[:, None, None]
    (v.valid_depth_mask if up else v.valid_depth_mask_small)[index] = masks
    if up:
        v.dirty[index] = False


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


def pair(hip, ref, floor_bytes, reps):
    r = {"hip": event_times(hip, reps), "torch": event_times(ref, reps), "floor_bytes": floor_bytes}
    r["ratio_hip_over_torch"] = round(r["hip"]["ms_median"] / r["torch"]["ms_median"], 4)
    r["hip_gb_per_s_of_floor"] = round(floor_bytes / (r["hip"]["ms_median"] * 1e-3) / 1e9, 1)
    r["hip_not_slower"] = r["hip"]["ms_median"] <= r["torch"]["ms_median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_video_times.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "hbm_peak_gb_per_s": 8000, "upsample": {},
           "valid_depth_mask": {}}
    h, w = HT // 8, WD // 8
    v, rng = video(25, 32)
    for n in (1, 12, 25):
        ix = torch.arange(n, device=DEV)
        for dtype, name in ((torch.float16, "fp16"), (torch.float32, "fp32")):
            mask = (torch.rand(n, 576, h, w, device=DEV) * 8 - 4).to(dtype)
            floor = n * (576 * h * w * mask.element_size() + 64 * h * w * 4)
            v.upsample(ix, mask)
            got = v.disps_up[:n].clone()
            torch_upsample(v, ix, mask)
            err = float((got - v.disps_up[:n]).abs().max())
            r = pair(lambda: v.upsample(ix, mask), lambda: torch_upsample(v, ix, mask), floor, a.reps)
            r["max_abs_difference"] = err
            res["upsample"][f"{n}_frames_{name}"] = r
            print("upsample", n, name, r["hip"]["ms_median"], "ms vs torch", r["torch"]["ms_median"], "ms;", r["hip_gb_per_s_of_floor"],
                  "GB/s of the floor", flush=True)
    del v
    # the mask: floor = the threshold pass and the final pass read the disparities (4 B) once each, the final pass reads the counts (4 B)
    # and writes a byte; depth_filter's own traffic (the 6 neighbour gathers) is the same in both paths and not part of the floor
    for name, (n, buffer, up) in {"up_12_frames_480x640": (12, 16, True), "small_100_frames_60x80": (100, 104, False)}.items():
        v, rng = video(n, buffer)
        P = HT * WD if up else h * w

        def hip():
            if up:
                v.dirty[:n] = True
            v.update_valid_depth_mask(up=up)

        def ref():
            if up:
                v.dirty[:n] = True
            torch_valid_mask(v, None if up else torch.arange(n, device=DEV), up)

        hip()
        out = v.valid_depth_mask if up else v.valid_depth_mask_small
        got = out.clone()
        out.zero_()
        ref()
        r = pair(hip, ref, n * P * 13, a.reps)
        r["pixels_that_differ"] = int((got != out).sum())
        r["mask_share"] = round(float(got[:n].float().mean()), 4)
        res["valid_depth_mask"][name] = r
        print(name, r["hip"]["ms_median"], "ms vs torch", r["torch"]["ms_median"], "ms; differing pixels", r["pixels_that_differ"], flush=True)
        del v
    res["hip_not_slower_everywhere"] = all(r["hip_not_slower"] for g in ("upsample", "valid_depth_mask") for r in res[g].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"hip_not_slower_everywhere": res["hip_not_slower_everywhere"]}))


if __name__ == "__main__":
    main()
