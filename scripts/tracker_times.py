"""GPU box: times of the backend's correlation lookup, corr.FusedAltCorrBlock (one sgr_corr_alt_pyramid_forward launch) next to
corr.AltCorrBlock (per level two gathered fp32 copies and one altcorr_forward launch, then a permute and a concatenation), in the same
process on the same inputs: one chunk of FactorGraph.update_lowmem (40 edges of 8 source frames) and 80 edges, both at 48 x 64 maps of
128 channels in fp16, radius 3, 4 levels.  Both sides are checked against each other: they may differ by twice the lookup's bound
(C + 8) * 2^-24 * magnitude (tests/test_gpu_alt_pyramid.py, 4), the magnitude summed here in fp64 on the device.  Separately one
Backend.dense_ba(2) over 12 keyframes with the synthetic network under both corr_impl values.  HIP-event medians after one warm-up.
Writes one JSON file.

    python scripts/tracker_times.py [--out profiles/tracker_times.json] [--reps 20]"""
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
H, W, CH, R, LEVELS = 48, 64, 128, 3, 4


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


def pair(hip, ref, reps, names=("hip", "baseline")):
    r = {names[0]: event_times(hip, reps), names[1]: event_times(ref, reps)}
    r["ratio_hip_over_baseline"] = round(r[names[0]]["ms_median"] / r[names[1]]["ms_median"], 4)
    r["hip_not_slower"] = r[names[0]]["ms_median"] <= r[names[1]]["ms_median"]
    return r


def magnitude(pyramid, ii, jj, coords, r):
    """[E, levels*rd*rd, H, W] fp64: per output the sum over its four corners of sum_c |fmap1| |fmap2| (corr_ref's magnitude)"""
    rd, rc = 2 * r + 1, 2 * r + 2
    f1 = pyramid[0][0][ii].double().abs().reshape(ii.shape[0], H * W, -1)
    out = []
    for lvl, maps in enumerate(pyramid):
        Hl, Wl = maps.shape[2:4]
        at = (coords / 2 ** lvl).reshape(ii.shape[0], H * W, 2)
        fx, fy = torch.floor(at[..., 0]), torch.floor(at[..., 1])
        live = (fx >= -(r + 2)) & (fx <= Wl + r + 1) & (fy >= -(r + 2)) & (fy <= Hl + r + 1)
        fx, fy = torch.where(live, fx, 0).long(), torch.where(live, fy, 0).long()
        f2 = maps[0][jj].double().abs().reshape(ii.shape[0], Hl * Wl, -1)
        adot = torch.zeros(rc, rc, ii.shape[0], H * W, dtype=torch.float64, device=DEV)
        for ix in range(rc):
            for iy in range(rc):
                x2, y2 = fx - r + ix, fy - r + iy
                inb = live & (x2 >= 0) & (x2 < Wl) & (y2 >= 0) & (y2 < Hl)
                rows = torch.where(inb, y2 * Wl + x2, 0)
                dot = (f1 * torch.gather(f2, 1, rows[..., None].expand(-1, -1, f2.shape[-1]))).sum(-1)
                adot[ix, iy] = torch.where(inb, dot, 0.0)
        mag = adot[:-1, :-1] + adot[1:, :-1] + adot[:-1, 1:] + adot[1:, 1:]             # [ax, ay, E, HW]
        out.append(mag.permute(2, 0, 1, 3).reshape(ii.shape[0], rd * rd, H, W))
    return torch.cat(out, 1)


def lookup_case(rng, frames, ii, jj, reps):
    from splat_slam_amd.corr import AltCorrBlock, FusedAltCorrBlock
    fmaps = torch.tensor(rng.normal(0, 1, (1, frames, CH, H, W)), dtype=torch.float32).half().to(DEV)
    ii, jj = torch.tensor(ii, device=DEV), torch.tensor(jj, device=DEV)
    grid = torch.stack(torch.meshgrid(torch.arange(W, device=DEV).float(), torch.arange(H, device=DEV).float(), indexing="xy"), -1)
    coords = (grid[None] + torch.tensor(rng.normal(0, 3.0, (ii.shape[0], H, W, 2)), dtype=torch.float32, device=DEV))[None].contiguous()
    fused, alt = FusedAltCorrBlock(fmaps, LEVELS, R), AltCorrBlock(fmaps, LEVELS, R)
    got, want = fused(coords, ii, jj), alt(coords, ii, jj)
    allowed = 2.0 * (CH + 8) * 2.0 ** -24 * magnitude(fused.pyramid, ii, jj, coords[0], R)
    diff = (got[0].double() - want[0].double()).abs()
    r = pair(lambda: fused(coords, ii, jj), lambda: alt(coords, ii, jj), reps, ("fused", "alt_corr_block"))
    r["edges"], r["source_frames"] = int(ii.shape[0]), int(torch.unique(ii).shape[0])
    r["max_abs_difference"] = float(diff.max())
    r["max_difference_over_allowance"] = float((diff / allowed.clamp(min=1e-300)).max())
    r["agree"] = bool((diff <= allowed).all())
    return r


def make_video(rng):
    """twelve keyframes on a smooth path in front of a gently varying surface, with random feature and context maps"""
    from splat_slam_amd.depth_video import DepthVideo
    v = DepthVideo(8 * H, 8 * W, buffer=16, device=DEV)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)
    for f in range(12):
        ang = 0.01 * f
        pose = [0.03 * f, 0.01 * np.sin(f), 0.015 * f, 0.0, np.sin(ang / 2), 0.0, np.cos(ang / 2)]
        disp = 0.5 + 0.05 * np.sin(0.09 * xx + 0.3 * f) * np.cos(0.06 * yy) + rng.uniform(-0.005, 0.005, (H, W))
        v.append(float(f), torch.zeros(3, 8 * H, 8 * W, dtype=torch.uint8, device=DEV), f32(pose), f32(disp), None,
                 f32([56.0, 60.0, 32.0, 24.0]))
    v.mono_disps[:12] = 1.7 * v.disps[:12] + 0.05
    for buf in (v.fmaps[:12, 0], v.nets[:12], v.inps[:12]):
        buf.copy_(torch.tensor(rng.normal(0, 1, (12, 128, H, W)), dtype=torch.float32))
    return v


def main():
    from splat_slam_amd.backend import Backend
    from splat_slam_amd.droid_net import DroidNet
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracker_times.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "shape": {"h": H, "w": W, "channels": CH, "radius": R, "levels": LEVELS, "maps": "fp16"}, "lookup": {}, "dense_ba": {}}
    rng = np.random.default_rng(0)
    ii = np.repeat(np.arange(8), 5)
    res["lookup"]["chunk_40_edges_8_sources"] = lookup_case(rng, 16, ii, (ii + np.tile([1, 2, 3, 4, 5], 8)) % 16, a.reps)
    ii = np.repeat(np.arange(16), 5)
    res["lookup"]["80_edges"] = lookup_case(rng, 16, ii, (ii + np.tile([1, 2, 3, 4, 5], 16)) % 16, a.reps)
    for name, r in res["lookup"].items():
        print(name, "fused", r["fused"]["ms_median"], "ms, AltCorrBlock", r["alt_corr_block"]["ms_median"], "ms; agree", r["agree"],
              flush=True)
    video = make_video(rng)
    state = {k: getattr(video, k).clone() for k in ("poses", "disps", "disps_up", "dirty", "npc_dirty")}
    cfg = {"device": DEV, "tracking": {"beta": 0.75, "backend": {"thresh": 22.0, "radius": 2, "nms": 3, "normalize": True, "loop_window": 25,
                                                                 "loop_thresh": 25.0, "loop_radius": 1, "loop_nms": 12}}}
    net = DroidNet.synthetic(7, device=DEV)
    edges = {}

    def dense(impl):
        for k, t in state.items():
            getattr(video, k).copy_(t)
        edges[impl] = Backend(net, video, cfg, corr_impl=impl).dense_ba(2)[1]

    r = pair(lambda: dense("alt_fused"), lambda: dense("alt"), a.reps, ("alt_fused", "alt"))
    r["frames"], r["edges"] = 12, edges
    res["dense_ba"]["12_frames_2_steps"] = r
    print("dense_ba(2), 12 frames:", r["alt_fused"]["ms_median"], "ms fused,", r["alt"]["ms_median"], "ms alt;", edges, "edges", flush=True)
    cases = list(res["lookup"].values()) + list(res["dense_ba"].values())
    res["hip_not_slower_everywhere"] = all(c["hip_not_slower"] for c in cases)
    res["lookups_agree_everywhere"] = all(c["agree"] for c in res["lookup"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"hip_not_slower_everywhere": res["hip_not_slower_everywhere"],
                      "lookups_agree_everywhere": res["lookups_agree_everywhere"]}))


if __name__ == "__main__":
    main()
