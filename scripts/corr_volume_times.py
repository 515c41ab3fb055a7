"""GPU box: times of the frontend's correlation operator, corr.FusedCorrBlock (sgr_corr_volume_pyramid into slots, one
sgr_corr_index_pyramid_forward launch per lookup) next to corr.CorrBlock under autocast (torch.matmul, three avg_pool2d, four
corr_index_forward launches and a concatenation; torch.cat / mask indexing of every stored volume when an edge comes or goes), in the
same process on the same maps: 48 x 64 maps of 128 channels in fp16, radius 3, 4 levels.  Cases: building 1, 8 and 32 edges (the
torch side's gathers included), the lookup at 60 and 75 edges, adding 4 edges to 71, dropping 4 of 75, and one FactorGraph.update
with each corr_impl under a stub operator, after which the largest difference of the two graphs' targets is reported (no threshold:
the two operators round differently, DESIGN.md section 3, "Fused correlation volume").  HIP-event medians after one warm-up.
GB/s are over the floor of a case: the bytes of the volumes written (25.07 MB per edge) for a build or an add, the lookup's output
and coordinates for a lookup.  Writes one JSON file.

    python scripts/corr_volume_times.py [--out profiles/corr_volume_times.json] [--reps 20]"""
import argparse
import copy
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
H, W, CH, R, LEVELS, FRAMES = 48, 64, 128, 3, 4, 16
EDGE_BYTES = sum(H * W * (H >> l) * (W >> l) * 2 for l in range(LEVELS))


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


def pair(hip, ref, reps, floor_bytes=None):
    r = {"fused": event_times(hip, reps), "corr_block": event_times(ref, reps)}
    r["ratio_hip_over_baseline"] = round(r["fused"]["ms_median"] / r["corr_block"]["ms_median"], 4)
    r["hip_not_slower"] = r["fused"]["ms_median"] <= r["corr_block"]["ms_median"]
    if floor_bytes is not None:
        r["floor_bytes"] = int(floor_bytes)
        for k in ("fused", "corr_block"):
            r[k]["GBps_over_floor"] = round(floor_bytes / (r[k]["ms_median"] * 1e-3) / 1e9, 1)
    return r


def edges(rng, n):
    ii = rng.integers(0, FRAMES, n)
    jj = (ii + rng.integers(1, FRAMES, n)) % FRAMES
    return torch.tensor(ii, device=DEV), torch.tensor(jj, device=DEV)


def corr_block(fmaps, ii, jj):
    from splat_slam_amd.corr import CorrBlock
    with torch.autocast("cuda", enabled=True):
        return CorrBlock(fmaps[ii, 0].unsqueeze(0), fmaps[jj, 0].unsqueeze(0), LEVELS, R)


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


_STUB = {}


def stub(net, inp, corr, motn, ii, jj):
    """a deterministic stand-in for the update operator whose flow correction depends on two correlation channels; its random
    damping and mask are drawn once per shape and kept on the device, so that a call costs next to nothing"""
    E, h, w = motn.shape[1], motn.shape[3], motn.shape[4]
    K = torch.unique(ii).shape[0]
    if (E, K) not in _STUB:
        g = torch.Generator(device="cpu").manual_seed(1234 + E)
        _STUB[E, K] = ((0.01 * torch.rand((1, K, h, w), generator=g)).to(motn.device),
                       (4.0 * torch.rand((1, K, 576, h, w), generator=g) - 2.0).to(motn.device))
    damping, upmask = _STUB[E, K]
    delta = (0.1 * motn[:, :, :2]).permute(0, 1, 3, 4, 2) + 0.01 * torch.tanh(corr[:, :, [24, 2 * 49 + 24]].float()).permute(0, 1, 3, 4, 2)
    weight = torch.full((1, E, h, w, 2), 0.5, device=motn.device)
    return net, delta.contiguous(), weight, damping, upmask


def graph_case(rng, reps):
    from splat_slam_amd.factor_graph import FactorGraph
    video = make_video(rng)
    state = {k: getattr(video, k).clone() for k in ("poses", "disps", "disps_up", "dirty", "npc_dirty")}
    graphs, saved = {}, {}
    for impl in ("volume_fused", "volume"):
        g = FactorGraph(video, stub, device=DEV, corr_impl=impl, max_factors=75)
        g.add_neighborhood_factors(0, 12, r=3)
        graphs[impl] = g
        saved[impl] = {k: getattr(g, k).clone() for k in ("target", "weight", "age", "net", "damping")}

    def update(impl):
        for k, t in state.items():
            getattr(video, k).copy_(t)
        g = graphs[impl]
        for k, t in saved[impl].items():
            setattr(g, k, t.clone())
        g.update(t0=1)

    r = pair(lambda: update("volume_fused"), lambda: update("volume"), reps)
    r["edges"] = int(graphs["volume"].ii.shape[0])
    r["max_abs_target_difference"] = float((graphs["volume_fused"].target - graphs["volume"].target).abs().max())
    return r


def main():
    from splat_slam_amd.corr import FusedCorrBlock
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_volume_times.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "shape": {"h": H, "w": W, "channels": CH, "radius": R, "levels": LEVELS, "maps": "fp16"}, "edge_bytes": EDGE_BYTES, "cases": {}}
    rng = np.random.default_rng(0)
    fmaps = torch.tensor(rng.normal(0, 1, (FRAMES, 1, CH, H, W)), dtype=torch.float32).half().to(DEV)
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    block = FusedCorrBlock(fmaps, LEVELS, R, capacity=80)

    def say(name):
        r = res["cases"][name]
        print(name, "fused", r["fused"]["ms_median"], "ms, CorrBlock", r["corr_block"]["ms_median"], "ms", flush=True)

    for n in (1, 8, 32):
        ii, jj = edges(rng, n)

        def hip():
            block.slots = none
            block.add(ii, jj)
        res["cases"][f"build_{n}_edges"] = pair(hip, lambda: corr_block(fmaps, ii, jj), a.reps, n * EDGE_BYTES)
        say(f"build_{n}_edges")
    ii, jj = edges(rng, 75)
    block.slots = none
    block.add(ii, jj)
    slots75 = block.slots
    ref75 = corr_block(fmaps, ii, jj)
    grid = torch.stack(torch.meshgrid(torch.arange(W, device=DEV).float(), torch.arange(H, device=DEV).float(), indexing="xy"), -1)
    coords = (grid[None] + torch.tensor(rng.normal(0, 3.0, (75, H, W, 2)), dtype=torch.float32, device=DEV))[None].contiguous()
    for n in (60, 75):
        block.slots = slots75[:n]
        ref = copy.copy(ref75)[torch.arange(n, device=DEV)]

        def base():
            with torch.autocast("cuda", enabled=True):
                return ref(coords[:, :n])
        out_bytes = n * H * W * (LEVELS * (2 * R + 1) ** 2 * 2 + 8)
        res["cases"][f"lookup_{n}_edges"] = pair(lambda: block(coords[:, :n]), base, a.reps, out_bytes)
        res["cases"][f"lookup_{n}_edges"]["max_abs_difference"] = float((block(coords[:, :n]).float() - base().float()).abs().max())
        say(f"lookup_{n}_edges")
    ref71 = copy.copy(ref75)[torch.arange(71, device=DEV)]

    def hip_add():
        block.slots = slots75[:71]
        block.add(ii[71:], jj[71:])
    res["cases"]["add_4_to_71"] = pair(hip_add, lambda: copy.copy(ref71).cat(corr_block(fmaps, ii[71:], jj[71:])), a.reps, 4 * EDGE_BYTES)
    say("add_4_to_71")
    keep = torch.ones(75, dtype=torch.bool, device=DEV)
    keep[[3, 20, 41, 74]] = False

    def hip_drop():
        block.slots = slots75
        block[keep, 71]
    res["cases"]["drop_4_of_75"] = pair(hip_drop, lambda: copy.copy(ref75)[keep], a.reps)
    say("drop_4_of_75")
    del ref, ref71, ref75
    torch.cuda.empty_cache()
    res["cases"]["graph_update"] = graph_case(rng, a.reps)
    say("graph_update")
    res["hip_not_slower_everywhere"] = all(c["hip_not_slower"] for c in res["cases"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"hip_not_slower_everywhere": res["hip_not_slower_everywhere"],
                      "max_abs_target_difference": res["cases"]["graph_update"]["max_abs_target_difference"]}))


if __name__ == "__main__":
    main()
