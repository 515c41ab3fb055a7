"""GPU box: times of LPIPS (splat_slam_amd.lpips, csrc/sgr_lpips.hip) next to the torch composition of the same weights on the same card
(tests/lpips_ref.lpips_torch restated with the weights held in fp16: F.conv2d / F.max_pool2d in fp16, i.e. the vendor library, the
distance in fp32), at 480 x 640 for n = 1 and n = 16 pairs: the whole metric, and the 14 launches of sgr_lpips_forward one by one on the
two scratch buffers as a whole call has left them (the maps alternate between them, so a launch repeated alone reads what the last
launches wrote there: the same shapes and work, other values), each next to the torch step that does the same work.  HIP events
around `inner` repeats of the timed work, medians over `reps` windows after a warm-up, the two sides alternating window by window in
this one process; the spread of a figure is the distance between the quartiles of its windows.  Bytes (every map read once and
written once, the packed weights once), operations (the products the definition needs: conv1 counts 3 channels, not the 8 it is
padded to) and workgroups come from the shapes.  A launch timed alone does not go below the 8-9 us of its enqueue and repeats on
cache-warm buffers: the share of the bound stored for the pack, the pools and the distances is not a share of the HBM peak.  No
threshold is attached to any of this.  Writes one JSON file (rewritten after every section).

    timeout 600 python scripts/lpips_times.py [--out profiles/lpips_times.json] [--reps 15] [--inner 50]"""
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
SEED = 3
PEAK_F16_TFLOPS = 2500.0         # MI355X dense fp16 matrix peak
PEAK_HBM_TBS = 8.0               # MI355X HBM3E peak bandwidth (spec)


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def summary(times):
    return {"ms_median": round(float(np.median(times)), 5), "ms_min": round(float(np.min(times)), 5), "ms_max": round(float(np.max(times)), 5),
            "spread_ms": round(float(np.percentile(times, 75) - np.percentile(times, 25)), 5), "windows": len(times)}


def two_variants(torch_fn, hip_fn, reps, inner):
    """warm both, then torch, hip, torch, hip, ...: a drift of the card's clock falls on both sides alike"""
    torch_fn(), hip_fn(), torch_fn(), hip_fn()
    tt, th = [], []
    for _ in range(reps):
        tt.append(window(torch_fn, inner))
        th.append(window(hip_fn, inner))
    r = {"torch": summary(tt), "hip": summary(th)}
    r["ratio_hip_over_torch"] = round(r["hip"]["ms_median"] / r["torch"]["ms_median"], 4)
    r["differ_beyond_the_spread"] = abs(r["torch"]["ms_median"] - r["hip"]["ms_median"]) > max(r["torch"]["spread_ms"], r["hip"]["spread_ms"])
    return r


def launch_model(n, H, W):
    """launch name -> (bytes, GFLOP, workgroups) of sgr_lpips_forward from the shapes alone"""
    from splat_slam_amd.lpips import CONV_SHAPES, LAUNCH_NAMES, tap_sizes
    sizes, m, out = tap_sizes(H, W), 2 * n, {}
    out["pack"] = (m * H * W * (3 * 4 + 8 * 2), 0.0, m * -(-H * W // 256))
    h, w, cin_pad = H, W, 8
    for i, ((cout, cin, k, _, _), (ho, wo)) in enumerate(zip(CONV_SHAPES, sizes)):
        k_pad = -(-k * k * cin_pad // 32) * 32
        out[f"conv{i + 1}"] = (m * h * w * cin_pad * 2 + cout * k_pad * 2 + m * ho * wo * cout * 2, 2.0 * m * ho * wo * cout * k * k * cin / 1e9,
                               -(-m * ho * wo // 128) * (cout // 64))
        blocks = -(-ho * wo // 128)
        out[f"distance{i + 1}"] = (m * ho * wo * cout * 2 + n * blocks * 4, 6.0 * m * ho * wo * cout / 1e9, n * blocks)
        h, w, cin_pad = ho, wo, cout
        if i < 2:
            h, w = (ho - 3) // 2 + 1, (wo - 3) // 2 + 1
            out[f"pool{i + 1}"] = (m * ho * wo * cout * 2 + m * h * w * cout * 2, 0.0, -(-m * h * w * (cout // 8) // 256))
    out["final"] = (n * sum(-(-a * b // 128) for a, b in sizes) * 4 + n * 24, 0.0, n)
    ordered = {k: out[k] for k in LAUNCH_NAMES}
    assert len(ordered) == len(out)
    return ordered


def torch_steps(P, x0, x1):
    """the torch composition step by step, weights held in fp16: (whole, {launch name: step on the inputs a whole call produced})"""
    import lpips_ref as LR
    w16 = [(P[f"conv{i + 1}.weight"].to(torch.float16), P[f"conv{i + 1}.bias"].to(torch.float16)) for i in range(5)]
    lin = [P[f"lin{i}"].float() for i in range(5)]
    shift, scale = P["shift"].float().reshape(1, 3, 1, 1), P["scale"].float().reshape(1, 3, 1, 1)
    n = x0.shape[0]

    def pack():
        return ((2.0 * torch.cat([x0, x1]) - 1.0 - shift) / scale).to(torch.float16)

    def conv(i, x):
        return torch.relu(F.conv2d(x, w16[i][0], w16[i][1], stride=LR.GEOMETRY[i][0], padding=LR.GEOMETRY[i][1]))

    def dist(i, f):
        a, b = f[:n].float(), f[n:].float()
        u, v = a / torch.sqrt(LR.EPS + (a * a).sum(1, keepdim=True)), b / torch.sqrt(LR.EPS + (b * b).sum(1, keepdim=True))
        return F.conv2d((u - v) ** 2, lin[i]).flatten(1).mean(1)

    def whole():
        x, lv = pack(), []
        for i in range(5):
            x = conv(i, x)
            lv.append(dist(i, x))
            if i < 2:
                x = F.max_pool2d(x, 3, 2)
        return torch.stack(lv, 1).sum(1)

    steps, x, lv = {"pack": pack}, pack(), []
    for i in range(5):
        steps[f"conv{i + 1}"] = (lambda i=i, x=x: conv(i, x))
        x = conv(i, x)
        steps[f"distance{i + 1}"] = (lambda i=i, x=x: dist(i, x))
        lv.append(dist(i, x))
        if i < 2:
            steps[f"pool{i + 1}"] = (lambda x=x: F.max_pool2d(x, 3, 2))
            x = F.max_pool2d(x, 3, 2)
    steps["final"] = lambda: torch.stack(lv, 1).sum(1)
    return whole, steps


def main():
    from splat_slam_amd import _native as nat
    from splat_slam_amd.lpips import LAUNCH_NAMES, LPIPS, normalize_state_dict, prepare, synthetic_state_dict
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_times.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--pairs", type=int, nargs="+", default=(1, 16))
    a = ap.parse_args()
    H, W = a.size
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "image": [H, W], "peak_f16_tflops": PEAK_F16_TFLOPS,
           "peak_hbm_tbs": PEAK_HBM_TBS, "windows": a.reps, "repeats_per_window": a.inner}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    canon = normalize_state_dict(synthetic_state_dict(SEED))
    net, P = LPIPS(canon, DEV), {k: v.to(DEV) for k, v in prepare(canon).items()}
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for n in a.pairs:
            g = torch.Generator().manual_seed(n)
            x0 = torch.rand(n, 3, H, W, generator=g).to(DEV)
            x1 = (x0 + 0.05 * torch.randn(n, 3, H, W, generator=g).to(DEV)).clamp(0, 1)
            whole, steps = torch_steps(P, x0, x1)
            out, levels = torch.empty(n, device=DEV), torch.empty((n, 5), device=DEV)
            call = net._call(n, H, W, out, levels)
            call.img0, call.img1, call.normalize = x0.data_ptr(), x1.data_ptr(), 1
            r = {"pairs": n}
            r["whole"] = two_variants(whole, lambda: net._run(call), a.reps, a.inner)
            net._run(call)
            r["max_abs_difference_hip_torch"] = float((out - whole()).abs().max())
            r["lpips_mean"] = float(out.mean())
            res[f"n{n}"] = r
            save()
            print(f"n={n} whole: torch", r["whole"]["torch"]["ms_median"], "hip", r["whole"]["hip"]["ms_median"], "ms", flush=True)
            model_of, launches = launch_model(n, H, W), {}
            for i, name in enumerate(LAUNCH_NAMES):
                one = net._call(n, H, W, out, levels)
                one.img0, one.img1, one.normalize = x0.data_ptr(), x1.data_ptr(), 1
                one.first_launch = one.last_launch = i
                t = two_variants(steps[name], lambda: net._run(one), a.reps, a.inner)
                nbytes, gflop, groups = model_of[name]
                t_bytes, t_flop = nbytes / (PEAK_HBM_TBS * 1e12) * 1e3, gflop / PEAK_F16_TFLOPS
                t.update({"mbytes": round(nbytes / 1e6, 3), "gflop": round(gflop, 4), "workgroups": groups,
                          "bound": "bytes" if t_bytes >= t_flop else "mfma", "ms_at_the_bound": round(max(t_bytes, t_flop), 5),
                          "hip_share_of_the_bound": round(max(t_bytes, t_flop) / t["hip"]["ms_median"], 4)})
                launches[name] = t
            r["launches"] = launches
            r["hip_sum_of_launches_ms"] = round(sum(t["hip"]["ms_median"] for t in launches.values()), 4)
            r["torch_sum_of_steps_ms"] = round(sum(t["torch"]["ms_median"] for t in launches.values()), 4)
            r["gflop"], r["mbytes"] = round(sum(v[1] for v in model_of.values()), 3), round(sum(v[0] for v in model_of.values()) / 1e6, 1)
            r["scratch_mbytes"] = round(nat.lib().sgr_lpips_scratch_bytes(n, H, W) / 1e6, 1)
            save()
            print(f"n={n} launches (hip ms):", {k: v["hip"]["ms_median"] for k, v in launches.items()}, flush=True)
            del whole, steps, x0, x1
            torch.cuda.empty_cache()
    print(json.dumps({k: v["whole"] for k, v in res.items() if isinstance(v, dict) and "whole" in v}))


if __name__ == "__main__":
    main()
