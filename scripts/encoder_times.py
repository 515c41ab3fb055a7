"""GPU box: times of the encoders (splat_slam_amd.encoder, csrc/sgr_encoder.hip) and of one MotionFilter.track, whole and launch by launch,
next to the torch composition of the same weights (tests/encoder_ref.TorchEncoder: F.conv2d and F.instance_norm under torch.autocast, i.e.
the vendor libraries), at n = 1 and n = 8 images of 384 x 512 (48 x 64 at one eighth).  HIP-event medians after a warm-up, everything in
this one process.  A single launch is timed on the buffers a whole call has left in scratch.  The bytes of a launch are those its
algorithm must move (inputs read once, outputs written once, weights once), not a counter.  Writes one JSON file (rewritten after every
section, so a run that is cut short leaves what it measured).  No ratio is required of the result: it reports what it finds.

    timeout 900 python scripts/encoder_times.py [--out profiles/encoder_times.json] [--reps 20]"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
SEED = 7
H, W = 384, 512
PEAK_F16_TFLOPS = 2500.0         # MI355X dense fp16 matrix peak
PEAK_HBM_GB_S = 8000.0


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


def launch_work(which, n):
    """launch name -> (GFLOP, MB) from the shapes: a convolution reads its input map and weights once and writes its output once (fp32
    sums and statistics when normalised, else fp16); a norm launch reads the fp32 sums, the statistics and the residual and writes fp16"""
    from splat_slam_amd import encoder as E
    normed = E.NORM[which] == "instance"
    size = {0: (H, W)}
    for lvl in range(1, 4):
        size[lvl] = ((size[lvl - 1][0] - 1) // 2 + 1, (size[lvl - 1][1] - 1) // 2 + 1)
    level_of = {32: 1, 64: 2, 128: 3}
    work = {"pack": (0.0, n * H * W * (3 * 4 + 16) / 1e6)}
    for name, (cout, cin, k, stride) in E.ENCODER_LAYERS.items():
        cout = E.OUT_DIM[which] if cout is None else cout
        lvl_out = 3 if name == "conv2" else level_of[cout]
        lvl_in = lvl_out - (stride == 2)
        px_in, px_out = n * size[lvl_in][0] * size[lvl_in][1], n * size[lvl_out][0] * size[lvl_out][1]
        cin_pad = max(cin, 8)
        gflop = 2.0 * px_out * cout * cin * k * k / 1e9
        is_normed = normed and name != "conv2"
        tail = name.endswith("conv2") and name != "conv2"
        nbytes = px_in * cin_pad * 2 + cout * cin_pad * k * k * 2 + px_out * cout * (4 if is_normed else 2)
        if is_normed:
            stats = n * ((px_out // n + 127) // 128) * cout * 16
            work[name] = (gflop, (nbytes + stats) / 1e6)
            work[name + ":norm"] = (0.0, (px_out * cout * (4 + 2 + (2 if tail else 0)) + stats) / 1e6)
        else:
            work[name] = (gflop, (nbytes + (px_out * cout * 2 if tail else 0)) / 1e6)
    return work


def time_encoder(enc, torch_enc, which, n, reps, save, out):
    from splat_slam_amd import encoder as E
    import encoder_ref as R
    x = R.make_images(1, n, H, W, seed=n, device=DEV, dtype=torch.float32)
    r = {"n": n, "H": H, "W": W, "hip": event_times(lambda: enc(x), reps)}
    out[f"{which}_n{n}"] = r
    print(which, n, "hip", r["hip"]["ms_median"], "ms", flush=True)
    call, outs = enc._prepare(x, None, None, False)
    enc._run(call)
    work, launches = launch_work(which, n), {}
    for i, lname in enumerate(E.LAUNCH_NAMES[which]):
        call.first_launch = call.last_launch = i
        t = event_times(lambda: enc._run(call), reps)
        gflop, mb = work[lname]
        t["gflop"], t["mbytes"] = round(gflop, 4), round(mb, 3)
        t["tflops"], t["gb_per_s"] = round(gflop / t["ms_median"], 2), round(mb / t["ms_median"], 1)
        t["fraction_of_bound"] = round(max(gflop / PEAK_F16_TFLOPS, mb / PEAK_HBM_GB_S) / t["ms_median"], 4)
        launches[lname] = t
    r["launches"] = launches
    r["gflop"] = round(sum(g for g, _ in work.values()), 3)
    r["mbytes"] = round(sum(m for _, m in work.values()), 2)
    r["sum_of_launches_ms"] = round(sum(t["ms_median"] for t in launches.values()), 4)
    save()
    r["torch"] = event_times(lambda: torch_enc(x), reps)
    r["ratio_hip_over_torch"] = round(r["hip"]["ms_median"] / r["torch"]["ms_median"], 4)
    r["hip_not_slower"] = r["hip"]["ms_median"] <= r["torch"]["ms_median"]
    slow = sorted(launches, key=lambda k: -launches[k]["ms_median"])[:4]
    r["slowest_launches"] = {k: launches[k]["ms_median"] for k in slow}
    print(which, n, "torch", r["torch"]["ms_median"], "ms; ratio", r["ratio_hip_over_torch"], flush=True)
    save()
    del x, call, outs
    torch.cuda.empty_cache()


class TorchNet:
    """the torch composition behind the interface MotionFilter takes: encoders with fused-normalisation arguments, and the update"""

    def __init__(self, fnet, cnet, update):
        self.fnet, self.cnet, self.update = fnet, cnet, update


def time_track(net, torch_net, reps, out):
    """one MotionFilter.track on a later frame that is dropped (fnet, CorrBlock, one update step, the decision read), and one that is
    appended (the context encoder on top): the threshold decides, the video buffer of 2 never fills"""
    from splat_slam_amd.depth_video import DepthVideo
    from splat_slam_amd.motion_filter import MotionFilter
    g = torch.Generator().manual_seed(1)
    a, b = torch.rand(1, 3, H, W, generator=g).to(DEV), torch.rand(1, 3, H, W, generator=g).to(DEV)
    intr = torch.tensor([500.0, 500.0, 256.0, 192.0], device=DEV)
    for label, model in (("hip", net), ("torch", torch_net)):
        for kind, thresh in (("dropped", 1e9), ("appended", -1.0)):
            video = DepthVideo(H, W, buffer=2, device=DEV)
            filt = MotionFilter(model, video, thresh=thresh, device=DEV)
            filt.track(0.0, a, intr)

            def step():
                video.counter.value = 1
                filt.track(1.0, b, intr)
            out.setdefault("track_" + kind, {})[label] = event_times(step, reps)
            print("track", kind, label, out["track_" + kind][label]["ms_median"], "ms", flush=True)
    for kind in ("dropped", "appended"):
        t = out["track_" + kind]
        t["ratio_hip_over_torch"] = round(t["hip"]["ms_median"] / t["torch"]["ms_median"], 4)


def main():
    import encoder_ref as R
    import update_ref
    from splat_slam_amd import encoder as E
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd import update_op as U
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_times.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "peak_f16_tflops": PEAK_F16_TFLOPS,
           "peak_hbm_gb_per_s": PEAK_HBM_GB_S, "times": {}}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    net = DroidNet.synthetic(SEED, DEV)
    torch_encs = {w: R.TorchEncoder(E.synthetic_encoder_state_dict(w, SEED), E.NORM[w], DEV) for w in ("fnet", "cnet")}
    for which in ("fnet", "cnet"):
        for n in (1, 8):
            time_encoder(getattr(net, which), torch_encs[which], which, n, a.reps, save, res["times"])
    torch_net = TorchNet(torch_encs["fnet"], torch_encs["cnet"], update_ref.TorchUpdate(U.synthetic_state_dict(SEED), DEV))
    time_track(net, torch_net, a.reps, res["times"])
    save()
    print(json.dumps({k: v.get("ratio_hip_over_torch") for k, v in res["times"].items()}))


if __name__ == "__main__":
    main()
