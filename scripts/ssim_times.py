"""GPU box: HIP-event times of the SSIM kernels and of the rendering evaluation, one line of JSON per case.

  ssim:  losses.ssim_native forward + backward (sgr_ssim + sgr_ssim_backward) against losses.ssim forward + backward (torch:
         five grouped 11x11 convolutions through MIOpen, their backward and the elementwise chain) at [3,480,640] and
         [12,3,480,640], fp32, upstream 0.37.
  eval:  eval.eval_rendering (renders + sgr_render_metrics, one host copy) against eval_rendering_psnr plus a torch SSIM per
         frame (the reference's evaluation loop without LPIPS) over 40 frames at 640x480.

    python scripts/ssim_times.py [--reps 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def timed(fn, reps, warmup=5):
    """median and minimum milliseconds of `fn` between two HIP events, each rep synchronised"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return round(times[len(times) // 2], 4), round(times[0], 4)


def ssim_case(shape, reps):
    from splat_slam_amd.losses import ssim, ssim_native
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.rand(shape, generator=g, device=DEV)
    y = (0.7 * x + 0.3 * torch.rand(shape, generator=g, device=DEV)).clamp(0, 1)
    xr = x.clone().requires_grad_(True)

    def run(f):
        def step():
            xr.grad = None
            (f(xr, y) * 0.37).backward()
        return step

    nat_fwd = timed(lambda: ssim_native(x, y), reps)
    tch_fwd = timed(lambda: ssim(x, y), reps)
    nat = timed(run(ssim_native), reps)
    tch = timed(run(ssim), reps)
    return {"case": "ssim", "shape": list(shape), "hip_fwd_ms": nat_fwd, "torch_fwd_ms": tch_fwd, "hip_fwd_bwd_ms": nat,
            "torch_fwd_bwd_ms": tch, "speedup_fwd_bwd_median": round(tch[0] / nat[0], 2)}


def eval_case(frames, reps):
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.eval import eval_rendering, eval_rendering_psnr
    from splat_slam_amd.losses import ssim
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.renderer import render
    intr = syn.INTRINSICS["metric"]
    params = syn.room_parameters(60000, seed=43, device=DEV)
    cams = syn.make_views(params, frames, intr, DEV, seed=43)
    gm = syn.model_from_parameters(params, device=DEV)
    bg = torch.zeros(3, device=DEV)
    pipe = PipelineParams()
    with torch.no_grad():
        for k, c in enumerate(cams[1:], 1):
            c.exposure_a.fill_(0.01 * (k % 3))

    def torch_eval():
        scores = eval_rendering_psnr(cams, gm, pipe, bg)
        with torch.no_grad():
            s = []
            for k, f in enumerate(cams):
                r = render(f, gm, pipe, bg)["render"]
                img = torch.clamp(torch.exp(f.exposure_a) * r + f.exposure_b if k > 0 else r, 0.0, 1.0)
                s.append(ssim(img[None], f.original_image[None]).item())
        return scores, s

    def renders_only():
        with torch.no_grad():
            for f in cams:
                render(f, gm, pipe, bg)

    return {"case": "eval", "frames": frames, "H": intr["H"], "W": intr["W"],
            "eval_rendering_ms": timed(lambda: eval_rendering(cams, gm, pipe, bg), reps, warmup=2),
            "psnr_plus_torch_ssim_ms": timed(torch_eval, reps, warmup=2),
            "renders_only_ms": timed(renders_only, reps, warmup=2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--eval-reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ssim_times.py needs a GPU"
    for shape in [(3, 480, 640), (12, 3, 480, 640)]:
        print(json.dumps(ssim_case(shape, args.reps)), flush=True)
    print(json.dumps(eval_case(40, args.eval_reps)), flush=True)


if __name__ == "__main__":
    main()
