"""A whole run from a config file (the reference's run.py and SLAM.__init__ / terminate, in their order; DESIGN.md section 3, "Run"):

    python -m splat_slam_amd.run CONFIG [--default PATH] [--root DIR] [--lpips-weights PATH] [--novel_views N]

    run(cfg, net=None, mono_depth=None, lpips=None, stream=None, novel_views=None) -> dict       what main calls; the result of Slam.evaluate with
        "output_dir", "psnr" (terminate()'s list) and "num_gaussians" (the rows of the written map) added.  Objects that are not given are
        built from the config: the stream by datasets.get_dataset(cfg), net by load_droid_net(cfg["tracking"]["pretrained"]), mono_depth
        by load_mono_depth(cfg["mono_prior"]["depth_pretrained"]).
    load_droid_net(path, device="cuda")                     torch.load on the CPU, then DroidNet.from_state_dict, which strips "module." and
                                                            cuts the three-row update.weight.2 / update.delta.2 to two rows (slam.py:79-82)
    load_mono_depth(path, cfg=MonoDepthConfig(), device="cuda")     MonoDepth.from_state_dict(sd, backbone="hip", decoder="hip"), which
                                                            unwraps {"state_dict": {"model.*"}} as src/mono_estimators.py does
    setup_seed(seed)                                        torch, numpy and random

The output tree under cfg["data"]["output"]/cfg["scene"]: cfg.yaml, video.npz, metrics_kf_traj.txt, metrics_full_traj.txt, kf_traj.png,
full_traj.png, plots_after_refine/ (one PNG per mapped keyframe and output.gif), mesh.ply with meshing.mesh,
psnr/after_refine/final_result.json (mean_psnr, mean_ssim, mean_depthl1 and, with LPIPS weights, mean_lpips), depth_stats.txt (the
reference's nine labels, slam.py:220-235) and point_cloud/final/point_cloud.ply.  With --novel_views N also
psnr/novel_views/final_result.json: the same means over every N-th frame that is no keyframe (splat_slam_amd.novel_view, exposure fitted
per frame), with the frames scored and the number of degenerate fits; without the flag the tree is unchanged.  Progress and results go to the logger
"splat_slam_amd.run"; there is no print process.

Not provided, each refused with NotImplementedError before anything is loaded: only_tracking (Slam has no mode without a mapper),
mapping.eval_before_final_ba, mono_prior.predict_online: False.
"""
import argparse
import json
import logging
import os
import random
import sys

import numpy as np
import torch

from splat_slam_amd import config as config_mod

__all__ = ["run", "main", "setup_seed", "load_droid_net", "load_mono_depth", "check_supported", "DEPTH_STATS_LABELS"]

log = logging.getLogger("splat_slam_amd.run")
DEPTH_STATS_LABELS = ("depth_l1", "depth_l1_global_scale", "depth_l1_mask_4m", "depth_l1_mask_4m_global_scale", "Average frame coverage",
                      "traj scaling", "traj rotation", "traj translation", "traj stats")


def setup_seed(seed):
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def check_supported(cfg):
    if cfg.get("only_tracking", False):
        raise NotImplementedError("only_tracking: Slam has no mode without a mapper")
    if cfg.get("mapping", {}).get("eval_before_final_ba", False):
        raise NotImplementedError("mapping.eval_before_final_ba: the evaluation runs once, after the final bundle adjustment")
    if not cfg.get("mono_prior", {}).get("predict_online", True):
        raise NotImplementedError("mono_prior.predict_online: False: the mono-depth prior is predicted as the frames arrive")


def load_droid_net(path, device="cuda"):
    from splat_slam_amd.droid_net import DroidNet
    return DroidNet.from_state_dict(torch.load(path, map_location="cpu"), device=device)


def load_mono_depth(path, cfg=None, device="cuda"):
    from splat_slam_amd.mono_depth import MonoDepth, MonoDepthConfig
    return MonoDepth.from_state_dict(torch.load(path, map_location="cpu"), MonoDepthConfig() if cfg is None else cfg, device=device,
                                     backbone="hip", decoder="hip")


def load_lpips(path, device="cuda"):
    from splat_slam_amd.lpips import LPIPS
    return LPIPS.from_state_dict(torch.load(path, map_location="cpu"), device=device)


def _write_results(out_dir, result):
    rendering = result["rendering"]
    if rendering is not None:
        final = {k: rendering[k] for k in ("mean_psnr", "mean_ssim", "mean_lpips", "mean_depthl1") if k in rendering}
        path = os.path.join(out_dir, "psnr", "after_refine", "final_result.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w", encoding="utf-8") as f:
            json.dump(final, f, indent=4)
        log.info("rendering: %s", final)
    novel = result.get("novel_views")
    if novel is not None:
        final = {k: novel[k] for k in ("mean_psnr", "mean_ssim", "mean_lpips", "mean_depthl1") if k in novel}
        final.update(frame_ids=novel["frame_ids"], exposure="fit", degenerate_fits=int(sum(novel["exposure_flags"])))
        path = os.path.join(out_dir, "psnr", "novel_views", "final_result.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w", encoding="utf-8") as f:
            json.dump(final, f, indent=4)
        log.info("novel views: %s", {k: v for k, v in final.items() if k != "frame_ids"})
    d = result["depth_l1"] or {}
    values = (d.get("depth_l1"), d.get("depth_l1_global_scale"), d.get("depth_l1_mask_4m"), d.get("depth_l1_mask_4m_global_scale"),
              d.get("coverage"), result["global_scale"], result["r_a"], result["t_a"], result["kf_traj"])
    with open(os.path.join(out_dir, "depth_stats.txt"), "w") as f:
        for label, value in zip(DEPTH_STATS_LABELS, values):
            f.write(f"{label}: {value}\n")
    log.info("keyframe trajectory: %s; sensor depth: %s", result["kf_traj"], result["depth_l1"])


def run(cfg, net=None, mono_depth=None, lpips=None, stream=None, novel_views=None):
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.slam import Slam
    check_supported(cfg)
    if novel_views is not None and int(novel_views) < 1:
        raise ValueError(f"novel_views={novel_views}: every N-th frame, N >= 1")
    setup_seed(cfg["setup_seed"])
    out_dir = os.path.join(cfg["data"]["output"], str(cfg["scene"]))
    os.makedirs(out_dir, exist_ok=True)
    config_mod.save_config(cfg, os.path.join(out_dir, "cfg.yaml"))
    log.info("scene %s-%s, output %s", cfg.get("dataset"), cfg["scene"], out_dir)
    own_stream = stream is None
    if own_stream:
        from splat_slam_amd.datasets import get_dataset
        stream = get_dataset(cfg)
    try:
        if net is None:
            net = load_droid_net(cfg["tracking"]["pretrained"])
            log.info("tracker weights from %s", cfg["tracking"]["pretrained"])
        if mono_depth is None:
            mono_depth = load_mono_depth(cfg["mono_prior"]["depth_pretrained"])
            log.info("mono-depth weights from %s", cfg["mono_prior"]["depth_pretrained"])
        loop = FusedMappingLoop(cfg, native_ssim=bool(cfg["mapping"]["Training"].get("ssim_loss", False)))
        slam = Slam(cfg, net, stream, loop, mono_depth)
        slam.run()
        log.info("tracking and mapping done: %d keyframes, %d mapped", slam.video.counter.value,
                 sum(1 for _, status in slam.log if status in ("init", "mapped")))
        psnr = slam.terminate()
        meshing = cfg.get("meshing", {})
        result = slam.evaluate(out_dir=out_dir, mesh=bool(meshing.get("mesh", False)), gt_mesh_path=meshing.get("gt_mesh_path") or None,
                               lpips=lpips, plots=True, **({} if novel_views is None else {"novel_views": int(novel_views)}))
        _write_results(out_dir, result)
        result["num_gaussians"] = 0
        if not slam.session.init:
            ply = os.path.join(out_dir, "point_cloud", "final", "point_cloud.ply")
            slam.session.loop.gaussians.save_ply(ply)
            result["num_gaussians"] = int(slam.session.loop.gaussians.get_xyz.shape[0])
            log.info("map of %d Gaussians written to %s", result["num_gaussians"], ply)
        result["output_dir"], result["psnr"] = out_dir, psnr
        return result
    finally:
        if hasattr(stream, "close"):
            stream.close()


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m splat_slam_amd.run", description="Runs the system on a dataset and evaluates it.")
    parser.add_argument("config", type=str, help="path to the config file")
    parser.add_argument("--default", type=str, default=None, help="the config the chain of inherit_from ends on (the reference's "
                        "configs/splat_slam.yaml)")
    parser.add_argument("--root", type=str, default=None, help="directory that relative inherit_from paths are resolved against")
    parser.add_argument("--lpips-weights", type=str, default=None, help="an LPIPS (AlexNet) state dict; without it LPIPS is not reported")
    parser.add_argument("--novel_views", type=int, default=None, metavar="N", help="also score every N-th frame that is no keyframe "
                        "(psnr/novel_views/final_result.json); without it only the mapped keyframes are scored")
    args = parser.parse_args(argv)
    if args.novel_views is not None and args.novel_views < 1:
        parser.error("--novel_views N: every N-th frame, N >= 1")
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s: %(message)s")
    cfg = config_mod.load_config(args.config, args.default, args.root)
    check_supported(cfg)
    lpips = load_lpips(args.lpips_weights) if args.lpips_weights else None
    result = run(cfg, lpips=lpips, **({} if args.novel_views is None else {"novel_views": args.novel_views}))
    return 0 if result is not None else 1


if __name__ == "__main__":
    sys.exit(main())
