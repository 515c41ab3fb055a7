"""Slam.evaluate on the MI355X: the synthetic tracker stream of tests/tracker_cases.py with ground-truth poses, through Slam.run(),
terminate() and evaluate().  The trajectory block is kf_traj_eval by hand, the aligned cameras and the scale reach eval_rendering, a
ground truth that is a known similarity of the estimate returns that similarity, and without ground truth the rest still runs."""
import copy
import os

import numpy as np
import pytest
import torch

import tracker_cases as T
import traj_eval_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_STREAM = 10


class PosedStream(T.SyntheticStream):
    """the synthetic stream with a `poses` list, camera -> world 4x4 per frame, as the reference's datasets carry"""

    def __init__(self, n, poses):
        super().__init__(n)
        self.poses = poses


def smooth_path(n):
    out = []
    for i in range(n):
        p = np.eye(4, dtype=np.float32)
        a = 0.05 * i
        p[:3, :3] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
        p[:3, 3] = [0.08 * i, 0.03 * np.sin(0.9 * i), 0.05 * i + 0.01 * i * i]
        out.append(p)
    return out


def mono_depth(timestamp, image):
    y, x = torch.meshgrid(torch.arange(T.HT, dtype=torch.float32, device=DEV), torch.arange(T.WD, dtype=torch.float32, device=DEV),
                          indexing="ij")
    return 2.0 + 0.3 * torch.sin(0.2 * x + 0.1 * float(timestamp)) * torch.cos(0.15 * y)


def make_cfg():
    """tests/test_gpu_slam.py's configuration (every frame a keyframe) with a video buffer that leaves the trajectory filler its 16 slots"""
    from splat_slam_amd import synthetic as syn
    cfg = T.make_cfg(**{"tracking.warmup": 4, "tracking.motion_filter.thresh": 0.0, "tracking.frontend.keyframe_thresh": -1.0,
                        "tracking.frontend.enable_online_ba": True, "tracking.backend.ba_freq": 3, "mapping.every_keyframe": 1,
                        "tracking.multiview_filter.thresh": 1e6, "tracking.multiview_filter.visible_num": 1, "tracking.buffer": 32})
    cfg["cam"] = {"H_out": T.HT, "W_out": T.WD}
    cfg["tracking"]["backend"]["final_ba"] = False
    mapping = copy.deepcopy(syn.DEFAULT_CONFIG["mapping"])
    tr = mapping["Training"]
    tr["init_itr_num"], tr["mapping_itr_num"], tr["window_size"] = 30, 4, 4
    tr["init_gaussian_update"], tr["init_gaussian_reset"] = 10, 10 ** 9
    mapping["opt_params"]["densify_from_iter"] = 10 ** 9
    mapping["final_refine_iters"] = 8
    cfg["mapping"].update(mapping)
    return cfg


@pytest.fixture(scope="module")
def run():
    """one Slam run and terminate(); every eval_rendering call of the module is recorded"""
    from splat_slam_amd import eval as eval_mod
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.slam import Slam
    cfg = make_cfg()
    torch.manual_seed(43)
    np.random.seed(43)
    slam = Slam(cfg, DroidNet.synthetic(7, device=DEV), PosedStream(N_STREAM, smooth_path(N_STREAM)), FusedMappingLoop(cfg, device=DEV),
                mono_depth)
    slam.run()
    psnr = slam.terminate()
    calls, real = [], eval_mod.eval_rendering

    def eval_rendering_(frames, *args, **kw):
        calls.append(dict(frames=list(frames), c2w=kw.get("c2w"), global_scale=kw.get("global_scale")))
        return real(frames, *args, **kw)

    eval_mod.eval_rendering = eval_rendering_
    try:
        yield slam, psnr, calls
    finally:
        eval_mod.eval_rendering = real


def test_the_trajectory_block_is_kf_traj_eval_by_hand_and_the_aligned_cameras_reach_eval_rendering(run, tmp_path):
    from splat_slam_amd import traj_eval as te
    slam, psnr, calls = run
    n = slam.video.counter.value
    assert n == N_STREAM and slam.video.timestamp[:n].tolist() == [float(i) for i in range(n)]
    del calls[:]
    out = slam.evaluate(out_dir=str(tmp_path))               # gt_poses: stream.poses
    print("evaluate:", {k: out[k] for k in ("kf_traj", "global_scale", "full_traj", "depth_l1")}, out.get("traj_error"))
    assert "traj_error" not in out and "full_traj_error" not in out
    stats, s, r_a, t_a = te.kf_traj_eval(slam.video, slam.stream.poses)
    assert out["kf_traj"] == stats and out["global_scale"] == s
    assert np.array_equal(out["r_a"], r_a) and np.array_equal(out["t_a"], t_a)
    assert sorted(stats) == ["max", "mean", "median", "min", "rmse", "sse", "std"] and all(np.isfinite(list(stats.values())))
    # what reached eval_rendering: the mapped viewpoints at their aligned poses, and the scale
    assert len(calls) == 1
    frames = [slam.session.loop.viewpoints[k] for k in sorted(slam.session.loop.viewpoints)]
    assert calls[0]["frames"] == frames and calls[0]["global_scale"] == s
    own = np.stack([np.linalg.inv(np.block([[f.R.double().cpu().numpy(), f.T.double().cpu().numpy()[:, None]], [np.array([[0, 0, 0, 1.0]])]]))
                    for f in frames])
    want = R.aligned_c2w(own, r_a, t_a, s)
    assert len(calls[0]["c2w"]) == len(frames) and np.abs(np.stack(calls[0]["c2w"]) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert len(out["rendering"]["psnr"]) == len(frames) == len(psnr) and all(np.isfinite(out["rendering"]["psnr"]))
    assert out["depth_l1"] is None                            # the stream yields no depth
    # every frame of this stream is a keyframe: the filled trajectory is the keyframes'
    assert out["full_traj"] == stats and out["full_traj_alignment"].s == s and tuple(out["traj_est"].shape) == (N_STREAM, 4, 4)
    for i in range(n):
        assert torch.equal(out["traj_est"][i], slam.video.get_pose(i, DEV))
    # the files of the reference
    text = open(os.path.join(tmp_path, "metrics_kf_traj.txt")).read()
    assert text.startswith("#" * 10 + "Keyframes traj" + "#" * 10 + f"\nscale: {s}\nrotation:\n") and f"statistics:\n{stats}" in text
    assert open(os.path.join(tmp_path, "metrics_full_traj.txt")).read().startswith("#" * 10 + "Full traj" + "#" * 10)
    saved = np.load(os.path.join(tmp_path, "video.npz"))
    assert float(saved["scale"]) == s and saved["poses"].shape == (n, 4, 4)


def test_a_ground_truth_that_is_a_similarity_of_the_estimate_returns_that_similarity(run):
    slam, _, calls = run
    n = slam.video.counter.value
    x = torch.stack([slam.video.get_pose(i, DEV)[:3, 3] for i in range(n)]).double().cpu().numpy()
    # exactly representable in fp32: twice the centres, turned by a quarter about z
    s0, r0 = 2.0, np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    gt = []
    for i in range(n):
        p = np.eye(4, dtype=np.float32)
        p[:3, 3] = s0 * (r0 @ x[i])
        assert np.array_equal(p[:3, 3].astype(np.float64), s0 * (r0 @ x[i]))
        gt.append(p)
    _, _, _, d = R.umeyama(x, np.stack(gt)[:, :3, 3].astype(np.float64))
    ext = float(np.abs(x - x.mean(0)).max())
    print("estimate's centres:", x.tolist(), "singular values:", d)
    assert d[1] / d[0] >= 1e-3                                # the tracked path is no line: the margin of rtol 1e-9 is 1e4 here
    del calls[:]
    out = slam.evaluate(gt_poses=gt)
    assert "traj_error" not in out
    assert abs(out["global_scale"] - s0) <= 1e-9 * s0 and np.abs(out["r_a"] - r0).max() <= 1e-9
    assert np.abs(out["t_a"]).max() <= 1e-9 * s0 * max(ext, float(np.abs(x).max()))
    assert out["kf_traj"]["rmse"] <= 1e-9 * s0 * ext and out["kf_traj"]["max"] <= 1e-9 * s0 * ext
    assert calls[0]["global_scale"] == out["global_scale"]


def test_without_ground_truth_poses_the_rest_still_runs(run):
    slam, psnr, calls = run
    poses, slam.stream.poses = slam.stream.poses, None
    try:
        del calls[:]
        out = slam.evaluate()
    finally:
        slam.stream.poses = poses
    assert out["kf_traj"] is None and out["full_traj"] is None and out["r_a"] is None and out["t_a"] is None and out["traj_est"] is None
    assert out["global_scale"] == 1.0 and "traj_error" not in out
    assert len(calls) == 1 and calls[0]["c2w"] is None and calls[0]["global_scale"] == 1.0
    assert len(out["rendering"]["psnr"]) == len(psnr) and all(np.isfinite(out["rendering"]["psnr"]))


def test_a_degenerate_pairing_is_reported_not_raised(run):
    """a degenerate fit (here: an estimate scored against fewer than three usable poses) leaves scale 1 and the cameras' own poses"""
    slam, psnr, calls = run
    gt = [np.full((4, 4), np.nan, dtype=np.float32) for _ in range(N_STREAM)]
    gt[0], gt[5] = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    del calls[:]
    out = slam.evaluate(gt_poses=gt)
    assert "traj_error" in out and "full_traj_error" in out and out["kf_traj"] is None and out["global_scale"] == 1.0
    assert calls[0]["c2w"] is None and len(out["rendering"]["psnr"]) == len(psnr)
