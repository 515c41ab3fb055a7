"""-m gpu: the evaluation's plots and the run entry point on the MI355X.  sgr_plot_panels against the restatement of tests/plots_ref.py,
bit for bit (tests/test_plots_cpu.py holds the inputs to their conditioning), plot_rendering's files against compose_panels,
Slam.evaluate(plots=True) and splat_slam_amd.run on the synthetic tracker stream, the two checkpoint loaders, and main on a folder."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import frame_ref
import plots_ref as ref
import tracker_cases as T
import update_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_STREAM = 10


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _compose(frames, s, global_scale, depth_max=ref.DEPTH_MAX):
    from splat_slam_amd import plots
    scalar = lambda v: None if v is None else torch.tensor([v], dtype=torch.float32, device=DEV)
    out = plots.compose_panels([_dev(f["render"]) for f in frames], [_dev(f["gt"]) for f in frames], [_dev(f["depth"]) for f in frames],
                               [_dev(f["gt_depth"]) for f in frames], [f["heading"] for f in frames], [f["titles"] for f in frames], s=s,
                               exposures=[(scalar(f["a"]), scalar(f["b"])) for f in frames], global_scale=global_scale, depth_max=depth_max)
    return out.cpu().numpy()


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


# ---- the panel
@pytest.mark.parametrize("case", ref.PANEL_CASES, ids=lambda c: "%dx%d_s%d_%s" % c[:4])
def test_panels_equal_the_restatement_bit_for_bit(case):
    H, W, s, variant, gs = case
    frames = ref.case_frames(H, W, variant, gs)
    got = _compose(frames, s, gs)
    assert got.shape == (3, *ref.panel_size(H, W, s), 3) and got.dtype == np.uint8
    for i, f in enumerate(frames):
        want, info = ref.panel(f, s, gs, ref.DEPTH_MAX)
        bad = np.argwhere((got[i] != want).any(-1))
        print(case, "frame", i, info, "pixels that differ:", len(bad), bad[:5].tolist())
        assert np.array_equal(got[i], want), (i, len(bad), bad[:5].tolist())
    assert (got[:, :ref.MARGIN] == 255).all() and (got[:, :, :ref.MARGIN] == 255).all()          # the white margin


def test_seventeen_frames_in_one_call_equal_the_frames_alone():
    H, W, s, gs = 5, 7, 1, 1.25
    frames = []
    for k in range(6):
        frames += ref.case_frames(H, W, "edges", gs, seed=k)
    frames = frames[:17]
    for k, f in enumerate(frames):
        f["heading"] = f"frame: {k}"
    together = _compose(frames, s, gs)
    assert together.shape[0] == 17
    for k, f in enumerate(frames):
        alone = _compose([f], s, gs)[0]
        assert np.array_equal(together[k], alone), k
    assert np.array_equal(together[16], ref.panel(frames[16], s, gs, ref.DEPTH_MAX)[0])           # the frame past the 16-frame boundary
    assert np.array_equal(_compose(frames[3:8], s, gs), together[3:8])                           # ... and in any batch


# ---- plot_rendering
def test_plot_rendering_writes_what_compose_panels_gives(tmp_path):
    from PIL import Image
    from splat_slam_amd import plots
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.eval import eval_rendering
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.renderer import render
    intr = syn.INTRINSICS["tiny"]
    params = syn.room_parameters(4000, seed=7, device=DEV)
    params["scaling"] = params["scaling"] + 1.2
    cams = syn.make_views(params, 6, intr, DEV, seed=7)
    gm = syn.model_from_parameters(params, device=DEV)
    with torch.no_grad():
        for k, cam in enumerate(cams[1:], 1):
            cam.exposure_a.fill_(0.03 * ((k % 5) - 2))
            cam.exposure_b.fill_(0.01 * ((k % 3) - 1))
    bg = torch.zeros(3, device=DEV)
    metrics = eval_rendering(cams, gm, PipelineParams(), bg, global_scale=1.5)
    names = [f"video_idx_{k}_kf_idx_{3 * k}" for k in range(6)]
    out_dir = str(tmp_path / "plots_after_refine")
    info = plots.plot_rendering(cams, gm, PipelineParams(), bg, metrics, out_dir, names, global_scale=1.5)
    print("plot_rendering:", {k: info[k] for k in ("s", "panel_size", "compose_s", "copy_s", "encode_s", "gif_s")})
    assert info["s"] == 1 and info["panel_size"] == ref.panel_size(intr["H"], intr["W"], 1)
    assert sorted(os.listdir(out_dir)) == sorted([n + ".png" for n in names] + ["output.gif"])
    with torch.no_grad():
        pk = [render(c, gm, PipelineParams(), bg) for c in cams]
    titles = [[t.format(metrics["psnr"][k]) if "PSNR" in t else t.format(metrics["depth_l1"][k]) for t in ref.TITLES] for k in range(6)]
    assert titles[2][3] == "Rasterized RGB, PSNR: %.2f" % metrics["psnr"][2] and titles[2][4].startswith("Rasterized Depth, L1: ")
    want = plots.compose_panels([p["render"] for p in pk], [c.original_image for c in cams], [p["depth"] for p in pk],
                                [c.depth for c in cams], ["frame: " + n for n in names], titles, s=1,
                                exposures=[None] + [(c.exposure_a, c.exposure_b) for c in cams[1:]], global_scale=1.5).cpu().numpy()
    for k, n in enumerate(names):
        assert np.array_equal(_decode(os.path.join(out_dir, n + ".png")), want[k]), n
    # the title's text is on the panel: the restated glyphs of the PSNR title, clipped at the cell
    cw = intr["W"]
    canvas = np.full((ref.CHAR_H, cw, 3), 255, np.int64)
    ref.draw_text(canvas, titles[2][3], 0, 0, cw)
    y0 = 2 * ref.MARGIN + ref.CHAR_H + (ref.CHAR_H + ref.TITLE_GAP + intr["H"] + ref.MARGIN)
    assert np.array_equal(want[2][y0:y0 + ref.CHAR_H, ref.MARGIN:ref.MARGIN + cw], canvas.astype(np.uint8))
    with Image.open(info["gif"]) as gif:
        assert gif.n_frames == 6 and gif.info["duration"] == 100 and gif.info.get("loop") == 0
    # without the GIF
    quiet = plots.plot_rendering(cams[:2], gm, PipelineParams(), bg, {k: v[:2] for k, v in metrics.items() if isinstance(v, list)},
                                 str(tmp_path / "two"), names[:2], gif=False)
    assert quiet["gif"] is None and sorted(os.listdir(tmp_path / "two")) == sorted(n + ".png" for n in names[:2])


# ---- Slam.evaluate(plots=True) and run.run on the run of tests/test_gpu_slam_evaluate.py (its fixture restated)
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


def run_cfg(out_root, scene="synthetic"):
    cfg = make_cfg()
    cfg.update({"setup_seed": 43, "scene": scene, "dataset": "synthetic", "data": {"output": str(out_root)},
                "meshing": {"mesh": False, "gt_mesh_path": ""}, "mono_prior": {"predict_online": True}, "only_tracking": False})
    return cfg


@pytest.fixture(scope="module")
def finished():
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.slam import Slam
    cfg = make_cfg()
    torch.manual_seed(43)
    np.random.seed(43)
    slam = Slam(cfg, DroidNet.synthetic(7, device=DEV), PosedStream(N_STREAM, smooth_path(N_STREAM)), FusedMappingLoop(cfg, device=DEV),
                mono_depth)
    slam.run()
    slam.terminate()
    return slam


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=True)
    if isinstance(a, float) and np.isnan(a):
        return isinstance(b, float) and np.isnan(b)
    if hasattr(a, "r_a"):                                            # an Alignment
        return np.array_equal(a.r_a, b.r_a) and np.array_equal(a.t_a, b.t_a) and a.s == b.s and a.n_used == b.n_used
    return a == b


NEW_FILES = ("kf_traj.png", "full_traj.png", "plots_after_refine")


def test_slam_evaluate_with_plots_writes_the_figures_and_returns_what_it_returns_without(finished, tmp_path):
    slam = finished
    with pytest.raises(ValueError, match="out_dir"):
        slam.evaluate(plots=True)
    plain = slam.evaluate(out_dir=str(tmp_path / "plain"), plots=False)
    drawn = slam.evaluate(out_dir=str(tmp_path / "drawn"), plots=True)
    assert "traj_error" not in drawn and "full_traj_error" not in drawn
    assert set(plain) == set(drawn)
    for key in plain:
        assert _same(plain[key], drawn[key]), key
    assert not any(os.path.exists(tmp_path / "plain" / f) for f in NEW_FILES)
    views = sorted(slam.session.loop.viewpoints)
    ts = slam.video.timestamp.cpu().tolist()
    want = sorted([f"video_idx_{k}_kf_idx_{int(ts[k])}.png" for k in views] + ["output.gif"])
    assert len(views) > 1 and sorted(os.listdir(tmp_path / "drawn" / "plots_after_refine")) == want
    from splat_slam_amd import plots
    H, W = slam.video.ht, slam.video.wd
    assert _decode(tmp_path / "drawn" / "plots_after_refine" / want[1]).shape == (*plots.panel_size(H, W, 1), 3)
    for name in ("kf_traj.png", "full_traj.png"):
        assert _decode(tmp_path / "drawn" / name).shape == (plots.TRAJ_SIZE[1], plots.TRAJ_SIZE[0], 3)
    assert sorted(set(os.listdir(tmp_path / "drawn")) - set(os.listdir(tmp_path / "plain"))) == sorted(NEW_FILES)


def _check_tree(out_dir, result, n_views):
    from splat_slam_amd import config
    for name in ("cfg.yaml", "video.npz", "depth_stats.txt", "kf_traj.png", "full_traj.png", "metrics_kf_traj.txt", "metrics_full_traj.txt"):
        assert os.path.isfile(os.path.join(out_dir, name)), name
    final = json.load(open(os.path.join(out_dir, "psnr", "after_refine", "final_result.json")))
    assert set(final) == {"mean_psnr", "mean_ssim", "mean_depthl1"}                  # no LPIPS weights: no mean_lpips
    for k, v in final.items():
        assert v == result["rendering"][k] or (np.isnan(v) and np.isnan(result["rendering"][k])), k
    lines = open(os.path.join(out_dir, "depth_stats.txt")).read().split("\n")
    labels = ["depth_l1", "depth_l1_global_scale", "depth_l1_mask_4m", "depth_l1_mask_4m_global_scale", "Average frame coverage",
              "traj scaling", "traj rotation", "traj translation", "traj stats"]
    starts = [next(i for i, line in enumerate(lines) if line.startswith(label + ": ")) for label in labels]
    assert starts == sorted(starts) and f"traj scaling: {result['global_scale']}" in lines
    plots_dir = os.path.join(out_dir, "plots_after_refine")
    assert len([f for f in os.listdir(plots_dir) if f.endswith(".png")]) == n_views and os.path.isfile(os.path.join(plots_dir, "output.gif"))
    assert config.load_config(os.path.join(out_dir, "cfg.yaml"))["scene"] == os.path.basename(out_dir)
    return os.path.join(out_dir, "point_cloud", "final", "point_cloud.ply")


def test_run_leaves_the_output_tree(tmp_path):
    from splat_slam_amd import run
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.droid_net import DroidNet
    cfg = run_cfg(tmp_path)
    closed = []
    stream = PosedStream(N_STREAM, smooth_path(N_STREAM))
    stream.close = lambda: closed.append(True)
    result = run.run(cfg, net=DroidNet.synthetic(7, device=DEV), mono_depth=mono_depth, stream=stream)
    out_dir = os.path.join(str(tmp_path), "synthetic")
    assert result["output_dir"] == out_dir and closed == [True]
    assert result["rendering"] is not None and len(result["psnr"]) == len(result["rendering"]["psnr"])
    ply = _check_tree(out_dir, result, len(result["rendering"]["psnr"]))
    from splat_slam_amd.gaussian_model import GaussianModel
    gm = GaussianModel(0, config=syn.DEFAULT_CONFIG, device=DEV, knn_fn=lambda p: torch.ones(p.shape[0], device=p.device))
    gm.load_ply(ply)
    assert gm.get_xyz.shape[0] == result["num_gaussians"] > 0


# ---- the loaders
def test_load_droid_net_reads_a_module_checkpoint_with_three_row_heads(tmp_path):
    from splat_slam_amd import droid_net, run
    sd = droid_net.synthetic_state_dict(7)
    saved = {}
    for k, v in sd.items():
        if k.startswith(("update.weight.2.", "update.delta.2.")):
            v = torch.cat([v, torch.full_like(v[:1], 0.25)], 0)                      # the third row the reference cuts off
            assert v.shape[0] == 3
        saved["module." + k] = v
    path = str(tmp_path / "droid.pth")
    torch.save(saved, path)
    loaded, want = run.load_droid_net(path, device=DEV), droid_net.DroidNet.synthetic(7, device=DEV)
    net, inp, corr, flow = update_ref.make_inputs(3, 6, 8, seed=103, device=DEV, dtype=torch.float16)
    ii = torch.tensor([2, 0, 2], device=DEV)
    a, b = loaded.update(net, inp, corr, flow, ii), want.update(net, inp, corr, flow, ii)
    assert len(a) == len(b) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_load_mono_depth_reads_a_wrapped_checkpoint(tmp_path):
    from splat_slam_amd import mono_depth as M
    from splat_slam_amd import run
    cfg = M.MonoDepthConfig(stem_chs=32, stage_chs=(64, 128, 256), stage_layers=(1, 1, 2), gn_groups=8, dim=128, heads=2, depth=4, taps=(2, 3),
                            pos_grid=4, features=32, net_size=(64, 96))
    sd = M.synthetic_state_dict(5, cfg)
    path = str(tmp_path / "omnidata.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "epoch": 1}, path)
    loaded = run.load_mono_depth(path, cfg, device=DEV)
    want = M.MonoDepth.synthetic(5, cfg, DEV, backbone="hip", decoder="hip")
    image = torch.rand(1, 3, 48, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    assert torch.equal(loaded.predict(image), want.predict(image))


# ---- main on a folder
def test_main_runs_a_replica_folder_to_its_final_result(tmp_path, monkeypatch):
    import yaml
    from splat_slam_amd import run
    from splat_slam_amd.droid_net import DroidNet
    data = frame_ref.write_replica(tmp_path / "data")
    H, W = T.HT, T.WD                                    # the 24 x 32 images enlarged to the tracker's test size, no edge cut
    cfg = make_cfg()
    cfg["cam"] = {**data["cam"], "H_out": H, "W_out": W, "H_edge": 0, "W_edge": 0}
    cfg.update({k: data[k] for k in ("dataset", "stride", "max_frames")})
    cfg["data"] = {**data["data"], "output": str(tmp_path / "out")}
    cfg.update({"setup_seed": 43, "scene": "room", "meshing": {"mesh": False, "gt_mesh_path": ""}, "mono_prior": {"predict_online": True,
                "depth_pretrained": "unused"}, "only_tracking": False})
    cfg["tracking"]["pretrained"] = "unused"
    base, own = str(tmp_path / "base.yaml"), str(tmp_path / "room.yaml")
    with open(base, "w") as f:
        yaml.safe_dump({k: v for k, v in cfg.items() if k != "scene"}, f)
    with open(own, "w") as f:
        yaml.safe_dump({"inherit_from": "base.yaml", "scene": "room"}, f)
    loaded = []

    def flat_depth(timestamp, image):
        y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=DEV), torch.arange(W, dtype=torch.float32, device=DEV), indexing="ij")
        return 2.0 + 0.3 * torch.sin(0.2 * x + 0.1 * float(timestamp)) * torch.cos(0.15 * y)

    monkeypatch.setattr(run, "load_droid_net", lambda path, device="cuda": loaded.append(path) or DroidNet.synthetic(7, device=DEV))
    monkeypatch.setattr(run, "load_mono_depth", lambda path, cfg=None, device="cuda": loaded.append(path) or flat_depth)
    assert run.main([own, "--root", str(tmp_path)]) == 0
    assert loaded == ["unused", "unused"]
    out_dir = str(tmp_path / "out" / "room")
    for name in ("cfg.yaml", "video.npz", "depth_stats.txt"):
        assert os.path.isfile(os.path.join(out_dir, name)), name
    final = json.load(open(os.path.join(out_dir, "psnr", "after_refine", "final_result.json")))
    assert set(final) == {"mean_psnr", "mean_ssim", "mean_depthl1"}
    # the folder carries sensor depth: the five depth figures are numbers here
    stats = open(os.path.join(out_dir, "depth_stats.txt")).read()
    assert "depth_l1: None" not in stats and "Average frame coverage: " in stats
