"""The whole system in one process (SLAM of the reference's src/slam.py, without its processes, pipes, printing and files): the tracker
finds keyframes, the keyframe depth fusion turns each into a depth map and a pose, and the mapping session maps it.  Stated in DESIGN.md
section 3, "Slam".

    Slam(cfg, net, stream, loop, mono_depth)
        cfg: the reference's dict: what Tracker, Frontend, Backend and DepthVideo.from_config read (cfg["cam"]["H_out"], ["W_out"],
        cfg["tracking"], cfg["mapping"]["every_keyframe"]) and cfg["tracking"]["backend"]["final_ba"]; net: a DroidNet; stream: what
        Tracker.run takes; loop: a MappingLoop or FusedMappingLoop (its own config is the mapper's); mono_depth(timestamp, image
        [1,3,H,W]) -> [H,W] depth, the callable MotionFilter accepts.
        Attributes: video (DepthVideo), tracker (Tracker), depth (KeyframeDepth), session (MappingSession), log: the list of
        (video_idx, status) of every keyframe the tracker reported, status "init", "mapped", "skipped" or "invalid".
    slam.run()            tracker.run(stream); every reported keyframe is mapped before tracking goes on
    slam.terminate()      with final_ba the two global bundle adjustments (dense_ba(7), dense_ba(12), slam.py:120-127), then the final
                          pose and depth update of every registered keyframe (mapper.py:620-647) and session.finish(); returns the
                          PSNR of every mapped viewpoint ([] when no keyframe was ever valid)

On a keyframe: its mono map goes into the depth cache (prepared once), KeyframeDepth.get fuses it with the video's current state, and
the result goes to session.process -- or, with fewer than 100 valid tracker pixels, the camera is registered as no mapping keyframe
(mapper.py:910-926).  When a keyframe is mapped, the session asks for the current pose and depth of all past keyframes: they come from
one batched fusion call (the pose source's prefetch).  The mono-depth network is splat_slam_amd.mono_depth.MonoDepth, itself such a callable.

    slam.evaluate(gt_poses=None, gt_depths=None, mesh=False, gt_mesh_path=None, lpips=None, out_dir=None, cull_mesh=False,
                  plots=False, rpe_delta=None, rotation_errors=False, novel_views=None, novel_exposure="fit") -> dict
        after terminate(): the rest of the reference's terminate() (slam.py:169-242) in its order, on splat_slam_amd.traj_eval.
        gt_poses: camera -> world 4x4 per frame of the stream, indexed by timestamp (default stream.poses when the stream has one).
        "kf_traj": the ATE statistics of the keyframes after the scaled Umeyama alignment (kf_traj_eval), "global_scale", "r_a", "t_a":
        that alignment; "rendering": eval_rendering over the session's viewpoints (what session.evaluate runs) with the mapped cameras
        moved into the ground-truth frame (aligned_c2w) as c2w and with global_scale (None without a map); "depth_l1":
        video.eval_depth_l1 per frame aligned and with global_scale, when stream[i][2] is a depth (None otherwise); "full_traj",
        "full_traj_alignment", "traj_est": full_traj_eval over a PoseTrajectoryFiller of the same net and video (the video needs 16
        free slots behind its keyframes).  Without ground-truth poses the trajectory entries are
        None, global_scale is 1 and the cameras keep their own poses.  A trajectory that determines no similarity
        (TrajectoryDegenerate) is reported under "traj_error" / "full_traj_error" and scored with scale 1 and the identity; the
        rendering evaluation still runs (the reference swallows the exception and then fails on an unbound name).  out_dir: video.npz
        (with `scale`), metrics_kf_traj.txt, metrics_full_traj.txt and, with mesh, mesh.ply are written there.
        cull_mesh=True: eval_rendering culls the predicted and the ground-truth mesh to what the keyframes saw before it scores them
        (splat_slam_amd.mesh_cull), from the ground-truth poses of the keyframes when there are ground-truth poses, else from the
        fusion poses.  Nothing is culled by default.
        plots=True (needs out_dir, ValueError otherwise): the two trajectory evaluations also write kf_traj.png and full_traj.png, and after
        eval_rendering, splat_slam_amd.plots.plot_rendering writes plots_after_refine/video_idx_{V}_kf_idx_{T}.png per mapped viewpoint (T
        the keyframe's timestamp as an integer) and output.gif from that result.  The returned dict is the same.  Nothing is drawn by default.
        rpe_delta=N: "kf_rpe" and "full_rpe", the statistics of the relative translation error over N used poses after the alignment
        (traj_eval.pose_errors); rotation_errors=True: "kf_rot" and "full_rot", those of the absolute rotation angle in degrees.  Each is
        None where its trajectory evaluation failed or left no item; none of the four keys exists unless asked for.
        novel_views=N: "novel_views", splat_slam_amd.novel_view.eval_novel_views over every N-th frame of the stream that is no keyframe
        of the video (select_frames: neither a warm-up keyframe nor one the session registered, mapped or not), at its pose of the filled trajectory (computed once, shared with full_traj_eval; without ground-truth
        poses it is computed for this alone), with global_scale, lpips and the exposure mode novel_exposure ("fit", "keyframes" or
        "none").  None without a map or when every such frame is a keyframe; the key does not exist unless asked for.

`stream` for a Replica, ScanNet or TUM RGB-D folder: splat_slam_amd.datasets.get_dataset(splat_slam_amd.config.load_config(...)).
The command line and the output tree: splat_slam_amd.run.  Not provided: a mode without a mapper (--only_tracking),
eval_before_final_ba, predict_online: False.
"""
import os
import tempfile

import numpy as np
import torch

from splat_slam_amd.backend import Backend
from splat_slam_amd.depth_fusion import KeyframeDepth
from splat_slam_amd.depth_video import DepthVideo
from splat_slam_amd.session import MappingSession
from splat_slam_amd.tracker import Tracker

__all__ = ["Slam"]


class _PoseSource:
    """MappingSession's pose source over a KeyframeDepth: prefetch fuses every keyframe that is about to be asked for in one call"""

    def __init__(self, depth):
        self.depth, self.ready = depth, {}

    def prefetch(self, video_idxs):
        depth, w2c, invalid = self.depth.get(video_idxs)
        self.ready = {i: (w2c[b], depth[b], invalid[b]) for b, i in enumerate(video_idxs)}

    def __call__(self, video_idx):
        if video_idx not in self.ready:
            self.prefetch([video_idx])
        return self.ready.pop(video_idx)               # an answer is used once: the video moves on


class Slam:
    def __init__(self, cfg, net, stream, loop, mono_depth):
        if mono_depth is None:
            raise ValueError("Slam: mono_depth is required (the mapper's depth outside the valid-depth mask comes from it)")
        self.cfg, self.net, self.stream, self.mono_depth = cfg, net, stream, mono_depth
        self.video = DepthVideo.from_config(cfg)
        self.tracker = Tracker(cfg, net, self.video, on_keyframe=self.on_keyframe, mono_depth=self._mono)
        self.depth = KeyframeDepth(self.video)
        fx, fy, cx, cy = (float(v) for v in stream.get_intrinsic().tolist())
        intr = dict(W=self.video.wd, H=self.video.ht, fx=fx, fy=fy, cx=cx, cy=cy)
        self.session = MappingSession(loop, intr, pose_source=_PoseSource(self.depth))
        self.log = []
        self._frames = {}                              # timestamp -> (image, mono map) of the frames that entered the video

    def _mono(self, timestamp, image):
        mono = self.mono_depth(timestamp, image)
        self._frames[float(timestamp)] = (image[0], mono)
        return mono

    def on_keyframe(self, video_idx, timestamp):
        if video_idx is None:                          # end of the stream
            return
        key = float(timestamp)
        if key not in self._frames:
            raise RuntimeError(f"Slam: the tracker reported keyframe {video_idx} at timestamp {timestamp}, which never entered the video")
        color, mono = self._frames.pop(key)
        self._frames = {t: f for t, f in self._frames.items() if t > key}
        self.depth.put_mono(video_idx, mono.to(device=self.video.disps_up.device, dtype=torch.float32).contiguous())
        depth, w2c, invalid = self.depth.get([video_idx])
        if invalid[0]:
            self.session.register_invalid(video_idx, timestamp, color, depth[0], w2c[0])
            status = "invalid"
        else:
            status = self.session.process(video_idx, timestamp, color, depth[0], w2c[0])
        self.log.append((video_idx, status))

    def run(self):
        self.tracker.run(self.stream)

    def terminate(self):
        if self.cfg["tracking"]["backend"].get("final_ba", False):
            ba = Backend(self.net, self.video, self.cfg)
            ba.dense_ba(7)
            ba.dense_ba(12)
        if self.session.init:                          # no keyframe was ever valid: there is no map
            return []
        self.session.refresh_keyframes()
        return self.session.finish()

    def evaluate(self, gt_poses=None, gt_depths=None, mesh=False, gt_mesh_path=None, lpips=None, out_dir=None, cull_mesh=False,
                 plots=False, rpe_delta=None, rotation_errors=False, novel_views=None, novel_exposure="fit"):
        from splat_slam_amd import traj_eval
        from splat_slam_amd.trajectory_filler import PoseTrajectoryFiller
        if plots and out_dir is None:
            raise ValueError("Slam.evaluate(plots=True) needs out_dir: the figures are files")
        plot = {"plot": True} if plots else {}
        extra = ([("translation_part", int(rpe_delta), False)] if rpe_delta is not None else []) + \
            ([("rotation_angle_deg", None, False)] if rotation_errors else [])
        if extra:
            plot = dict(plot, extra=extra)

        def more(prefix, results):                     # the entries of `extra` under their keys of the returned dict
            if rpe_delta is not None:
                out[prefix + "_rpe"] = results.get(traj_eval.extra_key(*extra[0]))
            if rotation_errors:
                out[prefix + "_rot"] = results.get(traj_eval.extra_key(*extra[-1]))
        if gt_poses is None:
            gt_poses = getattr(self.stream, "poses", None)
        out = {"kf_traj": None, "global_scale": 1.0, "r_a": None, "t_a": None, "rendering": None, "depth_l1": None, "full_traj": None,
               "full_traj_alignment": None, "traj_est": None}
        more("kf", {})
        more("full", {})
        novel_ids = []
        if novel_views is not None:
            from splat_slam_amd.novel_view import EXPOSURE_MODES, select_frames
            if novel_exposure not in EXPOSURE_MODES:
                raise ValueError(f"Slam.evaluate: novel_exposure={novel_exposure!r}, one of {EXPOSURE_MODES}")
            out["novel_views"] = None
            if not self.session.init:              # the video's keyframes: the warm-up ones and every one the session registered
                stamps = self.video.timestamp[:self.video.counter.value].cpu().tolist()
                novel_ids = select_frames(len(self.stream), stamps, every=novel_views)
        npz = None
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            npz = os.path.join(out_dir, "video.npz")
            self.video.save_video(npz)
        alignment = None
        if gt_poses is not None:
            try:
                out["kf_traj"], s, r_a, t_a, *rest = traj_eval.kf_traj_eval(self.video, gt_poses, out_dir=out_dir, npz_path=npz, **plot)
                more("kf", rest[0] if rest else {})
                alignment = traj_eval.Alignment(r_a, t_a, s, 0, 0)
                out["global_scale"], out["r_a"], out["t_a"] = s, r_a, t_a
            except traj_eval.TrajectoryDegenerate as e:
                out["traj_error"] = str(e)
        if not self.session.init:                      # there is a map: MappingSession.evaluate's call, with the two aligned arguments
            from splat_slam_amd.eval import eval_rendering
            from splat_slam_amd.mapper import PipelineParams
            loop = self.session.loop
            frames = [loop.viewpoints[k] for k in sorted(loop.viewpoints)]
            c2w = None if alignment is None else list(traj_eval.aligned_c2w(frames, alignment))
            cull = {}
            if cull_mesh:
                ts = self.video.timestamp.cpu().tolist()
                cull = dict(cull_mesh=True, cull_poses=None if gt_poses is None else
                            [gt_poses[int(ts[k])] for k in sorted(loop.viewpoints)])
            out["rendering"] = eval_rendering(
                frames, loop.gaussians, PipelineParams(), loop.background, gt_depths=gt_depths, global_scale=out["global_scale"],
                mesh=mesh, mesh_path=os.path.join(out_dir, "mesh.ply") if (mesh and out_dir is not None) else None, c2w=c2w,
                gt_mesh_path=gt_mesh_path, lpips=lpips, **cull)
            if plots:
                from splat_slam_amd.plots import plot_rendering
                ts = self.video.timestamp.cpu().tolist()
                names = [f"video_idx_{k}_kf_idx_{int(ts[k])}" for k in sorted(loop.viewpoints)]
                plot_rendering(frames, loop.gaussians, PipelineParams(), loop.background, out["rendering"],
                               os.path.join(out_dir, "plots_after_refine"), names, gt_depths=gt_depths, global_scale=out["global_scale"])
        if self.video.counter.value > 0 and hasattr(self.stream, "__getitem__") and self.stream[0][2] is not None:
            out["depth_l1"] = self._depth_l1(out["global_scale"], npz)
        filler = lambda: PoseTrajectoryFiller(self.net, self.video, device=self.video.device)
        traj = traj_eval.filled_trajectory(filler(), self.stream) if novel_ids else None      # once: full_traj_eval scores the same rows
        if gt_poses is not None:
            try:
                out["traj_est"], out["full_traj"], out["full_traj_alignment"], *rest = traj_eval.full_traj_eval(
                    filler() if traj is None else None, self.stream, gt_poses, out_dir=out_dir, traj=traj, **plot)
                more("full", rest[0] if rest else {})
            except traj_eval.TrajectoryDegenerate as e:
                out["full_traj_error"] = str(e)
        if novel_ids:
            import lietorch
            from splat_slam_amd.novel_view import eval_novel_views
            c2w = out["traj_est"] if out["traj_est"] is not None else lietorch.SE3(traj).inv().matrix()
            out["novel_views"] = eval_novel_views(self.session, self.stream, c2w, novel_ids, exposure=novel_exposure,
                                                  global_scale=out["global_scale"], lpips=lpips)
        return out

    def _depth_l1(self, global_scale, npz):
        """slam.py:206-216: the sensor-depth error of the video's depth maps, per frame aligned and with the trajectory's scale"""
        with tempfile.TemporaryDirectory() as tmp:
            if npz is None:                            # eval_depth_l1 reads the timestamps of a save_video file only
                npz = os.path.join(tmp, "video.npz")
                np.savez(npz, timestamps=self.video.timestamp[:self.video.counter.value].cpu().numpy())
            l1, l1_4m, coverage = self.video.eval_depth_l1(npz, self.stream)
            l1_g, l1_4m_g, _ = self.video.eval_depth_l1(npz, self.stream, global_scale)
        return {"depth_l1": float(l1), "depth_l1_mask_4m": float(l1_4m), "coverage": float(coverage),
                "depth_l1_global_scale": float(l1_g), "depth_l1_mask_4m_global_scale": float(l1_4m_g)}
