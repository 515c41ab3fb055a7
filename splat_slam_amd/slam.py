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
one batched fusion call (the pose source's prefetch).  The mono-depth network is splat_slam_amd.mono_depth.MonoDepth, itself such a callable.  Not provided: dataset loaders, trajectory
scoring, logging.
"""
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
