"""The tracking loop (Tracker of the reference's src/tracker.py): every frame of a stream goes through the motion filter and the frontend,
the backend runs a global bundle adjustment every `ba_freq` keyframes, and the mapper is told about finished keyframes.  Stated in
DESIGN.md section 3, "Tracker".

    Tracker(cfg, net, video, on_keyframe=None, only_tracking=False)
        cfg: the reference's dict, read at cfg["device"], cfg["tracking"]["motion_filter"]["thresh"],
        cfg["tracking"]["frontend"][window, enable_online_ba], cfg["tracking"]["backend"]["ba_freq"], cfg["mapping"]["every_keyframe"]
        (and what Frontend and Backend read); net: a DroidNet; video: a DepthVideo.  Attributes: motion_filter, frontend, online_ba.
        One more keyword, mono_depth=None: the mono-depth callable that is passed on to MotionFilter.
        frontend_corr_impl="volume": the correlation operator of the frontend's graph, passed on to Frontend ("volume_fused": one
        FusedCorrBlock over video.fmaps).  The motion filter keeps CorrBlock: its one edge is not in the video.
    tracker.run(stream)
        stream: len(stream), stream[i] -> (timestamp, image [1,3,H,W] in [0, 1], ...), stream.get_intrinsic() -> [4].
        Per frame: motion_filter.track(timestamp, image, intrinsic), then frontend().  When the index of the newest keyframe has
        changed and the frontend is initialised: online_ba.dense_ba(2) if enable_online_ba and ba_freq keyframe indices have passed
        since the last one, and on_keyframe(video_idx, timestamp) for every every_keyframe-th such frame.  on_keyframe(None, None)
        ends the run.  With only_tracking (or without a callback) nothing is called.

The callback stands where the reference sends a message through a pipe to the mapping process and waits for its answer: it returns
when the mapper is done with the keyframe (splat_slam_amd.session runs the mapper in the same process).
"""
import torch

from splat_slam_amd.backend import Backend
from splat_slam_amd.frontend import Frontend
from splat_slam_amd.motion_filter import MotionFilter

__all__ = ["Tracker"]


class Tracker:
    def __init__(self, cfg, net, video, on_keyframe=None, only_tracking=False, mono_depth=None, frontend_corr_impl="volume"):
        self.cfg, self.net, self.video, self.device = cfg, net, video, cfg["device"]
        self.on_keyframe, self.only_tracking = on_keyframe, only_tracking
        tr = cfg["tracking"]
        self.frontend_window = tr["frontend"]["window"]
        prior = {} if mono_depth is None else {"mono_depth": mono_depth}     # without one the filter is built exactly as before
        self.motion_filter = MotionFilter(net, video, thresh=tr["motion_filter"]["thresh"], device=self.device, **prior)
        self.enable_online_ba = tr["frontend"]["enable_online_ba"]
        self.every_kf = cfg["mapping"]["every_keyframe"]
        front = {} if frontend_corr_impl == "volume" else {"corr_impl": frontend_corr_impl}     # the default builds it exactly as before
        self.frontend = Frontend(net, video, cfg, **front)
        self.online_ba = Backend(net, video, cfg)
        self.ba_freq = tr["backend"]["ba_freq"]

    def _notify(self, video_idx, timestamp):
        if not self.only_tracking and self.on_keyframe is not None:
            self.on_keyframe(video_idx, timestamp)

    def run(self, stream):
        prev_kf_idx = prev_ba_idx = number_of_kf = 0
        intrinsic = stream.get_intrinsic()
        for i in range(len(stream)):
            item = stream[i]
            timestamp, image = item[0], item[1]
            with torch.no_grad():
                self.motion_filter.track(timestamp, image, intrinsic)     # is there enough motion for a keyframe
                self.frontend()                                           # local bundle adjustment
            curr_kf_idx = self.video.counter.value - 1
            if curr_kf_idx != prev_kf_idx and self.frontend.is_initialized:
                number_of_kf += 1
                if self.enable_online_ba and curr_kf_idx >= prev_ba_idx + self.ba_freq:
                    self.online_ba.dense_ba(2)
                    prev_ba_idx = curr_kf_idx
                if number_of_kf % self.every_kf == 0:
                    self._notify(curr_kf_idx, timestamp)
            prev_kf_idx = curr_kf_idx
        self._notify(None, None)
