"""Poses for the frames between the keyframes (PoseTrajectoryFiller of the reference's thirdparty/glorie_slam/trajectory_filler.py): every
frame of a stream starts from the constant-velocity interpolation of its two bracketing keyframes and is refined, pose only, against
them with the update operator.  Stated in DESIGN.md section 3, "Tracker".

    bracket(ts [N], tt [M]) -> (t0 [M], t1 [M]) int64
        t0 = #{ts <= t} - 1, t1 = t0 + 1 where t0 < N - 1 and t0 elsewhere: a timestamp after the last keyframe gets t0 = t1 = N - 1, one
        before the first gets t0 = -1, t1 = 0.  Plain torch on the device of ts.
    PoseTrajectoryFiller(net, video, device="cuda")
        net: a DroidNet (net.fnet, net.update); video: a DepthVideo with N = video.counter.value keyframes.  One more keyword,
        corr_impl="volume": the correlation operator of the graph of each block of frames, "volume" or "volume_fused" (FactorGraph)
    filler.interpolate(timestamps) -> [M,7]
        exp(log(P[t1] * P[t0]^-1) / dt * (t - ts[t0])) * P[t0] with dt = ts[t1] - ts[t0] + 1e-3, through lietorch.SE3: at a keyframe's
        timestamp exactly that keyframe's pose; after the last keyframe (t0 = t1) the last pose up to the rounding of P * P^-1, which
        dt = 1e-3 magnifies by (t - ts[t0]) * 1000, as in the reference.
    filler(stream) -> [T,7]
        stream yields (timestamp, image [1,3,H,W] in [0, 1], ...) and has get_intrinsic() -> [4] at image resolution.  Frames are taken
        16 at a time: encoded with fnet (ImageNet mean and std through the encoder's pack launch), written behind the keyframes into
        video[N:N+M] with the counter raised, connected to both bracketing keyframes (edges keyframe -> frame), refined by 12
        graph.update(N, N + M, motion_only=True), read back, and the counter lowered again.  ValueError when N + 16 exceeds the buffer.

Kept from the reference: t0 = -1 wraps to the last keyframe, as its negative index does (the first frame of a sequence is always a
keyframe, so no frame of the tracked stream precedes it); here the edge of such a frame starts at that same keyframe.  The slots
[N, N + 16) of the video and disps_up of the bracketing keyframes are overwritten; poses and disparities of the keyframes are not.
The brackets are counted on the device: no host synchronisation besides those of FactorGraph (the reference reads one count per frame).
"""
import torch

from splat_slam_amd.factor_graph import FactorGraph
from splat_slam_amd.motion_filter import MEAN, STDV

__all__ = ["bracket", "PoseTrajectoryFiller"]

BLOCK = 16


def bracket(ts, tt):
    n = ts.shape[0]
    t0 = (ts[None, :] <= tt[:, None]).sum(dim=1) - 1
    t1 = torch.where(t0 < n - 1, t0 + 1, t0)
    return t0, t1


class PoseTrajectoryFiller:
    def __init__(self, net, video, device="cuda", corr_impl="volume"):
        if corr_impl not in ("volume", "volume_fused"):
            raise ValueError(f"PoseTrajectoryFiller: corr_impl must be 'volume' or 'volume_fused', got {corr_impl!r}")
        self.fnet, self.update, self.corr_impl = net.fnet, net.update, corr_impl
        self.count = 0
        self.video, self.device = video, device

    def _bracket(self, tt):
        n = self.video.counter.value
        if n < 1:
            raise ValueError("PoseTrajectoryFiller: the video holds no keyframe")
        ts = self.video.timestamp[:n]
        t0, t1 = bracket(ts, tt)
        return ts, t0 % n, t1

    def _interpolate(self, tt):
        from lietorch import SE3
        ts, t0, t1 = self._bracket(tt)
        Ps = SE3(self.video.poses[:self.video.counter.value])
        dt = ts[t1] - ts[t0] + 1e-3
        dP = Ps[t1] * Ps[t0].inv()
        v = dP.log() / dt.unsqueeze(dim=-1)
        w = v * (tt - ts[t0]).unsqueeze(dim=-1)
        return (SE3.exp(w) * Ps[t0]).data, t0, t1

    @torch.no_grad()
    def interpolate(self, timestamps):
        tt = torch.as_tensor(timestamps, dtype=torch.float32, device=self.device).reshape(-1)
        return self._interpolate(tt)[0]

    def _fill(self, timestamps, images, intrinsic):
        tt = torch.as_tensor(timestamps, dtype=torch.float32, device=self.device)
        inputs = torch.stack(images, dim=0).to(self.device)                   # [M,1,3,H,W]
        N, M = self.video.counter.value, len(timestamps)
        Gs, t0, t1 = self._interpolate(tt)
        fmap = self.fnet(inputs, MEAN, STDV)                                  # no context features: the edges start at keyframes
        # the frames sit behind the keyframes while they are optimised
        self.video.counter.value += M
        intrinsics = (intrinsic.to(self.device) / float(self.video.down_scale)).expand(M, 4)
        self.video[N:N + M] = (tt, inputs[:, 0], Gs, 1, None, intrinsics, fmap)
        graph = FactorGraph(self.video, self.update, device=self.device, corr_impl=self.corr_impl)
        frames = torch.arange(N, N + M, device=self.device)
        graph.add_factors(t0, frames)
        graph.add_factors(t1, frames)
        for _ in range(12):
            graph.update(N, N + M, motion_only=True)
        Gs = self.video.poses[N:N + M].clone()
        self.video.counter.value -= M
        self.count += M
        return Gs

    @torch.no_grad()
    def __call__(self, stream):
        """fill in poses of non-keyframe images"""
        N = self.video.counter.value
        if N + BLOCK > self.video.poses.shape[0]:
            raise ValueError(f"PoseTrajectoryFiller: {N} keyframes and a block of {BLOCK} frames exceed the video buffer of "
                             f"{self.video.poses.shape[0]}")
        intrinsic = stream.get_intrinsic()
        poses, timestamps, images = [], [], []
        for item in stream:
            timestamps.append(item[0])
            images.append(item[1])
            if len(timestamps) == BLOCK:
                poses.append(self._fill(timestamps, images, intrinsic))
                timestamps, images = [], []
        if timestamps:
            poses.append(self._fill(timestamps, images, intrinsic))
        if not poses:
            return torch.zeros((0, 7), dtype=torch.float32, device=self.device)
        return torch.cat(poses, dim=0)
