"""The keyframe filter of the tracker (MotionFilter of the reference's thirdparty/glorie_slam/motion_filter.py): one RGB frame in, a keyframe
decision out, on this project's kernels alone.

    MotionFilter(net, video, thresh=2.5, mono_depth=None, device="cuda")
        net: a DroidNet (fnet, cnet, update); video: a DepthVideo; mono_depth: None or a callable (tstamp, image [1,3,H,W]) -> [H,W] depth
    filt.track(tstamp, image, intrinsics)
        image [1,3,H,W] in [0, 1] (fp16 or fp32, any strides), intrinsics [4] at image resolution

The ImageNet mean and std go through the encoders' fused pack launch; the image itself is not modified.  The first frame is always
appended, with the identity pose and disparity 1.  A later frame is appended when the mean flow magnitude of one UpdateOperator step on
CorrBlock(fmap of the last keyframe, fmap of the frame) at the identity grid exceeds `thresh`, which resets `count`; otherwise `count`
goes up by one.  The nine items appended are the reference's: (tstamp, image[0], pose, disparity, mono depth, intrinsics / 8, fmap, net,
inp); the context maps are encoded only for frames that are appended.  One difference: the reference's first-frame branch passes
`net[0, 0]`, which after its squeeze is a single channel plane that the video broadcasts over all 128 channels; here both branches store
the whole [128,h,w] maps, as its later-frame branch does.  The single host synchronisation is the `.item()` of the decision, as in the
reference.  splat_slam_amd.mono_depth.MonoDepth is such a mono_depth callable; this project builds no dataset loader.  With mono_depth
None no prior is appended and video.mono_disps keeps its zeros.
"""
import torch

from splat_slam_amd.corr import CorrBlock

__all__ = ["MotionFilter"]

MEAN, STDV = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class MotionFilter:
    def __init__(self, net, video, thresh=2.5, mono_depth=None, device="cuda"):
        self.fnet, self.cnet, self.update = net.fnet, net.cnet, net.update
        self.video, self.thresh, self.mono_depth = video, thresh, mono_depth
        self.device = torch.device(device)
        self.count = 0
        self.net = self.inp = self.fmap = None
        self._identity = torch.tensor([0, 0, 0, 0, 0, 0, 1], dtype=torch.float32, device=self.device)
        self._coords0 = None

    def _coords(self, ht, wd):
        if self._coords0 is None or tuple(self._coords0.shape[2:4]) != (ht, wd):
            y, x = torch.meshgrid(torch.arange(ht, device=self.device).float(), torch.arange(wd, device=self.device).float(), indexing="ij")
            self._coords0 = torch.stack([x, y], dim=-1)[None, None]
        return self._coords0

    def _append(self, tstamp, image, pose, disp, intrinsics, gmap, inputs):
        net, inp = self.cnet.context(inputs, MEAN, STDV)                     # [1,1,128,h,w] each
        self.net, self.inp, self.fmap = net[0], inp[0], gmap
        mono = None if self.mono_depth is None else self.mono_depth(tstamp, image)
        intr = None if intrinsics is None else intrinsics / float(self.video.down_scale)
        self.video.append(tstamp, image[0], pose, disp, mono, intr, gmap, net[0, 0], inp[0, 0])

    @torch.no_grad()
    def track(self, tstamp, image, intrinsics=None):
        """main update operation - run on every frame of the video"""
        if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[0] != 1 or image.shape[1] != 3:
            raise RuntimeError(f"motion_filter: image must be a [1,3,H,W] tensor, got {tuple(getattr(image, 'shape', ()))}")
        image = image.to(self.device)
        inputs = image[None]
        gmap = self.fnet(inputs, MEAN, STDV)[0]                               # [1,128,h,w]
        if self.video.counter.value == 0:
            self._append(tstamp, image, self._identity, 1.0, intrinsics, gmap, inputs)
            return
        ht, wd = gmap.shape[-2:]
        corr = CorrBlock(self.fmap[None, [0]], gmap[None, [0]])(self._coords(ht, wd))
        _, delta, _ = self.update(self.net[None], self.inp[None], corr)
        if delta.float().norm(dim=-1).mean().item() > self.thresh:
            self.count = 0
            self._append(tstamp, image, None, None, intrinsics, gmap, inputs)
        else:
            self.count += 1
