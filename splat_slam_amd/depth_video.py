"""The tracker's keyframe store (DepthVideo, thirdparty/glorie_slam/depth_video.py) on the gfx950 kernels: the factor graph writes into
it, both DSPO stages update it in place, and the mapper reads it through get_depth_and_pose.  New here are the kernels `sgr_video_*`
(include/splat_hip.h, csrc/sgr_video.hip); bundle adjustment and frame geometry are droid_backends, stage 2 is splat_slam_amd.dspo.

    cvx_upsample(disps [N,h,w], inds [n], mask [n,576,h,w] fp16|fp32, out=None) -> disps_up [N,8h,8w]
        convex upsampling of the frames named in inds: out[8y+dy, 8x+dx] = sum_k softmax_k(mask[k*64+dy*8+dx, y, x]) * d[y+ny, x+nx],
        k = 3(ny+1) + (nx+1), zero outside the map.  Only those frames of out are written (out=None: a zero-filled buffer).
    depth_thresh(disps, inds, rel) -> thresh [n] = rel * mean(1 / disp) per frame
    mask_from_counts(disps, inds, counts [n,h,w], visible_num, out [N,h,w] bool|uint8) -> out
        out[inds] = (counts >= visible_num) & (depth < 3 * lower median of the depths with counts >= visible_num)
    valid_depth_mask(poses, disps, intrinsics, inds, rel, visible_num, out) -> out
        depth_thresh -> droid_backends' depth_filter -> mask_from_counts in one call, with no host synchronisation
    DepthVideo(ht, wd, buffer=512, ...) / DepthVideo.from_config(cfg): the reference's class, see its docstring.

inds are distinct int64 frame indices (torch.unique gives them); an index outside [0, N) makes its slot a no-op.  Every tensor lives on
the GPU; there is no CPU path.  All work goes on the current torch stream.  Difference from the reference, deliberate: the softmax
weights of the upsampling stay fp32 for an fp16 mask (under autocast the reference rounds them to fp16 before the multiply).
"""
import contextlib
import types

import numpy as np
import torch

from splat_slam_amd import _native as nat

__all__ = ["cvx_upsample", "depth_thresh", "mask_from_counts", "valid_depth_mask", "DepthVideo"]

_MASK = (torch.bool, torch.uint8)
_UP = 8


def _gpu(name, t, dtype, ndim=None):
    """dtype, rank and layout of one argument; the device is checked by _same_device once every shape is known to be right."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"depth_video: {name} must be a torch.Tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"depth_video: {name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"depth_video: {name} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"depth_video: {name} must be contiguous")
    return t


def _same_device(*ts):
    dev = ts[0].device
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("depth_video (MI355X build): every tensor must be a GPU tensor; there is no CPU path")
    for t in ts[1:]:
        if t.device != dev:
            raise RuntimeError(f"depth_video: every tensor must be on {dev}, found one on {t.device}")
    return dev


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _frames(fn, disps, inds):
    _gpu("disps", disps, torch.float32, 3)
    _gpu("inds", inds, torch.int64, 1)
    n, h, w = disps.shape
    if h < 1 or w < 1:
        raise ValueError(f"depth_video.{fn}: disps must be [N,h,w] with h, w > 0, got {tuple(disps.shape)}")
    if inds.shape[0] > nat.SGR_VIDEO_MAX_FRAMES:
        raise ValueError(f"depth_video.{fn}: {inds.shape[0]} frames in one call exceed the supported {nat.SGR_VIDEO_MAX_FRAMES}")
    return n, h, w, inds.shape[0]


def _scratch(fn, lib, num, h, w, dev):
    nbytes = lib.sgr_video_scratch_bytes(num, h, w)
    if nbytes == 0:
        raise ValueError(f"depth_video.{fn}: unsupported sizes (frames={num} h={h} w={w})")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def cvx_upsample(disps, inds, mask, out=None):
    n, h, w, num = _frames("cvx_upsample", disps, inds)
    _gpu("mask", mask, (torch.float16, torch.float32), 4)
    if tuple(mask.shape) != (num, 9 * _UP * _UP, h, w):
        raise ValueError(f"depth_video.cvx_upsample: mask must be [len(inds),576,h,w] = {(num, 576, h, w)}, got {tuple(mask.shape)}")
    ts = (disps, inds, mask)
    if out is not None:
        _gpu("out", out, torch.float32, 3)
        if tuple(out.shape) != (n, _UP * h, _UP * w):
            raise ValueError(f"depth_video.cvx_upsample: out must be [N,8h,8w] = {(n, _UP * h, _UP * w)}, got {tuple(out.shape)}")
        ts += (out,)
    dev = _same_device(*ts)
    if out is None:
        out = torch.zeros((n, _UP * h, _UP * w), dtype=torch.float32, device=dev)
    if num and n:
        kind = nat.SGR_VIDEO_MASK_F32 if mask.dtype == torch.float32 else nat.SGR_VIDEO_MASK_F16
        with torch.cuda.device(dev):
            nat.check(nat.lib().sgr_video_cvx_upsample(disps.data_ptr(), n, h, w, inds.data_ptr(), num, mask.data_ptr(), kind,
                                                       out.data_ptr(), _stream(dev)), "sgr_video_cvx_upsample")
    return out


def depth_thresh(disps, inds, rel):
    n, h, w, num = _frames("depth_thresh", disps, inds)
    dev = _same_device(disps, inds)
    thresh = torch.empty((num,), dtype=torch.float32, device=dev)
    if num:
        with torch.cuda.device(dev):
            nat.check(nat.lib().sgr_video_depth_thresh(disps.data_ptr(), n, h, w, inds.data_ptr(), num, float(rel), thresh.data_ptr(),
                                                       _stream(dev)), "sgr_video_depth_thresh")
    return thresh


def _mask_out(fn, out, disps):
    _gpu("out", out, _MASK, 3)
    if out.shape != disps.shape:
        raise ValueError(f"depth_video.{fn}: out must have the shape of disps {tuple(disps.shape)}, got {tuple(out.shape)}")


def mask_from_counts(disps, inds, counts, visible_num, out):
    n, h, w, num = _frames("mask_from_counts", disps, inds)
    _gpu("counts", counts, torch.float32, 3)
    if tuple(counts.shape) != (num, h, w):
        raise ValueError(f"depth_video.mask_from_counts: counts must be [len(inds),h,w] = {(num, h, w)}, got {tuple(counts.shape)}")
    _mask_out("mask_from_counts", out, disps)
    visible_num = int(visible_num)
    dev = _same_device(disps, inds, counts, out)
    if num and n:
        lib = nat.lib()
        scratch, nbytes = _scratch("mask_from_counts", lib, num, h, w, dev)
        with torch.cuda.device(dev):
            nat.check(lib.sgr_video_mask_from_counts(disps.data_ptr(), n, h, w, inds.data_ptr(), num, counts.data_ptr(), visible_num,
                                                     out.data_ptr(), scratch.data_ptr(), nbytes, _stream(dev)),
                      "sgr_video_mask_from_counts")
    return out


def valid_depth_mask(poses, disps, intrinsics, inds, rel, visible_num, out):
    n, h, w, num = _frames("valid_depth_mask", disps, inds)
    _gpu("poses", poses, torch.float32, 2)
    _gpu("intrinsics", intrinsics, torch.float32, 1)
    if poses.shape[1] != 7:
        raise ValueError(f"depth_video: poses must be [N,7] (t, q xyzw), got {tuple(poses.shape)}")
    if poses.shape[0] < n:
        raise ValueError(f"depth_video.valid_depth_mask: poses ({poses.shape[0]} rows) must cover the {n} disparity maps")
    if intrinsics.shape[0] != 4:
        raise ValueError(f"depth_video: intrinsics must be [4] (fx, fy, cx, cy), got {tuple(intrinsics.shape)}")
    _mask_out("valid_depth_mask", out, disps)
    rel, visible_num = float(rel), int(visible_num)
    dev = _same_device(poses, disps, intrinsics, inds, out)
    if num and n:
        lib = nat.lib()
        scratch, nbytes = _scratch("valid_depth_mask", lib, num, h, w, dev)
        with torch.cuda.device(dev):
            nat.check(lib.sgr_video_valid_mask(poses.data_ptr(), disps.data_ptr(), n, h, w, intrinsics.data_ptr(), inds.data_ptr(), num,
                                               rel, visible_num, out.data_ptr(), scratch.data_ptr(), nbytes, _stream(dev)),
                      "sgr_video_valid_mask")
    return out


class DepthVideo:
    """Estimated poses and depth maps of the keyframes, with the reference's attribute names, shapes and dtypes (depth_video.py:44-69)
    and its methods: item access (`video[i] = (timestamp, image, pose, disp, mono_depth, intrinsics[, fmap, net, inp])`, `append`),
    `format_indicies`, `set_dirty`, `normalize`, `distance`, `upsample`, `update_valid_depth_mask`, `dspo`, `ba`, `get_pose`,
    `get_depth_and_pose`, `get_depth_scale_and_shift`, `save_video`, `eval_depth_l1`.

    One process: no shared memory; `counter` is an object with `.value` and `get_lock()` a no-op context manager, so glue written for
    the reference runs unchanged.  The multi-view filter's two settings (cfg tracking.multiview_filter.thresh / visible_num) are
    `filter_thresh` and `filter_visible_num`.

    Kept quirk: assigning with a tensor index moves the counter only when `index.max() > counter` (the integer branch compares with
    `>=`), as the reference has it.  Host synchronisations, all of which the reference has too: `update_valid_depth_mask(up=True)`
    finds the dirty frames with one torch.where; `ba` with stage 2 reads one device bool to decide on the fall-back to stage 1; `dspo`
    reads max(ii, jj) when t1 is None.  Stage 2 masks the edges of badly fitting frames on the device and clamps the frames it moved
    (splat_slam_amd.dspo).  Not provided: `reproject` (it belongs with the factor-graph port), a CPU path, multi-process sharing.
    """

    def __init__(self, ht, wd, buffer=512, device="cuda", BA_type="DSPO", mono_thres=0.1, filter_thresh=0.01, filter_visible_num=2):
        ht, wd, buffer = int(ht), int(wd), int(buffer)
        if ht < _UP or wd < _UP or ht % _UP or wd % _UP:
            raise ValueError(f"DepthVideo: ht and wd must be positive multiples of {_UP}, got {ht} x {wd}")
        if buffer < 1:
            raise ValueError(f"DepthVideo: buffer must be >= 1, got {buffer}")
        if BA_type not in ("DSPO", "DBA"):
            raise NotImplementedError(f"DepthVideo: BA_type must be 'DSPO' or 'DBA', got {BA_type!r}")
        device = torch.device(device)               # (the state may be built anywhere; every kernel-backed method needs GPU tensors)
        self.ht, self.wd, self.device, self.down_scale = ht, wd, device, _UP
        self.BA_type, self.mono_thres = BA_type, mono_thres
        self.filter_thresh, self.filter_visible_num = float(filter_thresh), int(filter_visible_num)
        self.counter = types.SimpleNamespace(value=0)
        h, w = ht // _UP, wd // _UP
        z = lambda *shape, dtype=torch.float: torch.zeros(*shape, device=device, dtype=dtype)
        self.timestamp = z(buffer)
        self.images = z(buffer, 3, ht, wd, dtype=torch.uint8)
        self.dirty = z(buffer, dtype=torch.bool)            # valid_depth_mask not yet recomputed for the frame
        self.npc_dirty = z(buffer, dtype=torch.bool)        # the frame's part of the point cloud not yet deformed
        self.poses = z(buffer, 7)
        self.poses[:, 6] = 1.0
        self.disps = torch.ones(buffer, h, w, device=device, dtype=torch.float)
        self.zeros = z(buffer, h, w)
        self.disps_up = z(buffer, ht, wd)
        self.intrinsics = z(buffer, 4)
        self.mono_disps = z(buffer, h, w)
        self.depth_scale = z(buffer)
        self.depth_shift = z(buffer)
        self.valid_depth_mask = z(buffer, ht, wd, dtype=torch.bool)
        self.valid_depth_mask_small = z(buffer, h, w, dtype=torch.bool)
        self.fmaps = z(buffer, 1, 128, h, w, dtype=torch.half)
        self.nets = z(buffer, 128, h, w, dtype=torch.half)
        self.inps = z(buffer, 128, h, w, dtype=torch.half)

    @classmethod
    def from_config(cls, cfg):
        tr = cfg["tracking"]
        return cls(cfg["cam"]["H_out"], cfg["cam"]["W_out"], buffer=tr["buffer"], device=cfg["device"], BA_type=tr["backend"]["BA_type"],
                   mono_thres=tr["mono_thres"], filter_thresh=tr["multiview_filter"]["thresh"],
                   filter_visible_num=tr["multiview_filter"]["visible_num"])

    def get_lock(self):
        return contextlib.nullcontext()

    # ---- item access
    def _item_setter(self, index, item):
        if isinstance(index, int) and index >= self.counter.value:
            self.counter.value = index + 1
        elif isinstance(index, torch.Tensor) and index.max().item() > self.counter.value:
            self.counter.value = index.max().item() + 1
        self.timestamp[index] = item[0]
        self.images[index] = item[1]
        if item[2] is not None:
            self.poses[index] = item[2]
        if item[3] is not None:
            self.disps[index] = item[3]
        if item[4] is not None:
            mono_depth = item[4][self.down_scale // 2 - 1::self.down_scale, self.down_scale // 2 - 1::self.down_scale]
            self.mono_disps[index] = torch.where(mono_depth > 0, 1.0 / mono_depth, 0)
        if item[5] is not None:
            self.intrinsics[index] = item[5]
        if len(item) > 6:
            self.fmaps[index] = item[6]
        if len(item) > 7:
            self.nets[index] = item[7]
        if len(item) > 8:
            self.inps[index] = item[8]

    def __setitem__(self, index, item):
        self._item_setter(index, item)

    def __getitem__(self, index):
        if isinstance(index, int) and index < 0:
            index = self.counter.value + index
        return (self.poses[index], self.disps[index], self.intrinsics[index], self.fmaps[index], self.nets[index], self.inps[index])

    def append(self, *item):
        self._item_setter(self.counter.value, item)

    # ---- geometry
    @staticmethod
    def format_indicies(ii, jj, device="cuda"):
        """to the device, int64, flat"""
        if not isinstance(ii, torch.Tensor):
            ii = torch.as_tensor(ii)
        if not isinstance(jj, torch.Tensor):
            jj = torch.as_tensor(jj)
        return ii.to(device=device, dtype=torch.long).reshape(-1), jj.to(device=device, dtype=torch.long).reshape(-1)

    def set_dirty(self, index_start, index_end):
        self.dirty[index_start:index_end] = True
        self.npc_dirty[index_start:index_end] = True

    def normalize(self):
        n = self.counter.value
        s = self.disps[:n].mean()
        self.disps[:n] /= s
        self.poses[:n, :3] *= s
        self.set_dirty(0, n)

    def distance(self, ii=None, jj=None, beta=0.3, bidirectional=True):
        """frame distance of the edges (ii, jj), or the N x N matrix over the first N = counter frames when ii is None"""
        import droid_backends
        N = None
        if ii is None:
            N = self.counter.value
            ii, jj = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
        ii, jj = self.format_indicies(ii, jj, self.device)
        if bidirectional:
            poses = self.poses[:self.counter.value].clone()
            d1 = droid_backends.frame_distance(poses, self.disps, self.intrinsics[0], ii, jj, beta)
            d2 = droid_backends.frame_distance(poses, self.disps, self.intrinsics[0], jj, ii, beta)
            d = .5 * (d1 + d2)
        else:
            d = droid_backends.frame_distance(self.poses, self.disps, self.intrinsics[0], ii, jj, beta)
        return d if N is None else d.reshape(N, N)

    def upsample(self, ix, mask):
        """disps_up[ix] = convex upsampling of disps[ix]; ix are distinct frame indices, mask is [len(ix),576,h,w] or views to it"""
        if not isinstance(ix, torch.Tensor):
            ix = torch.as_tensor(ix)
        ix = ix.to(device=self.device, dtype=torch.long).reshape(-1).contiguous()
        if not isinstance(mask, torch.Tensor):
            raise TypeError("depth_video: mask must be a torch.Tensor")
        h, w = self.ht // _UP, self.wd // _UP
        if mask.numel() != ix.shape[0] * 9 * _UP * _UP * h * w:
            raise ValueError(f"DepthVideo.upsample: mask must view to [len(ix),576,h,w] = {(ix.shape[0], 576, h, w)}, "
                             f"got {tuple(mask.shape)}")
        cvx_upsample(self.disps, ix, mask.reshape(ix.shape[0], 9 * _UP * _UP, h, w), out=self.disps_up)

    @torch.no_grad()
    def update_valid_depth_mask(self, up=True):
        """The two-view consistency check (eq. 4-7 of the paper).  up=True: the dirty frames at full resolution (intrinsics x 8), whose
        dirty flag is cleared; up=False: frames 0 .. counter-1 at 1/8 resolution, into valid_depth_mask_small."""
        if up:
            dirty_index, = torch.where(self.dirty)          # the one host synchronisation (the reference has it too)
            if dirty_index.shape[0] == 0:
                return
            disps, out, intr = self.disps_up, self.valid_depth_mask, self.intrinsics[0] * float(self.down_scale)
        else:
            if self.counter.value < 1:
                return
            dirty_index = torch.arange(self.counter.value, device=self.device)
            disps, out, intr = self.disps, self.valid_depth_mask_small, self.intrinsics[0].clone()
        valid_depth_mask(self.poses, disps, intr, dirty_index, self.filter_thresh, self.filter_visible_num, out)
        if up:
            self.dirty[dirty_index] = False

    # ---- bundle adjustment
    def dspo(self, target, weight, eta, ii, jj, t0=1, t1=None, itrs=2, lm=1e-4, ep=0.1, motion_only=False, opt_type="pose_depth"):
        """Disparity, Scale and Pose Optimization.  "pose_depth": stage 1 (droid_backends.ba, then the clamp to 1e-5), returns True;
        "depth_scale": stage 2 (update_valid_depth_mask(up=False), then dspo.depth_scale_step), returns the device bool "an edge was
        kept".  target and weight view to [E,h,w,2]."""
        import droid_backends
        from splat_slam_amd import dspo as stage2
        h, w = self.ht // _UP, self.wd // _UP
        if t1 is None:
            t1 = max(ii.max().item(), jj.max().item()) + 1
        if opt_type == "pose_depth":
            target = target.view(-1, h, w, 2).permute(0, 3, 1, 2).contiguous()
            weight = weight.view(-1, h, w, 2).permute(0, 3, 1, 2).contiguous()
            droid_backends.ba(self.poses, self.disps, self.intrinsics[0], self.zeros, target, weight, eta, ii, jj, t0, t1, itrs, lm, ep,
                              motion_only, False)
            self.disps.clamp_(min=1e-5)
            return True
        if opt_type == "depth_scale":
            if self.counter.value < 1:
                return False
            self.update_valid_depth_mask(up=False)
            return stage2.depth_scale_step(self.poses, self.disps, self.intrinsics[0].clone(), self.mono_disps, self.valid_depth_mask_small,
                                           self.depth_scale, self.depth_shift, self.counter.value,
                                           target.view(-1, h, w, 2).contiguous(), weight.view(-1, h, w, 2).contiguous(), eta, ii, jj,
                                           itrs=itrs, lm=lm, ep=ep, mono_thres=self.mono_thres, alpha=0.01)
        raise NotImplementedError(f"DepthVideo.dspo: opt_type must be 'pose_depth' or 'depth_scale', got {opt_type!r}")

    def ba(self, target, weight, eta, ii, jj, t0=1, t1=None, iters=2, lm=1e-4, ep=0.1, motion_only=False, opt_type="pose_depth"):
        if self.BA_type == "DSPO":
            success = self.dspo(target, weight, eta, ii, jj, t0, t1, iters, lm, ep, motion_only, opt_type)
            if not bool(success):                           # stage 2: one device bool read here
                self.dspo(target, weight, eta, ii, jj, t0, t1, iters, lm, ep, motion_only, "pose_depth")
        elif self.BA_type == "DBA":
            self.dspo(target, weight, eta, ii, jj, t0, t1, iters, lm, ep, motion_only, "pose_depth")
        else:
            raise NotImplementedError(f"DepthVideo.ba: BA_type must be 'DSPO' or 'DBA', got {self.BA_type!r}")

    # ---- what the mapper reads
    def get_depth_scale_and_shift(self, index, mono_depth, est_depth, weights):
        """index: int; mono_depth, est_depth, weights: [B,H,W]"""
        from splat_slam_amd import dspo as stage2
        scale, shift, _ = stage2.align_scale_and_shift(mono_depth, est_depth, weights)
        self.depth_scale[index] = scale
        self.depth_shift[index] = shift
        return [self.depth_scale[index], self.depth_shift[index]]

    def get_pose(self, index, device):
        import lietorch
        return lietorch.SE3(self.poses[index].clone()).inv().matrix().to(device)      # camera to world, [4,4]

    def get_depth_and_pose(self, index, device):
        est_depth = 1.0 / self.disps_up[index].clone().to(device)
        depth_mask = self.valid_depth_mask[index].clone().to(device)
        return est_depth, depth_mask, self.get_pose(index, device)

    def save_video(self, path):
        poses, depths, timestamps, masks = [], [], [], []
        for i in range(self.counter.value):
            depth, depth_mask, pose = self.get_depth_and_pose(i, "cpu")
            poses.append(pose)
            depths.append(depth)
            timestamps.append(self.timestamp[i].cpu())
            masks.append(depth_mask)
        np.savez(path, poses=torch.stack(poses, dim=0).numpy(), depths=torch.stack(depths, dim=0).numpy(),
                 timestamps=torch.stack(timestamps, dim=0).numpy(), valid_depth_masks=torch.stack(masks, dim=0).numpy())

    def eval_depth_l1(self, npz_path, stream, global_scale=None):
        """Mean depth L1 of the saved frames against stream[timestamp][2], over all valid pixels and over those with ground truth < 4 m,
        and the mean share of valid pixels.  Without global_scale each depth map is first aligned by scale and shift."""
        from splat_slam_amd import dspo as stage2
        l1, l1_max_4m, share = [], [], []
        video_timestamps = dict(np.load(npz_path))["timestamps"]
        for i in range(video_timestamps.shape[0]):
            valid = self.valid_depth_mask[i]
            share.append((valid.sum() / (valid.shape[0] * valid.shape[1])).cpu().numpy())
            depth_gt = stream[int(video_timestamps[i])][2].to(self.device)
            for limit, acc in ((None, l1), (4, l1_max_4m)):
                mask = torch.logical_and(depth_gt > 0, valid)
                if limit is not None:
                    mask = torch.logical_and(depth_gt < limit, mask)
                depth = 1 / self.disps_up[i]
                depth[mask == 0] = 0
                if global_scale is None:
                    scale, shift, _ = stage2.align_scale_and_shift(depth.unsqueeze(0).contiguous(), depth_gt.unsqueeze(0).contiguous(),
                                                                   mask.unsqueeze(0).contiguous())
                    depth = scale * depth + shift
                else:
                    depth = global_scale * depth
                acc.append((torch.abs(depth[mask] - depth_gt[mask]).sum() / mask.sum()).cpu().numpy())
        return np.asarray(l1).mean(), np.asarray(l1_max_4m).mean(), np.asarray(share).mean()
