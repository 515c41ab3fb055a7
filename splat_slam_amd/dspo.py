"""Stage 2 ("depth_scale") of the reference tracker's DSPO bundle adjustment (DepthVideo.dspo, thirdparty/glorie_slam/depth_video.py:236-299)
on the gfx950 kernels `sgr_dspo_*` (include/splat_hip.h, csrc/sgr_dspo.hip).  Stage 1 ("pose_depth") is droid_backends.ba.

    align_scale_and_shift(prediction, target, weights=None) -> (scale [n], shift [n], avg_error [n])
        weighted least squares of scale * prediction + shift against target per frame ([n,h,w] or [h,w]; weights float32 or bool)
    ba_with_scale_shift(target, weight, eta, poses, disps, intrinsics, ii, jj, mono_disps, scales, shifts, valid_depth_mask,
                        ignore_frames=0, lm=1e-4, ep=0.1, alpha=1.0, iterations=1, edge_keep=None) -> (dwq [M,2], dz [M,h*w])
        Gauss-Newton over the disparities of the frames kx = sorted unique(ii) and their scales and shifts, poses fixed; disps [N,h,w],
        scales [N] and shifts [N] are updated in place.  target and weight are [E,h,w,2], as the factor graph holds them.
    align_and_mask(disps, mono_disps, valid_depth_mask, scales, shifts, n_frames, ii, jj, mono_thres=0.1) -> edge_keep [E] (bool)
        fits the first n_frames mono maps to the disparities, writes the fit into scales and shifts, and marks the edges of badly
        fitting frames (error / mean disparity > mono_thres, NaN, scale < 0, fewer than half the pixels valid)
    depth_scale_step(poses, disps, intrinsics, mono_disps, valid_depth_mask, scales, shifts, n_frames, target, weight, eta, ii, jj,
                     itrs=2, lm=1e-4, ep=0.1, mono_thres=0.1, alpha=0.01) -> any_kept (0-dim bool tensor on the device)
        the whole stage-2 branch: align_and_mask, itrs iterations of ba_with_scale_shift, the final clamp to >= 1e-5.  An edge with a
        frame outside [0, min(N, len(poses))) takes part in nothing: it moves no frame and does not count as kept.

Poses are (t, q xyzw), world to camera.  Every tensor lives on the GPU; there is no CPU path.  All work goes on the current torch stream
and nothing synchronises with the host: M is eta.shape[0]; if it differs from the number of distinct ii, nothing is updated and dwq, dz
come back as NaN.  Differences from the reference, all deliberate: a frame whose reduced 2 x 2 system is not positive definite gets a
zero step on its own (the reference factors every frame as one matrix and zeroes them all); edges are masked (edge_keep) instead of
removed on the host; depth_scale_step clamps the disparities of the frames it moved (the reference clamps the whole buffer, whose other
frames stage 1 has clamped already).  What is not provided: a batch dimension, the Python dense BA and MoBA of geom/ba.py.  The two-view
consistency mask (update_valid_depth_mask) and the class around all of this are splat_slam_amd.depth_video.
"""
import ctypes as C

import torch

from splat_slam_amd import _native as nat

__all__ = ["align_scale_and_shift", "ba_with_scale_shift", "align_and_mask", "depth_scale_step"]


def _gpu(name, t, dtype, ndim=None):
    """dtype, rank and layout of one argument; the device is checked by _same_device once every shape is known to be right."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"dspo: {name} must be a torch.Tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"dspo: {name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"dspo: {name} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"dspo: {name} must be contiguous")
    return t


def _same_device(*ts):
    dev = ts[0].device
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("dspo (MI355X build): every tensor must be a GPU tensor; there is no CPU path")
    for t in ts[1:]:
        if t.device != dev:
            raise RuntimeError(f"dspo: every tensor must be on {dev}, found one on {t.device}")
    return dev


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


_MASK = (torch.bool, torch.uint8)


def _align(prediction, target, weights):
    """out [n,3] = (scale, shift, avg_error) of [n,h,w] inputs."""
    _gpu("prediction", prediction, torch.float32, 3)
    _gpu("target", target, torch.float32, 3)
    if target.shape != prediction.shape:
        raise ValueError(f"dspo.align_scale_and_shift: target must have the shape of prediction {tuple(prediction.shape)}, "
                         f"got {tuple(target.shape)}")
    kind, ts = nat.SGR_DSPO_WEIGHTS_NONE, (prediction, target)
    if weights is not None:
        _gpu("weights", weights, (torch.float32,) + _MASK, 3)
        if weights.shape != prediction.shape:
            raise ValueError(f"dspo.align_scale_and_shift: weights must have the shape of prediction {tuple(prediction.shape)}, "
                             f"got {tuple(weights.shape)}")
        kind = nat.SGR_DSPO_WEIGHTS_F32 if weights.dtype == torch.float32 else nat.SGR_DSPO_WEIGHTS_U8
        ts += (weights,)
    n, h, w = prediction.shape
    if h * w < 1:
        raise ValueError(f"dspo.align_scale_and_shift: prediction must be [n,h,w] with h, w > 0, got {tuple(prediction.shape)}")
    dev = _same_device(*ts)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n:
        with torch.cuda.device(dev):
            nat.check(nat.lib().sgr_dspo_align(prediction.data_ptr(), target.data_ptr(), nat.ptr(weights), kind, n, h * w, out.data_ptr(),
                                               _stream(dev)), "sgr_dspo_align")
    return out


def align_scale_and_shift(prediction, target, weights=None):
    if isinstance(prediction, torch.Tensor) and prediction.dim() == 2:
        if not isinstance(target, torch.Tensor) or target.dim() != 2 or (isinstance(weights, torch.Tensor) and weights.dim() != 2):
            raise ValueError("dspo.align_scale_and_shift: with a [h,w] prediction, target and weights must be [h,w] as well")
        prediction, target = prediction.unsqueeze(0), target.unsqueeze(0)
        weights = None if weights is None else weights.unsqueeze(0)
    out = _align(prediction, target, weights)
    return out[:, 0], out[:, 1], out[:, 2]


def ba_with_scale_shift(target, weight, eta, poses, disps, intrinsics, ii, jj, mono_disps, scales, shifts, valid_depth_mask,
                        ignore_frames=0, lm=1e-4, ep=0.1, alpha=1.0, iterations=1, edge_keep=None):
    _gpu("poses", poses, torch.float32, 2)
    _gpu("disps", disps, torch.float32, 3)
    _gpu("intrinsics", intrinsics, torch.float32, 1)
    if poses.shape[1] != 7:
        raise ValueError(f"dspo: poses must be [N,7] (t, q xyzw), got {tuple(poses.shape)}")
    if intrinsics.shape[0] != 4:
        raise ValueError(f"dspo: intrinsics must be [4] (fx, fy, cx, cy), got {tuple(intrinsics.shape)}")
    n, h, w = disps.shape
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"dspo: disps must be [N,h,w] with N, h, w > 0, got {tuple(disps.shape)}")
    _gpu("ii", ii, torch.int64, 1)
    _gpu("jj", jj, torch.int64, 1)
    if ii.shape != jj.shape:
        raise ValueError(f"dspo: ii and jj must have the same length, got {ii.shape[0]} and {jj.shape[0]}")
    E = ii.shape[0]
    if E < 1:
        raise ValueError("dspo.ba_with_scale_shift: the edge list is empty")
    _gpu("target", target, torch.float32, 4)
    _gpu("weight", weight, torch.float32, 4)
    for name, t in (("target", target), ("weight", weight)):
        if tuple(t.shape) != (E, h, w, 2):
            raise ValueError(f"dspo.ba_with_scale_shift: {name} must be [E,h,w,2] = {(E, h, w, 2)}, got {tuple(t.shape)}")
    _gpu("eta", eta, torch.float32, 3)
    if eta.shape[1:] != (h, w) or eta.shape[0] < 1:
        raise ValueError(f"dspo.ba_with_scale_shift: eta must be [M,{h},{w}], got {tuple(eta.shape)}")
    _gpu("mono_disps", mono_disps, torch.float32, 3)
    _gpu("valid_depth_mask", valid_depth_mask, _MASK, 3)
    for name, t in (("mono_disps", mono_disps), ("valid_depth_mask", valid_depth_mask)):
        if t.shape != disps.shape:
            raise ValueError(f"dspo.ba_with_scale_shift: {name} must have the shape of disps {tuple(disps.shape)}, got {tuple(t.shape)}")
    _gpu("scales", scales, torch.float32, 1)
    _gpu("shifts", shifts, torch.float32, 1)
    for name, t in (("scales", scales), ("shifts", shifts)):
        if t.shape[0] != n:
            raise ValueError(f"dspo.ba_with_scale_shift: {name} must be [N] = ({n},), got {tuple(t.shape)}")
    ts = (poses, disps, intrinsics, ii, jj, target, weight, eta, mono_disps, valid_depth_mask, scales, shifts)
    if edge_keep is not None:
        _gpu("edge_keep", edge_keep, _MASK, 1)
        if edge_keep.shape[0] != E:
            raise ValueError(f"dspo.ba_with_scale_shift: edge_keep must be [E] = ({E},), got {tuple(edge_keep.shape)}")
        ts += (edge_keep,)
    iterations, ignore_frames, alpha = int(iterations), int(ignore_frames), float(alpha)
    if iterations < 0:
        raise ValueError(f"dspo.ba_with_scale_shift: iterations must be >= 0, got {iterations}")
    if not alpha >= 0.0:
        raise ValueError(f"dspo.ba_with_scale_shift: alpha must be >= 0, got {alpha}")
    dev = _same_device(*ts)
    M = eta.shape[0]
    if iterations == 0:
        return torch.zeros((M, 2), dtype=torch.float32, device=dev), torch.zeros((M, h * w), dtype=torch.float32, device=dev)
    dwq = torch.empty((M, 2), dtype=torch.float32, device=dev)
    dz = torch.empty((M, h * w), dtype=torch.float32, device=dev)
    lib = nat.lib()
    nv = min(n, poses.shape[0])
    nbytes = lib.sgr_dspo_scratch_bytes(nv, E, M, h, w)
    if nbytes == 0:
        raise ValueError(f"dspo.ba_with_scale_shift: unsupported sizes (frames={nv} edges={E} M={M} h={h} w={w})")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pr = nat.SgrDspoProblem(poses.data_ptr(), poses.shape[0], disps.data_ptr(), n, h, w, intrinsics.data_ptr(), mono_disps.data_ptr(),
                            valid_depth_mask.data_ptr(), scales.data_ptr(), shifts.data_ptr(), target.data_ptr(), weight.data_ptr(),
                            eta.data_ptr(), ii.data_ptr(), jj.data_ptr(), nat.ptr(edge_keep), E, M, ignore_frames, iterations, float(lm),
                            float(ep), alpha, dwq.data_ptr(), dz.data_ptr())
    with torch.cuda.device(dev):
        nat.check(lib.sgr_dspo_ba(C.byref(pr), scratch.data_ptr(), nbytes, _stream(dev)), "sgr_dspo_ba")
    return dwq, dz


def align_and_mask(disps, mono_disps, valid_depth_mask, scales, shifts, n_frames, ii, jj, mono_thres=0.1):
    """Steps 1 and 2 of depth_scale_step: fits the first n_frames mono maps to the disparities (weights: valid_depth_mask), writes the
    fit into scales and shifts, and returns edge_keep [E] (bool): False for every edge that touches a frame whose fit is bad."""
    _gpu("disps", disps, torch.float32, 3)
    _gpu("mono_disps", mono_disps, torch.float32, 3)
    _gpu("valid_depth_mask", valid_depth_mask, _MASK, 3)
    _gpu("scales", scales, torch.float32, 1)
    _gpu("shifts", shifts, torch.float32, 1)
    _gpu("ii", ii, torch.int64, 1)
    _gpu("jj", jj, torch.int64, 1)
    n, h, w = disps.shape
    n_frames = int(n_frames)
    if not 1 <= n_frames <= n:
        raise ValueError(f"dspo: n_frames must lie in [1, {n}], got {n_frames}")
    if mono_disps.shape != disps.shape or valid_depth_mask.shape != disps.shape or scales.shape[0] != n or shifts.shape[0] != n:
        raise ValueError(f"dspo: mono_disps, valid_depth_mask must be {tuple(disps.shape)} and scales, shifts ({n},), got "
                         f"{tuple(mono_disps.shape)}, {tuple(valid_depth_mask.shape)}, {tuple(scales.shape)}, {tuple(shifts.shape)}")
    if ii.shape != jj.shape:
        raise ValueError(f"dspo: ii and jj must have the same length, got {ii.shape[0]} and {jj.shape[0]}")
    _same_device(disps, mono_disps, valid_depth_mask, scales, shifts, ii, jj)
    est, valid = disps[:n_frames], valid_depth_mask[:n_frames]
    fit = _align(mono_disps[:n_frames], est, valid)
    scales[:n_frames] = fit[:, 0]
    shifts[:n_frames] = fit[:, 1]
    bad = torch.zeros(n, dtype=torch.bool, device=disps.device)
    if mono_thres:
        err = fit[:, 2]
        bad[:n_frames] = ((err / est.mean(dim=[1, 2]) > mono_thres) | err.isnan() | (fit[:, 0] < 0)
                          | (valid.sum(dim=[1, 2]) < h * w * 0.5))
    return ~(bad[ii.clamp(0, n - 1)] | bad[jj.clamp(0, n - 1)])


def depth_scale_step(poses, disps, intrinsics, mono_disps, valid_depth_mask, scales, shifts, n_frames, target, weight, eta, ii, jj,
                     itrs=2, lm=1e-4, ep=0.1, mono_thres=0.1, alpha=0.01):
    keep = align_and_mask(disps, mono_disps, valid_depth_mask, scales, shifts, n_frames, ii, jj, mono_thres)
    ba_with_scale_shift(target, weight, eta, poses, disps, intrinsics, ii, jj, mono_disps, scales, shifts, valid_depth_mask, 0, lm, ep,
                        alpha, itrs, keep)
    # an edge with a frame outside [0, nv) takes part in nothing in the kernels: it moves no frame here either
    n = disps.shape[0]
    nv = min(n, poses.shape[0])
    keep = keep & (ii >= 0) & (ii < nv) & (jj >= 0) & (jj < nv)
    moved = torch.zeros(n, dtype=torch.int32, device=disps.device).index_add_(0, ii.clamp(0, n - 1), keep.to(torch.int32)) > 0
    disps.copy_(torch.where(moved[:, None, None], disps.clamp(min=1e-5), disps))
    return keep.any()
