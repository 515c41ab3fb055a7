"""Drop-in for the `droid_backends` extension of the reference tracker (thirdparty/glorie_slam/lib/droid.cpp), imported by
thirdparty/glorie_slam/depth_video.py.  Backed by the gfx950 kernels `sgr_dba_*` (include/splat_hip.h, csrc/sgr_dba.hip).

    ba(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, t0, t1, iterations, lm, ep, motion_only, depth_only)
        -> [dx, dz]; poses [N,7] and disps [N,h,w] are updated in place (dz is None with motion_only, as in the reference)
    frame_distance(poses, disps, intrinsics, ii, jj, beta) -> dist [E]
    projmap(poses, disps, intrinsics, ii, jj) -> [coords [E,h,w,3], valid [E,h,w,1]]
    depth_filter(poses, disps, intrinsics, ix, thresh) -> counts [len(ix),h,w]
    iproj(poses, disps, intrinsics) -> points [N,h,w,3]

Poses are (t, q xyzw), world to camera.  Every tensor lives on the GPU; there is no CPU path.  All work goes on the current torch
stream, and ba issues no host synchronisation: the number K of depth frames is eta.shape[0].  If that differs from the number of
distinct frames in cat([t0, t1), ii), nothing is updated and dx, dz come back as NaN.  The window t1 - t0 is limited to 512 frames.

The correlation kernels of the same extension (altcorr_forward / altcorr_backward, corr_index_forward / corr_index_backward) belong
to the DROID network and are not provided here.
"""
import ctypes as C

import torch

from splat_slam_amd import _native as nat

__all__ = ["ba", "frame_distance", "projmap", "depth_filter", "iproj"]


def _gpu(name, t, dtype, ndim=None):
    """dtype, rank and layout of one argument; the device is checked by _same_device once every shape is known to be right."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"droid_backends: {name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"droid_backends: {name} must be {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"droid_backends: {name} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"droid_backends: {name} must be contiguous")
    return t


def _same_device(*ts):
    dev = ts[0].device
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("droid_backends (MI355X build): every tensor must be a GPU tensor; there is no CPU path")
    for t in ts[1:]:
        if t.device != dev:
            raise RuntimeError(f"droid_backends: every tensor must be on {dev}, found one on {t.device}")
    return dev


def _geometry(poses, disps, intrinsics):
    _gpu("poses", poses, torch.float32, 2)
    _gpu("disps", disps, torch.float32, 3)
    _gpu("intrinsics", intrinsics, torch.float32, 1)
    if poses.shape[1] != 7:
        raise ValueError(f"droid_backends: poses must be [N,7] (t, q xyzw), got {tuple(poses.shape)}")
    if intrinsics.shape[0] != 4:
        raise ValueError(f"droid_backends: intrinsics must be [4] (fx, fy, cx, cy), got {tuple(intrinsics.shape)}")
    n, h, w = disps.shape
    if h <= 0 or w <= 0:
        raise ValueError(f"droid_backends: disps must be [N,h,w] with h, w > 0, got {tuple(disps.shape)}")
    return n, h, w


def _edges(ii, jj):
    _gpu("ii", ii, torch.int64, 1)
    _gpu("jj", jj, torch.int64, 1)
    if ii.shape != jj.shape:
        raise ValueError(f"droid_backends: ii and jj must have the same length, got {ii.shape[0]} and {jj.shape[0]}")
    return ii.shape[0]


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def ba(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, t0, t1, iterations, lm, ep, motion_only, depth_only):
    n, h, w = _geometry(poses, disps, intrinsics)
    E = _edges(ii, jj)
    _gpu("disps_sens", disps_sens, torch.float32, 3)
    _gpu("targets", targets, torch.float32, 4)
    _gpu("weights", weights, torch.float32, 4)
    _gpu("eta", eta, torch.float32, 3)
    if disps_sens.shape != disps.shape:
        raise ValueError(f"droid_backends.ba: disps_sens must have the shape of disps {tuple(disps.shape)}, got {tuple(disps_sens.shape)}")
    for name, t in (("targets", targets), ("weights", weights)):
        if tuple(t.shape) != (E, 2, h, w):
            raise ValueError(f"droid_backends.ba: {name} must be [E,2,h,w] = {(E, 2, h, w)}, got {tuple(t.shape)}")
    if eta.shape[1:] != (h, w) or eta.shape[0] < 1:
        raise ValueError(f"droid_backends.ba: eta must be [K,{h},{w}], got {tuple(eta.shape)}")
    if E < 1:
        raise ValueError("droid_backends.ba: the edge list is empty")
    t0, t1, iterations = int(t0), int(t1), int(iterations)
    nv = min(n, poses.shape[0])
    if not (0 <= t0 < t1 <= nv):
        raise ValueError(f"droid_backends.ba: window [t0, t1) = [{t0}, {t1}) must be non-empty and inside the {nv} frames")
    if t1 - t0 > nat.SGR_DBA_MAX_WINDOW:
        raise ValueError(f"droid_backends.ba: window of {t1 - t0} frames exceeds the supported {nat.SGR_DBA_MAX_WINDOW}")
    dev = _same_device(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj)
    if iterations < 1:
        return [None, None]
    K = eta.shape[0]
    motion_only, depth_only = bool(motion_only), bool(depth_only)
    dx = torch.empty((t1 - t0, 6), dtype=torch.float32, device=dev)
    dz = None if motion_only else torch.empty((K, h * w), dtype=torch.float32, device=dev)
    lib = nat.lib()
    nbytes = lib.sgr_dba_scratch_bytes(nv, E, K, t1 - t0, h, w)
    if nbytes == 0:
        raise ValueError(f"droid_backends.ba: unsupported sizes (frames={nv} edges={E} K={K} window={t1 - t0} h={h} w={w})")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pr = nat.SgrDbaProblem(poses.data_ptr(), poses.shape[0], disps.data_ptr(), n, h, w, intrinsics.data_ptr(), disps_sens.data_ptr(),
                           targets.data_ptr(), weights.data_ptr(), eta.data_ptr(), ii.data_ptr(), jj.data_ptr(), E, K, t0, t1,
                           iterations, float(lm), float(ep), int(motion_only), int(depth_only), dx.data_ptr(),
                           None if dz is None else dz.data_ptr())
    with torch.cuda.device(dev):
        nat.check(lib.sgr_dba_ba(C.byref(pr), scratch.data_ptr(), nbytes, _stream(dev)), "sgr_dba_ba")
    return [dx, dz]


def frame_distance(poses, disps, intrinsics, ii, jj, beta):
    n, h, w = _geometry(poses, disps, intrinsics)
    E = _edges(ii, jj)
    dev = _same_device(poses, disps, intrinsics, ii, jj)
    dist = torch.empty((E,), dtype=torch.float32, device=dev)
    if E == 0:
        return dist
    with torch.cuda.device(dev):
        nat.check(nat.lib().sgr_dba_frame_distance(poses.data_ptr(), poses.shape[0], disps.data_ptr(), n, h, w, intrinsics.data_ptr(),
                                                   ii.data_ptr(), jj.data_ptr(), E, float(beta), dist.data_ptr(), _stream(dev)),
                  "sgr_dba_frame_distance")
    return dist


def projmap(poses, disps, intrinsics, ii, jj):
    n, h, w = _geometry(poses, disps, intrinsics)
    E = _edges(ii, jj)
    dev = _same_device(poses, disps, intrinsics, ii, jj)
    coords = torch.empty((E, h, w, 3), dtype=torch.float32, device=dev)
    valid = torch.empty((E, h, w, 1), dtype=torch.float32, device=dev)
    if E == 0:
        return [coords, valid]
    with torch.cuda.device(dev):
        nat.check(nat.lib().sgr_dba_projmap(poses.data_ptr(), poses.shape[0], disps.data_ptr(), n, h, w, intrinsics.data_ptr(),
                                            ii.data_ptr(), jj.data_ptr(), E, coords.data_ptr(), valid.data_ptr(), _stream(dev)),
                  "sgr_dba_projmap")
    return [coords, valid]


def depth_filter(poses, disps, intrinsics, ix, thresh):
    n, h, w = _geometry(poses, disps, intrinsics)
    _gpu("ix", ix, torch.int64, 1)
    _gpu("thresh", thresh, torch.float32, 1)
    if thresh.shape[0] != ix.shape[0]:
        raise ValueError(f"droid_backends.depth_filter: thresh must have one entry per index ({ix.shape[0]}), got {thresh.shape[0]}")
    if poses.shape[0] < n:
        raise ValueError(f"droid_backends.depth_filter: poses ({poses.shape[0]} rows) must cover the {n} disparity maps")
    dev = _same_device(poses, disps, intrinsics, ix, thresh)
    counter = torch.empty((ix.shape[0], h, w), dtype=torch.float32, device=dev)
    if ix.shape[0] == 0:
        return counter
    with torch.cuda.device(dev):
        nat.check(nat.lib().sgr_dba_depth_filter(poses.data_ptr(), disps.data_ptr(), n, h, w, intrinsics.data_ptr(), ix.data_ptr(),
                                                 ix.shape[0], thresh.data_ptr(), counter.data_ptr(), _stream(dev)),
                  "sgr_dba_depth_filter")
    return counter


def iproj(poses, disps, intrinsics):
    n, h, w = _geometry(poses, disps, intrinsics)
    if poses.shape[0] < n:
        raise ValueError(f"droid_backends.iproj: poses ({poses.shape[0]} rows) must cover the {n} disparity maps")
    dev = _same_device(poses, disps, intrinsics)
    points = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    if n == 0:
        return points
    with torch.cuda.device(dev):
        nat.check(nat.lib().sgr_dba_iproj(poses.data_ptr(), disps.data_ptr(), n, h, w, intrinsics.data_ptr(), points.data_ptr(),
                                          _stream(dev)), "sgr_dba_iproj")
    return points
