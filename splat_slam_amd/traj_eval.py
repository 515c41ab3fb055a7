"""Trajectory scoring of the reference's terminate() (/root/reference/src/utils/eval_traj.py and src/slam.py:130-244): the scaled Umeyama
alignment of the estimated camera centres to the ground truth and the absolute trajectory error (evo's APE of the translation part), on
the HIP kernels of csrc/sgr_traj.hip.  evo is not used: DESIGN.md section 3, "Trajectory scoring", states the equations and the
conventions assumed about it.  No plots (evo.tools.plot has no counterpart here): the figures the reference saves are not produced.

    umeyama(sums, with_scale=True) -> (r, t, s)
        the fit y ~ s r x + t from sgr_traj_accumulate's 17 sums, numpy fp64; TrajectoryDegenerate (a ValueError) where evo raises its
        GeometryException (fewer than two singular values above machine epsilon) and for fewer than three pairs, a stationary
        estimate or sums that are not finite.
    align(est, ref, kind=POSE7_W2C, inds=None, with_scale=True) -> Alignment
        est: [.,7] world -> camera poses in the video's layout (read in place, rows `inds` or 0 .. n-1) or, kind MAT4_C2W, [.,4,4] camera
        -> world; ref: [n,4,4] camera -> world; a pair whose reference matrix holds a nan or an inf is skipped.  Alignment has r_a [3,3],
        t_a [3], s, n_used, n_skipped and `pairs`, the device state that ape() scores.
    ape(alignment, pairs=None) -> {rmse, mean, median, std, min, max, sse}
        evo's statistics of |s r_a x + t_a - y| over the used pairs; alignment None scores `pairs` (pair_centres) as they are.
    kf_traj_eval(video, gt_poses, out_dir=None, npz_path=None, plot=False) -> (stats, s, r_a, t_a)         eval_traj.py:113-140
    full_traj_eval(filler, stream, gt_poses, out_dir=None, plot=False) -> (traj_unaligned [T,4,4], stats, alignment)     eval_traj.py:143-175
        plot=True with an out_dir also writes kf_traj.png / full_traj.png beside the metrics file; the return values are the same.
    aligned_c2w(cameras_or_c2w, alignment) -> [K,4,4] fp64       slam.py:145-152: PosePath3D.scale(s), then .transform(se3(r_a, t_a))

GPU tensors only for the poses: there is no CPU path.  One read-back per align and one per ape.
"""
import math
import os

import numpy as np
import torch

from splat_slam_amd import _native as nat

POSE7_W2C = nat.SGR_TRAJ_POSE7_W2C
MAT4_C2W = nat.SGR_TRAJ_MAT4_C2W
LAUNCHES = {"accumulate": nat.SGR_TRAJ_ACCUMULATE_LAUNCHES, "errors": nat.SGR_TRAJ_ERRORS_LAUNCHES}

__all__ = ["TrajectoryDegenerate", "Alignment", "Pairs", "umeyama", "pair_centres", "align", "ape", "ape_statistics", "aligned_c2w",
           "kf_traj_eval", "full_traj_eval", "POSE7_W2C", "MAT4_C2W"]


class TrajectoryDegenerate(ValueError):
    """the trajectory does not determine a similarity: too few poses, no motion, or motion along one line only"""


class Alignment:
    def __init__(self, r_a, t_a, s, n_used, n_skipped, pairs=None):
        self.r_a, self.t_a, self.s, self.n_used, self.n_skipped, self.pairs = r_a, t_a, float(s), int(n_used), int(n_skipped), pairs

    @classmethod
    def identity(cls, pairs=None):
        used = pairs.n_used if pairs is not None else 0
        return cls(np.eye(3), np.zeros(3), 1.0, used, (pairs.n - used) if pairs is not None else 0, pairs)

    def __repr__(self):
        return f"Alignment(s={self.s}, r_a={self.r_a.tolist()}, t_a={self.t_a.tolist()}, n_used={self.n_used}, n_skipped={self.n_skipped})"


def umeyama(sums, with_scale=True):
    sums = np.asarray(sums, dtype=np.float64).reshape(17)
    n = sums[0]
    if not np.isfinite(sums).all():
        raise TrajectoryDegenerate("the sums of the trajectory are not finite")
    if n < 3:
        raise TrajectoryDegenerate(f"{int(n)} usable poses: a similarity needs three")
    mx, my = sums[1:4] / n, sums[4:7] / n
    var = sums[7] / n
    if not var > 0.0:
        raise TrajectoryDegenerate("the estimated trajectory does not move")
    u, d, vt = np.linalg.svd(sums[8:17].reshape(3, 3) / n)
    if np.count_nonzero(d > np.finfo(np.float64).eps) < 2:
        raise TrajectoryDegenerate("degenerate covariance rank: the poses lie on one line")
    S = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:
        S[2, 2] = -1.0
    r = u @ S @ vt
    s = float(np.trace(np.diag(d) @ S) / var) if with_scale else 1.0
    return r, my - s * (r @ mx), s


def ape_statistics(stats):
    """evo's get_all_statistics from sgr_traj_errors' stats[8]: std is the population form, the median np.median's"""
    stats = np.asarray(stats, dtype=np.float64).reshape(8)
    n = stats[0]
    if n < 1:
        raise TrajectoryDegenerate("no usable pose to score")
    return {"rmse": math.sqrt(stats[2] / n), "mean": float(stats[1] / n), "median": float(0.5 * (stats[5] + stats[6])),
            "std": math.sqrt(stats[7] / n), "min": float(stats[3]), "max": float(stats[4]), "sse": float(stats[2])}


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Pairs:
    """what sgr_traj_accumulate leaves on the device: pos [n,2,3] fp64 (estimate, reference), valid [n] u8, and the 17 sums (host)"""

    def __init__(self, n, pos, valid, sums, scratch):
        self.n, self.pos, self.valid, self.sums, self._scratch = n, pos, valid, sums, scratch
        self.n_used = int(sums[0])

    def errors(self, r=None, t=None, s=1.0):
        """(err [n] fp64 on the device, NaN where skipped; stats[8] numpy) of sgr_traj_errors under y ~ s r x + t"""
        r = np.eye(3) if r is None else np.asarray(r, dtype=np.float64).reshape(3, 3)
        t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).reshape(3)
        sim3 = (nat.C.c_double * 13)(float(s), *r.reshape(-1).tolist(), *t.tolist())
        err = torch.empty(self.n, dtype=torch.float64, device=self.pos.device)
        stats = torch.empty(8, dtype=torch.float64, device=self.pos.device)
        with torch.cuda.device(self.pos.device):
            nat.check(nat.lib().sgr_traj_errors(self.n, self.pos.data_ptr(), self.valid.data_ptr(), sim3, err.data_ptr(), stats.data_ptr(),
                                                self._scratch.data_ptr(), self._scratch.numel(), _stream()), "sgr_traj_errors")
        return err, stats.cpu().numpy()


def _mat4_rows(m, what, device):
    if not torch.is_tensor(m):
        m = torch.stack([torch.as_tensor(p) for p in m]) if isinstance(m, (list, tuple)) else torch.as_tensor(m)
    if m.dim() != 3 or tuple(m.shape[1:]) != (4, 4):
        raise ValueError(f"{what} must be [n,4,4], got {tuple(m.shape)}")
    return m.detach().to(device=device, dtype=torch.float32).reshape(-1, 16).contiguous()


def pair_centres(est, ref, kind=POSE7_W2C, inds=None):
    """sgr_traj_accumulate over the pairs (est[inds[i]] or est[i], ref[i]) -> Pairs"""
    if not torch.is_tensor(est) or est.device.type != "cuda":
        raise RuntimeError("splat_slam_amd.traj_eval needs the estimate on the GPU (HIP only, no CPU fallback)")
    if kind == POSE7_W2C:
        if est.dim() != 2 or est.shape[1] != 7 or est.dtype != torch.float32 or not est.is_contiguous():
            raise ValueError(f"est must be contiguous fp32 [.,7], got {est.dtype} {tuple(est.shape)}")
    elif kind == MAT4_C2W:
        est = _mat4_rows(est, "est", est.device)
    else:
        raise ValueError(f"kind must be POSE7_W2C or MAT4_C2W, got {kind!r}")
    ref = _mat4_rows(ref, "ref", est.device)
    n, rows = int(ref.shape[0]), int(est.shape[0])
    host = None
    if inds is not None:
        host = [int(i) for i in (inds.tolist() if torch.is_tensor(inds) else inds)]
        if len(host) != n:
            raise ValueError(f"{len(host)} indices for {n} reference poses")
        host = (nat.C.c_int64 * n)(*host)
    elif rows < n:
        raise ValueError(f"{rows} estimated poses for {n} reference poses")
    lib = nat.lib()
    nbytes = lib.sgr_traj_scratch_bytes(n)
    if nbytes == 0:
        raise ValueError(f"a trajectory of {n} poses is not supported (1 .. {nat.SGR_TRAJ_MAX_POSES})")
    dev = est.device
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pos = torch.empty(n, 2, 3, dtype=torch.float64, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    sums = torch.empty(17, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.sgr_traj_accumulate(kind, est.data_ptr(), rows, host, n, ref.data_ptr(), pos.data_ptr(), valid.data_ptr(),
                                          sums.data_ptr(), scratch.data_ptr(), nbytes, _stream()), "sgr_traj_accumulate")
        sums = sums.cpu().numpy()               # the read-back (the stream has passed the copy of `host` by now)
    return Pairs(n, pos, valid, sums, scratch)


def align(est, ref, kind=POSE7_W2C, inds=None, with_scale=True):
    pairs = pair_centres(est, ref, kind, inds)
    r, t, s = umeyama(pairs.sums, with_scale)
    return Alignment(r, t, s, pairs.n_used, pairs.n - pairs.n_used, pairs)


def ape(alignment, pairs=None):
    if alignment is None:
        alignment = Alignment.identity(pairs)
    pairs = alignment.pairs if pairs is None else pairs
    if pairs is None:
        raise ValueError("ape: no pairs to score (an Alignment from align(), or pairs=pair_centres(...))")
    return ape_statistics(pairs.errors(alignment.r_a, alignment.t_a, alignment.s)[1])


def aligned_c2w(cameras_or_c2w, alignment):
    """[[r_a R, s r_a t + t_a], [0, 1]] of camera -> world poses [K,4,4], or of cameras (objects with R, T world -> camera, inverted on the
    host in fp64 as slam.py:148 does), numpy fp64"""
    src = cameras_or_c2w
    if torch.is_tensor(src) or isinstance(src, np.ndarray):
        c2w = np.asarray(src.detach().double().cpu() if torch.is_tensor(src) else src, dtype=np.float64).reshape(-1, 4, 4)
    else:
        cams = list(src)
        if not cams:
            return np.zeros((0, 4, 4))
        if hasattr(cams[0], "R"):
            rt = torch.stack([torch.cat([c.R.detach().reshape(3, 3), c.T.detach().reshape(3, 1)], 1) for c in cams]).double().cpu().numpy()
            w2c = np.tile(np.eye(4), (len(cams), 1, 1))
            w2c[:, :3] = rt
            c2w = np.linalg.inv(w2c)
        else:
            c2w = np.stack([np.asarray(torch.as_tensor(p).detach().double().cpu()) for p in cams]).reshape(-1, 4, 4)
    out = np.tile(np.eye(4), (c2w.shape[0], 1, 1))
    out[:, :3, :3] = alignment.r_a @ c2w[:, :3, :3]
    out[:, :3, 3] = alignment.s * (c2w[:, :3, 3] @ alignment.r_a.T) + alignment.t_a
    return out


def _gt_rows(gt_poses, idxs, device):
    idxs = list(idxs)
    if isinstance(gt_poses, np.ndarray):
        rows = gt_poses[idxs]
    elif torch.is_tensor(gt_poses):
        rows = gt_poses[idxs].detach().cpu().numpy()
    else:                                                   # a list of 4x4 arrays or tensors, as the reference's datasets carry
        rows = np.stack([np.asarray(torch.as_tensor(gt_poses[i]).detach().cpu()) for i in idxs])
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 4, 4)).to(device)


def _report(title, alignment, stats, path):
    """the reference's wording (eval_traj.py:124-133, 161-172)"""
    text = "#" * 10 + title + "#" * 10 + "\n"
    text += f"scale: {alignment.s}\nrotation:\n{alignment.r_a}\ntranslation:{alignment.t_a}\nstatistics:\n{stats}"
    if path is not None:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w+") as fp:
            fp.write(text)
    return text


def _plot(alignment, out_dir, name, title):
    from splat_slam_amd.plots import plot_trajectory
    plot_trajectory(alignment, os.path.join(out_dir, name), title)


def kf_traj_eval(video, gt_poses, out_dir=None, npz_path=None, plot=False):
    """The keyframes of `video` against gt_poses[int(video.timestamp[i])] (camera -> world 4x4 each): video.poses[:counter] is scored in
    place.  Both trajectories come from one timestamp list, so evo's association step is the identity and is not restated.  With out_dir,
    metrics_kf_traj.txt is written there; with npz_path (a DepthVideo.save_video file), `scale` is added to it (eval_traj.py:137-138)."""
    n = int(video.counter.value)
    if n < 1:
        raise TrajectoryDegenerate("the video holds no keyframe")
    ts = [int(t) for t in video.timestamp[:n].cpu().tolist()]
    alignment = align(video.poses[:n], _gt_rows(gt_poses, ts, video.poses.device), POSE7_W2C)
    stats = ape(alignment)
    _report("Keyframes traj", alignment, stats, None if out_dir is None else os.path.join(out_dir, "metrics_kf_traj.txt"))
    if plot and out_dir is not None:
        _plot(alignment, out_dir, "kf_traj.png", "Keyframes traj")
    if npz_path is not None:
        saved = dict(np.load(npz_path))
        saved["scale"] = np.array(alignment.s)
        np.savez(npz_path, **saved)
    return stats, alignment.s, alignment.r_a, alignment.t_a


@torch.no_grad()
def full_traj_eval(filler, stream, gt_poses, out_dir=None, plot=False):
    """Every frame of the stream: the filler's poses with the keyframes' rows overwritten by the video's (a device index copy, as
    eval_traj.py:148-151 does on the host), aligned to gt_poses[i] and scored.  Returns the unaligned camera -> world trajectory
    [T,4,4] (device), the statistics and the Alignment; with out_dir, metrics_full_traj.txt is written there."""
    import lietorch
    traj = filler(stream).contiguous()
    video = filler.video
    n, T = int(video.counter.value), int(traj.shape[0])
    if len(gt_poses) != T:
        raise ValueError(f"full_traj_eval: {len(gt_poses)} ground-truth poses for {T} frames")
    traj.index_copy_(0, video.timestamp[:n].long(), video.poses[:n])
    alignment = align(traj, _gt_rows(gt_poses, range(T), traj.device), POSE7_W2C)
    stats = ape(alignment)
    _report("Full traj", alignment, stats, None if out_dir is None else os.path.join(out_dir, "metrics_full_traj.txt"))
    if plot and out_dir is not None:
        _plot(alignment, out_dir, "full_traj.png", "Full traj")
    return lietorch.SE3(traj).inv().matrix(), stats, alignment
