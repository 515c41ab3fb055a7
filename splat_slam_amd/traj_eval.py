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
    filled_trajectory(filler, stream) -> [T,7] world -> camera: what full_traj_eval scores (its `traj` keyword takes it back)
    aligned_c2w(cameras_or_c2w, alignment) -> [K,4,4] fp64       slam.py:145-152: PosePath3D.scale(s), then .transform(se3(r_a, t_a))

    associate(stamps_est, stamps_ref, max_diff=0.01, offset=0.0) -> Association(est_inds, ref_inds, n_matched)
        trajectories on different clocks: evo's associate_trajectories on sgr_traj_associate; ValueError on unsorted stamps.
    pose_errors(est, ref, alignment=None, relation="translation_part", delta=None, all_pairs=False, kind=POSE7_W2C, est_inds=None,
                ref_inds=None) -> PoseErrors(stats, err, pair_rows, n_items, n_used, n_skipped)
        evo's APE (delta None) and RPE (delta frames) under every pose relation of RELATIONS, on sgr_traj_pose_errors; the device
        index lists are what associate() returns.  rpe(...) and ape_pose(...) are its two thin wrappers.
    read_tum_trajectory(path) -> (stamps, c2w), write_tum_trajectory(path, stamps, c2w): `t tx ty tz qx qy qz qw` files.
    evaluate_files(est_path, ref_path, ...) -> dict, and the command line over it:
        python -m splat_slam_amd.traj_eval EST REF [--max-diff S] [--offset S] [--no-scale] [--rpe-delta N] [--all-pairs]
                                           [--relation NAME] [--out DIR]
    kf_traj_eval / full_traj_eval(..., extra=[(relation, delta, all_pairs), ...]) return one more element, a dict of those statistics.

GPU tensors only for the poses: there is no CPU path.  One read-back per align, one per ape, one per associate and one per pose_errors.
"""
import math
import os

import numpy as np
import torch

from splat_slam_amd import _native as nat

POSE7_W2C = nat.SGR_TRAJ_POSE7_W2C
MAT4_C2W = nat.SGR_TRAJ_MAT4_C2W
LAUNCHES = {"accumulate": nat.SGR_TRAJ_ACCUMULATE_LAUNCHES, "errors": nat.SGR_TRAJ_ERRORS_LAUNCHES}

POSE_LAUNCHES = {"associate": nat.SGR_TRAJ_ASSOCIATE_LAUNCHES, "pose_errors": nat.SGR_TRAJ_POSE_ERRORS_LAUNCHES}
# evo's PoseRelation names -> the `relation` of sgr_traj_pose_errors
RELATIONS = {"translation_part": nat.SGR_TRAJ_TRANSLATION_PART, "rotation_angle_rad": nat.SGR_TRAJ_ROTATION_ANGLE_RAD,
             "rotation_angle_deg": nat.SGR_TRAJ_ROTATION_ANGLE_DEG, "rotation_part": nat.SGR_TRAJ_ROTATION_PART,
             "full_transformation": nat.SGR_TRAJ_FULL_TRANSFORMATION}

__all__ = ["TrajectoryDegenerate", "Alignment", "Pairs", "umeyama", "pair_centres", "align", "ape", "ape_statistics", "aligned_c2w",
           "kf_traj_eval", "full_traj_eval", "filled_trajectory", "POSE7_W2C", "MAT4_C2W", "Association", "associate", "PoseErrors", "pose_errors", "rpe",
           "ape_pose", "item_pairs", "read_tum_trajectory", "write_tum_trajectory", "evaluate_files", "main", "RELATIONS"]


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


class Association:
    """matched pairs of two stamp lists: est_inds, ref_inds (device int32 [n_matched], in the order of the shorter list)"""

    def __init__(self, est_inds, ref_inds, n_matched):
        self.est_inds, self.ref_inds, self.n_matched = est_inds, ref_inds, int(n_matched)

    def __repr__(self):
        return f"Association(n_matched={self.n_matched})"


def _stamps(s, what, device):
    if torch.is_tensor(s):
        if s.device.type != "cuda":
            raise RuntimeError(f"splat_slam_amd.traj_eval needs {what} as a GPU tensor or a host array (HIP only, no CPU fallback)")
        s = s.detach().to(torch.float64)
    else:
        s = torch.from_numpy(np.ascontiguousarray(np.asarray(s, dtype=np.float64))).to(device)
    if s.dim() != 1 or s.numel() < 1:
        raise ValueError(f"{what} must be a non-empty 1-d list of stamps, got {tuple(s.shape)}")
    return s.contiguous()


def associate(stamps_est, stamps_ref, max_diff=0.01, offset=0.0, device="cuda"):
    """evo's associate_trajectories: every stamp of the SHORTER list is matched to the nearest stamp of the longer one (which must be
    non-decreasing: ValueError otherwise) where they differ by at most max_diff; `offset` is added to the reference's stamps (its sign
    flips where the estimate is the longer list and takes the offset instead).  Stamps: host arrays or GPU tensors, used as fp64."""
    if torch.is_tensor(stamps_est) and stamps_est.device.type == "cuda":
        device = stamps_est.device
    elif torch.is_tensor(stamps_ref) and stamps_ref.device.type == "cuda":
        device = stamps_ref.device
    te, tr = _stamps(stamps_est, "stamps_est", device), _stamps(stamps_ref, "stamps_ref", device)
    est_longer = te.numel() > tr.numel()
    a, b, off = (tr, te, -float(offset)) if est_longer else (te, tr, float(offset))
    na, nb = int(a.numel()), int(b.numel())
    lib = nat.lib()
    nbytes = lib.sgr_traj_associate_scratch_bytes(na, nb)
    if nbytes == 0:
        raise ValueError(f"stamp lists of {na} and {nb} are not supported (the shorter 1 .. {nat.SGR_TRAJ_MAX_POSES}, the longer up to "
                         f"{nat.SGR_TRAJ_MAX_STAMPS})")
    dev = a.device
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(3, na, dtype=torch.int32, device=dev)              # match, a_inds, b_inds
    header = torch.empty(nat.SGR_TRAJ_HEADER_WORDS, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.sgr_traj_associate(a.data_ptr(), na, b.data_ptr(), nb, off, float(max_diff), out[0].data_ptr(), out[1].data_ptr(),
                                         out[2].data_ptr(), header.data_ptr(), scratch.data_ptr(), nbytes, _stream()), "sgr_traj_associate")
        m, unsorted = header.cpu().tolist()[:2]                          # the read-back
    if unsorted:
        raise ValueError("associate: the stamps of the longer trajectory are not in non-decreasing order (or hold a NaN)")
    if m < 1:
        raise TrajectoryDegenerate(f"no stamp of the two trajectories lies within max_diff={max_diff} of one of the other")
    a_inds, b_inds = out[1, :m], out[2, :m]
    return Association(b_inds, a_inds, m) if est_longer else Association(a_inds, b_inds, m)


class PoseErrors:
    """sgr_traj_pose_errors' result: stats (evo's dictionary), err [n_items] fp64 and pair_rows [n_items,2] int32 on the device (the
    pair numbers i, j of each item; j = -1 for an absolute error), n_items, n_used and n_skipped pairs, raw (stats[8])"""

    def __init__(self, stats, err, pair_rows, n_items, n_used, n_skipped, raw):
        self.stats, self.err, self.pair_rows, self.raw = stats, err, pair_rows, raw
        self.n_items, self.n_used, self.n_skipped = int(n_items), int(n_used), int(n_skipped)


def _inds(t, what, device):
    if not torch.is_tensor(t) or t.device != device or t.dtype != torch.int32 or t.dim() != 1:
        raise ValueError(f"{what} must be a 1-d int32 tensor on {device} (what associate() returns)")
    return t.contiguous()


def pose_errors(est, ref, alignment=None, relation="translation_part", delta=None, all_pairs=False, kind=POSE7_W2C, est_inds=None,
                ref_inds=None):
    """Pose-to-pose errors of the pairs (est[est_inds[i]], ref[ref_inds[i]]) (row i where a list is None) after `alignment` (an
    Alignment; None: as they are): absolute (delta None, E = Q^-1 P) or relative over `delta` used poses.  relation: one of RELATIONS.
    est, kind as align(); ref [.,4,4].  One read-back.  TrajectoryDegenerate where no item is left to score."""
    if relation not in RELATIONS:
        raise ValueError(f"relation must be one of {sorted(RELATIONS)}, got {relation!r}")
    if delta is not None and (isinstance(delta, bool) or int(delta) != delta or int(delta) < 1):
        raise ValueError(f"delta must be None (absolute errors) or an integer >= 1, got {delta!r}")
    if est_inds is not None and ref_inds is not None and len(est_inds) != len(ref_inds):
        raise ValueError(f"{len(est_inds)} estimate indices for {len(ref_inds)} reference indices")
    if not torch.is_tensor(est) or est.device.type != "cuda":
        raise RuntimeError("splat_slam_amd.traj_eval needs the estimate on the GPU (HIP only, no CPU fallback)")
    if kind == POSE7_W2C:
        if est.dim() != 2 or est.shape[1] != 7 or est.dtype != torch.float32 or not est.is_contiguous():
            raise ValueError(f"est must be contiguous fp32 [.,7], got {est.dtype} {tuple(est.shape)}")
    elif kind == MAT4_C2W:
        est = _mat4_rows(est, "est", est.device)
    else:
        raise ValueError(f"kind must be POSE7_W2C or MAT4_C2W, got {kind!r}")
    dev = est.device
    ref = _mat4_rows(ref, "ref", dev)
    est_rows, ref_rows = int(est.shape[0]), int(ref.shape[0])
    est_inds = None if est_inds is None else _inds(est_inds, "est_inds", dev)
    ref_inds = None if ref_inds is None else _inds(ref_inds, "ref_inds", dev)
    given = est_inds if est_inds is not None else ref_inds
    n = int(given.numel()) if given is not None else ref_rows
    if (est_inds is None and est_rows < n) or (ref_inds is None and ref_rows < n):
        raise ValueError(f"{n} pairs of {est_rows} estimated and {ref_rows} reference poses")
    lib = nat.lib()
    nbytes = lib.sgr_traj_pose_errors_scratch_bytes(n)
    if nbytes == 0:
        raise ValueError(f"a trajectory of {n} poses is not supported (1 .. {nat.SGR_TRAJ_MAX_POSES})")
    al = Alignment.identity() if alignment is None else alignment
    sim3 = (nat.C.c_double * 13)(float(al.s), *np.asarray(al.r_a, dtype=np.float64).reshape(9).tolist(),
                                 *np.asarray(al.t_a, dtype=np.float64).reshape(3).tolist())
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    err = torch.empty(n, dtype=torch.float64, device=dev)
    pair_rows = torch.empty(n, 2, dtype=torch.int32, device=dev)
    tail = torch.empty(8 + nat.SGR_TRAJ_HEADER_WORDS // 2, dtype=torch.float64, device=dev)      # stats[8], then the header: one read-back
    with torch.cuda.device(dev):
        nat.check(lib.sgr_traj_pose_errors(kind, est.data_ptr(), est_rows, ref.data_ptr(), ref_rows, nat.ptr(est_inds), nat.ptr(ref_inds), n,
                                           sim3, nat.SGR_TRAJ_ABSOLUTE if delta is None else nat.SGR_TRAJ_RELATIVE,
                                           1 if delta is None else int(delta), 1 if all_pairs else 0, RELATIONS[relation], err.data_ptr(),
                                           pair_rows.data_ptr(), tail.data_ptr(), tail[8:].data_ptr(), scratch.data_ptr(), nbytes,
                                           _stream()), "sgr_traj_pose_errors")
        host = tail.cpu().numpy()
    raw = host[:8].copy()
    m, used, skipped = (int(v) for v in host[8:].view(np.int32)[:3])
    return PoseErrors(ape_statistics(raw), err[:m], pair_rows[:m], m, used, skipped, raw)


def rpe(est, ref, alignment=None, delta=1, relation="translation_part", all_pairs=False, **kw):
    """the relative pose error over `delta` used poses (evo's RPE with delta_unit frames) -> PoseErrors"""
    if delta is None:
        raise ValueError("rpe: delta must be an integer >= 1")
    return pose_errors(est, ref, alignment, relation, delta, all_pairs, **kw)


def ape_pose(est, ref, alignment=None, relation="translation_part", **kw):
    """the absolute pose error under any relation (evo's APE) -> PoseErrors"""
    return pose_errors(est, ref, alignment, relation, None, False, **kw)


def item_pairs(c, delta, all_pairs):
    """the rank pairs the relative error is formed over among c used poses (evo's id_pairs_from_delta, frames)"""
    if delta < 1:
        raise ValueError(f"delta must be >= 1, got {delta}")
    if all_pairs:
        return [(r, r + delta) for r in range(max(c - delta, 0))]
    return [(k * delta, (k + 1) * delta) for k in range((c - 1) // delta if c >= 1 else 0)]


def _quat_to_mat(q):
    q = np.asarray(q, dtype=np.float64)
    x, y, z, w = (q / np.linalg.norm(q, axis=-1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def _mat_to_quat(r):
    """(x, y, z, w) of a rotation matrix, by the largest of the four squares (Shepperd)"""
    t = (r[0, 0] + r[1, 1] + r[2, 2], r[0, 0], r[1, 1], r[2, 2])
    k = int(np.argmax(t))
    if k == 0:
        q = np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1], 1.0 + t[0]])
    elif k == 1:
        q = np.array([1.0 + r[0, 0] - r[1, 1] - r[2, 2], r[0, 1] + r[1, 0], r[0, 2] + r[2, 0], r[2, 1] - r[1, 2]])
    elif k == 2:
        q = np.array([r[0, 1] + r[1, 0], 1.0 - r[0, 0] + r[1, 1] - r[2, 2], r[1, 2] + r[2, 1], r[0, 2] - r[2, 0]])
    else:
        q = np.array([r[0, 2] + r[2, 0], r[1, 2] + r[2, 1], 1.0 - r[0, 0] - r[1, 1] + r[2, 2], r[1, 0] - r[0, 1]])
    return q / np.linalg.norm(q)


def read_tum_trajectory(path):
    """A TUM RGB-D trajectory file (`t tx ty tz qx qy qz qw` per line, `#` lines and empty lines skipped) -> (stamps [n] fp64,
    camera -> world [n,4,4] fp64), numpy"""
    rows = []
    with open(path) as fp:
        for no, line in enumerate(fp, 1):
            line = line.split("#", 1)[0].replace(",", " ").split()
            if not line:
                continue
            if len(line) != 8:
                raise ValueError(f"{path}:{no}: {len(line)} fields, expected t tx ty tz qx qy qz qw")
            rows.append([float(v) for v in line])
    a = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    c2w = np.tile(np.eye(4), (len(a), 1, 1))
    if len(a):
        c2w[:, :3, :3] = _quat_to_mat(a[:, 4:8])
        c2w[:, :3, 3] = a[:, 1:4]
    return a[:, 0].copy(), c2w


def write_tum_trajectory(path, stamps, c2w):
    """the inverse of read_tum_trajectory; every number is written with repr(), so fp64 stamps read back bit for bit"""
    stamps = np.asarray(stamps, dtype=np.float64).reshape(-1)
    c2w = np.asarray(c2w.detach().double().cpu() if torch.is_tensor(c2w) else c2w, dtype=np.float64).reshape(-1, 4, 4)
    if len(stamps) != len(c2w):
        raise ValueError(f"{len(stamps)} stamps for {len(c2w)} poses")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fp:
        fp.write("# timestamp tx ty tz qx qy qz qw\n")
        for t, p in zip(stamps, c2w):
            fp.write(" ".join(repr(float(v)) for v in (t, *p[:3, 3], *_mat_to_quat(p[:3, :3]))) + "\n")


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


def extra_key(relation, delta, all_pairs):
    """the name of one entry of `extra` in the dict kf_traj_eval and full_traj_eval return: ape_<relation>, rpe_<relation>_d<delta>[_all]"""
    return f"ape_{relation}" if delta is None else f"rpe_{relation}_d{int(delta)}" + ("_all" if all_pairs else "")


def _extras(extra, est, ref, alignment, path):
    """the statistics of every (relation, delta, all_pairs) of `extra` (None where no item is left), appended to the metrics file"""
    out = {}
    for relation, delta, all_pairs in extra:
        try:
            out[extra_key(relation, delta, all_pairs)] = pose_errors(est, ref, alignment, relation, delta, all_pairs).stats
        except TrajectoryDegenerate:
            out[extra_key(relation, delta, all_pairs)] = None
    if path is not None:
        with open(path, "a") as fp:
            for k, v in out.items():
                fp.write(f"\n{k}:\n{v}")
    return out


def kf_traj_eval(video, gt_poses, out_dir=None, npz_path=None, plot=False, extra=None):
    """The keyframes of `video` against gt_poses[int(video.timestamp[i])] (camera -> world 4x4 each): video.poses[:counter] is scored in
    place.  Both trajectories come from one timestamp list, so evo's association step is the identity and is not restated.  With out_dir,
    metrics_kf_traj.txt is written there; with npz_path (a DepthVideo.save_video file), `scale` is added to it (eval_traj.py:137-138).
    extra: a list of (relation, delta, all_pairs) for pose_errors after the alignment; their statistics are returned as a fifth element
    (a dict by extra_key) and appended to the metrics file."""
    n = int(video.counter.value)
    if n < 1:
        raise TrajectoryDegenerate("the video holds no keyframe")
    ts = [int(t) for t in video.timestamp[:n].cpu().tolist()]
    ref = _gt_rows(gt_poses, ts, video.poses.device)
    alignment = align(video.poses[:n], ref, POSE7_W2C)
    stats = ape(alignment)
    path = None if out_dir is None else os.path.join(out_dir, "metrics_kf_traj.txt")
    _report("Keyframes traj", alignment, stats, path)
    if plot and out_dir is not None:
        _plot(alignment, out_dir, "kf_traj.png", "Keyframes traj")
    if npz_path is not None:
        saved = dict(np.load(npz_path))
        saved["scale"] = np.array(alignment.s)
        np.savez(npz_path, **saved)
    if extra is not None:
        return stats, alignment.s, alignment.r_a, alignment.t_a, _extras(extra, video.poses[:n], ref, alignment, path)
    return stats, alignment.s, alignment.r_a, alignment.t_a


@torch.no_grad()
def filled_trajectory(filler, stream):
    """Every frame of the stream as a world -> camera pose7 row [T,7] (device): the filler's poses with the keyframes' rows overwritten
    by the video's (a device index copy, as eval_traj.py:148-151 does on the host).  What full_traj_eval scores and, as
    lietorch.SE3(.).inv().matrix(), returns; the novel-view evaluation needs it without ground-truth poses too."""
    traj = filler(stream).contiguous()
    video = filler.video
    n = int(video.counter.value)
    traj.index_copy_(0, video.timestamp[:n].long(), video.poses[:n])
    return traj


def full_traj_eval(filler, stream, gt_poses, out_dir=None, plot=False, extra=None, traj=None):
    """Every frame of the stream: filled_trajectory(filler, stream) (or `traj`, that very result computed by the caller), aligned to
    gt_poses[i] and scored.  Returns the unaligned camera -> world trajectory
    [T,4,4] (device), the statistics and the Alignment; with out_dir, metrics_full_traj.txt is written there.  extra: as kf_traj_eval
    (a fourth element)."""
    import lietorch
    if traj is None:
        traj = filled_trajectory(filler, stream)
    T = int(traj.shape[0])
    if len(gt_poses) != T:
        raise ValueError(f"full_traj_eval: {len(gt_poses)} ground-truth poses for {T} frames")
    ref = _gt_rows(gt_poses, range(T), traj.device)
    alignment = align(traj, ref, POSE7_W2C)
    stats = ape(alignment)
    path = None if out_dir is None else os.path.join(out_dir, "metrics_full_traj.txt")
    _report("Full traj", alignment, stats, path)
    if plot and out_dir is not None:
        _plot(alignment, out_dir, "full_traj.png", "Full traj")
    if extra is not None:
        return lietorch.SE3(traj).inv().matrix(), stats, alignment, _extras(extra, traj, ref, alignment, path)
    return lietorch.SE3(traj).inv().matrix(), stats, alignment


def evaluate_files(est_path, ref_path, max_diff=0.01, offset=0.0, with_scale=True, rpe_delta=None, all_pairs=False,
                   relation="translation_part", out_dir=None, device="cuda"):
    """Two TUM trajectory files on their own clocks: associate, align (scaled Umeyama unless with_scale=False) and score.  Returns
    {"n_matched", "alignment", "ate": the statistics of the aligned centres, "relation", "delta", "errors": the statistics of `relation`,
    absolute (rpe_delta None) or relative over rpe_delta matched poses, "report": the text}; with out_dir, metrics_traj.txt holds the text.
    The poses are scored as fp32 matrices, the precision every kernel of this module reads."""
    if relation not in RELATIONS:
        raise ValueError(f"relation must be one of {sorted(RELATIONS)}, got {relation!r}")
    ts_e, c2w_e = read_tum_trajectory(est_path)
    ts_r, c2w_r = read_tum_trajectory(ref_path)
    if len(ts_e) < 1 or len(ts_r) < 1:
        raise TrajectoryDegenerate(f"{est_path} holds {len(ts_e)} poses, {ref_path} {len(ts_r)}")
    est = torch.from_numpy(c2w_e.astype(np.float32)).to(device)
    ref = torch.from_numpy(c2w_r.astype(np.float32)).to(device)
    m = associate(ts_e, ts_r, max_diff, offset, device=est.device)
    alignment = align(est[m.est_inds.long()], ref[m.ref_inds.long()], MAT4_C2W, with_scale=with_scale)     # a gather, off the hot path
    ate = ape(alignment)
    errors = pose_errors(est, ref, alignment, relation, rpe_delta, all_pairs, MAT4_C2W, m.est_inds, m.ref_inds)
    text = _report("Associated traj", alignment, ate, None)
    text += f"\nmatched: {m.n_matched} of {len(ts_e)} estimated and {len(ts_r)} reference poses (max_diff {max_diff}, offset {offset})"
    text += f"\n{extra_key(relation, rpe_delta, all_pairs)} ({errors.n_items} items):\n{errors.stats}"
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "metrics_traj.txt"), "w+") as fp:
            fp.write(text)
    return {"n_matched": m.n_matched, "alignment": alignment, "ate": ate, "relation": relation, "delta": rpe_delta, "errors": errors.stats,
            "report": text}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m splat_slam_amd.traj_eval",
                                 description="Score an estimated trajectory against a reference one (TUM files: t tx ty tz qx qy qz qw): "
                                             "time association, scaled Umeyama alignment, ATE and one more pose relation.")
    ap.add_argument("est", metavar="EST")
    ap.add_argument("ref", metavar="REF")
    ap.add_argument("--max-diff", type=float, default=0.01, help="largest stamp difference of a match, seconds (0.01)")
    ap.add_argument("--offset", type=float, default=0.0, help="added to the reference's stamps (0)")
    ap.add_argument("--no-scale", action="store_true", help="rigid alignment: the scale stays 1")
    ap.add_argument("--rpe-delta", type=int, default=None, metavar="N", help="score the relative error over N matched poses (absolute without)")
    ap.add_argument("--all-pairs", action="store_true", help="relative error over every pair (r, r + N), not consecutive ones")
    ap.add_argument("--relation", default="translation_part", choices=sorted(RELATIONS))
    ap.add_argument("--out", metavar="DIR", default=None, help="metrics_traj.txt is written there")
    args = ap.parse_args(argv)
    result = evaluate_files(args.est, args.ref, args.max_diff, args.offset, not args.no_scale, args.rpe_delta, args.all_pairs, args.relation,
                            args.out)
    print(result["report"])
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
