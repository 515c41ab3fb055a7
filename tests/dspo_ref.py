"""fp64 numpy restatement of stage 2 ("depth_scale") of the tracker's DSPO bundle adjustment and of the scale-and-shift alignment
(splat_slam_amd.dspo), written from the algorithm as DESIGN.md section 3 ("DSPO stage 2") states it.  SE3 and the pixel rays come from
tests/dba_ref.py.

Unknowns: the disparity of every pixel of the depth frames kx = sorted unique(ii), and one scale s and shift q per depth frame; poses are
fixed.  An edge i -> j moves the pixel (u, v) of frame i with disparity h to X = R_ij ((u-cx)/fx, (v-cy)/fy, 1) + h t_ij (stereo edges,
i == j: R = I, t = (-0.1, 0, 0)); it counts when X.z > MIN_DEPTH.  The mono prior ties h to s m + q, m the mono disparity.
"""
import numpy as np

import dba_ref as R

MIN_DEPTH = 0.2
WEIGHT_SCALE = 0.001
MONO_MIN = 1e-6
VALID_GAIN = 10.0


def align_scale_and_shift(prediction, target, weights=None):
    """Per frame: (scale, shift) minimising sum w (s prediction + q - target)^2 and the mean error sum w |.| / sum w."""
    p, t = np.asarray(prediction, float), np.asarray(target, float)
    w = np.ones_like(p) if weights is None else np.asarray(weights, float)
    if p.ndim < 3:
        p, t, w = p[None], t[None], w[None]
    a00, a01, a11 = (w * p * p).sum((1, 2)), (w * p).sum((1, 2)), w.sum((1, 2))
    b0, b1 = (w * p * t).sum((1, 2)), (w * t).sum((1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        det = a00 * a11 - a01 * a01
        s, q = (a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det
        err = (w * np.abs(s[:, None, None] * p + q[:, None, None] - t)).sum((1, 2)) / a11
    return s, q, err


def relative(pose_i, pose_j, stereo):
    if stereo:
        return R.STEREO_T.copy(), np.eye(3)
    t, q = R.relative(np.asarray(pose_i, float), np.asarray(pose_j, float))
    return t, R.rotmat(q)


def transform(pose_i, pose_j, disp_i, intr, stereo, ddisp=0.0):
    """X [P,3] of every pixel of frame i in frame j, and t_ij."""
    ht, wd = disp_i.shape
    _, _, xr, yr = R.pixel_rays(ht, wd, intr)
    t, Rm = relative(pose_i, pose_j, stereo)
    h = disp_i.reshape(-1).astype(float) + ddisp
    return np.stack([xr, yr, np.ones_like(xr)], 1) @ Rm.T + h[:, None] * t[None], t


def project(pose_i, pose_j, disp_i, intr, stereo=False, ddisp=0.0):
    """Projection [P,2] of every pixel of frame i into frame j after a disparity offset (finite differences of Jz, flow targets)."""
    fx, fy, cx, cy = intr
    X, _ = transform(pose_i, pose_j, disp_i, intr, stereo, ddisp)
    return np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)


def edge_terms(pose_i, pose_j, disp_i, intr, target, weight, stereo):
    """Per pixel: Jz [P,2] (d proj / d disparity), r = target - proj [P,2], the scaled weights [P,2] (zero where the point does not
    land beyond MIN_DEPTH) and X.z [P].  target and weight are [ht,wd,2]."""
    fx, fy, cx, cy = intr
    X, t = transform(pose_i, pose_j, disp_i, intr, stereo)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    front = z > MIN_DEPTH
    d = np.where(front, 1.0 / np.where(front, z, 1.0), 0.0)
    Jz = np.stack([fx * (t[0] * d - t[2] * x * d * d), fy * (t[1] * d - t[2] * y * d * d)], 1)
    proj = np.stack([fx * d * x + cx, fy * d * y + cy], 1)
    r = np.asarray(target, float).reshape(-1, 2) - proj
    w = np.where(front[:, None], WEIGHT_SCALE * np.asarray(weight, float).reshape(-1, 2), 0.0)
    return Jz, r, w, z


def depth_frames(ii):
    return sorted(set(int(v) for v in ii))


def mono_terms(kx, disps, mono, scales, shifts, vmask, ignore_frames, alpha):
    """Per depth row and pixel [M,P]: Jd, Js, Jq, rd and the prior weight a."""
    M = len(kx)
    h = disps[kx].reshape(M, -1)
    m = np.asarray(mono, float)[kx].reshape(M, -1)
    vd = np.asarray(vmask)[kx].reshape(M, -1) != 0
    invalid = (m < MONO_MIN) | (np.array(kx)[:, None] < ignore_frames)
    a = np.sqrt(alpha) * np.where(vd, VALID_GAIN, 1.0)
    Jd = np.where(invalid & vd, 0.0, a)
    Js = np.where(invalid, 0.0, -m * a)
    Jq = np.where(invalid, 0.0, -a)
    rd = np.sqrt(alpha) * (h - (scales[kx][:, None] * m + shifts[kx][:, None]))
    return Jd, Js, Jq, rd, a


def linearize(target, weight, poses, disps, intr, ii, jj, edge_keep=None):
    """C_proj, b_proj [M,P] over the kept edges, the active flag of every depth row, and |X.z - MIN_DEPTH| and the counted flag of
    every (edge, pixel) [E,P] (kept or not)."""
    kx = depth_frames(ii)
    krow = {f: k for k, f in enumerate(kx)}
    P = disps.shape[1] * disps.shape[2]
    C, b = np.zeros((len(kx), P)), np.zeros((len(kx), P))
    active = np.zeros(len(kx), bool)
    margins, counted = np.zeros((len(ii), P)), np.zeros((len(ii), P), bool)
    for e, (i, j) in enumerate(zip(ii, jj)):
        i, j = int(i), int(j)
        Jz, r, w, z = edge_terms(poses[i], poses[j], disps[i], intr, target[e], weight[e], i == j)
        margins[e], counted[e] = np.abs(z - MIN_DEPTH), z > MIN_DEPTH
        if edge_keep is not None and not edge_keep[e]:
            continue
        active[krow[i]] = True
        C[krow[i]] += (w * Jz * Jz).sum(1)
        b[krow[i]] += (w * r * Jz).sum(1)
    return kx, C, b, active, margins, counted


def schur_step(Cp, bp, eta, Jd, Js, Jq, rd, lm, ep):
    """One frame: (dwq [2], dz [P]) from the ten sums of the reduced system; a system that is not positive definite gives dwq = 0."""
    C = Cp + Jd * Jd + eta
    b = bp - Jd * rd
    Q = 1.0 / C
    J = np.stack([Js, Jq])                          # [2,P]
    H = J @ J.T
    u = -(J * rd).sum(1)
    E = J * Jd                                      # [2,P]
    Hd = H + np.diag(ep + lm * np.diag(H))
    S = Hd - (E * Q) @ E.T
    g = u - (E * Q) @ b
    try:
        L = np.linalg.cholesky(S)
        dwq = np.linalg.solve(L.T, np.linalg.solve(L, g))
    except np.linalg.LinAlgError:
        dwq = np.zeros(2)
    return dwq, Q * (b - E.T @ dwq)


def ba_with_scale_shift(target, weight, eta, poses, disps, intr, ii, jj, mono, scales, shifts, vmask, ignore_frames=0, lm=1e-4, ep=0.1,
                        alpha=1.0, iterations=1, edge_keep=None, margins=False):
    """Returns (disps, scales, shifts, dwq [M,2], dz [M,P]) after `iterations` steps (inputs are not modified); with margins=True also
    |X.z - MIN_DEPTH| and the counted flag per (edge, pixel) of the first step.  Rows of inactive depth frames (no kept edge) are zero
    and their frames untouched."""
    disps, scales, shifts = np.array(disps, float), np.array(scales, float), np.array(shifts, float)
    N, ht, wd = disps.shape
    kx = depth_frames(ii)
    M, P = len(kx), ht * wd
    assert eta.shape[0] == M
    eta = np.asarray(eta, float).reshape(M, P)
    dwq, dz, first = np.zeros((M, 2)), np.zeros((M, P)), None
    for _ in range(iterations):
        _, Cp, bp, active, marg, counted = linearize(target, weight, poses, disps, intr, ii, jj, edge_keep)
        first = first or (marg, counted)
        Jd, Js, Jq, rd, _ = mono_terms(kx, disps, mono, scales, shifts, vmask, ignore_frames, alpha)
        dwq, dz = np.zeros((M, 2)), np.zeros((M, P))
        for k, f in enumerate(kx):
            if not active[k]:
                continue
            dwq[k], dz[k] = schur_step(Cp[k], bp[k], eta[k], Jd[k], Js[k], Jq[k], rd[k], lm, ep)
            disps[f] = np.maximum(disps[f] + dz[k].reshape(ht, wd), 0.0)
            scales[f] += dwq[k, 0]
            shifts[f] += dwq[k, 1]
    if margins:
        return disps, scales, shifts, dwq, dz, first[0], first[1]
    return disps, scales, shifts, dwq, dz


def dense_step(target, weight, eta, poses, disps, intr, ii, jj, mono, scales, shifts, vmask, ignore_frames, lm, ep, alpha):
    """The same step from the full normal equations over (s, q of every depth frame; every disparity), assembled from the Jacobian rows
    and solved directly: (dwq [M,2], dz [M,P]).  For tiny problems."""
    disps = np.asarray(disps, float)
    ht, wd = disps.shape[1:]
    kx = depth_frames(ii)
    krow = {f: k for k, f in enumerate(kx)}
    M, P = len(kx), ht * wd
    nvar = 2 * M + M * P
    rows, res, wts = [], [], []
    for e, (i, j) in enumerate(zip(ii, jj)):
        i, j = int(i), int(j)
        Jz, r, w, _ = edge_terms(poses[i], poses[j], disps[i], intr, target[e], weight[e], i == j)
        for p in range(P):
            for c in range(2):
                row = np.zeros(nvar)
                row[2 * M + krow[i] * P + p] = Jz[p, c]
                rows.append(row)
                res.append(r[p, c])
                wts.append(w[p, c])
    Jd, Js, Jq, rd, _ = mono_terms(kx, disps, mono, np.asarray(scales, float), np.asarray(shifts, float), vmask, ignore_frames, alpha)
    for k in range(M):
        for p in range(P):
            row = np.zeros(nvar)
            row[2 * k], row[2 * k + 1], row[2 * M + k * P + p] = Js[k, p], Jq[k, p], Jd[k, p]
            rows.append(row)
            res.append(-rd[k, p])
            wts.append(1.0)
    J, res, wts = np.stack(rows), np.array(res), np.array(wts)
    A = J.T @ (J * wts[:, None])
    g = J.T @ (wts * res)
    damp = np.zeros(nvar)
    damp[:2 * M] = ep + lm * np.diag(A)[:2 * M]
    damp[2 * M:] = np.asarray(eta, float).reshape(-1)
    x = np.linalg.solve(A + np.diag(damp), g)
    return x[:2 * M].reshape(M, 2), x[2 * M:].reshape(M, P)


def cost(target, weight, poses, disps, intr, ii, jj, mono, scales, shifts, vmask, ignore_frames=0, alpha=1.0, eta=None, anchor=None,
         edge_keep=None):
    """The cost a step works on: sum over kept edges of w |r|^2, plus sum over the pixels of the depth frames of (a rho)^2 with
    rho = h - (s m + q) (not where the prior is invalid on a valid-depth pixel: no Jacobian there), plus sum eta (h - anchor)^2 when an
    anchor (the disparities the step started from) is given."""
    disps = np.asarray(disps, float)
    kx = depth_frames(ii)
    M = len(kx)
    total = 0.0
    for e, (i, j) in enumerate(zip(ii, jj)):
        if edge_keep is not None and not edge_keep[e]:
            continue
        i, j = int(i), int(j)
        _, r, w, _ = edge_terms(poses[i], poses[j], disps[i], intr, target[e], weight[e], i == j)
        total += (w * r * r).sum()
    Jd, _, _, rd, a = mono_terms(kx, disps, mono, np.asarray(scales, float), np.asarray(shifts, float), vmask, ignore_frames, alpha)
    rho = rd / np.sqrt(alpha) if alpha > 0 else 0.0 * rd
    total += ((a * rho) ** 2)[Jd != 0].sum()
    if anchor is not None:
        total += (np.asarray(eta, float).reshape(M, -1) * (disps[kx] - np.asarray(anchor, float)[kx]).reshape(M, -1) ** 2).sum()
    return total


def bad_frames(mono, disps, vmask, n_frames, mono_thres):
    """(scale, shift, bad [n_frames]) of depth_scale_step's alignment and bad-frame rule."""
    est, valid = np.asarray(disps, float)[:n_frames], np.asarray(vmask)[:n_frames] != 0
    s, q, err = align_scale_and_shift(np.asarray(mono, float)[:n_frames], est, valid.astype(float))
    bad = np.zeros(n_frames, bool)
    if mono_thres:
        with np.errstate(invalid="ignore", divide="ignore"):
            bad = (err / est.mean((1, 2)) > mono_thres) | np.isnan(err) | (s < 0) | (valid.sum((1, 2)) < valid.shape[1] * valid.shape[2] * 0.5)
    return s, q, bad


def depth_scale_step(poses, disps, intr, mono, vmask, scales, shifts, n_frames, target, weight, eta, ii, jj, itrs=2, lm=1e-4, ep=0.1,
                     mono_thres=0.1, alpha=0.01):
    """Returns (disps, scales, shifts, edge_keep, any_kept); inputs are not modified."""
    disps, scales, shifts = np.array(disps, float), np.array(scales, float), np.array(shifts, float)
    s, q, bad = bad_frames(mono, disps, vmask, n_frames, mono_thres)
    scales[:n_frames], shifts[:n_frames] = s, q
    isbad = lambda f: f < n_frames and bad[f]
    keep = np.array([not (isbad(int(i)) or isbad(int(j))) for i, j in zip(ii, jj)])
    disps, scales, shifts, _, _ = ba_with_scale_shift(target, weight, eta, poses, disps, intr, ii, jj, mono, scales, shifts, vmask, 0, lm,
                                                      ep, alpha, itrs, keep)
    for f in set(int(i) for i, k in zip(ii, keep) if k):
        disps[f] = np.maximum(disps[f], 1e-5)
    return disps, scales, shifts, keep, bool(keep.any())
