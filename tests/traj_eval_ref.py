"""fp64 numpy restatement of splat_slam_amd.traj_eval ("Trajectory scoring"), written from the equations, and the
bounds the tests hold the HIP kernels of csrc/sgr_traj.hip to.  Tests only.

The equations.  x_i: centre of estimated camera i, y_i: centre of its reference camera; a pair is used iff all 16 entries of the
reference matrix are finite.  Over the n used pairs: xm = sum x / n, ym = sum y / n, var = sum |x - xm|^2 / n,
C = sum (y - ym)(x - xm)^T / n = U diag(d) V^T, S = diag(1, 1, sign(det U det V^T)), r = U S V^T, s = trace(diag(d) S) / var,
t = ym - s r xm; e_i = |s r x_i + t - y_i|; rmse = sqrt(sum e^2 / n), std the population form, median np.median's.

The bounds.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3 and 4: a sum of
terms through an addition tree of depth h errs by at most gamma_h sum |term|).  The restatement adds with math.fsum, whose result is
the correctly rounded exact sum: it errs by at most u |sum| <= u sum |term|.  The kernels' trees, from the code:

    partial_depth(n)   launch 1 leaves one term per thread; a workgroup adds 64 lanes by butterfly (6 levels) and its 4 waves left to
                       right (3 additions); launch 2 adds the ceil(n / 256) partials in order: 6 + 3 + ceil(n / 256)
    wide_depth(n)      launch 2's own pass: each of 1024 threads adds its ceil(n / 1024) terms in order, then 6 levels and the 16
                       waves left to right (15 additions): ceil(n / 1024) + 6 + 15

and no tree over n terms is deeper than n - 1.  So a kernel sum and the restatement of the same terms differ by at most
(gamma_min(h, n - 1) + u) sum |term|, which is never more than the 2 gamma_n sum |term| that two arbitrary fp64 summations may differ
by (min(h, n - 1) + 1 <= n): the *_bounds functions return both figures and the tests assert the first against the second.

Centred sums.  Both sides subtract their own rounded mean m' = m + dm, |dm| <= mean_err = (gamma_h sum |x|) / n + u |m| (the sum's
error divided by n, then the division's rounding).  Because sum (x - m) = 0 exactly,
    sum (y - ym')(x - xm')^T = sum (y - ym)(x - xm)^T + n dym dxm^T:
the means' errors enter in second order only.  Forming a centred term costs one rounding per factor and one for the product
(3 u |term|; the kernel's fused multiply-add saves one), the three squares of |x - xm|^2 two more additions (2 u), then the tree.  Kernel
plus restatement: n (dm_kernel^2 + dm_ref^2) + (2 * 3 u [+ 2 * 2 u] + gamma_h + u) sum |term|, constants rounded up for the terms of
second order in u (below 1e-10 of the first for n <= 65535).

A loose bound could pass a dropped or doubled pose, so the tests also assert every bound against 1e-10 of what its component carries:
the largest |coordinate| for sum x and sum y (a dropped pose moves them by a coordinate; one ulp of a sum of 2049 coordinates of 1e3
is already 5e-10, so the extent about the mean cannot be the yardstick there), and extent^2 about the means for the centred sums (a
dropped pose moves them by the square of its distance from the mean, of the order of extent^2).  With 2 gamma_n in the place of the
trees' depth neither would hold at n = 2049 (2 n^2 u = 9e-10): that is why the trees are counted.

Errors.  z_a = s (r_a0 x_0 + r_a1 x_1 + r_a2 x_2) + t_a - y_a passes every term through at most 6 roundings (product, two additions,
the scale, two additions), so |z'_a - z_a| <= gamma_6 M_a with M_a = s (|r| |x|)_a + |t_a| + |y_a|; the three squares, their two
additions and the square root are relative errors of the norm, (3 u / 2 + u) < 3 u of |z'| <= |M| (1 + gamma_6).  One evaluation errs by
at most (gamma_6 + 3 u) |M|_2 < 9.01 u |M|_2, the kernel's and the restatement's together by ERR_ROUNDINGS = 18 roundings of |M|_2
(a fused multiply-add only removes roundings).
"""
import math

import numpy as np

U = 2.0 ** -53
ERR_ROUNDINGS = 18.02


def gamma(k):
    return k * U / (1.0 - k * U)


def partial_depth(n):
    return 6 + 3 + -(-n // 256)


def wide_depth(n):
    return -(-n // 1024) + 6 + 15


def fsum(a):
    """correctly rounded sums over the first axis"""
    a = np.asarray(a, np.float64)
    if a.ndim == 1:
        return math.fsum(a.tolist())
    flat = a.reshape(a.shape[0], -1)
    return np.array([math.fsum(flat[:, k].tolist()) for k in range(flat.shape[1])]).reshape(a.shape[1:])


def valid_rows(ref):
    """eval_traj.py:30-33: a reference pose is skipped iff its sum is nan or inf, i.e. iff some entry is not finite"""
    return np.isfinite(np.asarray(ref, np.float64).reshape(len(ref), 16)).all(1)


def fit_sums(x, y, valid):
    """sgr_traj_accumulate's 17 sums of the centres x, y [n,3] over the valid pairs, and the absolute sums the bounds need"""
    x, y = np.asarray(x, np.float64)[valid], np.asarray(y, np.float64)[valid]
    n = len(x)
    out, mag = np.zeros(17), np.zeros(17)
    out[0] = n
    if n == 0:
        return out, mag
    out[1:4], out[4:7] = fsum(x), fsum(y)
    mag[1:4], mag[4:7] = fsum(np.abs(x)), fsum(np.abs(y))
    dx, dy = x - out[1:4] / n, y - out[4:7] / n
    out[7] = math.fsum(((dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2]).tolist())
    mag[7] = out[7]
    prod = dy[:, :, None] * dx[:, None, :]
    out[8:17] = fsum(prod).reshape(9)
    mag[8:17] = fsum(np.abs(prod)).reshape(9)
    return out, mag


def fit_sum_bounds(n_pairs, out, mag):
    """(bound, allowed): the componentwise bound on |kernel sums - fit_sums| (n_pairs: pairs of the call, used or not; the trees do not
    shrink with skips), and the same with 2 gamma_n in the place of the trees' figure: what two arbitrary summations may differ by"""
    n = int(out[0])
    b, allowed = np.zeros(17), np.zeros(17)
    if n == 0:
        return b, allowed
    h1, h2 = partial_depth(n_pairs), wide_depth(n_pairs)
    dm_k = gamma(min(h1, n - 1)) * mag[1:7] / n + U * np.abs(out[1:7]) / n           # the kernel's means
    dm_r = 2.0 * U * np.abs(out[1:7]) / n                                            # the restatement's: fsum, then the division
    slack = 1.0 + 1e-9
    for res, tree1, tree2 in ((b, gamma(min(h1, n - 1)) + U, gamma(min(h2, n - 1)) + U), (allowed, 2.0 * gamma(n), 2.0 * gamma(n))):
        res[1:7] = tree1 * mag[1:7]
        res[7] = (n * float((dm_k[:3] ** 2 + dm_r[:3] ** 2).sum()) + (10.0 * U + tree2) * mag[7]) * slack
        for a in range(3):
            for c in range(3):
                res[8 + 3 * a + c] = (n * (dm_k[3 + a] * dm_k[c] + dm_r[3 + a] * dm_r[c]) + (6.0 * U + tree2) * mag[8 + 3 * a + c]) * slack
    return b, allowed


def umeyama(x, y, with_scale=True):
    """(r, t, s, d) from the points themselves (not from sums); d: the singular values of the covariance"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = len(x)
    xm, ym = fsum(x) / n, fsum(y) / n
    dx, dy = x - xm, y - ym
    var = math.fsum((dx * dx).sum(1).tolist()) / n
    cov = fsum(dy[:, :, None] * dx[:, None, :]) / n
    u, d, vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0:
        S[2, 2] = -1.0
    r = u @ S @ vt
    s = float((d * np.diag(S)).sum() / var) if with_scale else 1.0
    return r, ym - s * (r @ xm), s, d


def errors(x, y, r, t, s):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    z = s * (x @ np.asarray(r).T) + t - y
    return np.sqrt((z * z).sum(1))


def error_bounds(x, y, r, t, s):
    """per-element bound on |kernel err - errors()|"""
    m = abs(s) * (np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(r)).T) + np.abs(t) + np.abs(np.asarray(y, np.float64))
    return ERR_ROUNDINGS * U * np.sqrt((m * m).sum(1))


def stat_sums(err):
    """sgr_traj_errors' stats[8] of the valid errors `err` (1-d, no NaN)"""
    e = np.sort(np.asarray(err, np.float64))
    n = len(e)
    out = np.full(8, np.nan)
    out[0] = n
    out[1], out[2], out[7] = 0.0, 0.0, 0.0
    if n == 0:
        return out
    out[1], out[2] = math.fsum(e.tolist()), math.fsum((e * e).tolist())
    out[3], out[4], out[5], out[6] = e[0], e[-1], e[(n - 1) // 2], e[n // 2]
    d = e - out[1] / n
    out[7] = math.fsum((d * d).tolist())
    return out


def stat_sum_bounds(n_pairs, out):
    """(bound, allowed) on the three sums of stats (index 1, 2, 7), as fit_sum_bounds"""
    n = int(out[0])
    h1, h2 = partial_depth(n_pairs), wide_depth(n_pairs)
    b, allowed = np.zeros(8), np.zeros(8)
    if n == 0:
        return b, allowed
    dm_k = gamma(min(h1, n - 1)) * out[1] / n + U * out[1] / n
    dm_r = 2.0 * U * out[1] / n
    slack = 1.0 + 1e-9
    for res, tree1, tree2 in ((b, gamma(min(h1, n - 1)) + U, gamma(min(h2, n - 1)) + U), (allowed, 2.0 * gamma(n), 2.0 * gamma(n))):
        res[1] = tree1 * out[1]
        res[2] = (2.0 * U + tree1) * out[2] * slack
        res[7] = (n * (dm_k ** 2 + dm_r ** 2) + (6.0 * U + tree2) * out[7]) * slack
    return b, allowed


def ape(err):
    """evo's statistics of the valid errors"""
    e = np.asarray(err, np.float64)
    sse = float((e * e).sum())
    return {"rmse": math.sqrt(sse / len(e)), "mean": float(e.mean()), "median": float(np.median(e)), "std": float(e.std()),
            "min": float(e.min()), "max": float(e.max()), "sse": sse}


def aligned_c2w(c2w, r, t, s):
    """PosePath3D.scale(s) (the translations times s), then .transform(se3(r, t)) (the poses multiplied from the left)"""
    out = []
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = r, t
    for p in np.asarray(c2w, np.float64).reshape(-1, 4, 4):
        q = p.copy()
        q[:3, 3] *= s
        out.append(T @ q)
    return np.stack(out) if out else np.zeros((0, 4, 4))


def centres_w2c(poses):
    """camera centres of world -> camera poses (t, q xyzw) in fp64: -R(q)^T t (for building test trajectories)"""
    p = np.asarray(poses, np.float64)
    t, q = p[:, :3], p[:, 3:]
    u, w = -q[:, :3], q[:, 3:4]
    c = np.cross(u, t)
    return -(t + 2.0 * (w * c + np.cross(u, c)))


def w2c_from_centres(centres, rng):
    """world -> camera poses (t, q xyzw), fp32, with random rotations, whose camera centres are close to `centres`"""
    c = np.asarray(centres, np.float64)
    q = rng.normal(size=(len(c), 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    u, w = q[:, :3], q[:, 3:4]
    cr = np.cross(u, c)
    t = -(c + 2.0 * (w * cr + np.cross(u, cr)))            # t = -R(q) c
    return np.concatenate([t, q], 1).astype(np.float32)
