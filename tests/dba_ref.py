"""fp64 numpy restatement of the tracker's dense bundle adjustment and frame geometry (droid_backends: ba, frame_distance, projmap,
iproj, depth_filter), written from the algorithm as DESIGN.md section 3 ("Dense bundle adjustment") states it.

Conventions: a pose is (t, q xyzw) and maps world to camera.  A pixel (u, v) of frame i with disparity d is the homogeneous point
X = ((u - cx)/fx, (v - cy)/fy, 1, d); the relative pose Gij = Gj Gi^-1 moves it to frame j, and its projection there is
(fx x/z + cx, fy y/z + cy).  An update xi = (tau, phi) acts on the left: G <- exp(xi) G.
"""
import numpy as np

MIN_DEPTH = 0.25
STEREO_T = np.array([-0.1, 0.0, 0.0])
SENSOR_ALPHA = 0.05
WEIGHT_SCALE = 0.001


# ---- SE3 on (t, q xyzw)
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def rotmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def relative(pi, pj):
    """Gij = Gj Gi^-1 as (t, q)."""
    qi, qj = pi[3:], pj[3:]
    q = qmul(qj, qconj(qi))
    return pj[:3] - rotmat(q) @ pi[:3], q


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def exp_se3(xi):
    tau, phi = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th = np.linalg.norm(phi)
    if th < 1e-9:
        q = np.array([0.5 * phi[0], 0.5 * phi[1], 0.5 * phi[2], 1.0])
        q /= np.linalg.norm(q)
        V = np.eye(3) + 0.5 * hat(phi)
    else:
        q = np.concatenate([np.sin(0.5 * th) / th * phi, [np.cos(0.5 * th)]])
        Ph = hat(phi)
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * Ph + (th - np.sin(th)) / th ** 3 * Ph @ Ph
    return V @ tau, q


def retract(pose, xi):
    """exp(xi) * pose."""
    dt, dq = exp_se3(xi)
    return np.concatenate([rotmat(dq) @ pose[:3] + dt, qmul(dq, pose[3:])])


def adjoint(t, q):
    """6x6 adjoint of (t, q) for twists ordered (translation, rotation)."""
    R = rotmat(q)
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[:3, 3:] = hat(t) @ R
    A[3:, 3:] = R
    return A


def pixel_rays(ht, wd, intr):
    fx, fy, cx, cy = intr
    v, u = np.meshgrid(np.arange(ht, dtype=float), np.arange(wd, dtype=float), indexing="ij")
    return u.reshape(-1), v.reshape(-1), (u.reshape(-1) - cx) / fx, (v.reshape(-1) - cy) / fy


# ---- one edge: projections, residuals and Jacobians over the pixels of frame ii
def edge_terms(pose_i, pose_j, disp_i, intr, target, weight, stereo):
    """Per pixel (P = ht*wd): Jp [P,2,6] (d proj / d xi_j), Ji [P,2,6] (d proj / d xi_i), Jz [P,2] (d proj / d disparity), residual
    r = target - proj [P,2] and the scaled weights [P,2] (zero where the point lands nearer than MIN_DEPTH)."""
    ht, wd = disp_i.shape
    fx, fy, cx, cy = intr
    _, _, xr, yr = pixel_rays(ht, wd, intr)
    h = disp_i.reshape(-1).astype(float)
    if stereo:
        t, q = STEREO_T.copy(), np.array([0.0, 0.0, 0.0, 1.0])
    else:
        t, q = relative(np.asarray(pose_i, float), np.asarray(pose_j, float))
    R = rotmat(q)
    X = np.stack([xr, yr, np.ones_like(xr)], 1) @ R.T + h[:, None] * t[None]
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    front = ~(z < MIN_DEPTH)
    d = np.where(front, 1.0 / np.where(front, z, 1.0), 0.0)
    P = h.shape[0]
    Jp = np.zeros((P, 2, 6))
    Jp[:, 0] = np.stack([fx * h * d, 0 * d, -fx * x * h * d * d, -fx * x * y * d * d, fx * (1 + x * x * d * d), -fx * y * d], 1)
    Jp[:, 1] = np.stack([0 * d, fy * h * d, -fy * y * h * d * d, -fy * (1 + y * y * d * d), fy * x * y * d * d, fy * x * d], 1)
    Ji = -np.einsum("pcn,nm->pcm", Jp, adjoint(t, q))
    Jz = np.stack([fx * (t[0] * d - t[2] * x * d * d), fy * (t[1] * d - t[2] * y * d * d)], 1)
    proj = np.stack([fx * d * x + cx, fy * d * y + cy], 1)
    r = target.reshape(2, -1).T.astype(float) - proj
    w = np.where(front[:, None], WEIGHT_SCALE * weight.reshape(2, -1).T.astype(float), 0.0)
    return Jp, Ji, Jz, r, w


def project(pose_i, pose_j, disp_i, intr, xi_i=None, xi_j=None, ddisp=0.0):
    """Projection of every pixel of frame i into frame j after the left updates xi_i, xi_j and a disparity offset (finite
    differences of the Jacobians)."""
    pi, pj = np.asarray(pose_i, float), np.asarray(pose_j, float)
    if xi_i is not None:
        pi = retract(pi, xi_i)
    if xi_j is not None:
        pj = retract(pj, xi_j)
    ht, wd = disp_i.shape
    fx, fy, cx, cy = intr
    _, _, xr, yr = pixel_rays(ht, wd, intr)
    t, q = relative(pi, pj)
    h = disp_i.reshape(-1).astype(float) + ddisp
    X = np.stack([xr, yr, np.ones_like(xr)], 1) @ rotmat(q).T + h[:, None] * t[None]
    return np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)


# ---- ba
def kept_edges(ii, jj, nv):
    """Indices of the edges whose two frames lie in [0, nv), in edge order."""
    return [e for e, (i, j) in enumerate(zip(ii, jj)) if 0 <= int(i) < nv and 0 <= int(j) < nv]


def ba(poses, disps, intr, disps_sens, targets, weights, eta, ii, jj, t0, t1, iterations, lm, ep, motion_only=False,
       depth_only=False):
    """Returns (poses, disps, dx, dz) after `iterations` Gauss-Newton steps (inputs are not modified).

    Per step: every edge contributes its pose blocks [Ji Jj]^T W [Ji Jj] and gradient [Ji Jj]^T W r where both frames lie in the
    window [t0, t1) (each block on its own: a block with a frame outside is dropped).  Stereo edges (ii == jj, fixed baseline)
    add only to the disparity terms.  The depth frames are kx = sorted unique(ii U [t0, t1)); each pixel's disparity has the
    information C = sum_e w Jz^2 + prior and gradient b = sum_e w r Jz - prior residual, the prior being SENSOR_ALPHA where the
    sensor disparity is positive and eta elsewhere.  The disparities are eliminated (Schur complement) from the system of the
    poses, which is damped (diag += ep + lm diag) and solved by Cholesky (not positive definite: dx = 0).  Back-substitution
    dz = (b - sum E^T dx) / C uses every coupling term whose pose is in the window except the first window pose t0 (as the
    reference does), then poses are retracted and disparities moved."""
    poses = np.array(poses, dtype=float)
    disps = np.array(disps, dtype=float)
    sens = np.asarray(disps_sens, float)
    keep = kept_edges(ii, jj, min(len(poses), len(disps)))      # an edge with a frame that does not exist takes part in nothing
    ii = [int(ii[e]) for e in keep]
    jj = [int(jj[e]) for e in keep]
    targets = [targets[e] for e in keep]
    weights = [weights[e] for e in keep]
    N, ht, wd = disps.shape
    P, T = ht * wd, t1 - t0
    kx = sorted(set(range(t0, t1)) | set(ii))
    krow = {f: k for k, f in enumerate(kx)}
    K = len(kx)
    assert eta.shape[0] == K
    eta = np.asarray(eta, float).reshape(K, P)
    dx = dz = None
    for _ in range(iterations):
        H = np.zeros((6 * T, 6 * T))
        g = np.zeros(6 * T)
        Csum = np.zeros((K, P))
        bsum = np.zeros((K, P))
        rows = []                  # (depth row, window pose a, E [6,P]) of every coupling term
        Ei = {f: np.zeros((6, P)) for f in range(t0, t1)}
        for e, (i, j) in enumerate(zip(ii, jj)):
            stereo = i == j
            Jp, Ji, Jz, r, w = edge_terms(poses[i], poses[j], disps[i], intr, targets[e], weights[e], stereo)
            Csum[krow[i]] += (w * Jz * Jz).sum(1)
            bsum[krow[i]] += (w * r * Jz).sum(1)
            if stereo:
                continue
            J = np.concatenate([Ji, Jp], 2)                                           # [P,2,12]
            Hb = np.einsum("pc,pcn,pcm->nm", w, J, J)
            vb = np.einsum("pc,pc,pcn->n", w, r, J)
            for (fa, ra), (fb, rb) in (((i, 0), (i, 0)), ((i, 0), (j, 6)), ((j, 6), (i, 0)), ((j, 6), (j, 6))):
                if t0 <= fa < t1 and t0 <= fb < t1:
                    a, b = fa - t0, fb - t0
                    H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += Hb[ra:ra + 6, rb:rb + 6]
            for f, ra in ((i, 0), (j, 6)):
                if t0 <= f < t1:
                    g[6 * (f - t0):6 * (f - t0) + 6] += vb[ra:ra + 6]
            Eii = np.einsum("pc,pc,pcn->np", w, Jz, Ji)
            Eij = np.einsum("pc,pc,pcn->np", w, Jz, Jp)
            if t0 <= i < t1:
                Ei[i] += Eii
            if t0 <= j < t1:
                rows.append((krow[i], j - t0, Eij))
        for f in range(t0, t1):
            rows.append((krow[f], f - t0, Ei[f]))
        if not motion_only:
            m = sens[kx].reshape(K, P) > 0
            C = Csum + np.where(m, SENSOR_ALPHA, eta)
            w_ = bsum - np.where(m, SENSOR_ALPHA * (disps[kx].reshape(K, P) - sens[kx].reshape(K, P)), 0.0)
            Q = 1.0 / C
            for k in range(K):
                mine = [(a, E) for (kk, a, E) in rows if kk == k]
                for a, Ea in mine:
                    g[6 * a:6 * a + 6] -= Ea @ (Q[k] * w_[k])
                    for b, Eb in mine:
                        H[6 * a:6 * a + 6, 6 * b:6 * b + 6] -= (Ea * Q[k]) @ Eb.T
        Hd = H.copy()
        Hd[np.diag_indices_from(Hd)] += ep + lm * np.diag(H)
        try:
            L = np.linalg.cholesky(Hd)
            x = np.linalg.solve(L.T, np.linalg.solve(L, g))
        except np.linalg.LinAlgError:
            x = np.zeros(6 * T)
        dx = x.reshape(T, 6)
        if motion_only or not depth_only:
            for a in range(T):
                poses[t0 + a] = retract(poses[t0 + a], dx[a])
        if not motion_only:
            s = np.zeros((K, P))
            for (k, a, E) in rows:
                if a >= 1:
                    s[k] += dx[a] @ E
            dz = Q * (w_ - s)
            for k, f in enumerate(kx):
                disps[f] += dz[k].reshape(ht, wd)
    return poses, disps, dx, dz


# ---- frame geometry
def frame_distance(poses, disps, intr, ii, jj, beta):
    fx, fy, cx, cy = intr
    out = []
    nv = min(len(poses), len(disps))
    for i, j in zip(ii, jj):
        i, j = int(i), int(j)
        if not (0 <= i < nv and 0 <= j < nv):        # a frame that does not exist: NaN
            out.append(np.nan)
            continue
        ht, wd = disps[i].shape
        u, v, xr, yr = pixel_rays(ht, wd, intr)
        h = disps[i].reshape(-1).astype(float)
        t, q = relative(np.asarray(poses[i], float), np.asarray(poses[j], float))
        X = np.stack([xr, yr, np.ones_like(xr)], 1) @ rotmat(q).T + h[:, None] * t[None]
        X2 = np.stack([xr, yr, np.ones_like(xr)], 1) + h[:, None] * t[None]
        acc = valid = 0.0
        total = u.size * (beta + (1 - beta))
        for Y, wgt in ((X, beta), (X2, 1 - beta)):
            flow = np.hypot(fx * Y[:, 0] / Y[:, 2] + cx - u, fy * Y[:, 1] / Y[:, 2] + cy - v)
            ok = Y[:, 2] > MIN_DEPTH
            acc += wgt * flow[ok].sum()
            valid += wgt * ok.sum()
        out.append(1000.0 if valid / (total + 1e-8) < 0.75 else acc / valid)
    return np.array(out)


def projmap(poses, disps, intr, ii, jj):
    fx, fy, cx, cy = intr
    ht, wd = disps.shape[1:]
    coords = np.zeros((len(ii), ht, wd, 3))
    valid = np.zeros((len(ii), ht, wd, 1))
    nv = min(len(poses), len(disps))
    for e, (i, j) in enumerate(zip(ii, jj)):
        i, j = int(i), int(j)
        if not (0 <= i < nv and 0 <= j < nv):        # a frame that does not exist: NaN coordinates, valid = 0
            coords[e] = np.nan
            continue
        u, v, xr, yr = pixel_rays(ht, wd, intr)
        t, q = relative(np.asarray(poses[i], float), np.asarray(poses[j], float))
        h = disps[i].reshape(-1).astype(float)
        X = np.stack([xr, yr, np.ones_like(xr)], 1) @ rotmat(q).T + h[:, None] * t[None]
        front = X[:, 2] > 0.01
        coords[e, ..., 0] = np.where(front, fx * X[:, 0] / X[:, 2] + cx, u).reshape(ht, wd)
        coords[e, ..., 1] = np.where(front, fy * X[:, 1] / X[:, 2] + cy, v).reshape(ht, wd)
        valid[e, ..., 0] = (X[:, 2] > MIN_DEPTH).reshape(ht, wd)
    return coords, valid


def iproj(poses, disps, intr):
    n, ht, wd = disps.shape
    _, _, xr, yr = pixel_rays(ht, wd, intr)
    out = np.zeros((n, ht, wd, 3))
    for f in range(n):
        p = np.asarray(poses[f], float)
        h = disps[f].reshape(-1).astype(float)
        X = np.stack([xr, yr, np.ones_like(xr)], 1) @ rotmat(p[3:]).T + h[:, None] * p[None, :3]
        out[f] = (X / h[:, None]).reshape(ht, wd, 3)
    return out


def depth_filter_neighbours(ix, n):
    """The six frames compared with frame ix: three before it and ix+3, ix+4, ix+5 (the reference's choice), inside [0, n)."""
    return [j for j in (ix - 1, ix - 2, ix - 3, ix + 3, ix + 4, ix + 5) if 0 <= j < n]


def depth_filter(poses, disps, intr, inds, thresh, margins=False):
    """Per pixel of each frame ix: the number of neighbours in which one of the four disparities around the reprojection gives a
    depth within thresh of the reprojected depth.  With margins=True also returns, per pixel, the smallest distance of any
    decision (floor of the reprojection, depth comparison) from its threshold, so tests can avoid the knife edge."""
    fx, fy, cx, cy = intr
    n, ht, wd = disps.shape
    _, _, xr, yr = pixel_rays(ht, wd, intr)
    out = np.zeros((len(inds), ht, wd))
    marg = np.full((len(inds), ht * wd), np.inf)
    for b, ix in enumerate(inds):
        ix = int(ix)
        h = disps[ix].reshape(-1).astype(float)
        cnt = np.zeros(ht * wd)
        for j in depth_filter_neighbours(ix, n):
            t, q = relative(np.asarray(poses[ix], float), np.asarray(poses[j], float))
            X = np.stack([xr, yr, np.ones_like(xr)], 1) @ rotmat(q).T + h[:, None] * t[None]
            uj, vj, dj = fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy, h / X[:, 2]
            u0, v0 = np.floor(uj), np.floor(vj)
            inside = (u0 >= 0) & (v0 >= 0) & (u0 < wd - 1) & (v0 < ht - 1)
            fu = np.minimum(np.abs(uj - np.round(uj)), np.abs(vj - np.round(vj)))
            edge = np.minimum.reduce([np.abs(uj), np.abs(vj), np.abs(uj - (wd - 1)), np.abs(vj - (ht - 1))])
            marg[b] = np.minimum(marg[b], np.minimum(fu, edge))
            uu, vv = np.clip(u0, 0, wd - 2).astype(int), np.clip(v0, 0, ht - 2).astype(int)
            dn = disps[j].astype(float)
            hit = np.zeros(ht * wd, bool)
            for dv, du in ((0, 0), (0, 1), (1, 0), (1, 1)):
                diff = np.abs(1.0 / dj - 1.0 / dn[vv + dv, uu + du])
                hit |= diff < thresh[b]
                marg[b] = np.where(inside, np.minimum(marg[b], np.abs(diff - thresh[b]) / max(thresh[b], 1e-12)), marg[b])
            cnt += inside & hit
        out[b] = cnt.reshape(ht, wd)
    if margins:
        return out, marg.reshape(len(inds), ht, wd)
    return out


# ================================================================================================================================
# One linearisation with magnitudes: what the three criteria of tests/dba_cases.py are held to
# ================================================================================================================================
# Every quantity the kernels form in fp32 is carried as a triple (value, magnitude, units) -- `Mag` -- through the SAME sequence of
# operations as csrc/sgr_dba.hip and sgr_dba_device.h, so that
#
#     |computed - value| <= units * 2^-24 * magnitude        (first order in 2^-24)
#
# holds for any fp32 evaluation of that sequence, with or without FMA contraction (an FMA only removes a rounding), and for a sum
# in any order.  The rules, each the standard one-step bound with |a| <= M_a:
#     input (an fp32 number the kernel reads)      M = |v|,            units 0
#     constant that fp32 does not hold exactly     M = |v|,            units 1      (0.001, 0.05, -0.1; 1, 2, 0.5 are exact)
#     a +- b                                        M = M_a + M_b,      units max(u_a, u_b) + 1
#     a * b                                         M = max(M_a |b|, M_b |a|),           units u_a + u_b + 1
#     a / b                                         M = max(M_a / |b|, |a| M_b / b^2),   units u_a + u_b + 2     (1 ulp of the HIP tables = 2 units)
#         (the error of a product is e_a |b| + e_b |a| + 2^-24 |a b|: each factor's inflation M / |v| enters once, they do not multiply)
#     sqrt(a), a a sum of squares (M_a = a)         M = sqrt(a),        units ceil(u_a / 2) + 2
#     sin(a), cos(a)                                M = |f| + |a f'(a)|, units u_a + 2           (the rounded argument moves f by |a f'| per unit)
#     a sum of N > 1 terms                          M = sum M_i,        units max u_i + N       ("addends + per-addend count")
# Multiplying by 2, 0.5 or -1 is exact.  A difference therefore always enters at the size of its operands: the residual is carried as
# |target| + |proj|, the sums inside rel_se3 / act_so3 / adjT_se3 as the sum of their products' sizes, 1 + x^2 d^2 as 1 + |x^2 d^2|,
# (1 - cos a) / a^2 as (1 + |cos a| + a |sin a|) / a^2: its error is 2^-24 / a^2 times a small count, not hidden in a constant.
#
# Per-addend units that follow from the formulas (`linearize` reports the largest met per quantity in `units`; DESIGN.md section 3
# tabulates them; tests/test_dba_cpu.py pins them).  A component of qij is a sum of four 1-unit products: 4.  act_so3(q, X) forms
# uv = 2 (q X - q X): u_q + u_X + 2, then X + q uv + (q uv - q uv): u_q + u_uv + 1 for the product and two more additions, u_uv + u_q + 3
# = 2 u_q + u_X + 5; so R ti has 13 and tij = tj - R ti 14.  A ray component (pixel - c) / f has 3, the transformed point
# act_so3(qij, Xi) + h tij has 17, d = 1 / z 19 and d^2 39.  The longest Jacobian entry is fx (1 + x x d^2): 35 for x x, 75 with d^2,
# 77 after the sum and the focal length.  Ji = -adjT_se3(tij, qij, Jj) rotates Jj (2 * 4 + 77 + 5 = 90) and adds the rotated cross
# term tij x Jj: at most 107.  The weight 0.001 w has 2 units (the literal, the product), so an addend (w Jn) Jm of a pose
# block has u_w + u_Jn + 1 + u_Jm + 1 units, 186 for the longest pair that is formed; (w r) Jn 135; w Jz Jn 170 and the sum over
# the two components 171 (two addends).  Cii = sum of two w Jz Jz: 154; bz = sum of two w r Jz: 120.
#
# The fp64 parts of the kernel (the CSR sums of the pose blocks, the damping, the Cholesky, the substitutions) get a term of the same
# form scaled by 2^-53 (`bound64`, and `fp64_solve_term` for the factorisation).
U32 = 2.0 ** -24
U64 = 2.0 ** -53
DENORMAL = 2.0 ** -149


def bound(addends, units, magnitude):
    """(addends + per-addend count) * 2^-24 * magnitude: a fixed-order fp32 sum of `addends` terms, in any order, FMA or not."""
    return (addends + units) * U32 * magnitude


def bound64(addends, magnitude):
    """the same for a sum the kernel forms in fp64 (each addend converted exactly from fp32)"""
    return (addends + 2) * U64 * magnitude


class Mag:
    """(value v, magnitude m >= |v|, units c): see the rules above.  v has the dtype of the run, m is always fp64."""
    __slots__ = ("v", "m", "c")

    def __init__(self, v, m=None, c=0):
        self.v = v if isinstance(v, np.ndarray) else np.asarray(v)
        self.m = np.abs(self.v).astype(np.float64) if m is None else m
        self.c = c

    def _o(self, b):
        return b if isinstance(b, Mag) else const(b, self.v.dtype)

    def __add__(self, b):
        b = self._o(b)
        return Mag(self.v + b.v, self.m + b.m, max(self.c, b.c) + 1)

    def __sub__(self, b):
        b = self._o(b)
        return Mag(self.v - b.v, self.m + b.m, max(self.c, b.c) + 1)

    def __mul__(self, b):
        b = self._o(b)
        return Mag(self.v * b.v, np.maximum(self.m * np.abs(b.v), b.m * np.abs(self.v)).astype(np.float64), self.c + b.c + 1)

    def __getitem__(self, idx):
        return Mag(self.v[idx], self.m[idx], self.c)

    def __neg__(self):
        return Mag(-self.v, self.m, self.c)

    def __truediv__(self, b):
        b = self._o(b)
        bv = np.abs(b.v.astype(np.float64))
        return Mag(self.v / b.v, np.maximum(self.m / bv, np.abs(self.v) * b.m / bv ** 2), self.c + b.c + 2)

    def scaled(self, k):
        """times a power of two or -1: exact"""
        return Mag(self.v * self.v.dtype.type(k), self.m * abs(k), self.c)

    def where(self, mask, other=0.0):
        o = self._o(other)
        return Mag(np.where(mask, self.v, o.v), np.where(mask, self.m, o.m), max(self.c, o.c))

    def sum(self, axis=-1):
        n = self.v.shape[axis]
        return Mag(self.v.sum(axis, dtype=self.v.dtype), self.m.sum(axis), self.c + (n if n > 1 else 0))

    def sqrt(self):
        return Mag(np.sqrt(self.v), np.sqrt(self.m), -(-self.c // 2) + 2)

    def sin(self):
        x = self.v.astype(np.float64)
        return Mag(np.sin(self.v), np.abs(np.sin(x)) + np.abs(x * np.cos(x)) * (self.m / np.where(x == 0, 1.0, np.abs(x))), self.c + 2)

    def cos(self):
        x = self.v.astype(np.float64)
        return Mag(np.cos(self.v), np.abs(np.cos(x)) + np.abs(x * np.sin(x)) * (self.m / np.where(x == 0, 1.0, np.abs(x))), self.c + 2)

    def bound(self):
        return self.c * U32 * self.m + DENORMAL


def const(x, dt):
    """a literal of the kernel: exact when fp32 holds it, one unit otherwise"""
    x = float(x)
    return Mag(np.asarray(x, dt), np.asarray(abs(x)), 0 if float(np.float32(x)) == x else 1)


def msum(terms):
    """a running sum of a list of Mag, in list order"""
    v, m = terms[0].v, terms[0].m
    for t in terms[1:]:
        v, m = v + t.v, m + t.m
    n = len(terms)
    return Mag(v, m, max(t.c for t in terms) + (n if n > 1 else 0))


def mstack(terms):
    shape = np.broadcast_shapes(*[t.v.shape for t in terms])
    return Mag(np.stack([np.broadcast_to(t.v, shape) for t in terms]), np.stack([np.broadcast_to(t.m, shape) for t in terms]),
               max(t.c for t in terms))


def m_act_so3(q, X):
    uv0 = (q[1] * X[2] - q[2] * X[1]).scaled(2)
    uv1 = (q[2] * X[0] - q[0] * X[2]).scaled(2)
    uv2 = (q[0] * X[1] - q[1] * X[0]).scaled(2)
    return [X[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1), X[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2),
            X[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0)]


def m_rel_se3(pi, pj):
    ti, qi, tj, qj = pi[:3], pi[3:], pj[:3], pj[3:]
    q = [-(qj[3] * qi[0]) + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1], -(qj[3] * qi[1]) + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2],
         -(qj[3] * qi[2]) + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0], qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2]]
    r = m_act_so3(q, ti)
    return [tj[0] - r[0], tj[1] - r[1], tj[2] - r[2]], q


def m_adjT_se3(t, q, X):
    qinv = [-q[0], -q[1], -q[2], q[3]]
    Y = m_act_so3(qinv, X[:3]) + m_act_so3(qinv, X[3:])
    u = [t[2] * X[1] - t[1] * X[2], t[0] * X[2] - t[2] * X[0], t[1] * X[0] - t[0] * X[1]]
    v = m_act_so3(qinv, u)
    return Y[:3] + [Y[3] + v[0], Y[4] + v[1], Y[5] + v[2]]


def _vec(a, dt):
    return [Mag(np.asarray(x, dt)) for x in a]


def m_edge(pose_i, pose_j, disp_i, intr, target, weight, stereo, dt, drop_last=False):
    """linearize_kernel for one edge.  Returns a dict of Mag: Hs [12,12] and vs [12] (sums over 2P addends; None for a stereo edge,
    whose pose weights are zero), Eii, Eij [6,P], Cii, bz [P]; and the distance of z from MIN_DEPTH per pixel."""
    ht, wd = disp_i.shape
    P = ht * wd
    fx, fy, cx, cy = _vec(intr, dt)
    if stereo:
        t, q = [const(STEREO_T[0], dt), const(0, dt), const(0, dt)], [const(0, dt), const(0, dt), const(0, dt), const(1, dt)]
    else:
        t, q = m_rel_se3(_vec(pose_i, dt), _vec(pose_j, dt))
    k = np.arange(P)
    Xi = [(Mag((k % wd).astype(dt)) - cx) / fx, (Mag((k // wd).astype(dt)) - cy) / fy, const(1, dt)]
    h = Mag(np.asarray(disp_i, dt).reshape(-1))
    Y = m_act_so3(q, Xi)
    x, y, z = Y[0] + h * t[0], Y[1] + h * t[1], Y[2] + h * t[2]
    front = ~(z.v < dt(MIN_DEPTH))
    zs = z.where(front, 1.0)
    d = (const(1, dt) / zs).where(front, 0.0)
    d2 = d * d
    tg, wt = np.asarray(target, dt).reshape(2, P), np.asarray(weight, dt).reshape(2, P)
    zero, one = const(0, dt), const(1, dt)
    J2, Jz2, w2, r2 = [], [], [], []
    for c2 in range(2):
        if c2 == 0:
            Jj = [fx * (h * d), zero, fx * ((-x) * h * d2), fx * ((-x) * y * d2), fx * (one + x * x * d2), fx * ((-y) * d)]
            Jz = fx * (t[0] * d - t[2] * (x * d2))
            r = Mag(tg[0]) - (fx * d * x + cx)
        else:
            Jj = [zero, fy * (h * d), fy * ((-y) * h * d2), fy * (-one - y * y * d2), fy * (x * y * d2), fy * (x * d)]
            Jz = fy * (t[1] * d - t[2] * (y * d2))
            r = Mag(tg[1]) - (fy * d * y + cy)
        Ji = [-a for a in m_adjT_se3(t, q, Jj)]
        J2.append(mstack(Ji + Jj))                                               # [12,P]
        Jz2.append(Jz)
        w2.append((const(WEIGHT_SCALE, dt) * Mag(wt[c2])).where(front, 0.0))
        r2.append(r)
    out = dict(zdist=np.abs(z.v.astype(np.float64) - MIN_DEPTH), behind=int((~front).sum()))
    out["Cii"] = msum([w2[c] * Jz2[c] * Jz2[c] for c in range(2)])
    out["bz"] = msum([w2[c] * r2[c] * Jz2[c] for c in range(2)])
    if stereo:
        return out
    cat = lambda a, b: Mag(np.concatenate([a.v, b.v], -1), np.concatenate([a.m, b.m], -1), max(a.c, b.c))
    lim = 2 * P - 1 if drop_last else 2 * P

    def cut(a):
        return Mag(a.v[..., :lim], a.m[..., :lim], a.c)
    wJ = [w2[c][None] * J2[c] for c in range(2)]
    Hp = [wJ[c][:, None] * J2[c][None] for c in range(2)]
    out["Hs"] = cut(cat(Hp[0], Hp[1])).sum()                                    # [12,12]: (w Jn) Jm over pixels and components
    wr = [w2[c] * r2[c] for c in range(2)]
    vp = [wr[c][None] * J2[c] for c in range(2)]
    out["vs"] = cut(cat(vp[0], vp[1])).sum()                                    # [12]
    wz = [w2[c] * Jz2[c] for c in range(2)]
    E = msum([wz[c][None] * J2[c] for c in range(2)])                           # [12,P]
    out["Eii"], out["Eij"] = E[:6], E[6:]
    return out


def linearize(poses, disps, intr, disps_sens, targets, weights, eta, ii, jj, t0, t1, lm, ep, motion_only=False, dtype=np.float64,
              mutate=None):
    """One linearisation at (poses, disps), as the kernels of one ba iteration form it, every fp32 quantity with its magnitude.

    dtype=np.float32 runs the same restatement in fp32 (the fp64 parts of the kernel stay fp64): the stand-in for the kernel on the
    CPU.  `mutate` plants one of the faults of tests/test_dba_cpu.py.  Returns a dict:
        keep, kx, T, K, P       kept edges (both frames in [0, nv)), depth frames, sizes
        H [6T,6T], g [6T]       the damped reduced system (fp64), H_bound, g_bound entrywise, H_mag, g_mag, H_addends, g_addends
        C, w, Q                 Mag [K,P] per depth row and pixel (None under motion_only)
        F                       {(k, a): Mag [6,P]}: the coupling rows, duplicates merged
        units                   the largest per-addend count met, per quantity
        zmargin, behind         smallest |z - MIN_DEPTH| of any pixel of any edge; how many pixels lie behind it
        fail                    the factorisation of H fails (not positive definite)"""
    dt = dtype
    poses, disps = np.asarray(poses, np.float64), np.asarray(disps, np.float64)
    nv = min(len(poses), len(disps))
    keep = kept_edges(ii, jj, nv)
    if mutate == "clamp_oob":            # a bad jj is clamped into range instead of dropping the edge
        rows = set(range(t0, t1)) | {int(ii[e]) for e in keep}                   # (the depth rows stay the true ones)
        keep = [e for e in range(len(ii)) if int(ii[e]) in rows]
        jj = [min(max(int(v), 0), nv - 1) for v in jj]
    ei, ej = [int(ii[e]) for e in keep], [int(jj[e]) for e in keep]
    N, ht, wd = disps.shape
    P, T = ht * wd, t1 - t0
    kx = sorted(set(range(t0, t1)) | set(ei))
    krow = {f: k for k, f in enumerate(kx)}
    K, n6 = len(kx), 6 * T
    inwin = lambda f: t0 <= f < t1
    units = {}

    def note(name, m):
        units[name] = max(units.get(name, 0), m.c)
        return m

    terms, zmargin, behind = [], np.inf, 0
    first_pose_edge = True
    for n, e in enumerate(keep):
        i, j = ei[n], ej[n]
        drop = mutate == "drop_last_pixel" and i != j and inwin(i) and inwin(j) and first_pose_edge
        if drop:
            first_pose_edge = False
        tm = m_edge(poses[i], poses[j], disps[i], intr, targets[e], weights[e], i == j, dt, drop_last=drop)
        zmargin, behind = min(zmargin, tm["zdist"].min()), behind + tm["behind"]
        note("Cii", tm["Cii"]), note("bz", tm["bz"])
        if i != j:
            note("Hs", tm["Hs"]), note("vs", tm["vs"]), note("E", tm["Eii"])
        terms.append(tm)

    # ---- pose blocks: fp64 sums (CSR order) of the fp32 per-edge records
    H, Hb, Hm = np.zeros((n6, n6)), np.zeros((n6, n6)), np.zeros((n6, n6))
    g, gb, gm = np.zeros(n6), np.zeros(n6), np.zeros(n6)
    Hn, gn = np.zeros((n6, n6)), np.zeros(n6)                                  # fp64 addends per entry
    for n, tm in enumerate(terms):
        i, j = ei[n], ej[n]
        if i == j:
            continue
        Hs, vs = tm["Hs"], tm["vs"]
        hv = Hs.v.astype(np.float64)
        if mutate == "swap_Hij":
            hv = hv.copy()
            hv[:6, 6:], hv[6:, :6] = hv[:6, 6:].T.copy(), hv[6:, :6].T.copy()
        hbnd = bound(0, Hs.c, Hs.m)
        for (fa, ra), (fb, rb) in (((i, 0), (i, 0)), ((i, 0), (j, 6)), ((j, 6), (i, 0)), ((j, 6), (j, 6))):
            if inwin(fa) and inwin(fb):
                sa, sb = slice(6 * (fa - t0), 6 * (fa - t0) + 6), slice(6 * (fb - t0), 6 * (fb - t0) + 6)
                H[sa, sb] += hv[ra:ra + 6, rb:rb + 6]
                Hb[sa, sb] += hbnd[ra:ra + 6, rb:rb + 6]
                Hm[sa, sb] += Hs.m[ra:ra + 6, rb:rb + 6]
                Hn[sa, sb] += 1
        for f, ra in ((i, 0), (j, 6)):
            if inwin(f):
                sa = slice(6 * (f - t0), 6 * (f - t0) + 6)
                g[sa] += vs.v[ra:ra + 6].astype(np.float64)
                gb[sa] += bound(0, vs.c, vs.m[ra:ra + 6])
                gm[sa] += vs.m[ra:ra + 6]
                gn[sa] += 1

    C = w_ = Q = None
    F = {}
    if not motion_only:
        # ---- depth rows: C, w, Q per pixel
        Cs, ws, Qs = [], [], []
        sens = np.asarray(disps_sens, np.float64)
        eta = np.asarray(eta, np.float64).reshape(K, P)
        seen, skipped_c = set(), False
        for k, f in enumerate(kx):
            mine = []
            for n in range(len(keep)):
                if ei[n] != f:
                    continue
                if mutate == "dup_skip_C" and not skipped_c and (ei[n], ej[n]) in seen:     # the second of two duplicates is left out
                    skipped_c = True
                    continue
                seen.add((ei[n], ej[n]))
                mine.append(n)
            has = Mag(np.asarray(sens[f].reshape(-1), dt)).v > 0
            alpha = const(SENSOR_ALPHA, dt)
            prior_c = Mag(np.where(has, alpha.v, np.asarray(eta[k], dt)), np.where(has, alpha.m, np.abs(eta[k])), alpha.c)
            c = msum([terms[n]["Cii"] for n in mine] + [prior_c])
            pr = (alpha * (Mag(np.asarray(disps[f].reshape(-1), dt)) - Mag(np.asarray(sens[f].reshape(-1), dt)))).where(has, 0.0)
            wsum = msum([terms[n]["bz"] for n in mine]) if mine else const(0, dt)
            wk = wsum - pr
            wk = Mag(np.broadcast_to(wk.v, (P,)), np.broadcast_to(wk.m, (P,)), wk.c)
            Cs.append(note("C", c)), ws.append(note("w", wk)), Qs.append(note("Q", const(1, dt) / c))
        C, w_, Q = mstack(Cs), mstack(ws), mstack(Qs)
        # ---- slots: Ei[a] of the window frames, merged Eij of every (ii -> window pose) group
        for a in range(T):
            f = t0 + a
            mine = [terms[n]["Eii"] for n in range(len(keep)) if ei[n] == f and ej[n] != f]
            F[(krow[f], a)] = note("F", msum(mine)) if mine else Mag(np.zeros((6, P), dt))
        groups = {}
        for n in range(len(keep)):
            if ei[n] != ej[n] and inwin(ej[n]):
                groups.setdefault((krow[ei[n]], ej[n] - t0), []).append(n)
        skipped = False
        for key, mem in groups.items():
            if mutate == "dup_skip_E" and len(mem) > 1 and not skipped:
                mem, skipped = mem[:1] + mem[2:], True
            F[key] = note("F", msum([terms[n]["Eij"] for n in mem]))
        # ---- Schur complement: one fp32 sum per (a, b) over every shared depth row and pixel
        for a in range(T):
            for b in range(a + 1):
                rows = [k for k in range(K) if (k, a) in F and (k, b) in F]
                if not rows:
                    continue
                Fa = Mag(np.concatenate([F[(k, a)].v for k in rows], 1), np.concatenate([F[(k, a)].m for k in rows], 1),
                         max(F[(k, a)].c for k in rows))
                Fb = Mag(np.concatenate([F[(k, b)].v for k in rows], 1), np.concatenate([F[(k, b)].m for k in rows], 1),
                         max(F[(k, b)].c for k in rows))
                q = Mag(np.concatenate([Q.v[k] for k in rows]), np.concatenate([Q.m[k] for k in rows]), Q.c)
                S = note("S", ((Fa * q[None])[:, None] * Fb[None]).sum())                                          # [6,6]
                sa, sb = slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6)
                H[sa, sb] -= S.v.astype(np.float64)
                Hb[sa, sb] += S.bound()
                Hm[sa, sb] += S.m
                Hn[sa, sb] += 1
                if a != b:
                    H[sb, sa] -= S.v.astype(np.float64).T
                    Hb[sb, sa] += S.bound().T
                    Hm[sb, sa] += S.m.T
                    Hn[sb, sa] += 1
                else:
                    QW = Q * w_
                    qw = Mag(np.concatenate([QW.v[k] for k in rows]), np.concatenate([QW.m[k] for k in rows]), QW.c)
                    sg = note("Sg", (Fa * qw[None]).sum())                                                         # [6]
                    g[sa] -= sg.v.astype(np.float64)
                    gb[sa] += sg.bound()
                    gm[sa] += sg.m
                    gn[sa] += 1
    # ---- fp64: the sums above and the damping diag += ep + lm diag (lm, ep reach the kernel as fp32)
    lm, ep = float(np.float32(lm)), float(np.float32(ep))
    Hb += bound64(Hn, Hm)
    gb += bound64(gn, gm)
    dg = np.diag_indices(n6)
    Hb[dg] = Hb[dg] * (1 + lm) + 3 * U64 * (ep + (1 + lm) * Hm[dg])
    Hm[dg] = ep + (1 + lm) * Hm[dg]
    H[dg] += ep + lm * H[dg]
    try:
        np.linalg.cholesky(H)
        fail = not bool(np.all(np.diag(H) > 0))
    except np.linalg.LinAlgError:
        fail = True
    return dict(keep=keep, kx=kx, T=T, K=K, P=P, t0=t0, H=H, g=g, H_bound=Hb, g_bound=gb, H_mag=Hm, g_mag=gm, H_addends=Hn,
                g_addends=gn, C=C, w=w_, Q=Q, F=F, units=units, zmargin=float(zmargin), behind=behind, fail=fail, dtype=dt)


def blocked_cholesky(H, nb=64, skip_tile=None):
    """The kernel's right-looking blocked factorisation (potrf, trsm, syrk of the trailing lower tiles) in fp64.  skip_tile =
    (kb, ib, jb) leaves that one trailing-tile update out (a planted fault).  Returns L, or None when a pivot is not > 0."""
    A = np.tril(H).astype(np.float64)
    n = A.shape[0]
    nbk = (n + nb - 1) // nb
    for kb in range(nbk):
        k0, k1 = kb * nb, min(n, kb * nb + nb)
        try:
            A[k0:k1, k0:k1] = np.linalg.cholesky(A[k0:k1, k0:k1] + np.tril(A[k0:k1, k0:k1], -1).T)
        except np.linalg.LinAlgError:
            return None
        if k1 < n:
            A[k1:, k0:k1] = np.linalg.solve(A[k0:k1, k0:k1], A[k1:, k0:k1].T).T
            for ib in range(kb + 1, nbk):
                for jb in range(kb + 1, ib + 1):
                    if skip_tile == (kb, ib, jb):
                        continue
                    r, c = slice(ib * nb, min(n, ib * nb + nb)), slice(jb * nb, min(n, jb * nb + nb))
                    A[r, c] -= A[r, k0:k1] @ A[c, k0:k1].T
            A[:] = np.tril(A)
    return A


def solve(sys, mutate=None):
    """dx [T,6] of the damped system in fp64 (0 where the factorisation fails), as solve_kernel leaves it"""
    n6 = 6 * sys["T"]
    if sys["fail"]:
        return np.zeros((sys["T"], 6))
    L = blocked_cholesky(sys["H"], skip_tile=(0, 1, 1) if mutate == "chol_skip_tile" else None)
    if L is None:
        return np.zeros((sys["T"], 6))
    return np.linalg.solve(L.T, np.linalg.solve(L, sys["g"])).reshape(sys["T"], 6)


def fp64_solve_term(sys, dx):
    """Row-wise residual the fp64 factorisation and substitutions may leave: |dH| <= (3n + 2) 2^-53 |L| |L^T| (Higham, Accuracy and
    Stability, Thm 10.4), and (|L| |L^T|)_rc <= sqrt(H_rr H_cc) by Cauchy-Schwarz on the rows of L."""
    s = np.sqrt(np.abs(np.diag(sys["H"])))
    return (3 * len(s) + 2) * U64 * s * (s @ np.abs(np.asarray(dx, np.float64).reshape(-1)))


def back_substitute(sys, dx, dtype=np.float64, mutate=None):
    """dz_kernel: Mag [K,P] of Q (w - sum_{a >= 1} F_(k,a) . dx[a]) at the given dx (taken as exact fp32 inputs)"""
    dt = dtype
    dx = np.asarray(dx, dt).reshape(sys["T"], 6)
    rows = []
    dropped = False
    for k in range(sys["K"]):
        parts = []
        for a in range(sys["T"]):
            if (k, a) not in sys["F"] or (a < 1 and mutate != "no_t0_skip"):
                continue
            if mutate == "dz_missing_edge" and not dropped and sys["kx"][k] != sys["t0"] + a and np.any(sys["F"][(k, a)].v != 0):
                dropped = True
                continue
            Fk = sys["F"][(k, a)]
            parts.append(msum([Fk[n] * Mag(dx[a, n]) for n in range(6)]))
        inner = sys["w"][k] - msum(parts) if parts else sys["w"][k]
        rows.append(sys["Q"][k] * inner)
    return mstack(rows)


def _cross_m(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def retract_mag(pose, xi, dtype=np.float64):
    """pose_retr_kernel for one pose: (list of 7 Mag, extra [7]).  In fp64 the value is the exact retraction exp(xi) * pose; the
    kernel's exp_se3 keeps the cancelling (1 - cos a)/a^2 and (a - sin a)/a^3, which Mag carries at (1 + |cos a| + a |sin a|) / a^2
    and (a + |sin a| + a |cos a|) / a^3 times the cross products they multiply, and at a <= 1e-4 drops both terms: `extra` is then
    the size of what was dropped (a truncation, added to the bound as it stands)."""
    dt = dtype
    P, X = _vec(pose, dt), _vec(xi, dt)
    t, q, tau, phi = P[:3], P[3:], X[:3], X[3:]
    th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    th = th2.sqrt()
    x32 = np.asarray(xi, np.float32)
    th2_32 = np.float32(x32[3] * x32[3] + x32[4] * x32[4]) + x32[5] * x32[5]
    if th2_32 < np.float32(1e-8):
        th4 = th2 * th2
        imag = const(0.5, dt) - const(1 / 48, dt) * th2 + const(1 / 3840, dt) * th4
        real = const(1, dt) - const(0.125, dt) * th2 + const(1 / 384, dt) * th4
    else:
        imag = th.scaled(0.5).sin() / th
        real = th.scaled(0.5).cos()
    dq = [imag * phi[0], imag * phi[1], imag * phi[2], real]
    extra = np.zeros(7)
    dtr = list(tau)
    if np.sqrt(th2_32) > np.float32(1e-4):
        c1 = _cross_m(phi, tau)
        c2 = _cross_m(phi, c1)
        a = (const(1, dt) - th.cos()) / th2
        b = (th - th.sin()) / (th * th2)
        dtr = [dtr[n] + a * c1[n] + b * c2[n] for n in range(3)]
    elif float(th.v) > 0 and dt == np.float64:
        p, u = np.asarray(xi[3:], np.float64), np.asarray(xi[:3], np.float64)
        c1 = np.cross(p, u)
        c2 = np.cross(p, c1)
        full = 0.5 * c1 + c2 / 6.0
        dtr = [Mag(dtr[n].v + full[n], dtr[n].m, dtr[n].c) for n in range(3)]
        extra[:3] = np.abs(0.5 * c1) + np.abs(c2 / 6.0)
    q1 = [dq[3] * q[0] + dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1], dq[3] * q[1] + dq[1] * q[3] + dq[2] * q[0] - dq[0] * q[2],
          dq[3] * q[2] + dq[2] * q[3] + dq[0] * q[1] - dq[1] * q[0], dq[3] * q[3] - dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2]]
    r = m_act_so3(dq, t)
    return [r[0] + dtr[0], r[1] + dtr[1], r[2] + dtr[2]] + q1, extra


def emulate(poses, disps, intr, disps_sens, targets, weights, eta, ii, jj, t0, t1, lm, ep, motion_only=False, depth_only=False,
            dtype=np.float32, mutate=None):
    """One ba iteration through `linearize`, `solve`, `back_substitute` and `retract_mag` in `dtype`: (poses, disps, dx, dz) as fp32
    arrays (dz None under motion_only), the stand-in for the device on the CPU."""
    f32 = lambda a: np.asarray(a, np.float32)
    poses, disps = f32(poses).copy(), f32(disps).copy()
    sys = linearize(poses, disps, intr, disps_sens, targets, weights, eta, ii, jj, t0, t1, lm, ep, motion_only, dtype, mutate)
    dx = f32(solve(sys, mutate))
    if motion_only or not depth_only:
        for a in range(sys["T"]):
            comp, _ = retract_mag(poses[t0 + a], dx[a], dtype)
            poses[t0 + a] = f32([c.v for c in comp])
    dz = None
    if not motion_only:
        dz = f32(back_substitute(sys, dx, dtype, mutate).v)
        ht, wd = disps.shape[1:]
        for k, f in enumerate(sys["kx"]):
            disps[f] = f32(disps[f] + dz[k].reshape(ht, wd))
    return poses, disps, dx, dz
