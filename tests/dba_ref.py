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
    ii = [int(v) for v in ii]
    jj = [int(v) for v in jj]
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
    for i, j in zip(ii, jj):
        i, j = int(i), int(j)
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
    for e, (i, j) in enumerate(zip(ii, jj)):
        i, j = int(i), int(j)
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
