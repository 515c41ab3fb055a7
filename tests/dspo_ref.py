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


def depth_frames(ii, jj=None, nv=None):
    """kx: the frames some edge starts from.  With jj and nv, only edges whose two frames lie in [0, nv) count (R.kept_edges): an edge
    with a frame that does not exist adds no depth frame, no term and no moved frame."""
    if jj is None or nv is None:
        return sorted(set(int(v) for v in ii))
    return sorted(set(int(ii[e]) for e in R.kept_edges(ii, jj, nv)))


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
    every (edge, pixel) [E,P] (kept or not; inf and False for an edge with a frame outside [0, nv), nv = min(len(poses), len(disps)),
    which takes part in nothing)."""
    nv = min(len(poses), len(disps))
    kx = depth_frames(ii, jj, nv)
    krow = {f: k for k, f in enumerate(kx)}
    P = disps.shape[1] * disps.shape[2]
    C, b = np.zeros((len(kx), P)), np.zeros((len(kx), P))
    active = np.zeros(len(kx), bool)
    margins, counted = np.full((len(ii), P), np.inf), np.zeros((len(ii), P), bool)
    for e in R.kept_edges(ii, jj, nv):
        i, j = int(ii[e]), int(jj[e])
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
    kx = depth_frames(ii, jj, min(len(poses), N))
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
    """(scale, shift, bad [n_frames]) of depth_scale_step's alignment and bad-frame rule (no edge takes part in it)."""
    est, valid = np.asarray(disps, float)[:n_frames], np.asarray(vmask)[:n_frames] != 0
    s, q, err = align_scale_and_shift(np.asarray(mono, float)[:n_frames], est, valid.astype(float))
    bad = np.zeros(n_frames, bool)
    if mono_thres:
        with np.errstate(invalid="ignore", divide="ignore"):
            bad = (err / est.mean((1, 2)) > mono_thres) | np.isnan(err) | (s < 0) | (valid.sum((1, 2)) < valid.shape[1] * valid.shape[2] * 0.5)
    return s, q, bad


def depth_scale_step(poses, disps, intr, mono, vmask, scales, shifts, n_frames, target, weight, eta, ii, jj, itrs=2, lm=1e-4, ep=0.1,
                     mono_thres=0.1, alpha=0.01):
    """Returns (disps, scales, shifts, edge_keep, any_kept); inputs are not modified.  An edge with a frame outside [0, nv),
    nv = min(len(poses), len(disps)), is never kept: it moves no frame and does not count towards any_kept (the device's edge_keep is
    compared with this one on the in-range edges only)."""
    disps, scales, shifts = np.array(disps, float), np.array(scales, float), np.array(shifts, float)
    s, q, bad = bad_frames(mono, disps, vmask, n_frames, mono_thres)
    scales[:n_frames], shifts[:n_frames] = s, q
    inrange = set(R.kept_edges(ii, jj, min(len(poses), len(disps))))
    isbad = lambda f: 0 <= f < n_frames and bad[f]
    keep = np.array([e in inrange and not (isbad(int(i)) or isbad(int(j))) for e, (i, j) in enumerate(zip(ii, jj))])
    disps, scales, shifts, _, _ = ba_with_scale_shift(target, weight, eta, poses, disps, intr, ii, jj, mono, scales, shifts, vmask, 0, lm,
                                                      ep, alpha, itrs, keep)
    for f in set(int(i) for i, k in zip(ii, keep) if k):
        disps[f] = np.maximum(disps[f], 1e-5)
    return disps, scales, shifts, keep, bool(keep.any())


# ================================================================================================================================
# One iteration with magnitudes: what the criteria of tests/dspo_cases.py are held to
# ================================================================================================================================
# system_kernel and the sums of update_kernel (csrc/sgr_dspo.hip) restated in the kernel's order of operations, every fp32 quantity a
# dba_ref.Mag (value, magnitude, units; the rules stand at the head of that section of tests/dba_ref.py).  A `problem` is a dict:
# poses [Np,7], disps [N,h,w], intr [4], tgt, wgt [E,h,w,2], eta [M,h,w], ii, jj, mono, vmask [N,h,w], scales, shifts [N], ignore_frames,
# lm, ep, alpha, keep ([E] or None), every array fp32-representable.
#
# Units that follow from the formulas (`linearize_mag` reports the largest met per quantity in `units`; DESIGN.md section 3 tabulates
# them; tests/test_dspo_cpu.py pins them): tij 14 and the point X = act_so3(qij, ray) + h tij 17, d = 1/z 19, d^2 39, as in ba.
# jx = fx (t0 d - t2 (x d^2)): x d^2 57, t2 (.) 72, the difference 73, fx 74.  rx = target - (fx d x + cx): fx d 20, (fx d) x 38, + cx 39,
# the difference 40.  0.001 w: 2.  (w jx) jx: 77 + 74 + 1 = 152;  (w rx) jx: 43 + 74 + 1 = 118.  C_proj and b_proj add two such terms per
# kept edge, in edge order: 152 + 2n and 118 + 2n for n edges.  Prior: a = sqrt_alpha gain 1, Js = (-m) a 2, Jq 1, Jd 1,
# rd = sqrt_alpha (h - (s m + q)) 4.  cpe = C_proj + eta: u_C + 1; Q = 1 / (cpe + Jd^2): u_C + 4; bb = b_proj - Jd rd: max(u_b, 6) + 1;
# Q bb: u_Q + u_bb + 1; Q (Js Jd): u_Q + 5; Q (Jq Jd): u_Q + 4.
#
# The seven frame sums are fp64 from the first product on: a product formed in fp64 from fp32 factors inherits their units and adds
# none (`_mul64`, `_add64`); its own roundings and those of the fp64 summation enter through dba_ref.bound64.
def _m64(a):
    return R.Mag(a.v.astype(np.float64), a.m, a.c)


def _mul64(a, b):
    return R.Mag(a.v * b.v, np.maximum(a.m * np.abs(b.v), b.m * np.abs(a.v)), a.c + b.c)


def _add64(a, b):
    return R.Mag(a.v + b.v, a.m + b.m, max(a.c, b.c))


MUTATIONS = ("thresh_025", "targets_chw", "pix_div_ht", "drop_last_pixel", "drop_last_edge", "dup_once", "count_masked", "clamp_oob",
             "eta_by_frame", "scale_by_row", "gain_on_rd", "jd_kept", "ignore_le", "lm_from_S", "sums_fp32", "S_subtracted_fp32",
             "nonpd_zero_all", "no_floor", "dz_prev_row")


def graph(problem, mutate=None):
    """mark_kernel, scan_kernel and the order of fill_kernel: nv, kx, and per depth row the kept in-range edges (i, j, e) in edge order
    (an empty run: the row is inactive)."""
    ii, jj = [int(v) for v in problem["ii"]], [int(v) for v in problem["jj"]]
    nv = min(len(problem["poses"]), len(problem["disps"]))
    keep = problem.get("keep")
    kept = lambda e: keep is None or bool(keep[e]) or mutate == "count_masked"
    kx = depth_frames(ii, jj, nv)
    runs = {f: [] for f in kx}
    for e in R.kept_edges(ii, jj, nv):
        if kept(e):
            runs[ii[e]].append((ii[e], jj[e], e))
    if mutate == "clamp_oob":          # both frames of an out-of-range edge clamped into range; counted where the frame has a depth row
        inr = set(R.kept_edges(ii, jj, nv))
        for e in range(len(ii)):
            i, j = min(max(ii[e], 0), nv - 1), min(max(jj[e], 0), nv - 1)
            if e not in inr and kept(e) and i in runs:
                runs[i].append((i, j, e))
        runs = {f: sorted(r, key=lambda t: t[2]) for f, r in runs.items()}
    if mutate == "dup_once":
        for f, run in runs.items():
            seen, out = set(), []
            for t in run:
                if t[:2] not in seen:
                    seen.add(t[:2])
                    out.append(t)
            runs[f] = out
    if mutate == "drop_last_edge":
        runs = {f: (r[:-1] if len(r) > 1 else r) for f, r in runs.items()}
    return nv, kx, [runs[f] for f in kx]


def linearize_mag(problem, dtype=np.float64, mutate=None):
    """One iteration's system at the problem's state.  dtype=np.float32 runs the same restatement in fp32 where the kernel is fp32 (the
    frame sums, the damping and the solve stay fp64): the stand-in for the kernel on the CPU.  `mutate` plants one of MUTATIONS.
    Returns a dict:
        nv, kx, M, P, active [M]
        S [M,2,2], g [M,2]          the damped reduced system of every active row (fp64), S_bound, g_bound entrywise
        fail [M]                    S is not positive definite, by the kernel's own test (dwq = 0 for that row)
        pivots [M,2]                the two Cholesky pivots over their diagonal entries
        QB                          list of three Mag [M,P]: the stored Q bb, Q Js Jd, Q Jq Jd (zero rows where inactive)
        zmargin, behind, between    smallest |X.z - 0.2| over every (kept edge, pixel); how many lie behind the threshold; how many
                                    have z in (0.2 + 1e-3, 0.25 - 1e-3)
        units                       the largest per-addend count met, per quantity"""
    dt = dtype
    pr = problem
    nv, kx, runs = graph(pr, mutate)
    disps = np.asarray(pr["disps"], np.float64)
    ht, wd = disps.shape[1:]
    M, P = len(kx), ht * wd
    mg = lambda a: R.Mag(np.asarray(a, dt))
    vec = lambda a: [mg(x) for x in a]
    fx, fy, cx, cy = vec(pr["intr"])
    zero, one = R.const(0, dt), R.const(1, dt)
    sa = mg(np.float32(np.sqrt(np.float64(pr["alpha"]))))                        # one fp32 rounding of the fp64 square root
    lm, ep = float(np.float32(pr["lm"])), float(np.float32(pr["ep"]))
    k_ = np.arange(P)
    div = ht if mutate == "pix_div_ht" else wd
    Xi = [(mg(k_ - (k_ // div) * div) - cx) / fx, (mg(k_ // div) - cy) / fy, one]
    thresh = 0.25 if mutate == "thresh_025" else MIN_DEPTH
    eta = np.asarray(pr["eta"], np.float64).reshape(M, P)
    mono, vmask = np.asarray(pr["mono"], np.float64), np.asarray(pr["vmask"])
    units = {}

    def note(name, m):
        units[name] = max(units.get(name, 0), m.c)
        return m

    active = np.array([len(r) > 0 for r in runs])
    S, Sb, g, gb = np.zeros((M, 2, 2)), np.zeros((M, 2, 2)), np.zeros((M, 2)), np.zeros((M, 2))
    fail, pivots = np.zeros(M, bool), np.zeros((M, 2))
    QB = [[], [], []]
    zmargin, behind, between = np.inf, 0, 0
    for k, f in enumerate(kx):
        if not active[k]:
            for n in range(3):
                QB[n].append(R.Mag(np.zeros(P, dt)))
            continue
        h = mg(disps[f].reshape(-1))
        cs, bs = [], []
        for (i, j, e) in runs[k]:
            if i == j:
                t, q = [R.const(R.STEREO_T[0], dt), zero, zero], [zero, zero, zero, one]
            else:
                t, q = R.m_rel_se3(vec(pr["poses"][i]), vec(pr["poses"][j]))
            note("t", t[0])
            Y = R.m_act_so3(q, Xi)
            X = [note("X", Y[n] + h * t[n]) for n in range(3)]
            z64 = X[2].v.astype(np.float64)
            front = X[2].v > dt(thresh)
            zmargin = min(zmargin, float(np.abs(z64 - MIN_DEPTH).min()))
            behind += int((z64 <= MIN_DEPTH).sum())
            between += int(((z64 > MIN_DEPTH + 1e-3) & (z64 < 0.25 - 1e-3)).sum())
            d = note("d", (one / X[2].where(front, 1.0)).where(front, 0.0))
            d2 = note("d2", d * d)
            tg, wt = np.asarray(pr["tgt"][e], dt), np.asarray(pr["wgt"][e], dt).reshape(P, 2)
            tg = tg.reshape(2, P).T if mutate == "targets_chw" else tg.reshape(P, 2)
            ws = R.const(WEIGHT_SCALE, dt)
            for c2, (fc, cc) in enumerate(((fx, cx), (fy, cy))):
                w = note("w", (ws * mg(wt[:, c2])).where(front, 0.0))
                r = note("r", mg(tg[:, c2]) - (fc * d * X[c2] + cc))
                jz = note("jz", fc * (t[c2] * d - t[2] * (X[c2] * d2)))
                cs.append(note("wjj", w * jz * jz))
                bs.append(note("wrj", w * r * jz))
        c, b = note("c", R.msum(cs)), note("b", R.msum(bs))
        m = mg(mono[f].reshape(-1))
        vd = vmask[f].reshape(-1) != 0
        ign = f <= pr["ignore_frames"] if mutate == "ignore_le" else f < pr["ignore_frames"]
        invalid = (m.v < dt(MONO_MIN)) | ign
        a = note("a", sa * mg(np.where(vd, VALID_GAIN, 1.0)))
        Jd = note("Jd", a if mutate == "jd_kept" else a.where(~(invalid & vd), 0.0))
        Js = note("Js", ((-m) * a).where(~invalid, 0.0))
        Jq = note("Jq", (-a).where(~invalid, 0.0))
        row = k if mutate == "scale_by_row" else f
        rd = note("rd", (a if mutate == "gain_on_rd" else sa) * (h - (mg(pr["scales"][row]) * m + mg(pr["shifts"][row]))))
        cpe = note("cpe", c + mg(eta[f % M] if mutate == "eta_by_frame" else eta[k]))
        Q = note("Q", one / (cpe + Jd * Jd))
        bb = note("bb", b - Jd * rd)
        for n, qb in enumerate((Q * bb, Q * (Js * Jd), Q * (Jq * Jd))):
            QB[n].append(note(f"QB{n}", qb))
        # ---- the seven frame sums
        js, jq, q64, c64, r64, d64, b64 = (_m64(x) for x in (Js, Jq, Q, cpe, rd, Jd, b))
        qc = _mul64(q64, c64)
        gr = _mul64(q64, _add64(_mul64(r64, c64), _mul64(d64, b64)))
        v = [_mul64(js, js), _mul64(jq, jq), _mul64(_mul64(js, js), qc), _mul64(_mul64(js, jq), qc), _mul64(_mul64(jq, jq), qc),
             -_mul64(js, gr), -_mul64(jq, gr)]
        for n, x in enumerate(v):
            note(f"v{n}", x)
        last = P - 1 if mutate == "drop_last_pixel" else P
        sums = np.array([x.v[:last].sum() for x in v])
        if mutate == "sums_fp32":                                                # terms and running sums in fp32
            qc32, gr32 = Q * cpe, Q * (rd * cpe + Jd * b)
            v32 = [Js * Js, Jq * Jq, Js * Js * qc32, Js * Jq * qc32, Jq * Jq * qc32, -(Js * gr32), -(Jq * gr32)]
            sums = np.array([float(np.add.accumulate(x.v.astype(np.float32))[-1]) for x in v32])
        if mutate == "S_subtracted_fp32":                                        # S = H - sum Q E E^T, each an fp32 sum
            f32sum = lambda x: float(np.add.accumulate(x.v.astype(np.float32))[-1])
            E0, E1 = Js * Jd, Jq * Jd
            H = [f32sum(Js * Js), f32sum(Js * Jq), f32sum(Jq * Jq)]
            QEE = [f32sum(Q * E0 * E0), f32sum(Q * E0 * E1), f32sum(Q * E1 * E1)]
            sums[2:5] = [float(np.float32(H[n]) - np.float32(QEE[n])) for n in range(3)]
        mag = np.array([x.m.sum() for x in v])
        bnd = np.array([x.bound().sum() for x in v]) + R.bound64(P + 4, mag)     # P addends, each a product of up to five fp64 roundings
        damp = (sums[2], sums[4]) if mutate == "lm_from_S" else (sums[0], sums[1])
        S[k] = [[sums[2] + ep + lm * damp[0], sums[3]], [sums[3], sums[4] + ep + lm * damp[1]]]
        Sb[k] = [[bnd[2] + lm * bnd[0] + 3 * R.U64 * (mag[2] + ep + lm * mag[0]), bnd[3]],
                 [bnd[3], bnd[4] + lm * bnd[1] + 3 * R.U64 * (mag[4] + ep + lm * mag[1])]]
        g[k], gb[k] = sums[5:7], bnd[5:7]
        s00, s01, s11 = S[k, 0, 0], S[k, 0, 1], S[k, 1, 1]
        dd = s11 - s01 * s01 / s00 if s00 > 0 else -1.0
        fail[k] = not (s00 > 0 and dd > 0)
        pivots[k] = [1.0 if s00 > 0 else 0.0, dd / s11 if s11 > 0 else 0.0]
    QB = [R.mstack(q) for q in QB]
    return dict(nv=nv, kx=kx, M=M, P=P, active=active, S=S, g=g, S_bound=Sb, g_bound=gb, fail=fail, pivots=pivots, QB=QB,
                zmargin=float(zmargin), behind=behind, between=between, units=units, dtype=dt)


def solve_rows(sys, mutate=None):
    """update_kernel's fp64 Cholesky of every active row: dwq [M,2] (0 where the row is inactive or not positive definite)"""
    dwq = np.zeros((sys["M"], 2))
    for k in range(sys["M"]):
        if not sys["active"][k] or sys["fail"][k]:
            continue
        (s00, s01), (_, s11) = sys["S"][k]
        l00 = np.sqrt(s00)
        l10 = s01 / l00
        l11 = np.sqrt(s11 - l10 * l10)
        y0 = sys["g"][k, 0] / l00
        y1 = (sys["g"][k, 1] - l10 * y0) / l11
        x1 = y1 / l11
        dwq[k] = [(y0 - l10 * x1) / l00, x1]
    if mutate == "nonpd_zero_all" and np.any(sys["fail"] & sys["active"]):
        dwq[:] = 0.0
    return dwq


def fp64_solve_term(S, dwq):
    """Row-wise residual the fp64 2 x 2 factorisation and substitutions may leave, as dba_ref.fp64_solve_term derives it:
    (3n + 2) 2^-53 sqrt(S_rr S_cc) |dwq_c| summed over c, n = 2."""
    s = np.sqrt(np.abs(np.diag(S)))
    return (3 * 2 + 2) * R.U64 * s * (s @ np.abs(dwq))


def back_substitute(sys, dwq, dtype=np.float64, mutate=None):
    """Mag [M,P] of dz = QB0 - (QB1 dwq0 + QB2 dwq1) at the given dwq (taken as exact fp32 inputs); zero on inactive rows"""
    dwq = np.asarray(dwq, dtype).reshape(sys["M"], 2)
    if mutate == "dz_prev_row":
        dwq = np.roll(dwq, 1, axis=0)
    rows = []
    for k in range(sys["M"]):
        q0, q1, q2 = (sys["QB"][n][k] for n in range(3))
        rows.append(q0 - (q1 * R.Mag(dwq[k, 0]) + q2 * R.Mag(dwq[k, 1])) if sys["active"][k] else R.Mag(np.zeros(sys["P"], dtype)))
    return R.mstack(rows)


def emulate(problem, dtype=np.float32, mutate=None):
    """One iteration through `linearize_mag`, `solve_rows` and `back_substitute` in `dtype`: (disps, scales, shifts, dwq, dz) as fp32
    arrays, the stand-in for the device on the CPU."""
    f32 = lambda a: np.asarray(a, np.float32)
    disps, scales, shifts = f32(problem["disps"]).copy(), f32(problem["scales"]).copy(), f32(problem["shifts"]).copy()
    sys = linearize_mag(problem, dtype, mutate)
    dwq = f32(solve_rows(sys, mutate))
    dz = f32(back_substitute(sys, dwq, dtype, mutate).v)
    ht, wd = disps.shape[1:]
    for k, f in enumerate(sys["kx"]):
        if not sys["active"][k]:
            continue
        moved = f32(disps[f] + dz[k].reshape(ht, wd))
        disps[f] = moved if mutate == "no_floor" else np.maximum(moved, np.float32(0))
        scales[f] = np.float32(scales[f] + dwq[k, 0])
        shifts[f] = np.float32(shifts[f] + dwq[k, 1])
    return disps, scales, shifts, dwq, dz
