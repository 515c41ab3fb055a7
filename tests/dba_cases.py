"""The cases and the three criteria that hold droid_backends.ba to the fp64 oracle with magnitudes (tests/dba_ref.py: linearize,
back_substitute, retract_mag).  Shared by tests/test_dba_cpu.py, which proves them on the fp32 restatement and on planted faults,
and tests/test_gpu_dba_edges.py, which holds the kernels to them.  Every case is one Gauss-Newton iteration.

A case is a dict: poses [N,7], disps [n,h,w], intr, sens, tgt, wgt [E,2,h,w], eta [K,h,w], ii, jj, t0, t1, lm, ep, mode.  All
arrays are already fp32-representable, so the oracle linearises at exactly what the device reads.
"""
import functools

import numpy as np

import dba_ref as R

GRAPH_II = [2, 3, 3, 4, 4, 5, 5, 2, 3, 0, 1, 6, 7, 4, 3]          # the 15 edges of test_gpu_dba.problem(): window [2, 6) of 9 frames,
GRAPH_JJ = [3, 2, 4, 3, 5, 4, 2, 5, 3, 2, 3, 5, 4, 6, 0]          # a stereo edge (3, 3), edges from and to frames outside it
MODES = ("pose_depth", "motion_only", "depth_only")
PIXEL_SHAPES = ((3, 5), (7, 9), (5, 13), (1, 257))
CHOL_T = (10, 11, 21, 22, 32)                                       # n = 6 T = 60, 66, 126, 132, 192 around the 64-wide blocks
OOB = (-1, "nv", "nv+5", 2 ** 40, -2 ** 63)
# per-addend fp32 units that dba_ref.Mag derives from the kernel's formulas (DESIGN.md section 3 tabulates them); Cii and bz include
# their two addends
DOCUMENTED_UNITS = dict(Hs=186, vs=135, E=171, Cii=154, bz=120)


def r32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def intrinsics(ht, wd):
    """scaled to the frame, so reprojections stay in view"""
    f = 0.8 * max(ht, wd)
    return np.array([f, f * 1.04, (wd - 1) / 2.0, (ht - 1) / 2.0])


def scene(ht, wd, n, seed, phase=None):
    """n cameras along a gentle track (phase[f] places frame f on it; default f), disparities 0.3-1 with the first three pixels
    of every frame far behind MIN_DEPTH for edges that move backwards (z = 1 - 60 tz)"""
    rng = np.random.default_rng(seed)
    poses = []
    for f in range(n):
        s = f if phase is None else phase(f)
        t, q = R.exp_se3(np.concatenate([[0.03 * s, 0.01 * np.sin(s), 0.02 * s], rng.normal(0, 0.02, 3)]))
        poses.append(np.concatenate([t, q]))
    disps = rng.uniform(0.3, 1.0, (n, ht, wd))
    disps[:, 0, :3] = -60.0
    return rng, np.stack(poses), disps


def flow_target(poses, disps, intr, i, j):
    ht, wd = disps.shape[1:]
    if i != j:
        return R.project(poses[i], poses[j], disps[i], intr).T.reshape(2, ht, wd)
    u, v, _, _ = R.pixel_rays(ht, wd, intr)
    return np.stack([u + intr[0] * R.STEREO_T[0] * disps[i].reshape(-1), v]).reshape(2, ht, wd)


def make(name, ht, wd, ii, jj, t0, t1, n=9, seed=0, mode="pose_depth", lm=1e-4, ep=0.1, extra_pose_rows=0, phase=None):
    """Builds the case: true geometry, noisy flow targets with their own weights per edge, perturbed poses and disparities, sensor
    disparity on a third of the pixels.  Edges with a frame outside [0, n) get random targets (they must take part in nothing)."""
    rng, poses, disps = scene(ht, wd, n + extra_pose_rows, seed, phase)
    disps = disps[:n]
    intr = intrinsics(ht, wd)
    ok = lambda f: 0 <= f < n
    tgt = np.stack([flow_target(poses, disps, intr, i, j) if ok(i) and ok(j) else rng.uniform(0, wd, (2, ht, wd))
                    for i, j in zip(ii, jj)])
    tgt += rng.normal(0, 0.5, tgt.shape)
    wgt = rng.uniform(0.2, 1.0, tgt.shape)
    p0 = poses.copy()
    for f in range(1, len(poses)):
        p0[f] = R.retract(poses[f], np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.01, 3)]))
    d0 = np.where(disps < 0, disps, disps * rng.uniform(0.95, 1.05, disps.shape))
    sens = np.where(rng.uniform(size=disps.shape) < 0.3, disps, 0.0)
    keep = R.kept_edges(ii, jj, n)
    K = len(set(range(t0, t1)) | {ii[e] for e in keep})
    eta = rng.uniform(1e-3, 1e-2, (K, ht, wd))
    return dict(name=name, poses=r32(p0), disps=r32(d0), intr=r32(intr), sens=r32(sens), tgt=r32(tgt), wgt=r32(wgt), eta=r32(eta),
                ii=list(ii), jj=list(jj), t0=t0, t1=t1, lm=lm, ep=ep, mode=mode)


def resolve_oob(v, nv):
    return {"nv": nv, "nv+5": nv + 5}.get(v, v)


def duplicate_graph():
    """the 15 edges plus: two more copies of the window edge 3 -> 4 (one first, one last), a copy of 3 -> 2 (into t0), of 1 -> 3 (from
    outside the window) and of the stereo edge 3 -> 3 in the middle, so the first edge of a group is not always its first member"""
    ii = [3] + GRAPH_II[:6] + [3, 1, 3] + GRAPH_II[6:] + [3]
    jj = [4] + GRAPH_JJ[:6] + [2, 3, 3] + GRAPH_JJ[6:] + [4]
    return ii, jj


def oob_graph(nv, extra_rows=0):
    """the 15 edges with out-of-range edges spread through them: the bad end is ii, jj or both; frame 8, which no other edge
    uses, is the ii of one of them and must not get a depth row.  With extra_rows, edges into pose rows that have no disparity."""
    bad = [resolve_oob(v, nv) for v in OOB]
    ins = {0: (bad[0], 3), 2: (4, bad[1]), 5: (bad[2], bad[3]), 7: (8, bad[1]), 9: (bad[4], 2), 11: (3, bad[3]), 13: (bad[4], bad[0]),
           15: (2, bad[2])}
    if extra_rows:
        ins[4] = (3, nv)
        ins[10] = (nv + extra_rows - 1, 4)
        ins[14] = (nv + 1, nv + 1)
    ii, jj = [], []
    for e in range(len(GRAPH_II) + 1):
        if e in ins:
            ii.append(ins[e][0]), jj.append(ins[e][1])
        if e < len(GRAPH_II):
            ii.append(GRAPH_II[e]), jj.append(GRAPH_JJ[e])
    return ii, jj


def chain_graph(n):
    ii, jj = [], []
    for i in range(n):
        for j in range(max(0, i - 2), min(n, i + 3)):
            if i != j:
                ii.append(i), jj.append(j)
    return ii, jj


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.partition(":")
    if kind == "pix":
        ht, wd, mode = arg.split(",")
        return make(name, int(ht), int(wd), GRAPH_II, GRAPH_JJ, 2, 6, seed=20 + int(wd), mode=mode)
    if kind == "dup":
        ii, jj = duplicate_graph()
        return make(name, 7, 9, ii, jj, 2, 6, seed=31)
    if kind == "oob":
        extra = 3 if arg == "long_poses" else 0
        ii, jj = oob_graph(9, extra)
        return make(name, 7, 9, ii, jj, 2, 6, seed=32, extra_pose_rows=extra)
    if kind == "win":
        g = list(zip(GRAPH_II, GRAPH_JJ))
        if arg == "t0=0":
            return make(name, 7, 9, GRAPH_II, GRAPH_JJ, 0, 4, seed=33)
        if arg == "t1=nv":
            return make(name, 7, 9, GRAPH_II, GRAPH_JJ, 5, 9, seed=34)
        if arg == "T=1":
            return make(name, 7, 9, GRAPH_II, GRAPH_JJ, 3, 4, seed=35)
        if arg == "no_outgoing":                        # frame 5 keeps its incoming edges only: its depth row is the prior
            g = [e for e in g if e[0] != 5]
            return make(name, 7, 9, [e[0] for e in g], [e[1] for e in g], 2, 6, seed=36)
        if arg in ("no_edge", "no_edge_singular"):      # frame 6 is in the window [2, 7) and has no edge at all
            g = [e for e in g if 6 not in e]
            lm, ep = (0.0, 0.0) if arg == "no_edge_singular" else (1e-4, 0.1)
            return make(name, 7, 9, [e[0] for e in g], [e[1] for e in g], 2, 7, seed=37, lm=lm, ep=ep)
        if arg == "both_outside":                       # 0 -> 7 and 7 -> 8 touch no window pose: depth only
            g = g + [(0, 7), (7, 8)]
            return make(name, 7, 9, [e[0] for e in g], [e[1] for e in g], 2, 6, seed=38)
    if kind == "chol":
        T, mode = arg.split(",")
        T = int(T)
        ii, jj = chain_graph(T + 2)
        return make(name, 3, 5, ii, jj, 1, T + 1, n=T + 2, seed=40 + T, mode=mode)
    if kind == "big":                                   # 1030 frames: the scans give each thread more than one element
        n, t0 = 1030, 1020
        ii, jj = chain_graph(6)
        ii, jj = [t0 + i for i in ii] + [3, 7], [t0 + j for j in jj] + [t0 + 1, t0 + 3]
        return make(name, 3, 5, ii, jj, t0, t0 + 6, n=n, seed=50, phase=lambda f: f % 12)
    if kind == "iter":
        return make(name, 5, 13, GRAPH_II, GRAPH_JJ, 2, 6, seed=60)
    raise KeyError(name)


CASES = ([f"pix:{h},{w},{m}" for (h, w) in PIXEL_SHAPES for m in MODES] + ["dup", "oob", "oob:long_poses"] +
         [f"win:{a}" for a in ("t0=0", "t1=nv", "T=1", "no_outgoing", "no_edge", "no_edge_singular", "both_outside")] +
         [f"chol:{T},{m}" for T in CHOL_T for m in ("pose_depth", "motion_only")] + ["big"])


def lin_args(c):
    return (c["poses"], c["disps"], c["intr"], c["sens"], c["tgt"], c["wgt"], c["eta"], c["ii"], c["jj"], c["t0"], c["t1"], c["lm"], c["ep"],
            c["mode"] == "motion_only")


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the fp64 linearisation of the case, computed once and shared"""
    return R.linearize(*lin_args(case(name)))


def check_scene(name, want_behind=True):
    """no decision can flip between fp32 and fp64: no z within 1e-3 of MIN_DEPTH (pixels clearly behind it are present), no sensor
    disparity in (0, 1e-6)"""
    c, o = case(name), oracle(name)
    assert o["zmargin"] > 1e-3, (name, o["zmargin"])
    if want_behind:
        assert o["behind"] > 0, name
    assert not np.any((c["sens"] > 0) & (c["sens"] < 1e-6)), name


def criteria(name, poses, disps, dx, dz):
    """The device's (or a stand-in's) outputs of one iteration against the oracle.  Returns {criterion: largest err / bound} for A (dx,
    componentwise backward error), B (dz per pixel), C (poses), and a list of the exact conditions that do not hold.  A case passes
    when every ratio is <= 1 and the list is empty."""
    c, o = case(name), oracle(name)
    T, t0, t1, kx, mode = o["T"], c["t0"], c["t1"], o["kx"], c["mode"]
    dx = np.asarray(dx, np.float64).reshape(T, 6)
    ratios, broken = {}, []
    x = dx.reshape(-1)
    if not np.all(np.isfinite(x)):
        broken.append("dx is not finite")
    if o["fail"]:
        if np.any(x != 0):
            broken.append("dx != 0 where the factorisation fails")
    else:
        # A: |H dx - g| <= bound_H |dx| + bound_g + the fp32 store of dx (one rounding of every |H_rc dx_c|) + the fp64 solve
        res = np.abs(o["H"] @ x - o["g"])
        bnd = o["H_bound"] @ np.abs(x) + o["g_bound"] + R.U32 * (np.abs(o["H"]) @ np.abs(x)) + R.fp64_solve_term(o, x) + R.DENORMAL
        ratios["A"] = float(np.max(res / bnd))
    # C: poses
    p_in, p_out = c["poses"], np.asarray(poses, np.float64)
    if mode == "depth_only":
        if not np.array_equal(p_out, p_in):
            broken.append("depth_only moved a pose")
    else:
        outside = [f for f in range(len(p_in)) if not t0 <= f < t1]
        if not np.array_equal(p_out[outside], p_in[outside]):
            broken.append("a pose outside the window moved")
        worst = 0.0
        for a in range(T):
            comp, extra = R.retract_mag(p_in[t0 + a], np.asarray(dx[a], np.float32))
            ref = np.array([float(m.v) for m in comp])
            bnd = np.array([float(m.bound()) for m in comp]) + extra
            worst = max(worst, float(np.max(np.abs(p_out[t0 + a] - ref) / bnd)))
        ratios["C"] = worst
    # B: dz and disps
    d_in, d_out = c["disps"], np.asarray(disps, np.float64)
    if mode == "motion_only":
        if dz is not None:
            broken.append("motion_only returned a dz")
        if not np.array_equal(d_out, d_in):
            broken.append("motion_only moved a disparity")
    else:
        dz = np.asarray(dz, np.float64)
        ref = R.back_substitute(o, np.asarray(dx, np.float32))
        if dz.shape != ref.v.shape:
            broken.append(f"dz has shape {dz.shape}, not {ref.v.shape}")
        else:
            ratios["B"] = float(np.max(np.abs(dz - ref.v) / ref.bound()))
            ht, wd = d_in.shape[1:]
            moved = np.asarray(d_in[kx].astype(np.float32) + dz.reshape(len(kx), ht, wd).astype(np.float32), np.float32)
            if not np.array_equal(d_out[kx].astype(np.float32), moved):
                broken.append("disps_after != fp32(disps_before + dz) on a depth row")
        rest = [f for f in range(len(d_in)) if f not in set(kx)]
        if not np.array_equal(d_out[rest], d_in[rest]):
            broken.append("a disparity map outside kx moved")
    return ratios, broken


def passes(ratios, broken):
    return not broken and all(r <= 1.0 for r in ratios.values())


def emulate(name, dtype=np.float32, mutate=None):
    c = case(name)
    return R.emulate(*lin_args(c)[:-1], c["mode"] == "motion_only", c["mode"] == "depth_only", dtype, mutate)
