"""The cases and the criteria that hold splat_slam_amd.dspo.ba_with_scale_shift to the fp64 oracle with magnitudes (tests/dspo_ref.py:
linearize_mag, solve_rows, back_substitute).  Shared by tests/test_dspo_cpu.py, which proves them on the fp32 restatement and on planted
faults, and tests/test_gpu_dspo_edges.py, which holds the kernels to them.  Every case is one Gauss-Newton iteration.

A case is the `problem` dict of dspo_ref.linearize_mag plus its name.  All arrays are already fp32-representable, so the oracle
linearises at exactly what the device reads.
"""
import functools

import numpy as np

import dba_cases as BC
import dba_ref as R
import dspo_ref as D

GRAPH_II = [2, 3, 3, 4, 4, 5, 5, 2, 3, 6, 7, 4, 3]    # the 13 edges of tests/test_gpu_dspo.py: depth frames 2..7; frames 0, 1 only receive
GRAPH_JJ = [3, 2, 4, 3, 5, 4, 2, 5, 3, 5, 4, 6, 0]    # edges, frame 8 has none; (3, 3) is a stereo edge
PIXEL_SHAPES = ((3, 5), (7, 9), (5, 13), (16, 16), (1, 257))       # P = 15, 63, 65 (below one wave, one workgroup), 256, 257
ALPHAS = (1.0, 0.01)
# tile:E -- chain_graph(n) links every frame to its two neighbours on either side: E = 4 n - 6, always even.  n = 65 gives 254 edges and
# n = 129 gives 510; the first edges of the list are appended again (duplicates, whose place in their frame's run counts an edge of the
# first 256-wide tile from the last one) until E is 255, 256, 257 or 513.
TILE_E = {255: 65, 256: 65, 257: 65, 513: 129}
MASK_VALUES = (1, 2, 255)
# per-quantity fp32 units that dba_ref.Mag derives from the kernel's formulas (DESIGN.md section 3 tabulates them).  Up to rd they do
# not depend on the case; from c on they are those of a frame with n = 1 kept edge (the case one_edge): c, b, cpe, Q, bb, QB1 and QB2
# grow by 2 (n - 1), QB0 and v2 .. v6, which hold both C_proj and b_proj or C_proj twice, by 4 (n - 1).  v0 .. v6 are the per-pixel
# terms of the seven frame sums.
DOCUMENTED_UNITS = dict(t=14, X=17, d=19, d2=39, jz=74, r=40, w=2, wjj=152, wrj=118, a=1, Jd=1, Js=2, Jq=1, rd=4, c=154, b=120, cpe=155,
                        Q=158, bb=121, QB0=280, QB1=163, QB2=162, v0=4, v1=2, v2=317, v3=316, v4=315, v5=319, v6=318)

r32 = BC.r32


def make(name, ht, wd, ii, jj, n=9, seed=0, alpha=1.0, lm=1e-4, ep=0.1, ignore_frames=0, keep=None, pose_rows=0, phase=None,
         no_prior=None, plant=True, prior_off=(0.0, 0.0)):
    """Builds the case like dba_cases.make: the track and the intrinsics scaled to the frame, three pixels per frame at -60 (behind the
    threshold for edges that move backwards), noisy flow targets [E,h,w,2] with their own weights (random ones for an edge with a frame
    that does not exist), perturbed disparities, the prior m = 1.7 h + 0.05 (+ noise) with holes (exactly 0), a valid-depth mask on
    ~60 % of the pixels that overlaps the holes.  pose_rows: poses has that many rows more (or, negative, fewer) than disps.  no_prior:
    a frame whose every pixel is a hole.  plant: one pixel of the first kept non-stereo edge is placed at z = 0.225, between this
    stage's threshold 0.2 and the 0.25 of stage 1, and is given no prior."""
    rng, poses, disps = BC.scene(ht, wd, n + max(pose_rows, 0), seed, phase)
    poses, disps = r32(poses[:n + pose_rows]), disps[:n]
    nv = min(len(poses), n)
    intr = r32(BC.intrinsics(ht, wd))
    ok = lambda f: 0 <= f < nv
    tgt = np.stack([D.project(poses[i], poses[j], disps[i], intr, i == j).reshape(ht, wd, 2) if ok(i) and ok(j)
                    else rng.uniform(0, wd, (ht, wd, 2)) for i, j in zip(ii, jj)])
    tgt += rng.normal(0, 0.5, tgt.shape)
    wgt = rng.uniform(0.2, 1.0, tgt.shape)
    d0 = r32(np.where(disps < 0, disps, disps * rng.uniform(0.95, 1.05, disps.shape)))
    mono = 1.7 * disps + 0.05 + rng.normal(0, 0.01, disps.shape)
    mono[rng.uniform(size=mono.shape) < 0.1] = 0.0
    if no_prior is not None:
        mono[no_prior] = 0.0
    vmask = rng.uniform(size=mono.shape) < 0.6
    scales = 1 / 1.7 + prior_off[0] + rng.normal(0, 0.02, n)
    shifts = -0.05 / 1.7 + prior_off[1] + rng.normal(0, 0.01, n)
    kx = D.depth_frames(ii, jj, nv)
    eta = rng.uniform(1e-3, 1e-2, (len(kx), ht, wd))
    if plant:
        e = next(e for e in R.kept_edges(ii, jj, nv) if ii[e] != jj[e] and (keep is None or keep[e]))
        i, j, p = ii[e], jj[e], (ht * wd) // 2 + 1
        _, _, xr, yr = R.pixel_rays(ht, wd, intr)
        t, Rm = D.relative(poses[i], poses[j], False)
        d0[i].reshape(-1)[p] = (0.225 - (Rm @ np.array([xr[p], yr[p], 1.0]))[2]) / t[2]
        d0 = r32(d0)
        mono[i].reshape(-1)[p] = 0.0                      # a hole: the planted disparity is far from any prior
    return dict(name=name, poses=poses, disps=d0, intr=intr, tgt=r32(tgt), wgt=r32(wgt), eta=r32(eta), ii=list(ii), jj=list(jj),
                mono=r32(mono), vmask=vmask, scales=r32(scales), shifts=r32(shifts), ignore_frames=ignore_frames, lm=lm, ep=ep,
                alpha=alpha, keep=None if keep is None else np.asarray(keep))


def duplicate_graph():
    """the 13 edges plus two more copies of the window edge 3 -> 4, one first and one last, and a copy of the stereo edge 3 -> 3 in the
    middle, so the first edge of a group is not always its first member"""
    return [3] + GRAPH_II[:6] + [3] + GRAPH_II[6:] + [3], [4] + GRAPH_JJ[:6] + [3] + GRAPH_JJ[6:] + [4]


def oob_graph(nv, n, pose_rows):
    """the 13 edges with out-of-range edges spread through them: the bad end is ii, jj or both; frame 8, which no other edge uses, is
    the ii of one of them and must not get a depth row.  With more pose rows than disparity maps (or fewer), edges into frames that
    have a pose and no disparity (a disparity and no pose)."""
    bad = [BC.resolve_oob(v, nv) for v in BC.OOB]
    ins = {0: (bad[0], 3), 2: (4, bad[1]), 5: (bad[2], bad[3]), 7: (8, bad[1]), 9: (bad[4], 2), 11: (3, bad[3]), 13: (bad[4], bad[0])}
    if pose_rows > 0:
        ins[4], ins[10], ins[12] = (3, n), (n + pose_rows - 1, 4), (n + 1, n + 1)
    if pose_rows < 0:
        ins[4], ins[10], ins[12] = (3, nv), (n - 1, 4), (nv, nv)
    ii, jj = [], []
    for e in range(len(GRAPH_II) + 1):
        if e in ins:
            ii.append(ins[e][0]), jj.append(ins[e][1])
        if e < len(GRAPH_II):
            ii.append(GRAPH_II[e]), jj.append(GRAPH_JJ[e])
    return ii, jj


def edge_mask(dtype):
    """frames 4 and 7 lose every edge (7's only edge ends in 4); as uint8 the kept edges carry 1, 2 and 255 in turn"""
    keep = np.array([i != 4 and j != 4 for i, j in zip(GRAPH_II, GRAPH_JJ)])
    if dtype == "bool":
        return keep
    vals = np.zeros(len(keep), np.uint8)
    vals[keep] = [MASK_VALUES[n % 3] for n in range(int(keep.sum()))]
    return vals


SEEDS = {}


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    kind, _, arg = name.partition(":")
    sd = lambda default: SEEDS.get(name, default) if seed is None else seed
    G = (GRAPH_II, GRAPH_JJ)
    if kind == "pix":
        ht, wd, alpha = arg.split(",")
        return make(name, int(ht), int(wd), *G, seed=sd(120 + int(wd)), alpha=float(alpha))
    if kind == "alpha0":
        return make(name, 7, 9, *G, seed=sd(131), alpha=0.0)
    if kind == "dup":
        return make(name, 7, 9, *duplicate_graph(), seed=sd(132))
    if kind == "oob":
        rows = {"": 0, "long_poses": 3, "short_poses": -2}[arg]
        return make(name, 7, 9, *oob_graph(9 + min(rows, 0), 9, rows), seed=sd(133), pose_rows=rows)
    if kind == "mask":
        return make(name, 7, 9, *G, seed=sd(134), keep=edge_mask(arg))
    if kind == "far":                                       # the prior starts far from the disparities: a large step in s and q
        ht, wd = arg.split(",")
        return make(name, int(ht), int(wd), *G, seed=sd(170 + int(wd)), prior_off=(0.2, 0.1))
    if kind == "flat":
        # One edge whose flow has no confidence (every weight 0, so C_proj = b_proj = 0 exactly) from a frame that is uniform below its
        # first row: one disparity, one mono value, one eta, valid depth everywhere.  Every pixel then adds the SAME term to each of
        # the seven frame sums, and a running fp32 sum rounds every addition of a binade the same way: its error grows with P instead
        # of sqrt(P).  A bound of ~317 units per addend hides an fp32 sum of P addends (at most P units) until P is far above 317;
        # 384 x 512 is where the drift is clearly outside it.  The first row keeps the scene's pixels behind the threshold, its
        # holes and both mask values.
        ht, wd = arg.split(",")
        c = make(name, int(ht), int(wd), [2], [5], seed=sd(190), plant=False)
        c["wgt"] = np.zeros_like(c["wgt"])
        c["disps"][2, 1:], c["mono"][2, 1:], c["vmask"][2, 1:], c["eta"][0, 1:] = r32(0.7), r32(1.7 * 0.7 + 0.05), True, r32(5e-3)
        return c
    if kind == "one_edge":
        return make(name, 7, 9, [2], [5], seed=sd(135))
    if kind == "stereo_only":                               # z = 1 for every pixel: nothing behind the threshold, nothing to plant
        return make(name, 7, 9, [2, 3, 5, 3], [2, 3, 5, 3], seed=sd(136), plant=False)
    if kind == "ignore":
        return make(name, 7, 9, *G, seed=sd(137), ignore_frames={"some": 4, "all": 100}[arg])
    if kind == "singular":                                  # frame 5 has no prior at all and nothing damps: its S is zero
        return make(name, 7, 9, *G, seed=sd(138), lm=0.0, ep=0.0, no_prior=5)
    if kind == "tile":
        E = int(arg)
        ii, jj = BC.chain_graph(TILE_E[E])
        extra = E - len(ii)
        assert 0 < extra <= 3
        return make(name, 3, 5, ii + ii[:extra], jj + jj[:extra], n=TILE_E[E], seed=sd(140 + E))
    if kind == "big":                                       # 1030 frames: the scans give each thread more than one element
        n, t0 = 1030, 1020
        ii, jj = BC.chain_graph(6)
        ii, jj = [t0 + i for i in ii] + [3, 7], [t0 + j for j in jj] + [t0 + 1, t0 + 3]
        return make(name, 3, 5, ii, jj, n=n, seed=sd(150), phase=lambda f: f % 12)
    if kind == "iter":
        return make(name, 5, 13, *G, seed=sd(160))
    raise KeyError(name)


CASES = ([f"pix:{h},{w},{a}" for (h, w) in PIXEL_SHAPES for a in ALPHAS] + ["alpha0", "dup", "oob", "oob:long_poses", "oob:short_poses",
         "mask:bool", "mask:u8", "one_edge", "stereo_only", "ignore:some", "ignore:all", "singular", "far:16,16"] +
         [f"tile:{E}" for E in TILE_E] + ["big", "flat:384,512"])
SINGULAR_FRAME = {"singular": 5}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the fp64 linearisation of the case, computed once and shared"""
    return D.linearize_mag(case(name))


def check_scene(name, want_between=False):
    """No decision can flip between fp32 and fp64: no (edge, pixel) within 1e-3 of the depth threshold, pixels clearly behind it are
    present (not on stereo edges, where z = 1), no mono value in (0, 0.1); every (hole, valid-depth) combination occurs; every
    non-singular S is positive definite with both Cholesky pivots at least 1e-6 of their diagonal entry.  want_between: pixels with z
    clearly between 0.2 and 0.25 are present (what a threshold of 0.25 would get wrong)."""
    c, o = case(name), oracle(name)
    assert o["zmargin"] > 1e-3, (name, o["zmargin"])
    if name == "stereo_only":
        assert all(i == j for i, j in zip(c["ii"], c["jj"])) and o["behind"] == 0
    else:
        assert o["behind"] > 0, name
    if want_between:
        assert o["between"] > 0, name
    m = c["mono"]
    assert not np.any((m > 0) & (m < 0.1)), name
    kx = o["kx"]
    hole, vd = m[kx] < 1e-6, c["vmask"][kx]
    assert all((hole[vd == b] == a).any() for a in (False, True) for b in (False, True)), name
    sing = SINGULAR_FRAME.get(name)
    for k, f in enumerate(kx):
        if not o["active"][k]:
            continue
        if f == sing:
            assert o["fail"][k] and not o["S"][k].any() and not o["g"][k].any(), (name, f)
            continue
        assert not o["fail"][k] and o["pivots"][k].min() >= 1e-6, (name, f, o["pivots"][k])


def criteria_for(c, o, disps, scales, shifts, dwq, dz):
    """The device's (or a stand-in's) outputs of one iteration of problem c against its oracle o.  Returns {criterion: largest
    err / bound} for A (dwq, componentwise backward error of every active non-singular row) and B (dz per pixel at the device's own
    dwq), and a list of the exact conditions that do not hold."""
    kx, M, P = o["kx"], o["M"], o["P"]
    ratios, broken = {}, []
    f32 = lambda a: np.asarray(a, np.float32)
    disps, scales, shifts, dwq, dz = f32(disps), f32(scales), f32(shifts), f32(dwq), f32(dz)
    if dwq.shape != (M, 2) or dz.shape != (M, P):
        return ratios, [f"dwq, dz have shapes {dwq.shape}, {dz.shape}, not {(M, 2)}, {(M, P)}"]
    for nm, a in (("disps", disps), ("scales", scales), ("shifts", shifts), ("dwq", dwq), ("dz", dz)):
        if not np.all(np.isfinite(a)):
            broken.append(f"{nm} is not finite")
    x = dwq.astype(np.float64)
    worst = None
    for k in range(M):
        if not o["active"][k] or o["fail"][k]:
            if np.any(dwq[k] != 0):
                broken.append(f"dwq != 0 on the {'singular' if o['active'][k] else 'inactive'} row {k}")
            continue
        S, g = o["S"][k], o["g"][k]
        res = np.abs(S @ x[k] - g)
        # the bounds of S and g, the fp32 store of dwq (one rounding of every |S_rc dwq_c|), the fp64 solve
        bnd = (o["S_bound"][k] @ np.abs(x[k]) + o["g_bound"][k] + R.U32 * (np.abs(S) @ np.abs(x[k])) + D.fp64_solve_term(S, x[k])
               + R.DENORMAL)
        worst = max(worst or 0.0, float(np.max(res / bnd)))
    if worst is not None:
        ratios["A"] = worst
    ref = D.back_substitute(o, dwq)
    act = np.asarray(o["active"])
    if act.any():
        ratios["B"] = float(np.max(np.abs(dz.astype(np.float64) - ref.v)[act] / ref.bound()[act]))
    if np.any(dz[~act] != 0):
        broken.append("dz != 0 on an inactive row")
    d_in, s_in, q_in = f32(c["disps"]), f32(c["scales"]), f32(c["shifts"])
    ht, wd = d_in.shape[1:]
    rows = {f: k for k, f in enumerate(kx) if o["active"][k]}
    for f in range(len(d_in)):
        if f in rows:
            k = rows[f]
            if not np.array_equal(disps[f], np.maximum(f32(d_in[f] + dz[k].reshape(ht, wd)), np.float32(0))):
                broken.append(f"disps_after != fp32(max(fp32(disps + dz), 0)) on frame {f}")
            if scales[f] != np.float32(s_in[f] + dwq[k, 0]) or shifts[f] != np.float32(q_in[f] + dwq[k, 1]):
                broken.append(f"scales, shifts after != fp32(before + dwq) on frame {f}")
        elif not (np.array_equal(disps[f], d_in[f]) and scales[f] == s_in[f] and shifts[f] == q_in[f]):
            broken.append(f"frame {f} (inactive, no depth frame or out of range) did not keep its bits")
    return ratios, broken


def from_problem(pr, alpha=1.0, lm=1e-4, ep=0.1, ignore_frames=0, keep=None):
    """a case from the problem dict of tests/test_gpu_dspo.py, rounded to what the device reads"""
    c = {k: r32(pr[k]) for k in ("poses", "disps", "intr", "tgt", "wgt", "eta", "mono", "scales", "shifts")}
    c.update(ii=list(pr["ii"]), jj=list(pr["jj"]), vmask=np.asarray(pr["vmask"]), ignore_frames=ignore_frames, lm=lm, ep=ep, alpha=alpha,
             keep=None if keep is None else np.asarray(keep))
    return c


def criteria(name, disps, scales, shifts, dwq, dz):
    return criteria_for(case(name), oracle(name), disps, scales, shifts, dwq, dz)


def passes(ratios, broken):
    return not broken and all(r <= 1.0 for r in ratios.values())


def emulate(name, dtype=np.float32, mutate=None):
    return D.emulate(case(name), dtype, mutate)
