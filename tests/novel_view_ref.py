"""The novel-view evaluation restated in plain numpy and Python (splat_slam_amd/novel_view.py, csrc/sgr_novel.hip): the exposure fit
from exactly rounded sums, the bound a kernel that adds in fp64 must stay within, the frame selection, the interpolation of the
keyframes' exposure, and the seeded cases the CPU and the GPU tests share."""
import bisect
import math

import numpy as np

U64 = 2.0 ** -53                    # unit roundoff of fp64
FIT_FLOOR = 2.0 ** -40              # det must exceed m^2 FIT_FLOOR max(S_rr / m, 1)


def fit_sums(render, gt):
    """(m, S_r, S_t, S_rr, S_rt, S_tt) over gt > 0: every term exact in fp64 (a product of two fp32 values is), every sum correctly rounded"""
    r = np.asarray(render, dtype=np.float32).reshape(-1)
    t = np.asarray(gt, dtype=np.float32).reshape(-1)
    mask = t > 0
    r, t = r[mask].astype(np.float64), t[mask].astype(np.float64)
    return (float(len(r)),) + tuple(math.fsum(v.tolist()) for v in (r, t, r * r, r * t, t * t))


def solve(sums):
    """(a, b, flag, g) of the six sums by the kernel's rule: degenerate frames give (0, 0) and flag 1"""
    m, sr, st, srr, srt, _ = sums
    if m < 2:
        return 0.0, 0.0, 1, None
    det = m * srr - sr * sr
    if not (det > 0 and det > m * m * FIT_FLOOR * max(srr / m, 1.0)):
        return 0.0, 0.0, 1, None
    g = (m * srt - sr * st) / det
    if not (g > 0 and math.isfinite(g)):
        return 0.0, 0.0, 1, g
    return math.log(g), (st - g * sr) / m, 0, g


def fit_ref(render, gt):
    """the reference fit: (a, b, flag) in fp64"""
    return solve(fit_sums(render, gt))[:3]


def fit_bound(render, gt):
    """first-order bound (da, db) on the fit of a kernel whose every sum may be off by (m - 1) 2^-53 sum |term| (any order of m fp64
    additions of exact terms); m itself is exact."""
    sums = fit_sums(render, gt)
    m, sr, st, srr, srt, _ = sums
    a, b, flag, g = solve(sums)
    assert flag == 0
    r = np.asarray(render, dtype=np.float64).reshape(-1)[np.asarray(gt).reshape(-1) > 0]
    t = np.asarray(gt, dtype=np.float64).reshape(-1)[np.asarray(gt).reshape(-1) > 0]
    e = (m - 1) * U64
    d_sr, d_st, d_srr, d_srt = (e * float(np.abs(v).sum()) for v in (r, t, r * r, r * t))
    det, num = m * srr - sr * sr, m * srt - sr * st
    d_num = m * d_srt + abs(st) * d_sr + abs(sr) * d_st
    d_det = m * d_srr + 2 * abs(sr) * d_sr
    d_g = d_num / abs(det) + abs(num) * d_det / det ** 2
    d_b = (d_st + abs(g) * d_sr + abs(sr) * d_g) / m
    return d_g / g, d_b


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def select_ref(num_frames, keyframe_timestamps, every=5, first=0):
    keys = set(int(t) for t in keyframe_timestamps)
    out, i = [], first
    while i < num_frames:
        if i not in keys:
            out.append(i)
        i += every
    return out


def interpolate_ref(kf_timestamps, kf_a, kf_b, timestamps):
    """linear in time between the two bracketing keyframes, constant outside; keyframe 0 counts as (0, 0)"""
    ts = [float(t) for t in kf_timestamps]
    va = [0.0] + [float(v) for v in kf_a[1:]]
    vb = [0.0] + [float(v) for v in kf_b[1:]]
    a, b = [], []
    for t in timestamps:
        t = float(t)
        if t <= ts[0] or len(ts) == 1:
            a.append(va[0]); b.append(vb[0])
        elif t >= ts[-1]:
            a.append(va[-1]); b.append(vb[-1])
        else:
            hi = bisect.bisect_right(ts, t)
            lo = hi - 1
            w = (t - ts[lo]) / (ts[hi] - ts[lo])
            a.append(va[lo] + w * (va[hi] - va[lo])); b.append(vb[lo] + w * (vb[hi] - vb[lo]))
    return np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)


# ---- the fit cases: (C, H, W) the smallest shapes at which the kernel can go wrong, n frames per call, and the exposure applied
SHAPES = ((1, 1, 2),        # the minimum, m = 2
          (3, 1, 1),        # m = 3
          (3, 7, 9),        # under one wave
          (3, 8, 8),        # exactly a multiple of 64
          (3, 31, 33),      # odd: a scalar tail behind the 16-byte groups
          (3, 64, 65))      # more than one workgroup per frame (12480 elements, 4096 a workgroup)
COUNTS = (1, 16)
EXPOSURES = ((1.0, 0.0), (1.3, -0.05), (0.6, 0.2))
# The identity (1, 0) is kept where m <= 3.  From 3 x 7 x 9 up it is replaced by NEAR_IDENTITY: the fit of an identity is (a, b) of the
# order of the noise, 1e-5, whose fp32 ulp (1e-12) lies below what m fp64 additions may lose, so fit_bound is no longer under a quarter
# of that ulp (tests/test_novel_view_cpu.py holds every case listed here to that); at (0.049, 0.03) an ulp is 4e-9 and it is.
NEAR_IDENTITY = (1.05, 0.03)
CASES = [(s, n, e) for s in SHAPES for n in COUNTS
         for e in (EXPOSURES if s[0] * s[1] * s[2] <= 3 else (NEAR_IDENTITY,) + EXPOSURES[1:])]


def case_id(case):
    (C, H, W), n, (g0, b0) = case
    return f"{C}x{H}x{W}-n{n}-g{g0}-b{b0}"


def make_case(case, seed=0):
    """(render, gt) [n,C,H,W] fp32: render uniform in [0.1, 0.9], gt = clamp(g0 render + b0 + 1e-3 noise, 0, 1) in fp32 with a fifth
    of its elements (rounded down) set to 0, so that the mask matters"""
    (C, H, W), n, (g0, b0) = case
    rng = np.random.default_rng([seed, C, H, W, n, int(round(1000 * g0)), int(round(1000 * (b0 + 1)))])
    N = C * H * W
    render = rng.uniform(0.1, 0.9, size=(n, N)).astype(np.float32)
    noise = rng.standard_normal((n, N)).astype(np.float32)
    gt = np.clip(np.float32(g0) * render + np.float32(b0) + noise * np.float32(1e-3), np.float32(0), np.float32(1)).astype(np.float32)
    for f in range(n):
        gt[f, rng.permutation(N)[:N // 5]] = 0
    return render.reshape(n, C, H, W), gt.reshape(n, C, H, W)
