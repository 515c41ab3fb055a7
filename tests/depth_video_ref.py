"""numpy restatement of the depth-video kernels (splat_slam_amd/depth_video.py, csrc/sgr_video.hip), written from the algorithm as
DESIGN.md section 3 ("Depth video") states it: the convex upsampling and the threshold in fp64, the lower-median mask in the fp32
arithmetic the text prescribes (one IEEE division, one IEEE product, comparisons: nothing to round differently), and the chain
threshold -> depth_filter -> mask with the bracket of medians and the per-pixel `safe` flag that tests need to stay off the knife
edge.  Also the scenes the chain is tested on (the CPU tests check their properties with this file alone)."""
import numpy as np

import dba_ref as R

KNIFE = 1e-3            # decision margin below which a depth_filter count may differ (the bound tests/test_gpu_dba.py uses)


def cvx_upsample(d, mask):
    """d [h,w], mask [576,h,w] logits -> [8h,8w]: out[8y+dy, 8x+dx] = sum_k softmax_k(mask[k*64+dy*8+dx, y, x]) d[y+ny, x+nx],
    k = 3 (ny+1) + (nx+1), d = 0 outside the map."""
    d, mask = np.asarray(d, float), np.asarray(mask, float)
    h, w = d.shape
    m = mask.reshape(9, 8, 8, h, w)
    e = np.exp(m - m.max(axis=0, keepdims=True))
    wgt = e / e.sum(axis=0, keepdims=True)
    pad = np.zeros((h + 2, w + 2))
    pad[1:-1, 1:-1] = d
    out = np.zeros((8, 8, h, w))
    for k in range(9):
        ny, nx = k // 3 - 1, k % 3 - 1
        out += wgt[k] * pad[1 + ny:1 + ny + h, 1 + nx:1 + nx + w][None, None]
    return out.transpose(2, 0, 3, 1).reshape(8 * h, 8 * w)                       # [y, dy, x, dx]


def neighbourhood_max(d):
    """max |d| over each pixel's 3 x 3 neighbourhood, repeated to the upsampled grid: the scale of the upsampling's error bound"""
    a = np.abs(np.asarray(d, float))
    h, w = a.shape
    pad = np.zeros((h + 2, w + 2))
    pad[1:-1, 1:-1] = a
    m = np.max([pad[i:i + h, j:j + w] for i in range(3) for j in range(3)], axis=0)
    return np.repeat(np.repeat(m, 8, axis=0), 8, axis=1)


def depths32(disps):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(1.0) / np.asarray(disps, np.float32)                   # the IEEE fp32 division of the text


def depth_thresh(disps, inds, rel):
    """fp64: fp32(rel) * mean over the frame of the fp32 quotients 1 / disp"""
    dep = depths32(disps).astype(float)
    return np.array([float(np.float32(rel)) * dep[i].mean() for i in inds])


def lower_median(values):
    """element of 0-based rank (m-1)//2 in ascending order; NaN for an empty set"""
    v = np.sort(np.asarray(values).reshape(-1))
    return v[(len(v) - 1) // 2] if len(v) else np.float32(np.nan)


def mask_from_counts(disps, inds, counts, visible_num):
    """[len(inds),h,w] bool and the medians: candidate = counts >= visible_num and depth not NaN; mask = candidate and
    depth < fp32(3 * median).  The row of an index outside [0, N) is all False with a NaN median (the kernels write nothing for it)."""
    dep = depths32(disps)
    out, meds = [], []
    for b, i in enumerate(inds):
        if not 0 <= i < len(dep):                       # a slot that names no frame is a no-op: nothing to compare with
            out.append(np.zeros(dep.shape[1:], bool)), meds.append(np.float32(np.nan))
            continue
        cand = (np.asarray(counts[b]) >= visible_num) & ~np.isnan(dep[i])
        med = np.float32(lower_median(dep[i][cand]))
        with np.errstate(invalid="ignore"):
            out.append(cand & (dep[i] < np.float32(3.0) * med))
        meds.append(med)
    return np.stack(out), np.array(meds, np.float32)


def valid_depth_mask(poses, disps, intr, inds, rel, visible_num):
    """The chain on fp32-valued inputs.  Returns mask [n,h,w], med_lo, med_hi [n] and safe [n,h,w].  A count is safe when no decision
    behind it came within KNIFE of its threshold.  With A the depths of the safe candidates (m0 of them, ascending) and k pixels
    that may or may not be candidates, the median of any admissible candidate set lies in
    [A[(m0-k-1)//2], A[(m0+k-1)//2]] (ranks clipped to A; the k extra values all below, or all above); this contains the medians with
    every knife-edge pixel counted in and with every one counted out.  A pixel is safe when its count is and its depth lies outside
    [3 med_lo, 3 med_hi] widened by one fp32 ulp."""
    p, d, K = (np.asarray(a, np.float32).astype(float) for a in (poses, disps, intr))
    thresh = depth_thresh(d, inds, rel).astype(np.float32).astype(float)
    counts, marg = R.depth_filter(p, d, K, list(inds), thresh, margins=True)
    mask, _ = mask_from_counts(d, inds, counts, visible_num)
    dep = depths32(d)
    sure = marg > KNIFE
    lo, hi, safe = [], [], []
    for b, i in enumerate(inds):
        ok = ~np.isnan(dep[i])
        A = np.sort(dep[i][sure[b] & (counts[b] >= visible_num) & ok])
        k = int((~sure[b] & ok).sum())
        m0 = len(A)
        if m0 == 0 or (m0 - k - 1) // 2 < 0 or (m0 + k - 1) // 2 > m0 - 1:
            lo.append(np.nan), hi.append(np.nan), safe.append(np.zeros_like(sure[b]))
            continue
        a, c = np.float32(A[(m0 - k - 1) // 2]), np.float32(A[(m0 + k - 1) // 2])
        t_lo = np.nextafter(np.float32(3.0) * a, np.float32(-np.inf))
        t_hi = np.nextafter(np.float32(3.0) * c, np.float32(np.inf))
        lo.append(a), hi.append(c)
        safe.append(sure[b] & ((dep[i] < t_lo) | (dep[i] > t_hi)))
    return mask, np.array(lo), np.array(hi), np.stack(safe)


# ---- scenes
SHAPES = {(48, 64): np.array([50.0, 52.0, 31.5, 23.5]), (40, 80): np.array([60.0, 58.0, 39.5, 19.5])}
REL, VISIBLE = 0.05, 2


def chain_scene(shape, n=10, seed=0):
    """A nearly planar scene (disparities 0.45 .. 0.55, as in test_depth_filter_counts_match_away_from_the_knife_edge) under a slow
    camera motion, with a block of far pixels at about 10 x the typical depth in every frame (consistent across views, so they are
    candidates, and beyond 3 x the median) and a block whose disparity changes from frame to frame (no two views agree on it)."""
    ht, wd = shape
    rng = np.random.default_rng(seed)
    poses = []
    for f in range(n):
        t, q = R.exp_se3(np.concatenate([[0.03 * f, 0.01 * np.sin(f), 0.02 * f], rng.normal(0, 0.02, 3)]))
        poses.append(np.concatenate([t, q]))
    disps = rng.uniform(0.45, 0.55, (n, ht, wd))
    disps[:, ht // 2:ht // 2 + 12, wd // 2:wd // 2 + 16] = 0.05 * rng.uniform(0.999, 1.001, (n, 12, 16))
    for f in range(n):
        disps[f, 4:12, 4:14] = 0.25 + 0.08 * f
    return np.stack(poses), disps, SHAPES[shape]
