"""Shared inputs of tests/test_depth_fusion_cpu.py, tests/test_gpu_depth_fusion.py and tests/test_gpu_slam.py: mono-depth maps with every
defect the preparation has to deal with, at the shapes the kernels change path at, and a video buffer to fuse them into.  Nothing here
touches a GPU at import."""
import numpy as np

import depth_fusion_ref as F

# H, W -> where the defects sit: the 4 x 4 outlier patch (top-left corner of it), the inside zero, the top-edge zero's column, the hole.
# 12 x 9 is smaller than the erosion window: the defects are placed so that the 3 x 3 block at the bottom left stays known and the
# fill has to walk the whole map from there.
LAYOUT = {
    (12, 9): dict(patch=(0, 5), inside=(2, 3), top=2, corner=2),
    (37, 53): dict(patch=(10, 30), inside=(25, 10), top=20, corner=3),
    (48, 64): dict(patch=(20, 40), inside=(35, 12), top=30, corner=3),
    (67, 63): dict(patch=(30, 20), inside=(50, 45), top=40, corner=3),          # 4221 pixels: two spans of sgr_fuse_depth, odd rows
    (80, 104): dict(patch=(30, 60), inside=(60, 20), top=50, corner=3),         # 8320 pixels: three spans, 16-byte aligned rows
}
HOLE = (5, 5, 15)           # the 15 x 15 hole of the one 48 x 64 case that needs at least 8 passes
OUTLIER_GAIN = 25.0
SEEDS = {(12, 9): 1, (37, 53): 2, (48, 64): 3, (67, 63): 4, (80, 104): 5}


def surface(H, W, seed):
    """a smooth positive surface plus noise, fp32"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    s = 2.0 + 0.2 * np.sin(0.23 * x + 0.1 * seed) * np.cos(0.17 * y) + 0.004 * (x + y) * 32.0 / (H + W)
    return (s + rng.uniform(-0.02, 0.02, (H, W))).astype(np.float32)


def make_map(H, W, seed=None, hole=False):
    """the surface with a 4 x 4 patch at 25 x its value, outliers in the bottom-right corner, one zero inside, one on the top edge and,
    with hole, a 15 x 15 block of zeros"""
    lay = LAYOUT[(H, W)]
    m = surface(H, W, SEEDS[(H, W)] if seed is None else seed)
    py, px = lay["patch"]
    m[py:py + 4, px:px + 4] *= np.float32(OUTLIER_GAIN)
    c = lay["corner"]
    for k in range(c):                                  # a small staircase in the corner
        m[H - 1 - k, W - c + k:] *= np.float32(OUTLIER_GAIN)
    m[lay["inside"]] = 0.0
    m[0, lay["top"]] = 0.0
    if hole:
        hy, hx, hs = HOLE
        m[hy:hy + hs, hx:hx + hs] = 0.0
    return m


def threshold_margin(mono):
    """the smallest relative distance of a pixel from the outlier threshold 4 mean"""
    t = F.OUTLIER * F.mean32(mono)
    return float(np.abs(np.asarray(mono, float) - t).min() / t)


def check_map(mono):
    """the outlier threshold is not a rounding question, and the map has what it is there for"""
    assert threshold_margin(mono) > 1e-3, threshold_margin(mono)
    t = F.OUTLIER * F.mean32(mono)
    assert (mono > t).sum() >= 16 and (mono == 0).sum() >= 2 and ((mono > 0) & (mono < t)).sum() > mono.size // 2


def make_buffer(H, W, n=9, seed=0):
    """a video buffer of n frames: upsampled disparities in [0.3, 1], a valid-depth mask on ~60 % of the pixels, and one mono map per
    frame that is roughly 1.7 x the depth + 0.3 where it is sound"""
    rng = np.random.default_rng(100 + seed)
    disps = rng.uniform(0.3, 1.0, (n, H, W)).astype(np.float32)
    valid = rng.uniform(size=(n, H, W)) < 0.6
    monos = []
    for f in range(n):
        m = make_map(H, W, seed=10 * seed + f + 20)
        sound = m < 5.0
        m = np.where(sound & (m > 0), (1.7 / disps[f] + 0.3) * (1.0 + 0.02 * (m - 2.0)), m).astype(np.float32)
        monos.append(m)
    return disps, valid, np.stack(monos)
