"""fp64 numpy restatement of sgr_corr_volume_pyramid (include/splat_hip.h), written from its definition: level 0 is the all-pairs
correlation of two planes of channels-first maps divided by 16, level l the mean of level 0 over the aligned 2^l x 2^l blocks of the
second map's pixels, for block rows < h >> l and block columns < w >> l (an odd last row or column is dropped).  Every level comes
as (value, magnitude): the magnitude is the same expression with every product replaced by its absolute value.  The lookup's oracle
is corr_ref.corr_index_forward, level by level."""
import numpy as np


def block_mean(v0, level):
    """[..., h, w] -> [..., h >> level, w >> level]: the mean over aligned 2^level x 2^level blocks, written as one reshape"""
    k = 1 << level
    h, w = v0.shape[-2:]
    hl, wl = h >> level, w >> level
    return v0[..., :hl * k, :wl * k].reshape(v0.shape[:-2] + (hl, k, wl, k)).mean(axis=(-3, -1))


def volume_pyramid(maps, src, dst, levels):
    """maps [planes,C,h,w] (any float dtype, widened), src, dst [E] plane indices -> [(value, magnitude)] per level, each
    [E,h,w,h >> l,w >> l] fp64.  An edge with a plane outside [0, planes) is zeros."""
    planes, C, h, w = maps.shape
    m = maps.astype(np.float64).reshape(planes, C, h * w)
    E = len(src)
    val, mag = np.zeros((E, h * w, h * w)), np.zeros((E, h * w, h * w))
    for e, (s, d) in enumerate(zip(src, dst)):
        if 0 <= s < planes and 0 <= d < planes:
            val[e] = m[s].T @ m[d] / 16.0
            mag[e] = np.abs(m[s]).T @ np.abs(m[d]) / 16.0
    val, mag = val.reshape(E, h, w, h, w), mag.reshape(E, h, w, h, w)
    return [(block_mean(val, l), block_mean(mag, l)) for l in range(levels)]
