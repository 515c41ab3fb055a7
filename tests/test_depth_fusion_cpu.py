"""CPU checks of the keyframe depth fusion: the fp64 restatement (tests/depth_fusion_ref.py) is a sound yardstick -- its erosion is the
reference's padded scipy erosion, its fill keeps what is known and stays a convex combination --, the test maps keep the outlier
threshold away from rounding, and the library exports and binds sgr_fuse_*.  No GPU."""
import ctypes

import numpy as np
import pytest

import depth_fusion_cases as C
import depth_fusion_ref as F


def holed(H, W, seed):
    """positive flags with zeros at a corner, on an edge and inside"""
    rng = np.random.default_rng(seed)
    pos = np.ones((H, W), bool)
    pos[0, 0] = pos[H - 1, W - 1] = False                  # corners
    pos[0, W // 2] = pos[H // 2, 0] = pos[H - 1, 1] = False  # edges
    pos[H // 2, W // 2] = False                            # inside
    if H * W > 500:
        pos[rng.integers(8, H - 8, 3), rng.integers(8, W - 8, 3)] = False
    return pos


@pytest.mark.parametrize("H,W", [(12, 9), (37, 53)])
def test_oracle_erosion_is_the_padded_scipy_erosion(H, W):
    ndimage = pytest.importorskip("scipy.ndimage")
    for seed, pos in enumerate([holed(H, W, 0), np.ones((H, W), bool), np.zeros((H, W), bool)]):
        single = np.ones((H, W), bool)
        single[H - 1, 0] = False                           # one corner alone: what the padding protects is visible
        for p in (pos, single):
            padded = np.pad(p.astype(int), pad_width=5, mode="constant", constant_values=1)
            want = ndimage.binary_erosion(padded, structure=np.ones((3, 3), dtype=int), iterations=5)[5:-5, 5:-5]
            np.testing.assert_array_equal(F.erode(p), want)
    assert F.erode(single).sum() == H * W - min(6, H) * min(6, W) and F.erode(single).any()


@pytest.mark.parametrize("H,W,hole", [(12, 9, False), (37, 53, False), (48, 64, False), (48, 64, True)])
def test_oracle_fill_keeps_known_pixels_and_stays_a_convex_combination(H, W, hole):
    mono = C.make_map(H, W, hole=hole)
    C.check_map(mono)
    filled, er, passes = F.prepare(mono)
    assert er.any() and not er.all()
    np.testing.assert_array_equal(filled[er], mono[er].astype(float))
    lo, hi = mono[er].min(), mono[er].max()
    assert filled.min() >= lo and filled.max() <= hi and (filled > 0).all()
    assert passes >= (8 if hole or (H, W) == (12, 9) else 6)
    # the passes are layers of chessboard distance from the known set
    _, _, stamp = F.fill(np.where(er, mono, 0.0), er)
    assert stamp.max() == passes and (stamp[er] == 0).all() and (stamp[~er] >= 1).all()


def test_oracle_all_zero_map_stays_zero_and_a_known_map_takes_no_pass():
    filled, er, passes = F.prepare(np.zeros((12, 9), np.float32))
    assert not filled.any() and not er.any() and passes == 0
    mono = C.surface(37, 53, 7)
    filled, er, passes = F.prepare(mono)
    assert er.all() and passes == 0
    np.testing.assert_array_equal(filled, mono.astype(float))
    # known pixels nowhere (every pixel an outlier of its own erosion): nothing to fill from
    lone = np.zeros((12, 9), np.float32)
    lone[6, 4] = 1.0
    filled, er, passes = F.prepare(lone)
    assert not filled.any() and passes == 0


def test_oracle_fit_recovers_an_exact_scale_and_shift_and_counts_valid_pixels():
    disps, valid, monos = C.make_buffer(37, 53)
    filled, er, _ = F.prepare(monos[0])
    target = (np.float32(1.0) / disps[0]).astype(float)
    depth, s, q, invalid = F.fuse((target - 0.25) / 1.5, disps[0], valid[0], er)
    assert not invalid and abs(s - 1.5) < 1e-9 and abs(q - 0.25) < 1e-9
    np.testing.assert_allclose(depth, target, rtol=1e-9)
    few = np.zeros_like(valid[0])
    few.reshape(-1)[np.flatnonzero(er)[:99]] = True
    depth, s, q, invalid = F.fuse(filled, disps[0], few, er)
    assert invalid and s is None and not depth[~few].any() and (depth[few] == target[few]).all()
    few.reshape(-1)[np.flatnonzero(er)[99]] = True
    assert not F.fuse(filled, disps[0], few, er)[3]
    # every valid pixel eroded away: a zero determinant, IEEE 0 / 0
    gone = np.zeros_like(valid[0])
    gone.reshape(-1)[np.flatnonzero(~er)[:120]] = True
    _, s, q, invalid = F.fuse(filled, disps[0], gone, er)
    assert not invalid and np.isnan(s) and np.isnan(q)


@pytest.mark.parametrize("H,W", sorted(C.LAYOUT))
def test_every_test_map_keeps_the_outlier_threshold_away_from_rounding(H, W):
    C.check_map(C.make_map(H, W))
    if (H, W) == (48, 64):
        C.check_map(C.make_map(H, W, hole=True))
    if (H, W) != (12, 9):
        for mono in C.make_buffer(H, W)[2]:
            C.check_map(mono)


def test_library_exports_and_binds_the_fuse_entry_points():
    from splat_slam_amd.build import build_native
    from splat_slam_amd import _native as nat
    h = ctypes.CDLL(build_native(verbose=False))
    for name in ("sgr_fuse_prepare", "sgr_fuse_depth", "sgr_fuse_scratch_bytes"):
        assert name in nat.SIGNATURES, name
        assert hasattr(h, name), name
        assert getattr(nat.lib(), name).argtypes == nat.SIGNATURES[name][1]
    lib = nat.lib()
    small, large = lib.sgr_fuse_scratch_bytes(1, 48, 64), lib.sgr_fuse_scratch_bytes(64, 480, 640)
    assert 2 * 4 * 48 * 64 <= small < large                 # the fill's stamps and hole list, one int per pixel each
    assert small % 16 == 0 and large % 16 == 0
    assert lib.sgr_fuse_scratch_bytes(0, 48, 64) == 0 and lib.sgr_fuse_scratch_bytes(70000, 48, 64) == 0
    assert lib.sgr_fuse_scratch_bytes(1, 0, 64) == 0 and lib.sgr_fuse_scratch_bytes(1, 1 << 14, 1 << 14) == 0


def test_the_wrappers_reject_cpu_tensors_and_bad_arguments_before_the_device():
    import torch
    from splat_slam_amd import depth_fusion as df
    with pytest.raises(RuntimeError, match="GPU tensor"):
        df.prepare_mono(torch.ones(6, 8))
    with pytest.raises(TypeError, match="mono must be torch.float32"):
        df.prepare_mono(torch.ones(6, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="mono must have 3 dimensions"):
        df.prepare_mono(torch.ones(2, 2, 6, 8))
    a = dict(disps_up=torch.ones(4, 6, 8), valid_depth_mask=torch.ones(4, 6, 8, dtype=torch.bool), mono_filled=torch.ones(4, 6, 8),
             eroded=torch.ones(4, 6, 8, dtype=torch.uint8), inds=[0, 1])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        df.fuse_depth(**a)
    for kw, err, msg in [(dict(eroded=torch.ones(4, 6, 8, dtype=torch.bool)), TypeError, "eroded must be torch.uint8"),
                         (dict(valid_depth_mask=torch.ones(4, 6, 8)), TypeError, "valid_depth_mask must be torch.bool or torch.uint8"),
                         (dict(mono_filled=torch.ones(4, 6, 9)), ValueError, "mono_filled must have the shape of disps_up"),
                         (dict(disps_up=torch.ones(4, 6, 16)[:, :, ::2]), ValueError, "disps_up must be contiguous")]:
        with pytest.raises(err, match=msg):
            df.fuse_depth(**{**a, **kw})
    assert "deliberate" in df.__doc__
