"""splat_slam_amd.depth_fusion on the MI355X against the fp64 restatement (tests/depth_fusion_ref.py): the preparation of a mono map at
every shape at which the kernels change path, the fusion read in place through frame indices, the invalid-frame rule, KeyframeDepth on a
DepthVideo, and the argument checks.  Where a result is a selection or one rounded operation it is held bit for bit; the fill is held to
P * 64 * 2^-24 * max(known): P passes, each a convex combination of at most 48 fp32 terms (a quotient of two sums of 48 rounded
products: under 64 roundings of a value that never exceeds the largest known one)."""
import types

import numpy as np
import pytest
import torch

import depth_fusion_cases as C
import depth_fusion_ref as F
import tracker_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
PREPARE_CASES = [(12, 9, False), (37, 53, False), (48, 64, False), (48, 64, True)]
FUSE_SHAPES = [(37, 53), (48, 64), (67, 63), (80, 104)]
INDS = [7, 2, 2, 5]


def gpu(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def np_(t):
    return t.detach().cpu().numpy()


def bits(t):
    return np_(t).view(np.int32) if t.dtype == torch.float32 else np_(t)


def check_prepared(mono, filled, eroded):
    """one map against the oracle; returns the largest error of a filled pixel over its bound"""
    want, er, passes = F.prepare(mono)
    np.testing.assert_array_equal(eroded.astype(bool), er)
    assert set(np.unique(eroded)) <= {0, 1}
    np.testing.assert_array_equal(filled[er].view(np.int32), mono[er].view(np.int32))
    if er.all() or not er.any():
        np.testing.assert_array_equal(filled, want.astype(np.float32))
        return 0.0
    bound = passes * 64 * 2.0 ** -24 * float(mono[er].max())
    err = np.abs(filled.astype(float) - want)[~er].max()
    print(f"fill {mono.shape}: passes {passes}, err {err:.3e}, bound {bound:.3e}, err / bound {err / bound:.4f}")
    assert err <= bound, (err, bound)
    assert filled.min() >= mono[er].min() - bound and filled.max() <= mono[er].max() + bound
    return err / bound


@pytest.mark.parametrize("H,W,hole", PREPARE_CASES)
def test_prepare_mono_matches_the_oracle(H, W, hole):
    from splat_slam_amd import depth_fusion as df
    mono = C.make_map(H, W, hole=hole)
    C.check_map(mono)
    filled, eroded = df.prepare_mono(gpu(mono))
    assert filled.shape == (H, W) and eroded.shape == (H, W) and eroded.dtype == torch.uint8
    check_prepared(mono, np_(filled), np_(eroded))
    if hole:
        assert F.prepare(mono)[2] >= 8


def test_prepare_mono_all_zero_fully_known_and_batched():
    from splat_slam_amd import depth_fusion as df
    H, W = 37, 53
    maps = np.stack([np.zeros((H, W), np.float32), C.surface(H, W, 7), C.make_map(H, W), C.make_map(H, W, seed=9)])
    filled, eroded = df.prepare_mono(gpu(maps))
    assert filled.shape == (4, H, W)
    f, e = np_(filled), np_(eroded)
    assert not f[0].any() and not e[0].any()
    assert e[1].all() and np.array_equal(f[1].view(np.int32), maps[1].view(np.int32))
    for k in range(4):
        check_prepared(maps[k], f[k], e[k])
    # a map gives the same bits alone, and a second run the same bits again
    one_f, one_e = df.prepare_mono(gpu(maps[3]))
    assert np.array_equal(bits(one_f), f[3].view(np.int32)) and np.array_equal(np_(one_e), e[3])
    again_f, again_e = df.prepare_mono(gpu(maps))
    assert torch.equal(again_f, filled) and torch.equal(again_e, eroded)
    # a map of one pixel, and one with a single row
    f1, e1 = df.prepare_mono(gpu(np.full((1, 1), 2.0, np.float32)))
    assert f1.item() == 2.0 and e1.item() == 1
    row = C.surface(1, 70, 3)
    row[0, 40] = 0.0
    fr, er_ = df.prepare_mono(gpu(row))
    check_prepared(row, np_(fr), np_(er_))


@pytest.fixture(scope="module")
def buffers():
    """per shape: the numpy inputs, their GPU copies and the GPU's own preparation of the nine mono maps (computed once, never changed)"""
    from splat_slam_amd import depth_fusion as df
    out = {}
    for H, W in FUSE_SHAPES:
        disps, valid, monos = C.make_buffer(H, W)
        for m in monos:
            C.check_map(m)
        g = types.SimpleNamespace(disps=gpu(disps), valid=gpu(valid, torch.bool), monos=gpu(monos))
        g.filled, g.eroded = df.prepare_mono(g.monos)
        out[(H, W)] = (disps, valid, monos, g)
    return out


@pytest.mark.parametrize("H,W", FUSE_SHAPES)
@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.uint8])
def test_fuse_depth_reads_frames_in_place_and_matches_the_oracle(buffers, H, W, mask_dtype):
    from splat_slam_amd import depth_fusion as df
    disps, valid, monos, g = buffers[(H, W)]
    vmask = g.valid if mask_dtype == torch.bool else (g.valid.to(torch.uint8) * 255)
    depth, scale, shift, invalid = df.fuse_depth(g.disps, vmask, g.filled, g.eroded, INDS)
    assert depth.shape == (4, H, W) and scale.shape == (4,) and invalid.dtype == torch.uint8 and not invalid.any()
    filled, eroded = np_(g.filled), np_(g.eroded)
    for b, f in enumerate(INDS):
        v = g.valid[f]
        tracker = 1.0 / g.disps[f]
        mono_wq = g.filled[f] * scale[b] + shift[b]
        assert np.array_equal(bits(depth[b])[np_(v)], bits(tracker)[np_(v)])
        assert np.array_equal(bits(depth[b])[~np_(v)], bits(mono_wq)[~np_(v)])
        _, s, q, inv = F.fuse(filled[f], disps[f], valid[f], eroded[f])
        print(f"frame {f} of {(H, W)}: s {scale[b].item():.8f} / {s:.8f}, q {shift[b].item():.8f} / {q:.8f}")
        assert not inv
        np.testing.assert_allclose(scale[b].item(), s, rtol=1e-5)
        np.testing.assert_allclose(shift[b].item(), q, rtol=1e-5)
    # the two entries of frame 2 are identical, and frame 5 alone gives the bits it gives in the batch
    assert torch.equal(depth[1], depth[2]) and scale[1] == scale[2] and shift[1] == shift[2]
    d5, s5, q5, i5 = df.fuse_depth(g.disps, vmask, g.filled, g.eroded, torch.tensor([5], device=DEV))
    assert torch.equal(d5[0], depth[3]) and s5[0] == scale[3] and q5[0] == shift[3] and not i5.any()
    # the same fit as sgr_dspo_align's, which reads copies
    from splat_slam_amd import dspo
    ix = torch.tensor(INDS, device=DEV)
    target = torch.where(g.valid[ix], 1.0 / g.disps[ix], torch.zeros((), device=DEV)).contiguous()
    s_al, q_al, _ = dspo.align_scale_and_shift(g.filled[ix].contiguous(), target, (g.valid[ix] & (g.eroded[ix] != 0)).contiguous())
    np.testing.assert_allclose(np_(scale), np_(s_al), rtol=1e-5)
    np.testing.assert_allclose(np_(shift), np_(q_al), rtol=1e-5)


def test_fuse_depth_invalid_frames_and_a_fit_without_support(buffers):
    from splat_slam_amd import depth_fusion as df
    from splat_slam_amd import dspo
    H, W = 48, 64
    disps, valid, monos, g = buffers[(H, W)]
    er = np_(g.eroded).astype(bool)
    vm = np.zeros_like(valid)
    vm[0].reshape(-1)[np.flatnonzero(er[0])[:99]] = True            # 99 valid pixels: invalid
    vm[1].reshape(-1)[np.flatnonzero(er[0])[:100]] = True           # frame 1 is frame 0 with one more valid pixel: fused
    vm[2].reshape(-1)[np.flatnonzero(~er[2])[:150]] = True          # every valid pixel in the eroded-away region: 0 / 0
    mask = gpu(vm, torch.bool)
    filled, eroded, disps_g = g.filled.clone(), g.eroded.clone(), g.disps.clone()
    filled[1], eroded[1], disps_g[1] = g.filled[0], g.eroded[0], g.disps[0]
    depth, scale, shift, invalid = df.fuse_depth(disps_g, mask, filled, eroded, [0, 1, 2])
    assert invalid.tolist() == [1, 0, 0]
    d = np_(depth)
    assert not d[0][~vm[0]].any() and np.array_equal(d[0][vm[0]], np_(1.0 / disps_g[0])[vm[0]])
    _, s, q, inv = F.fuse(np_(filled[1]), np_(disps_g[1]), vm[1], np_(eroded[1]))
    assert not inv
    np.testing.assert_allclose(scale[1].item(), s, rtol=1e-5)
    np.testing.assert_allclose(shift[1].item(), q, rtol=1e-5)
    assert np.array_equal(bits(depth[1])[~vm[1]], bits(filled[1] * scale[1] + shift[1])[~vm[1]])
    # no support: what sgr_dspo_align gives for the same sums
    target = torch.where(mask[2], 1.0 / disps_g[2], torch.zeros((), device=DEV))[None].contiguous()
    s_al, q_al, _ = dspo.align_scale_and_shift(filled[2:3].contiguous(), target, (mask[2] & (eroded[2] != 0))[None].contiguous())
    assert torch.isnan(s_al).all() and torch.isnan(q_al).all()
    assert np.isnan(scale[2].item()) and np.isnan(shift[2].item())
    assert np.array_equal(d[2][vm[2]], np_(1.0 / disps_g[2])[vm[2]]) and np.isnan(d[2][~vm[2]]).all()
    # min_valid is an argument
    assert df.fuse_depth(disps_g, mask, filled, eroded, [0, 1], min_valid=99)[3].tolist() == [0, 0]
    assert df.fuse_depth(disps_g, mask, filled, eroded, [0, 1], min_valid=101)[3].tolist() == [1, 1]
    # a device index tensor is not read by the host: an entry out of range is a slot flagged invalid, the others are unaffected
    dd, ss, qq, ii = df.fuse_depth(disps_g, mask, filled, eroded, torch.tensor([1, 9, -1], device=DEV))
    assert ii.tolist() == [0, 1, 1] and torch.equal(dd[0], depth[1]) and ss[0] == scale[1]
    assert not dd[1:].any()                                         # no such frame: a depth of zeros


def video_with_depth():
    """tracker_cases.make_video with upsampled disparities, a valid-depth mask and one mono map per frame"""
    v = T.make_video()
    disps, valid, monos = C.make_buffer(T.HT, T.WD, n=T.N_FRAMES, seed=1)
    v.disps_up[:T.N_FRAMES] = gpu(disps)
    v.valid_depth_mask[:T.N_FRAMES] = gpu(valid, torch.bool)
    v.depth_scale[:] = 7.0
    v.depth_shift[:] = -3.0
    return v, gpu(monos)


def test_keyframe_depth_is_prepare_fuse_and_pose_by_hand():
    from splat_slam_amd import depth_fusion as df
    v, monos = video_with_depth()
    v2, _ = video_with_depth()
    v.valid_depth_mask[4] = False
    v.valid_depth_mask[4, 0, :99] = True                             # frame 4: 99 valid pixels
    v2.valid_depth_mask[4] = v.valid_depth_mask[4]
    kd = df.KeyframeDepth(v)
    idxs = [6, 1, 4, 9]
    for i in idxs:
        kd.put_mono(i, monos[i])
    with pytest.raises(KeyError, match="no mono map"):
        kd.get([6, 3])
    depth, w2c, invalid = kd.get(idxs)
    assert invalid == [False, False, True, False] and depth.shape == (4, T.HT, T.WD) and w2c.shape == (4, 4, 4)
    # by hand on the second video
    filled, eroded = torch.zeros_like(v2.disps_up), torch.zeros(v2.disps_up.shape, dtype=torch.uint8, device=DEV)
    for i in idxs:
        filled[i], eroded[i] = df.prepare_mono(monos[i])
    d2, s2, q2, i2 = df.fuse_depth(v2.disps_up, v2.valid_depth_mask, filled, eroded, idxs)
    assert torch.equal(depth, d2) and i2.tolist() == [0, 0, 1, 0]
    for b, i in enumerate(idxs):
        c2w = v2.get_pose(i, DEV)
        # w2c is the inverse of c2w to the rounding of a 4 x 4 inverse: entries of size <= 1 + |t|, a few units of 2^-24 each
        err = (w2c[b].double() @ c2w.double() - torch.eye(4, device=DEV, dtype=torch.double)).abs().max().item()
        assert err < 64 * 2.0 ** -24 * (1.0 + v2.poses[i, :3].abs().max().item()), err
        assert torch.equal(w2c[b, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV))
        est, msk, _ = v2.get_depth_and_pose(i, DEV)
        assert torch.equal(depth[b][msk], est[msk])
        if b == 2:
            assert v.depth_scale[i] == 7.0 and v.depth_shift[i] == -3.0 and not depth[b][~msk].any()
        else:
            assert v.depth_scale[i] == s2[b] and v.depth_shift[i] == q2[b] and v.depth_scale[i] != 7.0
    untouched = [i for i in range(v.depth_scale.shape[0]) if i not in idxs]
    assert (v.depth_scale[untouched] == 7.0).all() and (v.depth_shift[untouched] == -3.0).all()
    # the single-frame form, in the reference's order
    d1, w1, inv1 = kd.get_w2c_and_depth(9)
    assert torch.equal(d1, depth[3]) and torch.equal(w1, w2c[3]) and inv1 is False


def test_prepare_and_fuse_do_not_synchronise_and_get_reads_the_host_once(buffers):
    import warnings
    from splat_slam_amd import depth_fusion as df
    g = buffers[(48, 64)][3]
    v, monos = video_with_depth()
    kd = df.KeyframeDepth(v)
    kd.put_mono(2, monos[2])                                         # (allocates the cache)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        df.prepare_mono(g.monos)
        df.fuse_depth(g.disps, g.valid, g.filled, g.eroded, INDS)
        kd.put_mono(3, monos[3])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            kd.get([2, 3, 2])
        finally:
            torch.cuda.set_sync_debug_mode(0)
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, syncs


class _NoLaunch:
    """splat_slam_amd._native without its library: any kernel call is an error"""

    def __init__(self, nat):
        self._nat = nat

    def __getattr__(self, name):
        if name == "lib":
            raise AssertionError("a kernel was about to be launched")
        return getattr(self._nat, name)


def test_bad_arguments_raise_and_launch_nothing(monkeypatch, buffers):
    from splat_slam_amd import depth_fusion as df
    monkeypatch.setattr(df, "nat", _NoLaunch(df.nat))
    H, W = 48, 64
    g = buffers[(H, W)][3]
    a = dict(disps_up=g.disps, valid_depth_mask=g.valid, mono_filled=g.filled, eroded=g.eroded, inds=[0, 1])
    cases = [
        (dict(disps_up=g.disps.double()), TypeError, "disps_up must be torch.float32"),
        (dict(mono_filled=g.filled.half()), TypeError, "mono_filled must be torch.float32"),
        (dict(eroded=g.eroded.bool()), TypeError, "eroded must be torch.uint8"),
        (dict(valid_depth_mask=g.valid.float()), TypeError, "valid_depth_mask must be torch.bool or torch.uint8"),
        (dict(inds=torch.tensor([0, 1], dtype=torch.int32, device=DEV)), TypeError, "inds must be torch.int64"),
        (dict(inds=3), TypeError, "inds must be a sequence"),
        (dict(disps_up=g.disps[0]), ValueError, "disps_up must have 3 dimensions"),
        (dict(eroded=g.eroded[:4]), ValueError, "eroded must have the shape of disps_up"),
        (dict(inds=torch.zeros((2, 1), dtype=torch.int64, device=DEV)), ValueError, "inds must have 1 dimensions"),
        (dict(mono_filled=g.filled.transpose(1, 2)), ValueError, "mono_filled must be contiguous"),
        (dict(disps_up=g.disps.cpu()), RuntimeError, "GPU tensor"),
        (dict(eroded=g.eroded.cpu()), RuntimeError, "GPU tensor"),
        (dict(inds=[0, 9]), IndexError, r"frame index 9 lies outside \[0, 9\)"),
        (dict(inds=[-1]), IndexError, r"frame index -1 lies outside"),
        (dict(inds=torch.tensor([2, 12])), IndexError, r"frame index 12 lies outside"),
    ]
    for kw, err, msg in cases:
        with pytest.raises(err, match=msg):
            df.fuse_depth(**{**a, **kw})
    for mono, err, msg in [(g.monos.double(), TypeError, "mono must be torch.float32"),
                           (g.monos[None], ValueError, "mono must have 3 dimensions"),
                           (g.monos.transpose(1, 2), ValueError, "mono must be contiguous"),
                           (g.monos.cpu(), RuntimeError, "GPU tensor"),
                           (np_(g.monos), TypeError, "mono must be a torch.Tensor")]:
        with pytest.raises(err, match=msg):
            df.prepare_mono(mono)
    with pytest.raises(AssertionError, match="about to be launched"):      # the guard itself works
        df.fuse_depth(**a)
