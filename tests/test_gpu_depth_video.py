"""splat_slam_amd.depth_video on the MI355X against the numpy restatement (tests/depth_video_ref.py): the convex upsampling to a bound
that follows from its arithmetic, the threshold to 2 ulp, the lower-median mask bit for bit, the chain on every pixel away from the
knife edge and bit for bit against its three stages, and the DepthVideo class on top of them."""
import numpy as np
import pytest
import torch

import dba_ref as R
import depth_video_ref as V

pytestmark = pytest.mark.gpu

DEV = "cuda"


def f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def li(a):
    return torch.tensor(np.asarray(a), dtype=torch.int64, device=DEV)


def r32(a):
    return np.asarray(a, np.float32).astype(float)


# ---- upsampling
@pytest.mark.parametrize("shape", [(48, 64), (40, 80)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_upsampling_matches_the_ref(shape, dtype):
    """|out - ref| <= 1e-5 max|d| over the pixel's 3 x 3 neighbourhood: x - max rounds once (<= 16 * 2^-24 absolute in the exponent),
    expf is good to a few ulp, nine additions and one division follow, so each weight is off by at most ~3e-6 relative and the
    weights sum to 1; the bound leaves ~3 x over that."""
    from splat_slam_amd import depth_video as dv
    h, w = shape
    rng = np.random.default_rng(20)
    n, inds = 6, [4, 1, 7, 3]                                                    # 7 is out of range: a no-op
    disps = f32(rng.uniform(0.1, 3.0, (n, h, w)))
    mask = torch.tensor(rng.uniform(-8, 8, (len(inds), 576, h, w)), dtype=torch.float32, device=DEV).to(dtype).contiguous()
    out = f32(rng.uniform(5, 6, (n, 8 * h, 8 * w)))
    before = out.clone()
    res = dv.cvx_upsample(disps, li(inds), mask, out=out)
    torch.cuda.synchronize()
    assert res is out
    d_np, m_np = disps.cpu().numpy().astype(float), mask.float().cpu().numpy().astype(float)     # the rounded inputs the GPU sees
    worst = 0.0
    for b, f in enumerate(inds):
        if f >= n:
            continue
        ref = V.cvx_upsample(d_np[f], m_np[b])
        err = np.abs(out[f].cpu().numpy() - ref) / V.neighbourhood_max(d_np[f])
        worst = max(worst, err.max())
    print("cvx_upsample", shape, dtype, "worst error / max|d| of the neighbourhood:", worst)
    assert worst <= 1e-5
    for f in set(range(n)) - set(inds):                                          # frames not named keep their bits
        assert torch.equal(out[f], before[f])
    again = dv.cvx_upsample(disps, li(inds), mask, out=before.clone())
    assert torch.equal(again, out)                                               # two runs, the same bits
    fresh = dv.cvx_upsample(disps, li([1]), mask[1:2].contiguous())              # out=None: zeros elsewhere
    assert torch.equal(fresh[1], out[1]) and not fresh[0].any() and fresh.shape == out.shape


def test_upsampling_with_equal_logits_is_the_zero_padded_mean():
    from splat_slam_amd import depth_video as dv
    rng = np.random.default_rng(21)
    d = rng.uniform(0.5, 2.0, (1, 48, 64))
    out = dv.cvx_upsample(f32(d), li([0]), torch.full((1, 576, 48, 64), 0.25, device=DEV, dtype=torch.float16)).cpu().numpy()[0]
    ref = V.cvx_upsample(r32(d[0]), np.zeros((576, 48, 64)))
    assert np.abs(out - ref).max() <= 1e-5 * 2.0
    assert abs(out[0, 0] - r32(d[0])[:2, :2].sum() / 9) <= 2e-5


# ---- threshold
def ulp_diff(a, b):
    a, b = (np.asarray(x, np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    return np.abs(a - b)


@pytest.mark.parametrize("shape", [(48, 64), (480, 640), (7, 9)])
def test_depth_thresh_is_within_two_ulp(shape):
    from splat_slam_amd import depth_video as dv
    rng = np.random.default_rng(22)
    disps = rng.uniform(0.05, 2.0, (5, ) + shape).astype(np.float32)
    inds = [3, 0, 4]
    got = dv.depth_thresh(f32(disps), li(inds), 0.01).cpu().numpy()
    ref = V.depth_thresh(disps, inds, 0.01).astype(np.float32)
    print("depth_thresh", shape, got, ref, ulp_diff(got, ref))
    assert (ulp_diff(got, ref) <= 2).all()
    again = dv.depth_thresh(f32(disps), li(inds), 0.01).cpu().numpy()
    assert np.array_equal(got, again)


# ---- the lower-median mask
def run_mask(disps, inds, counts, visible=2, dtype=torch.bool):
    from splat_slam_amd import depth_video as dv
    out = torch.zeros(disps.shape, dtype=dtype, device=DEV)
    if dtype == torch.bool:
        out[:] = True                                                            # stale content: rows of inds are overwritten
    dv.mask_from_counts(f32(disps), li(inds), f32(counts), visible, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_mask(disps, inds, counts, visible=2):
    got = run_mask(disps, inds, counts, visible)
    ref, med = V.mask_from_counts(disps, inds, counts, visible)
    n = len(disps)
    for b, f in enumerate(inds):
        if 0 <= f < n:
            assert np.array_equal(got[f], ref[b]), (b, f, med[b], (got[f] != ref[b]).sum())
    for f in set(range(n)) - set(inds):
        assert got[f].all()                                                      # untouched
    return ref, med


def test_mask_from_counts_small_cases_bit_exact():
    rng = np.random.default_rng(23)
    h, w = 48, 64
    disps = rng.uniform(0.2, 1.0, (8, h, w)).astype(np.float32)
    disps[:, :4, :8] = 0.02                                                      # far pixels: beyond 3 x the median
    counts = rng.integers(0, 7, (7, h, w)).astype(np.float32)
    inds = [0, 1, 2, 3, 4, 5, 9]                                                 # 9 is out of range: a no-op
    counts[0] = 0                                                                # m = 0
    counts[1] = 6                                                                # every pixel a candidate (even m)
    counts[2] = 6
    counts[2, 0, 0] = 1                                                          # odd m
    disps[3] = np.float32(0.5)                                                   # ties at the median ...
    disps[3, :10] = rng.uniform(0.05, 2.0, (10, w))
    disps[4, 5, :] = 0.0                                                         # depth inf
    disps[4, 6, :5] = np.nan                                                     # NaN: no candidate
    disps[4, 7, :5] = -0.3                                                       # negative depths order first
    disps[5] = np.float32(0.25)                                                  # one value everywhere: the median is that value
    ref, med = check_mask(disps, inds, counts)
    assert np.isnan(med[0]) and not ref[0].any() and ref[1].any() and not ref[1].all()
    assert med[3] == np.float32(2.0) and ref[5].sum() == (counts[5] >= 2).sum()
    got8 = run_mask(disps, inds[:6], counts[:6], dtype=torch.uint8)
    assert np.array_equal(got8[:6] != 0, ref[:6]) and set(np.unique(got8)) <= {0, 1}
    a, b = run_mask(disps, inds, counts), run_mask(disps, inds, counts)
    assert np.array_equal(a, b)
    check_mask(disps, [6, 2], counts[:2], visible=4)


def test_mask_from_counts_one_full_size_frame():
    rng = np.random.default_rng(24)
    disps = rng.uniform(0.1, 1.0, (2, 480, 640)).astype(np.float32)
    disps[1, 100:140, 200:300] = 0.01
    counts = rng.integers(0, 7, (1, 480, 640)).astype(np.float32)
    ref, med = check_mask(disps, [1], counts)
    assert 0.3 < ref.mean() < 0.9 and np.isfinite(med[0])


def test_mask_from_counts_three_hundred_small_frames():
    rng = np.random.default_rng(25)
    disps = rng.uniform(0.1, 1.0, (300, 60, 80)).astype(np.float32)
    disps *= rng.uniform(0.5, 2.0, (300, 1, 1)).astype(np.float32)
    counts = rng.integers(0, 5, (300, 60, 80)).astype(np.float32)
    inds = list(rng.permutation(300))
    ref, med = check_mask(disps, inds, counts)
    assert len(np.unique(med)) > 250


# ---- the chain
@pytest.mark.parametrize("shape", list(V.SHAPES))
def test_chain_matches_the_ref_on_safe_pixels_and_its_stages_bit_for_bit(shape):
    import droid_backends
    from splat_slam_amd import depth_video as dv
    poses, disps, intr = V.chain_scene(shape)
    n = len(disps)
    inds = list(range(n))
    ref, lo, hi, safe = V.valid_depth_mask(poses, disps, intr, inds, V.REL, V.VISIBLE)
    assert all(s.mean() >= 0.9 for s in safe)
    P, D, K, I = f32(poses), f32(disps), f32(intr), li(inds)
    out = torch.zeros(D.shape, dtype=torch.bool, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                      # no host synchronisation
    try:
        dv.valid_depth_mask(P, D, K, I, V.REL, V.VISIBLE, out)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = (got != ref) & safe
    print("chain", shape, "safe share", safe.mean(), "mask share", got.mean(), "differences on unsafe pixels", (got != ref).sum())
    assert not bad.any(), bad.sum()
    thresh = dv.depth_thresh(D, I, V.REL)
    counts = droid_backends.depth_filter(P, D, K, I, thresh)
    staged = dv.mask_from_counts(D, I, counts, V.VISIBLE, torch.zeros_like(out))
    assert torch.equal(staged, out)
    sub = li([7, 2])                                                             # a subset, in another order: only its rows change
    out2 = torch.zeros_like(out)
    dv.valid_depth_mask(P, D, K, sub, V.REL, V.VISIBLE, out2)
    assert torch.equal(out2[7], out[7]) and torch.equal(out2[2], out[2]) and not out2[[0, 1, 3, 4, 5, 6, 8, 9]].any()


# ---- DepthVideo
def make_video(ht=48 * 8, wd=64 * 8, n=10, buffer=12, coarse=(48, 64), **kw):
    from splat_slam_amd.depth_video import DepthVideo
    poses, disps, intr = V.chain_scene(coarse, n=n)
    v = DepthVideo(ht, wd, buffer=buffer, device=DEV, **kw)
    rng = np.random.default_rng(30)
    for f in range(n):
        v.append(float(f), torch.zeros(3, ht, wd, dtype=torch.uint8, device=DEV), f32(poses[f]), f32(disps[f]), None, f32(intr))
    v.mono_disps[:n] = f32(1.7 * disps + 0.05 + rng.normal(0, 0.01, disps.shape))
    return v, rng


def test_video_upsample_and_masks_agree_with_the_functions():
    from splat_slam_amd import depth_video as dv
    v, rng = make_video(filter_thresh=V.REL, filter_visible_num=V.VISIBLE)
    assert v.counter.value == 10
    ix = li([0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
    mask = torch.tensor(rng.uniform(-4, 4, (1, 10, 576, 48, 64)), dtype=torch.float16, device=DEV)      # views to [10,576,h,w]
    v.upsample(ix, mask)
    want = dv.cvx_upsample(v.disps, ix, mask.view(10, 576, 48, 64))
    assert torch.equal(v.disps_up, want) and not v.disps_up[10:].any() and (v.disps_up[:10] > 0).all()
    v.set_dirty(2, 6)
    v.update_valid_depth_mask()
    dirty = li([2, 3, 4, 5])
    want = dv.valid_depth_mask(v.poses, v.disps_up, v.intrinsics[0] * 8, dirty, V.REL, V.VISIBLE, torch.zeros_like(v.valid_depth_mask))
    assert torch.equal(v.valid_depth_mask, want) and v.valid_depth_mask[2:6].any() and not v.valid_depth_mask[:2].any()
    assert not v.dirty.any() and v.npc_dirty[2:6].all()                        # dirty cleared, the point-cloud flag is the mapper's
    before = v.valid_depth_mask.clone()
    v.update_valid_depth_mask()                                                  # nothing dirty: nothing changes
    assert torch.equal(v.valid_depth_mask, before)
    v.update_valid_depth_mask(up=False)
    want = dv.valid_depth_mask(v.poses, v.disps, v.intrinsics[0].clone(), li(range(10)), V.REL, V.VISIBLE,
                               torch.zeros_like(v.valid_depth_mask_small))
    assert torch.equal(v.valid_depth_mask_small, want) and v.valid_depth_mask_small[:10].any()
    ref, lo, hi, safe = V.valid_depth_mask(v.poses.cpu().numpy()[:10], v.disps.cpu().numpy()[:10], v.intrinsics[0].cpu().numpy(),
                                           list(range(10)), V.REL, V.VISIBLE)
    # (frames beyond the counter are identity poses with disparity 1: the ref sees only the ten, so compare frames whose six
    # neighbours all lie inside them)
    got = v.valid_depth_mask_small.cpu().numpy()
    for f in range(3, 5):
        assert not ((got[f] != ref[f]) & safe[f]).any()


def graph(n, radius=2):
    ii, jj = [], []
    for i in range(n):
        for j in range(max(0, i - radius), min(n, i + radius + 1)):
            if i != j:
                ii.append(i)
                jj.append(j)
    return ii, jj


def ba_inputs(v, n, rng, t0=1):
    import dspo_ref as D
    ii, jj = graph(n)
    h, w = v.ht // 8, v.wd // 8
    poses, disps, intr = v.poses.cpu().numpy().astype(float), v.disps.cpu().numpy().astype(float), v.intrinsics[0].cpu().numpy().astype(float)
    tgt = np.stack([D.project(poses[i], poses[j], disps[i], intr, False).reshape(h, w, 2) for i, j in zip(ii, jj)])
    tgt += rng.normal(0, 0.3, tgt.shape)
    wgt = rng.uniform(0.2, 1.0, tgt.shape)
    K = len(set(ii) | set(range(t0, n)))
    return f32(tgt[None]), f32(wgt[None]), f32(rng.uniform(1e-3, 1e-2, (K, h, w))), li(ii), li(jj)


def test_video_ba_dba_equals_droid_backends_plus_clamp():
    import droid_backends
    v, rng = make_video(BA_type="DBA")
    tgt, wgt, eta, ii, jj = ba_inputs(v, 10, rng)
    poses, disps = v.poses.clone(), v.disps.clone()
    v.ba(tgt, wgt, eta, ii, jj, t0=1, t1=None, iters=2)
    t = tgt.view(-1, 48, 64, 2).permute(0, 3, 1, 2).contiguous()
    wt = wgt.view(-1, 48, 64, 2).permute(0, 3, 1, 2).contiguous()
    droid_backends.ba(poses, disps, v.intrinsics[0], v.zeros, t, wt, eta, ii, jj, 1, 10, 2, 1e-4, 0.1, False, False)
    disps.clamp_(min=1e-5)
    assert torch.equal(v.poses, poses) and torch.equal(v.disps, disps)
    assert not torch.equal(poses[1:10], make_video()[0].poses[1:10])              # it moved


def test_video_ba_dspo_stage_two_and_its_fall_back():
    from splat_slam_amd import dspo
    v, rng = make_video(filter_thresh=V.REL, filter_visible_num=V.VISIBLE)
    tgt, wgt, eta, ii, jj = ba_inputs(v, 10, rng, t0=10)                         # stage 2: eta has one row per distinct ii
    twin, _ = make_video(filter_thresh=V.REL, filter_visible_num=V.VISIBLE)
    v.ba(tgt, wgt, eta, ii, jj, t0=1, t1=None, iters=2, opt_type="depth_scale")
    twin.update_valid_depth_mask(up=False)
    assert torch.equal(twin.valid_depth_mask_small, v.valid_depth_mask_small) and v.valid_depth_mask_small[:10].float().mean() > 0.5
    kept = dspo.depth_scale_step(twin.poses, twin.disps, twin.intrinsics[0].clone(), twin.mono_disps, twin.valid_depth_mask_small,
                                 twin.depth_scale, twin.depth_shift, 10, tgt.view(-1, 48, 64, 2), wgt.view(-1, 48, 64, 2), eta, ii, jj,
                                 itrs=2, lm=1e-4, ep=0.1, mono_thres=0.1, alpha=0.01)
    assert bool(kept)
    for k in ("disps", "depth_scale", "depth_shift", "poses"):
        assert torch.equal(getattr(v, k), getattr(twin, k)), k
    assert (v.depth_scale[:10] - 1 / 1.7).abs().max() < 0.1 and not torch.equal(v.disps[:10], make_video()[0].disps[:10])

    # every frame's mono prior bad (opposite sign: the fitted scale is negative): stage 2 keeps no edge and ba falls back to stage 1
    import droid_backends
    v, rng = make_video(filter_thresh=V.REL, filter_visible_num=V.VISIBLE)
    v.mono_disps[:10] = -v.mono_disps[:10]
    tgt, wgt, eta, ii, jj = ba_inputs(v, 10, rng, t0=1)
    poses, disps = v.poses.clone(), v.disps.clone()
    assert not bool(v.dspo(tgt, wgt, eta, ii, jj, t0=1, t1=10, itrs=2, opt_type="depth_scale"))
    assert torch.equal(v.poses, poses) and torch.equal(v.disps, disps)           # stage 2 alone moved nothing
    v.ba(tgt, wgt, eta, ii, jj, t0=1, t1=10, iters=2, opt_type="depth_scale")
    t = tgt.view(-1, 48, 64, 2).permute(0, 3, 1, 2).contiguous()
    wt = wgt.view(-1, 48, 64, 2).permute(0, 3, 1, 2).contiguous()
    droid_backends.ba(poses, disps, v.intrinsics[0], v.zeros, t, wt, eta, ii, jj, 1, 10, 2, 1e-4, 0.1, False, False)
    assert torch.equal(v.poses, poses) and torch.equal(v.disps, disps.clamp(min=1e-5)) and not torch.equal(poses[1:10], make_video()[0].poses[1:10])


def test_video_distance_pose_and_depth_access():
    import lietorch
    v, rng = make_video()
    d = v.distance()                                                             # N x N, bidirectional
    assert d.shape == (10, 10) and torch.equal(d, d.T) and (d[0, 1:] > 0).all()
    ii, jj = [0, 3, 5], [1, 1, 9]
    e = v.distance(ii, jj, beta=0.3, bidirectional=True)
    assert torch.equal(e, torch.stack([d[0, 1], d[3, 1], d[5, 9]]))
    one = v.distance(ii, jj, bidirectional=False)
    back = v.distance(jj, ii, bidirectional=False)
    assert torch.equal(e, 0.5 * (one + back)) and not torch.equal(one, back)
    v.disps_up[:10] = f32(rng.uniform(0.2, 2.0, (10, v.ht, v.wd)))
    v.valid_depth_mask[3, 5:9] = True
    depth, mask, c2w = v.get_depth_and_pose(3, DEV)
    assert torch.equal(depth, 1.0 / v.disps_up[3]) and torch.equal(mask, v.valid_depth_mask[3]) and c2w.shape == (4, 4)
    assert torch.equal(c2w, lietorch.SE3(v.poses[3].clone()).inv().matrix())
    w2c = lietorch.SE3(v.poses[3].clone()).matrix()
    assert (c2w @ w2c - torch.eye(4, device=DEV)).abs().max() < 1e-5
    depth, mask, c2w = v.get_depth_and_pose(3, "cpu")
    assert not depth.is_cuda and not mask.is_cuda and not c2w.is_cuda
    s, q = v.get_depth_scale_and_shift(4, v.mono_disps[4:5], v.disps[4:5], torch.ones_like(v.disps[4:5]))
    assert abs(float(s) - 1 / 1.7) < 0.02 and v.depth_scale[4] == s and v.depth_shift[4] == q


def test_video_save_and_eval_depth_l1_round_trip(tmp_path):
    from splat_slam_amd.depth_video import DepthVideo
    v = DepthVideo(64, 96, buffer=6, device=DEV)
    rng = np.random.default_rng(31)
    gt = rng.uniform(1.0, 6.0, (4, 64, 96))
    for f in range(4):
        v.append(float(f), torch.zeros(3, 64, 96, dtype=torch.uint8, device=DEV), None, None, None, None)
    v.disps_up[:4] = f32(1.0 / ((gt - 0.3) / 2.0))                               # depth = (gt - 0.3) / 2: a scale and a shift away
    v.valid_depth_mask[:4] = torch.tensor(rng.uniform(size=gt.shape) < 0.7, device=DEV)
    path = str(tmp_path / "video.npz")
    v.save_video(path)
    z = dict(np.load(path))
    assert sorted(z) == ["depths", "poses", "timestamps", "valid_depth_masks"] and z["timestamps"].tolist() == [0, 1, 2, 3]
    np.testing.assert_allclose(z["depths"], (gt - 0.3) / 2.0, rtol=1e-5)
    np.testing.assert_allclose(z["poses"], np.tile(np.eye(4), (4, 1, 1)), atol=1e-7)
    stream = [(None, None, torch.tensor(gt[f], dtype=torch.float32)) for f in range(4)]
    l1, l1_4m, share = v.eval_depth_l1(path, stream)
    print("eval_depth_l1 aligned", l1, l1_4m, share)
    assert l1 < 1e-4 and l1_4m < 1e-4 and abs(share - 0.7) < 0.02
    l1g, l1g_4m, _ = v.eval_depth_l1(path, stream, global_scale=2.0)
    assert abs(l1g - 0.3) < 1e-4 and abs(l1g_4m - 0.3) < 1e-4                    # 2 * depth = gt - 0.3


def test_video_full_size_update():
    """480 x 640, 25 frames, a 25-frame window of edges: one ba with both stages, the upsampling and the full-resolution mask"""
    ht, wd, n = 480, 640, 25
    from splat_slam_amd.depth_video import DepthVideo
    rng = np.random.default_rng(32)
    v = DepthVideo(ht, wd, buffer=32, device=DEV, filter_thresh=V.REL, filter_visible_num=V.VISIBLE)
    intr = np.array([75.0, 75.0, 39.5, 29.5])
    disps = rng.uniform(0.45, 0.55, (n, 60, 80))
    for f in range(n):
        t, q = R.exp_se3(np.concatenate([[0.03 * f, 0.01 * np.sin(f), 0.02 * f], rng.normal(0, 0.01, 3)]))
        v.append(float(f), torch.zeros(3, ht, wd, dtype=torch.uint8, device=DEV), f32(np.concatenate([t, q])), f32(disps[f]), None, f32(intr))
    v.mono_disps[:n] = f32(1.7 * disps + 0.05)
    tgt, wgt, eta, ii, jj = ba_inputs(v, n, rng, t0=1)
    d0, p0 = v.disps.clone(), v.poses.clone()
    v.ba(tgt, wgt, eta, ii, jj, t0=1, t1=None, iters=2, opt_type="pose_depth")
    assert not torch.equal(v.poses[1:n], p0[1:n]) and torch.equal(v.poses[0], p0[0]) and torch.isfinite(v.disps).all()
    d1 = v.disps.clone()
    v.ba(tgt, wgt, eta, ii, jj, t0=1, t1=None, iters=2, opt_type="depth_scale")
    assert torch.isfinite(v.disps).all() and (v.disps >= 1e-5).all() and not torch.equal(v.disps[:n], d1[:n])
    assert torch.isfinite(v.depth_scale).all() and v.valid_depth_mask_small[:n].float().mean() > 0.3
    v.set_dirty(0, n)
    mask = (torch.rand(n, 576, 60, 80, device=DEV, generator=torch.Generator(device=DEV).manual_seed(33)) * 8 - 4).half()
    v.upsample(torch.arange(n, device=DEV), mask)
    assert (v.disps_up[:n] > 0).all() and not v.disps_up[n:].any()
    top = torch.nn.functional.max_pool2d(v.disps[:n, None], 3, 1, 1)[:, 0]       # a convex combination of the neighbourhood and zeros
    assert (v.disps_up[:n] <= top.repeat_interleave(8, 1).repeat_interleave(8, 2) * (1 + 1e-5)).all()
    v.update_valid_depth_mask(up=True)
    assert not v.dirty.any() and v.valid_depth_mask[:n].any() and not v.valid_depth_mask[n:].any()
    depth, m, c2w = v.get_depth_and_pose(n - 1, DEV)
    assert depth.shape == (ht, wd) and m.dtype == torch.bool and torch.isfinite(c2w).all()
