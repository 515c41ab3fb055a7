"""splat_slam_amd.factor_graph and splat_slam_amd.corr on the MI355X against tests/factor_graph_ref.py and tests/corr_ref.py: the
reprojection to its derived bound, the motion features bit for bit from the kernel's own coords, both selections to the exact list
of the sequential rule, the correlation blocks level by level, and the FactorGraph class against the bookkeeping restatement and,
bit for bit, against its own stages called by hand on a second video."""
import numpy as np
import pytest
import torch

import corr_ref as C
import factor_graph_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def li(a):
    return torch.tensor(np.asarray(a), dtype=torch.int64, device=DEV).reshape(-1)


def np_(t):
    return t.detach().cpu().numpy()


# ---- reprojection
@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("h,w", [(6, 8), (11, 13)])
def test_reprojection_is_within_its_bound_and_motion_features_are_exact(h, w, E):
    from splat_slam_amd import factor_graph as fg
    poses, disps, intr, ii, jj, target = R.reproject_case(h, w, E)
    ref = R.reproject(poses, disps, intr, ii, jj)
    args = (f32(poses), f32(disps), f32(intr), li(ii), li(jj))
    out = fg.reproject(*args)
    assert len(out) == 2                                                        # no target: no motion features
    coords, valid, motn = fg.reproject(*args, f32(target))
    assert torch.equal(out[0], coords) and torch.equal(out[1], valid)
    assert tuple(coords.shape) == (E, h, w, 2) and tuple(valid.shape) == (E, h, w, 1) and tuple(motn.shape) == (E, 4, h, w)
    again = fg.reproject(*args, f32(target))
    assert all(torch.equal(a, b) for a, b in zip(again, (coords, valid, motn)))
    # coords away from the Z branch, valid away from its threshold; the scene keeps both exclusions under 1 % (checked without a GPU too)
    assert ref["near_branch"].mean() <= 0.01 and ref["near_valid"].mean() <= 0.01
    err = np.abs(np_(coords).astype(np.float64) - ref["coords"])
    ratio = np.where(ref["bound"] > 0, err / np.where(ref["bound"] > 0, ref["bound"], 1.0), np.where(err > 0, np.inf, 0.0))
    ratio[ref["near_branch"]] = 0.0
    print(f"reproject {h}x{w} E={E}: worst error / bound = {ratio.max():.3f}, largest error {err.max():.3e}")
    assert ratio.max() <= 1.0
    bad = (np_(valid)[..., 0] != ref["valid"][..., 0]) & ~ref["near_valid"]
    assert not bad.any()
    if E == 5:
        assert np_(valid)[:3].all() and not np_(valid)[3].any()                 # (1,4) lies behind the camera: Z = 1 there
        assert torch.equal(coords[0], coords[2]) and torch.equal(motn[0, :2], motn[2, :2])      # the repeated edge
        assert not coords[4].any() and not valid[4].any() and not motn[4].any()                # the out-of-range edge
    grid = torch.stack(torch.meshgrid(torch.arange(w, device=DEV).float(), torch.arange(h, device=DEV).float(), indexing="xy"), -1)
    want = torch.cat([coords - grid, f32(target) - coords], -1).permute(0, 3, 1, 2).clamp(-64.0, 64.0)
    live = [e for e in range(E) if 0 <= ii[e] < 5 and 0 <= jj[e] < 5]
    assert torch.equal(motn[live], want[live]) and (motn.abs() == 64).any() and (motn.abs() < 64).any()


def test_reproject_on_a_videos_buffers_uses_each_frames_intrinsics():
    from splat_slam_amd import factor_graph as fg
    v = make_video()
    v.intrinsics[3] = v.intrinsics[3] * 1.25
    coords, valid = fg.reproject(v.poses, v.disps, v.intrinsics, li([1, 3, 2]), li([3, 1, 2]))
    assert tuple(coords.shape) == (3, 6, 8, 2) and tuple(valid.shape) == (3, 6, 8, 1)
    ref = R.reproject(np_(v.poses), np_(v.disps), np_(v.intrinsics), [1, 3, 2], [3, 1, 2])
    assert (np.abs(np_(coords) - ref["coords"]) <= ref["bound"]).all()


# ---- selection
def run_proximity(d, t0, t1, t, old, rad, nms, thresh, mf):
    from splat_slam_amd import factor_graph as fg
    dd, io, jo = f32(d), li(old[:, 0]), li(old[:, 1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                     # the device part: no host synchronisation
    try:
        es, counts = fg.proximity_edges_on_device(dd, t0, t1, t, io, jo, rad, nms, thresh, mf)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    num = counts.tolist()[0]
    assert num <= es.shape[0]
    got = [tuple(p) for p in es[:num].tolist()]
    ii, jj = fg.select_proximity_edges(dd, t0, t1, t, io, jo, rad, nms, thresh, mf)
    assert list(zip(ii.tolist(), jj.tolist())) == got and ii.dtype == torch.int64
    return got


def matrix(rng, n, levels=None):
    d = rng.uniform(0.0, 30.0, size=n).astype(np.float32)
    if levels:
        d = (np.floor(d / 30.0 * levels) * (30.0 / levels)).astype(np.float32)
    return d


NO_OLD = np.zeros((0, 2), np.int64)


def test_proximity_selection_equals_the_sequential_rule():
    rng = np.random.default_rng(11)
    old40 = np.concatenate([rng.integers(0, 40, size=(30, 2)), np.array([[-3, 5], [41, 2], [7, 45], [10 ** 12, 3], [39, 0], [0, 39]])])
    cases = [("1 x 1", matrix(rng, 1), 0, 0, 1, NO_OLD, 2, 2, 16.0, 10),
             ("5 x 7", matrix(rng, 35), 2, 0, 7, NO_OLD, 2, 2, 16.0, 30),
             ("7 x 5", matrix(rng, 35), 0, 2, 7, NO_OLD, 1, 1, 29.0, 30),
             ("40 x 40 with old edges", matrix(rng, 1600), 0, 0, 40, old40, 2, 2, 16.0, 400),
             ("8 levels", matrix(rng, 1600, 8), 0, 0, 40, old40[:10], 2, 2, 16.0, 400),
             ("2 levels, nms 0", matrix(rng, 990, 2), 3, 0, 33, NO_OLD, 1, 0, 16.0, 2000),
             ("all inf", np.full(400, np.inf, np.float32), 0, 0, 20, NO_OLD, 2, 2, 16.0, 100),
             ("stops midway", matrix(rng, 1600), 0, 0, 40, NO_OLD, 2, 1, 25.0, 251),
             ("max_factors -1", matrix(rng, 400), 0, 0, 20, NO_OLD, 2, 2, 16.0, -1),
             ("thresh below every entry", matrix(rng, 400) + 1.0, 0, 0, 20, NO_OLD, 2, 2, 0.5, 100),
             ("rad 0, wide nms", matrix(rng, 625), 0, 0, 25, NO_OLD, 0, 5, 29.0, 75)]
    nan = matrix(rng, 1600)
    nan[rng.integers(0, 1600, size=200)] = np.nan
    nan[rng.integers(0, 1600, size=200)] = np.inf
    nan[rng.integers(0, 1600, size=50)] = -0.0
    cases.append(("NaN, inf and -0", nan, 0, 0, 40, old40[:5], 2, 2, 16.0, 400))
    for name, d, t0, t1, t, old, rad, nms, thresh, mf in cases:
        want = R.proximity_edges(d, t0, t1, t, old[:, 0], old[:, 1], rad, nms, thresh, mf)
        got = run_proximity(d, t0, t1, t, old, rad, nms, thresh, mf)
        assert got == want, (name, len(got), len(want))
    picked = [len(R.proximity_edges(c[1], *c[2:5], c[5][:, 0], c[5][:, 1], *c[6:])) for c in cases]
    assert picked[0] == 0 and picked[2] > 22 and picked[3] > 300 and picked[7] == 252


def test_proximity_selection_at_512_x_512():
    rng = np.random.default_rng(12)
    d = matrix(rng, 512 * 512, 4096)                                            # 64 entries per level: ties in every batch
    old = rng.integers(0, 512, size=(200, 2))
    want = R.proximity_edges(d, 0, 0, 512, old[:, 0], old[:, 1], 2, 2, 16.0, 6000)
    assert run_proximity(d, 0, 0, 512, old, 2, 2, 16.0, 6000) == want and len(want) == 6002


def run_backend(d, t_start, t_end, tsl, loop, nms, radius, thresh, mf):
    from splat_slam_amd import factor_graph as fg
    dd = f32(d)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        es, counts = fg.backend_edges_on_device(dd, t_start, t_end, tsl, loop, nms, radius, thresh, mf)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    num, num_loop = counts.tolist()
    assert num <= es.shape[0]
    ii, jj, nl = fg.select_backend_edges(dd, t_start, t_end, tsl, loop, nms, radius, thresh, mf)
    got = [tuple(p) for p in es[:num].tolist()]
    assert list(zip(ii.tolist(), jj.tolist())) == got and nl == num_loop
    return got, num_loop


@pytest.mark.parametrize("loop", [False, True])
def test_backend_selection_equals_the_sequential_rule(loop):
    rng = np.random.default_rng(13)
    cases = [("1 x 1", 0, 1, 0, 1, 1, 10.0, 10, None), ("60 frames", 0, 60, 35, 2, 1, 12.0, 300, None),
             ("offset window", 3, 70, 40, 1, 2, 20.0, 1000, None), ("8 levels", 0, 64, 30, 2, 1, 15.0, 500, 8),
             ("nms 0", 0, 50, 28, 0, 1, 29.0, 100000, 4), ("stops midway", 0, 60, 30, 1, 1, 25.0, 150, None),
             ("thresh below every entry", 0, 40, 25, 2, 1, -1.0, 100, None), ("128 frames", 0, 128, 64, 3, 2, 10.0, 5000, 64)]
    loops = []
    for name, t_start, t_end, tsl, nms, radius, thresh, mf, levels in cases:
        rows = t_end - (tsl if loop else t_start)
        d = matrix(rng, rows * (t_end - t_start), levels)
        d[rng.integers(0, d.size, size=d.size // 20)] = np.nan
        want = R.backend_edges(d, t_start, t_end, tsl, loop, nms, radius, thresh, mf)
        got = run_backend(d, t_start, t_end, tsl, loop, nms, radius, thresh, mf)
        assert got[0] == want[0] and got[1] == want[1], (name, len(got[0]), len(want[0]), got[1], want[1])
        loops.append(want[1])
    assert (max(loops) > 50) == loop and loops[0] == 0 and loops[6] == 0


def test_backend_selection_at_512_columns_with_loops():
    rng = np.random.default_rng(14)
    d = matrix(rng, 212 * 512, 1024)
    want = R.backend_edges(d, 0, 512, 300, True, 2, 1, 6.0, 4000)
    got = run_backend(d, 0, 512, 300, True, 2, 1, 6.0, 4000)
    assert got[0] == want[0] and got[1] == want[1] and want[1] > 1000


def test_selection_refuses_513_rows():
    from splat_slam_amd import factor_graph as fg
    e = li([])
    with pytest.raises(ValueError, match="exceeds the supported 512 x 512"):
        fg.select_proximity_edges(torch.zeros(513 * 3, device=DEV), 0, 510, 513, e, e, 2, 2, 16.0, 10)
    with pytest.raises(ValueError, match="exceeds the supported 512 x 512"):
        fg.select_backend_edges(torch.zeros(513 * 513, device=DEV), 0, 513, None, False, 2, 1, 16.0, 10)


# ---- correlation blocks
def eighths(rng, shape):
    """values that are multiples of 1/8 in [-2, 2]: the products of the maps / 4, their sums over 8 channels and every 2 x 2 average are
    exact in fp32, so the device pyramid equals the fp64 one and only the lookup rounds"""
    return (rng.integers(-16, 17, size=shape) / 8.0).astype(np.float32)


def pool(a):
    """2 x 2 average over the last two axes, odd remainders dropped"""
    h, w = a.shape[-2] // 2 * 2, a.shape[-1] // 2 * 2
    a = a[..., :h, :w]
    return 0.25 * (a[..., 0::2, 0::2] + a[..., 0::2, 1::2] + a[..., 1::2, 0::2] + a[..., 1::2, 1::2])


def check_levels(name, got, refs, units):
    """got [1,E,levels*rd*rd,h,w] against one (value, magnitude) per level, (units + level) * 2^-24 * magnitude"""
    got = np_(got).astype(np.float64)
    n = refs[0][0].shape[1]
    for lvl, (val, mag) in enumerate(refs):
        err = np.abs(got[0][:, lvl * n:(lvl + 1) * n] - val)
        lim = C.bound(val, mag, units + lvl)
        assert (err <= lim).all(), (name, lvl, float(err.max()))


@pytest.mark.parametrize("radius", [1, 3])
def test_corr_block_matches_the_lookup_on_a_numpy_pyramid(radius):
    """Bound per element: what tests/test_gpu_corr.py allows the lookup, 8 * 2^-24 * magnitude (four-corner sample), plus one fp32
    rounding, 2^-24 * magnitude, per pooled level: (8 + level) * 2^-24 * magnitude.  The maps hold multiples of 1/8, for which the
    all-pairs product and the averages are exact, so the device pyramid is the numpy one and the bound is the lookup's own."""
    from splat_slam_amd.corr import CorrBlock
    rng = np.random.default_rng(20 + radius)
    E, ch, h, w, levels = 2, 8, 6, 8, 3
    f1, f2 = eighths(rng, (1, E, ch, h, w)), eighths(rng, (1, E, ch, h, w))
    coords = (np.stack(np.meshgrid(np.arange(w), np.arange(h), indexing="xy"), -1)[None, None] + rng.normal(0, 2.0, (1, E, h, w, 2)))
    coords = coords.astype(np.float32)
    block = CorrBlock(f32(f1), f32(f2), num_levels=levels, radius=radius)
    out = block(f32(coords))
    rd = 2 * radius + 1
    assert tuple(out.shape) == (1, E, levels * rd * rd, h, w) and out.dtype == torch.float32
    vol = np.einsum("ecp,ecq->epq", f1[0].reshape(E, ch, h * w).astype(np.float64) / 4, f2[0].reshape(E, ch, h * w).astype(np.float64) / 4)
    vol = vol.reshape(E, h, w, h, w)
    c2 = coords[0].transpose(0, 3, 1, 2)
    refs = []
    for lvl in range(levels):
        assert np.array_equal(np_(block.corr_pyramid[lvl]).astype(np.float64), vol)
        val, mag, _ = C.corr_index_forward(vol, c2 / np.float32(2 ** lvl), radius)
        refs.append((val.reshape(E, rd * rd, h, w), mag.reshape(E, rd * rd, h, w)))
        vol = pool(vol)
    check_levels(f"CorrBlock r={radius}", out, refs, 8)
    four = CorrBlock(f32(f1), f32(f2), num_levels=4, radius=radius)(f32(coords))               # 6 x 8 has no fourth level: zeros
    assert torch.equal(four[:, :, :levels * rd * rd], out) and not four[:, :, levels * rd * rd:].any()
    # cat and __getitem__ against blocks built from the concatenated / indexed maps
    g1, g2 = eighths(rng, (1, 1, ch, h, w)), eighths(rng, (1, 1, ch, h, w))
    both = block.cat(CorrBlock(f32(g1), f32(g2), num_levels=levels, radius=radius))
    assert both is block
    whole = CorrBlock(f32(np.concatenate([f1, g1], 1)), f32(np.concatenate([f2, g2], 1)), num_levels=levels, radius=radius)
    c3 = f32(np.concatenate([coords, coords[:, :1]], 1))
    assert all(torch.equal(a, b) for a, b in zip(both.corr_pyramid, whole.corr_pyramid)) and torch.equal(both(c3), whole(c3))
    keep = torch.tensor([True, False, True], device=DEV)
    part = both[keep]
    sub = CorrBlock(f32(np.concatenate([f1[:, :1], g1], 1)), f32(np.concatenate([f2[:, :1], g2], 1)), num_levels=levels, radius=radius)
    assert part is block and torch.equal(part(c3[:, keep]), sub(c3[:, keep]))


@pytest.mark.parametrize("radius", [1, 3])
def test_alt_corr_block_matches_the_lookup_on_a_numpy_pyramid(radius):
    """Bound per element: what tests/test_gpu_corr.py allows altcorr_forward, (channels + 8) * 2^-24 * magnitude, plus one fp32
    rounding per pooled level: (channels + 8 + level) * 2^-24 * magnitude; the maps hold multiples of 1/8 (exact averages)."""
    from splat_slam_amd.corr import AltCorrBlock
    rng = np.random.default_rng(30 + radius)
    N, ch, h, w, levels = 4, 8, 6, 8, 3
    maps = eighths(rng, (1, N, ch, h, w))
    ii, jj = [0, 3], [2, 3]
    coords = (np.stack(np.meshgrid(np.arange(w), np.arange(h), indexing="xy"), -1)[None, None] + rng.normal(0, 2.0, (1, 2, h, w, 2)))
    coords = coords.astype(np.float32)
    block = AltCorrBlock(f32(maps), num_levels=levels, radius=radius)
    out = block(f32(coords), li(ii), li(jj))
    rd = 2 * radius + 1
    assert tuple(out.shape) == (1, 2, levels * rd * rd, h, w) and out.is_contiguous()
    full = maps[0].astype(np.float64) / 4
    lvl_maps, refs = full, []
    for lvl in range(levels):
        assert np.array_equal(np_(block.pyramid[lvl])[0].astype(np.float64), lvl_maps.transpose(0, 2, 3, 1))
        val, mag, _ = C.altcorr_forward(full[ii].transpose(0, 2, 3, 1), lvl_maps[jj].transpose(0, 2, 3, 1),
                                        (coords[0] / np.float32(2 ** lvl))[:, None], radius)
        refs.append((val[:, 0], mag[:, 0]))
        lvl_maps = pool(lvl_maps)
    check_levels(f"AltCorrBlock r={radius}", out, refs, ch + 8)
    four = AltCorrBlock(f32(maps), num_levels=4, radius=radius)(f32(coords), li(ii), li(jj))
    assert torch.equal(four[:, :, :levels * rd * rd], out) and not four[:, :, levels * rd * rd:].any()


# ---- FactorGraph
N_FRAMES, HT, WD = 12, 48, 64


def make_video(**kw):
    """twelve keyframes on a smooth path in front of a gently varying surface, DepthVideo(48, 64, buffer=16)"""
    from splat_slam_amd.depth_video import DepthVideo
    rng = np.random.default_rng(40)
    v = DepthVideo(HT, WD, buffer=16, device=DEV, **kw)
    h, w = HT // 8, WD // 8
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for f in range(N_FRAMES):
        ang = 0.01 * f
        pose = np.array([0.03 * f, 0.01 * np.sin(f), 0.015 * f, 0.0, np.sin(ang / 2), 0.0, np.cos(ang / 2)])
        disp = 0.5 + 0.05 * np.sin(0.7 * xx + 0.3 * f) * np.cos(0.5 * yy) + rng.uniform(-0.005, 0.005, (h, w))
        v.append(float(f), torch.zeros(3, HT, WD, dtype=torch.uint8, device=DEV), f32(pose), f32(disp), None, f32([7.0, 7.5, 4.0, 3.0]))
    v.mono_disps[:N_FRAMES] = 1.7 * v.disps[:N_FRAMES] + 0.05
    v.fmaps[:N_FRAMES] = torch.tensor(rng.integers(-8, 9, size=(N_FRAMES, 1, 128, h, w)) / 8.0, dtype=torch.half, device=DEV)
    v.nets[:N_FRAMES] = torch.tensor(rng.normal(size=(N_FRAMES, 128, h, w)), dtype=torch.half, device=DEV)
    v.inps[:N_FRAMES] = torch.tensor(rng.normal(size=(N_FRAMES, 128, h, w)), dtype=torch.half, device=DEV)
    return v


def stub(net, inp, corr, motn, ii, jj):
    """a deterministic stand-in for the update operator, with the shapes of the reference's (GraphAgg: one eta and one mask per
    distinct source frame)"""
    E, h, w = motn.shape[1], motn.shape[3], motn.shape[4]
    K = torch.unique(ii).shape[0]
    g = torch.Generator(device="cpu").manual_seed(1234 + E)
    delta = (0.1 * motn[:, :, :2]).permute(0, 1, 3, 4, 2).contiguous()
    weight = torch.full((1, E, h, w, 2), 0.5, device=motn.device)
    damping = (0.01 * torch.rand((1, K, h, w), generator=g)).to(motn.device)
    upmask = (4.0 * torch.rand((1, K, 576, h, w), generator=g) - 2.0).to(motn.device)
    return net, delta, weight, damping, upmask


def same_lists(g, b):
    assert g.ii.tolist() == b.ii and g.jj.tolist() == b.jj and g.age.tolist() == b.age
    assert g.ii_inac.tolist() == b.ii_inac and g.jj_inac.tolist() == b.jj_inac
    assert g.ii_bad.tolist() == b.ii_bad and g.jj_bad.tolist() == b.jj_bad
    E, I = len(b.ii), len(b.ii_inac)
    assert tuple(g.target.shape) == (1, E, 6, 8, 2) == tuple(g.weight.shape) and tuple(g.net.shape) == (1, E, 128, 6, 8) == tuple(g.inp.shape)
    assert g.corr.corr_pyramid[0].shape[0] == E and tuple(g.target_inac.shape) == (1, I, 6, 8, 2) == tuple(g.weight_inac.shape)
    assert g.target.dtype == torch.float32 and g.ii.dtype == torch.int64 and g.age.dtype == torch.int64


def test_graph_bookkeeping_equals_the_sequential_restatement():
    from splat_slam_amd.factor_graph import FactorGraph
    v = make_video()
    g, b = FactorGraph(v, stub, device=DEV, max_factors=30), R.Book(30)
    assert tuple(g.coords0.shape) == (6, 8, 2) and g.coords0[2, 5].tolist() == [5.0, 2.0] and tuple(g.damping.shape) == (16, 6, 8)
    g.add_neighborhood_factors(0, 6, r=2)
    b.add_neighborhood_factors(0, 6, r=2)
    same_lists(g, b)
    g.add_factors([0, 1, 5], [1, 0, 0])                                         # two duplicates and one new edge
    b.add_factors([0, 1, 5], [1, 0, 0])
    same_lists(g, b)
    g.update(t0=1)
    b.tick()
    same_lists(g, b)
    g.weight[:, -1] = 0.0                                                       # (5, 0): distant, and now weak
    conf = g.weight.mean(dim=[0, 2, 3, 4]).tolist()
    g.filter_edges()
    b.filter_edges(conf)
    assert b.ii_bad == [5] and b.jj_bad == [0]
    same_lists(g, b)
    # the frontend's edges over frames [2, 12) x [0, 12); the graph is over its limit afterwards, so old edges become inactive
    d = np_(g._distance_matrix(2, 0, 12, 0.25))
    es = R.proximity_edges(d, 2, 0, 12, b.ii + b.ii_bad + b.ii_inac, b.jj + b.jj_bad + b.jj_inac, 2, 2, 16.0, 30)
    g.add_proximity_factors(t0=2, t1=0, rad=2, nms=2, beta=0.25, thresh=16.0, remove=True)
    b.add_factors([e[0] for e in es], [e[1] for e in es], remove=True)
    assert len(b.ii_inac) > 0 and len(es) > 30
    same_lists(g, b)
    g.update(t0=1)
    b.tick()
    mask = [i == 4 or j == 9 for i, j in zip(b.ii, b.jj)]
    g.rm_factors(torch.tensor(mask, device=DEV), store=True)
    b.rm_factors(mask, store=True)
    same_lists(g, b)
    poses5 = v.poses[5].clone()
    g.rm_keyframe(4)
    b.rm_keyframe(4)
    assert torch.equal(v.poses[4], poses5)
    same_lists(g, b)
    g.add_factors(b.ii_inac[:2] + [1], b.jj_inac[:2] + [7])                     # inactive edges count as duplicates
    b.add_factors(b.ii_inac[:2] + [1], b.jj_inac[:2] + [7])
    same_lists(g, b)
    # the backend's two refusals: fewer than 3 pairs, and a loop request that finds no loop pair
    before = g.ii.tolist()
    assert g.add_backend_proximity_factors(0, 2, 2, 1, 16.0, 100, 0.25) == 0
    assert g.add_backend_proximity_factors(0, 11, 2, 1, 16.0, 100, 0.25, t_start_loop=5, loop=True) == 0 and g.ii.tolist() == before
    d = np_(g._distance_matrix(0, 0, 11, 0.25))
    es, _ = R.backend_edges(d, 0, 11, None, False, 2, 1, 16.0, 100)
    num = g.add_backend_proximity_factors(0, 11, 2, 1, 16.0, 100, 0.25)
    b.add_factors([e[0] for e in es], [e[1] for e in es], remove=True)
    assert num == len(b.ii) > 0
    same_lists(g, b)
    g.clear_edges()
    assert g.ii is None and g.target is None and g.corr is None


def by_hand_update(v, net, target, ii, jj, t0, itrs=2, extra=None):
    """the stages of FactorGraph.update on the video v: reproject, the stub, bundle adjustment, upsampling"""
    from splat_slam_amd import factor_graph as fg
    coords, _, motn = fg.reproject(v.poses, v.disps, v.intrinsics, ii, jj, target[0].contiguous())
    net, delta, weight, damping, upmask = stub(net, None, None, motn[None], ii, jj)
    target = coords[None] + delta.float()
    damp = 1e-6 * torch.ones_like(v.disps)
    damp[torch.unique(ii)] = damping
    bi, bj, bt, bw = ii, jj, target, weight
    if extra is not None:
        bi, bj = torch.cat([extra[0], ii]), torch.cat([extra[1], jj])
        bt, bw = torch.cat([extra[2], target], 1), torch.cat([extra[3], weight], 1)
    eta = .2 * damp[torch.unique(bi)].contiguous() + 1e-7
    v.ba(bt, bw, eta, bi, bj, t0, None, iters=itrs, lm=1e-4, ep=0.1, motion_only=False, opt_type="pose_depth")
    v.upsample(torch.unique(ii), upmask)
    return target, weight


def same_video(v, u):
    assert torch.equal(v.poses, u.poses) and torch.equal(v.disps, u.disps) and torch.equal(v.disps_up, u.disps_up)
    assert torch.isfinite(v.poses).all() and torch.isfinite(v.disps).all()


def test_graph_update_equals_its_stages_called_by_hand():
    from splat_slam_amd import factor_graph as fg
    from splat_slam_amd.factor_graph import FactorGraph
    v, u = make_video(), make_video()
    g = FactorGraph(v, stub, device=DEV, max_factors=-1)
    g.add_neighborhood_factors(0, 8, r=2)
    ii, jj, first = g.ii.clone(), g.jj.clone(), g.target.clone()
    assert torch.equal(first[0], fg.reproject(u.poses, u.disps, u.intrinsics, ii, jj)[0]) and not g.weight.any()   # a new edge's target is its reprojection
    g.update(t0=1, itrs=2)
    target, weight = by_hand_update(u, g.net, first, ii, jj, 1)
    assert torch.equal(g.target, target) and torch.equal(g.weight, weight) and g.age.tolist() == [1] * len(ii)
    same_video(v, u)
    assert not torch.equal(v.poses[1:8], make_video().poses[1:8]) and v.disps_up[:8].any() and not v.disps_up[8:].any()
    g.update(t0=None, itrs=2)                                                   # t0 = max(1, ii.min() + 1) = 1
    target, weight = by_hand_update(u, g.net, target, ii, jj, 1)
    assert torch.equal(g.target, target) and g.age.tolist() == [2] * len(ii)
    same_video(v, u)
    # inactive edges: those with both ends >= t0 - 3 go in front of the active ones
    mask = (g.ii <= 1) | (g.jj == 7)
    g.rm_factors(mask, store=True)
    inac = (g.ii_inac.clone(), g.jj_inac.clone(), g.target_inac.clone(), g.weight_inac.clone())
    assert torch.equal(inac[2], target[:, mask]) and inac[0].shape[0] > 4
    seen = {}
    real_ba = v.ba
    v.ba = lambda t, w, eta, bi, bj, *a, **k: (seen.update(ii=bi.tolist(), jj=bj.tolist()), real_ba(t, w, eta, bi, bj, *a, **k))[1]
    ii, jj, target = g.ii.clone(), g.jj.clone(), g.target.clone()
    g.update(t0=5, itrs=2, use_inactive=True)
    m = (inac[0] >= 2) & (inac[1] >= 2)
    assert 0 < int(m.sum()) < m.shape[0]
    assert seen["ii"] == inac[0][m].tolist() + ii.tolist() and seen["jj"] == inac[1][m].tolist() + jj.tolist()
    target, weight = by_hand_update(u, g.net, target, ii, jj, 5, extra=(inac[0][m], inac[1][m], inac[2][:, m], inac[3][:, m]))
    assert torch.equal(g.target, target) and g.age.tolist() == [3] * len(ii)
    same_video(v, u)


def test_graph_update_lowmem_equals_its_stages_called_by_hand():
    from splat_slam_amd import factor_graph as fg
    from splat_slam_amd.corr import AltCorrBlock
    v, u = make_video(), make_video()
    g = fg.FactorGraph(v, stub, device=DEV, corr_impl="alt", max_factors=-1)
    g.add_neighborhood_factors(0, 12, r=2)                                     # source frames 0..11: the chunks [0, 8) and [8, 16)
    ii, jj = g.ii.clone(), g.jj.clone()
    assert g.corr is None and g.inp is None
    net, target, weight = g.net.clone(), g.target.clone(), g.weight.clone()
    g.update_lowmem(t0=1, t1=12, itrs=2, steps=2)
    corr_op = AltCorrBlock(u.fmaps.view(1, 16, 128, 6, 8))
    damp = 1e-6 * torch.ones_like(u.disps)
    for step in range(2):
        coords, _, motn = fg.reproject(u.poses, u.disps, u.intrinsics, ii, jj, target[0].contiguous())
        for first in (0, 8):
            c = (ii >= first) & (ii < first + 8)
            assert 0 < int(c.sum()) < ii.shape[0]
            corr = corr_op(coords[None][:, c], ii[c], jj[c])
            assert tuple(corr.shape) == (1, int(c.sum()), 4 * 49, 6, 8)
            n, delta, w, damping, upmask = stub(net[:, c], u.inps[None, ii[c]], corr, motn[None][:, c], ii[c], jj[c])
            u.upsample(torch.unique(ii[c]), upmask)
            net[:, c], target[:, c], weight[:, c] = n, coords[None][:, c] + delta.float(), w.float()
            damp[torch.unique(ii[c])] = damping
        eta = .2 * damp[torch.unique(ii)].contiguous() + 1e-7
        u.ba(target, weight, eta, ii, jj, 1, 12, iters=2, lm=1e-5, ep=1e-2, motion_only=False,
             opt_type="pose_depth" if step == 0 else "depth_scale")
    assert torch.equal(g.target, target) and torch.equal(g.weight, weight) and torch.equal(g.net, net)
    same_video(v, u)
    assert g.age.tolist() == [0] * len(ii)                                      # (the low-memory pass does not age the edges)
