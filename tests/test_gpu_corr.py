"""GPU checks of the four correlation functions of droid_backends (csrc/sgr_corr.hip) against the fp64 restatement tests/corr_ref.py,
fed the same fp16 / fp32-rounded inputs.  The bounds are the worst-case bounds of an fp32 sum in any order, with or without FMA:
units * 2^-24 * magnitude per element (magnitude: the sum of the absolute products, corner weights taken as 1), units = 8 for the
four-corner sample, C + 8 for a sample of C-term dot products, terms + 8 for the backwards with the restatement's own term count; an
fp16 output adds its one final rounding (corr_ref.bound).  No element is excluded anywhere."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(48, 64, 48, 64), (40, 80, 20, 40), (7, 9, 3, 5)]


def axis_set(rng, n, size, r):
    """interior fractional points, exact integers, points within r+1 of both borders on both sides, points wholly outside, -1e-7"""
    k = rng.integers(0, 7, n)
    v = rng.uniform(0, size - 1, n)
    v = np.where(k == 1, np.round(rng.uniform(-(r + 2), size + r + 1, n)), v)
    v = np.where(k == 2, rng.uniform(-(r + 1), r + 1, n), v)
    v = np.where(k == 3, rng.uniform(size - 1 - (r + 1), size - 1 + (r + 1), n), v)
    v = np.where(k == 4, np.where(rng.random(n) < 0.5, -(r + 1.5) - rng.uniform(0, 40, n), size + r + 0.5 + rng.uniform(0, 4000, n)), v)
    v = np.where(k == 5, -1e-7, v)
    return v                                            # k == 0 and 6: interior


def coord_set(rng, B, h1, w1, h2, w2, r):
    n = B * h1 * w1
    return torch.tensor(np.stack([axis_set(rng, n, w2, r).reshape(B, h1, w1), axis_set(rng, n, h2, r).reshape(B, h1, w1)], 1),
                        dtype=torch.float32)


def alt_coord_set(rng, B, N, H1, W1, H2, W2, r):
    n = B * N * H1 * W1
    return torch.tensor(np.stack([axis_set(rng, n, W2, r), axis_set(rng, n, H2, r)], -1).reshape(B, N, H1, W1, 2), dtype=torch.float32)


def randn(rng, shape, dtype=torch.float32):
    return torch.tensor(rng.normal(0, 1, shape), dtype=torch.float32).to(dtype)


def np_(t):
    return t.detach().cpu().numpy()


def check(what, out, ref, mag, units, half=False):
    out = np_(out).astype(np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    err, lim = np.abs(out - ref), R.bound(ref, mag, units, half)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0))
    print(f"{what}: max |err| {err.max():.3e}, max err/bound {ratio.max():.3f}, {out.size} elements")
    assert np.all(err <= lim), (what, float(ratio.max()), int((err > lim).sum()))


def index_case(rng, shape, B, r, dtype):
    h1, w1, h2, w2 = shape
    return randn(rng, (B, h1, w1, h2, w2), dtype), coord_set(rng, B, h1, w1, h2, w2, r)


# ---- 1. corr_index_forward
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("r", [3, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_corr_index_forward(shape, r, dtype):
    import droid_backends as db
    rng = np.random.default_rng(sum(shape) + r)
    B = 3 if shape[0] < 10 else 2
    vol, coords = index_case(rng, shape, B, r, dtype)
    gv, gc = vol.to(DEV), coords.to(DEV)
    for i in range(4):
        ci = gc / 2 ** i
        corr, = db.corr_index_forward(gv, ci.contiguous(), r)
        assert corr.dtype == dtype and tuple(corr.shape) == (B, 2 * r + 1, 2 * r + 1) + shape[:2]
        ref, mag, _ = R.corr_index_forward(np_(vol), np_(ci), r)
        check(f"corr_index_forward {shape} r={r} {dtype} /2^{i}", corr, ref, mag, 8, dtype == torch.float16)


def test_corr_index_forward_beyond_the_register_radius_and_layout():
    """radius 5 takes the kernel without a register window; a ramp in w2 varies along the x-offset axis only"""
    import droid_backends as db
    rng = np.random.default_rng(5)
    vol, coords = index_case(rng, (7, 9, 12, 10), 2, 5, torch.float32)
    corr, = db.corr_index_forward(vol.to(DEV), coords.to(DEV), 5)
    ref, mag, _ = R.corr_index_forward(np_(vol), np_(coords), 5)
    check("corr_index_forward r=5", corr, ref, mag, 8)
    ramp = torch.arange(11, dtype=torch.float32).expand(1, 2, 3, 9, 11).contiguous().to(DEV)
    at = torch.stack([torch.full((1, 2, 3), 5.25), torch.full((1, 2, 3), 4.5)], 1).to(DEV)
    out, = db.corr_index_forward(ramp, at, 2)
    want = (5.25 - 2 + torch.arange(5, dtype=torch.float32))[:, None].expand(5, 5)
    assert torch.allclose(out[0, :, :, 0, 0].cpu(), want, rtol=0, atol=1e-5)


# ---- 2. altcorr_forward
ALT = [(C, N, half) for C in (128, 20) for N in (1, 3) for half in (False, True)]


def alt_case(rng, B, N, H1, W1, C, half, r):
    H2, W2 = (H1 // 2, W1 // 2) if half else (H1, W1)
    return randn(rng, (B, H1, W1, C)), randn(rng, (B, H2, W2, C)), alt_coord_set(rng, B, N, H1, W1, H2, W2, r)


@pytest.mark.parametrize("C,N,half", ALT)
def test_altcorr_forward(C, N, half):
    import droid_backends as db
    rng = np.random.default_rng(C + N + half)
    for (B, H1, W1, r) in ((2, 12, 16, 3), (1, 7, 9, 0)):
        f1, f2, coords = alt_case(rng, B, N, H1, W1, C, half, r)
        corr, = db.altcorr_forward(f1.to(DEV), f2.to(DEV), coords.to(DEV), r)
        ref, mag, _ = R.altcorr_forward(np_(f1), np_(f2), np_(coords), r)
        check(f"altcorr_forward C={C} N={N} half={half} r={r}", corr, ref, mag, C + 8)


def test_altcorr_forward_at_the_tracker_size_and_with_many_channels():
    import droid_backends as db
    rng = np.random.default_rng(11)
    for (B, N, H1, W1, C, half, r) in ((1, 1, 48, 64, 128, False, 3), (1, 2, 40, 80, 128, True, 3), (1, 1, 6, 5, 260, False, 1),
                                       (1, 1, 5, 7, 8, False, 9)):
        f1, f2, coords = alt_case(rng, B, N, H1, W1, C, half, r)
        corr, = db.altcorr_forward(f1.to(DEV), f2.to(DEV), coords.to(DEV), r)
        ref, mag, _ = R.altcorr_forward(np_(f1), np_(f2), np_(coords), r)
        check(f"altcorr_forward {H1}x{W1} C={C} N={N} r={r}", corr, ref, mag, C + 8)


# ---- 3. the backwards
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("r", [3, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_corr_index_backward(shape, r, dtype):
    import droid_backends as db
    rng = np.random.default_rng(sum(shape) + r + 100)
    B = 3 if shape[0] < 10 else 1
    h1, w1, h2, w2 = shape
    vol, coords = index_case(rng, shape, B, r, dtype)
    cg = randn(rng, (B, 2 * r + 1, 2 * r + 1, h1, w1), dtype)
    out, = db.corr_index_backward(vol.to(DEV), coords.to(DEV), cg.to(DEV), r)
    assert out.dtype == dtype
    ref, mag, cnt = R.corr_index_backward(tuple(vol.shape), np_(coords), np_(cg), r)
    check(f"corr_index_backward {shape} r={r} {dtype}", out, ref, mag, cnt + 8, dtype == torch.float16)
    assert np.all(np_(out)[cnt == 0] == 0) and (cnt == 0).any() and (cnt > 0).any()


class CorrLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fmap1, fmap2, coords, r):
        import droid_backends as db
        ctx.r = r
        ctx.save_for_backward(fmap1, fmap2, coords)
        return db.altcorr_forward(fmap1, fmap2, coords, r)[0]

    @staticmethod
    def backward(ctx, grad):
        import droid_backends as db
        g1, g2, gc = db.altcorr_backward(*ctx.saved_tensors, grad.contiguous(), ctx.r)
        return g1, g2, gc, None


@pytest.mark.parametrize("C,N,half", ALT)
def test_altcorr_backward(C, N, half):
    import droid_backends as db
    rng = np.random.default_rng(C + N + half + 50)
    for (B, H1, W1, r) in ((2, 12, 16, 3), (1, 7, 9, 0)):
        f1, f2, coords = alt_case(rng, B, N, H1, W1, C, half, r)
        cg = randn(rng, (B, N, (2 * r + 1) ** 2, H1, W1))
        g1, g2, gc = db.altcorr_backward(f1.to(DEV), f2.to(DEV), coords.to(DEV), cg.to(DEV), r)
        (r1, m1, k1), (r2, m2, k2) = R.altcorr_backward(np_(f1), np_(f2), np_(coords), np_(cg), r)
        check(f"fmap1_grad C={C} N={N} half={half} r={r}", g1, r1, m1, k1 + 8)
        check(f"fmap2_grad C={C} N={N} half={half} r={r}", g2, r2, m2, k2 + 8)
        assert gc.shape == coords.shape and gc.dtype == torch.float32 and not gc.any()
        # the same through autograd
        a1, a2, ac = (t.to(DEV).requires_grad_(True) for t in (f1, f2, coords))
        (CorrLayer.apply(a1, a2, ac, r) * cg.to(DEV)).sum().backward()
        check("fmap1_grad through autograd", a1.grad, r1, m1, k1 + 8)
        check("fmap2_grad through autograd", a2.grad, r2, m2, k2 + 8)
        assert not ac.grad.any()


# ---- 4. the pyramid as the tracker uses it
class CorrSampler(torch.autograd.Function):
    @staticmethod
    def forward(ctx, volume, coords, r):
        import droid_backends as db
        ctx.save_for_backward(volume, coords)
        ctx.r = r
        return db.corr_index_forward(volume, coords, r)[0]

    @staticmethod
    def backward(ctx, grad):
        import droid_backends as db
        volume, coords = ctx.saved_tensors
        return db.corr_index_backward(volume, coords, grad.contiguous(), ctx.r)[0], None, None


def test_pyramid_lookup_and_its_gradients():
    rng = np.random.default_rng(21)
    E, C, ht, wd, r = 2, 128, 48, 64, 3
    fmap1, fmap2 = (randn(rng, (1, E, C, ht, wd), torch.float16).to(DEV) for _ in range(2))
    a = fmap1.reshape(E, C, ht * wd) / 4.0
    b = fmap2.reshape(E, C, ht * wd) / 4.0
    corr = torch.matmul(a.transpose(1, 2), b).reshape(E * ht * wd, 1, ht, wd)
    assert corr.dtype == torch.float16
    pyramid = []
    for i in range(4):
        pyramid.append(corr.view(E, ht, wd, ht // 2 ** i, wd // 2 ** i).detach().clone().requires_grad_(True))
        corr = F.avg_pool2d(corr, kernel_size=2, stride=2)
    flow = torch.tensor(rng.normal(0, 6, (1, E, ht, wd, 2)), dtype=torch.float32)
    grid = torch.stack(torch.meshgrid(torch.arange(wd, dtype=torch.float32), torch.arange(ht, dtype=torch.float32), indexing="xy"), -1)
    coords = (grid[None, None] + flow).to(DEV)
    c2 = coords.permute(0, 1, 4, 2, 3).contiguous().view(E, 2, ht, wd)
    levels = [CorrSampler.apply(pyramid[i], c2 / 2 ** i, r) for i in range(4)]
    out = torch.cat([l.view(1, E, -1, ht, wd) for l in levels], dim=2)
    assert tuple(out.shape) == (1, E, 4 * 49, ht, wd) and out.dtype == torch.float16
    weight = randn(rng, tuple(out.shape), torch.float16).to(DEV)
    (out * weight).sum().backward()
    wl = weight.view(E, 4, 7, 7, ht, wd)
    for i in range(4):
        ci = np_(c2 / 2 ** i)
        ref, mag, _ = R.corr_index_forward(np_(pyramid[i]), ci, r)
        check(f"pyramid level {i}", levels[i], ref, mag, 8, True)
        gref, gmag, gcnt = R.corr_index_backward(tuple(pyramid[i].shape), ci, np_(wl[:, i]), r)
        check(f"pyramid level {i} volume_grad", pyramid[i].grad, gref, gmag, gcnt + 8, True)
        assert pyramid[i].grad.dtype == torch.float16 and np.all(np_(pyramid[i].grad)[gcnt == 0] == 0)
        del ref, mag, gref, gmag, gcnt


# ---- 5. identical calls, identical bits (fmap2_grad, summed with atomics, is the one exception)
def test_identical_calls_give_identical_bits():
    import droid_backends as db
    rng = np.random.default_rng(31)
    for dtype in (torch.float16, torch.float32):
        vol, coords = index_case(rng, (40, 80, 20, 40), 2, 3, dtype)
        cg = randn(rng, (2, 7, 7, 40, 80), dtype)
        gv, gc, gg = vol.to(DEV), coords.to(DEV), cg.to(DEV)
        assert torch.equal(db.corr_index_forward(gv, gc, 3)[0], db.corr_index_forward(gv, gc, 3)[0])
        assert torch.equal(db.corr_index_backward(gv, gc, gg, 3)[0], db.corr_index_backward(gv, gc, gg, 3)[0])
    f1, f2, coords = alt_case(rng, 2, 3, 24, 32, 128, False, 3)
    cg = randn(rng, (2, 3, 49, 24, 32))
    g = [t.to(DEV) for t in (f1, f2, coords, cg)]
    assert torch.equal(db.altcorr_forward(*g[:3], 3)[0], db.altcorr_forward(*g[:3], 3)[0])
    x, y = db.altcorr_backward(*g, 3), db.altcorr_backward(*g, 3)
    assert torch.equal(x[0], y[0]) and torch.equal(x[2], y[2])
    assert torch.allclose(x[1], y[1], rtol=1e-4, atol=1e-4)


# ---- 6. no host synchronisation
def test_correlation_functions_issue_no_host_synchronisation():
    import droid_backends as db
    rng = np.random.default_rng(41)
    vol, coords = index_case(rng, (7, 9, 3, 5), 2, 3, torch.float16)
    gv, gc, gg = vol.to(DEV), coords.to(DEV), randn(rng, (2, 7, 7, 7, 9), torch.float16).to(DEV)
    f1, f2, ac = alt_case(rng, 2, 2, 7, 9, 20, False, 3)
    g = [t.to(DEV) for t in (f1, f2, ac, randn(rng, (2, 2, 49, 7, 9)))]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [db.corr_index_forward(gv, gc, 3)[0], db.corr_index_backward(gv, gc, gg, 3)[0], db.altcorr_forward(*g[:3], 3)[0]]
        outs += db.altcorr_backward(*g, 3)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert all(torch.isfinite(o.float()).all() for o in outs)


# ---- 7. guarded coordinates (pins defined behaviour: run after 1-3 pass)
BAD = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]


def poison(rng, flat_xy):
    """flat_xy [n, 2] (a view): a fifth of the pixels get an unusable x, y or both; returns their mask"""
    n = flat_xy.shape[0]
    dead = torch.zeros(n, dtype=torch.bool)
    for p in rng.choice(n, max(n // 5, len(BAD) * 3), replace=False):
        k, v = rng.integers(0, 3), BAD[rng.integers(0, len(BAD))]
        if k != 1:
            flat_xy[p, 0] = v
        if k != 0:
            flat_xy[p, 1] = BAD[rng.integers(0, len(BAD))]
        dead[p] = True
    return dead


def test_unusable_coordinates_give_exact_zeros_and_touch_nothing():
    import droid_backends as db
    rng = np.random.default_rng(51)
    for dtype in (torch.float32, torch.float16):
        B, h1, w1, h2, w2, r = 2, 12, 16, 12, 16, 3
        vol, coords = index_case(rng, (h1, w1, h2, w2), B, r, dtype)
        xy = coords.permute(0, 2, 3, 1).reshape(-1, 2).clone()
        dead = poison(rng, xy).view(B, h1, w1)
        coords = xy.view(B, h1, w1, 2).permute(0, 3, 1, 2).contiguous()
        cg = randn(rng, (B, 7, 7, h1, w1), dtype)
        corr, = db.corr_index_forward(vol.to(DEV), coords.to(DEV), r)
        vg, = db.corr_index_backward(vol.to(DEV), coords.to(DEV), cg.to(DEV), r)
        ref, mag, _ = R.corr_index_forward(np_(vol), np_(coords), r)
        check(f"guarded corr_index_forward {dtype}", corr, ref, mag, 8, dtype == torch.float16)
        gref, gmag, gcnt = R.corr_index_backward(tuple(vol.shape), np_(coords), np_(cg), r)
        check(f"guarded corr_index_backward {dtype}", vg, gref, gmag, gcnt + 8, dtype == torch.float16)
        assert not corr.cpu().permute(0, 3, 4, 1, 2)[dead].any() and not vg.cpu()[dead].any()
        assert corr.cpu().permute(0, 3, 4, 1, 2)[~dead].any()
    B, N, H1, W1, C, r = 2, 2, 8, 12, 20, 3
    f1, f2, coords = alt_case(rng, B, N, H1, W1, C, False, r)
    dead = poison(rng, coords.view(-1, 2)).view(B, N, H1, W1)
    cg = randn(rng, (B, N, 49, H1, W1))
    g = [t.to(DEV) for t in (f1, f2, coords, cg)]
    corr, = db.altcorr_forward(*g[:3], r)
    g1, g2, gc = db.altcorr_backward(*g, r)
    ref, mag, _ = R.altcorr_forward(np_(f1), np_(f2), np_(coords), r)
    check("guarded altcorr_forward", corr, ref, mag, C + 8)
    (r1, m1, k1), (r2, m2, k2) = R.altcorr_backward(np_(f1), np_(f2), np_(coords), np_(cg), r)
    check("guarded fmap1_grad", g1, r1, m1, k1 + 8)
    check("guarded fmap2_grad", g2, r2, m2, k2 + 8)
    assert not corr.cpu().permute(0, 1, 3, 4, 2)[dead].any() and not gc.any()
    all_dead = dead.all(1)                             # a pixel dead for every n receives no fmap1 gradient at all
    assert not g1.cpu()[all_dead].any()


# ---- 8. another stream, empty batches
def test_non_default_stream_and_empty_batches():
    import droid_backends as db
    rng = np.random.default_rng(61)
    vol, coords = index_case(rng, (40, 80, 20, 40), 2, 3, torch.float16)
    f1, f2, ac = alt_case(rng, 2, 2, 12, 16, 128, True, 3)
    gv, gc = vol.to(DEV), coords.to(DEV)
    ga = [t.to(DEV) for t in (f1, f2, ac)]
    cg, acg = randn(rng, (2, 7, 7, 40, 80), torch.float16).to(DEV), randn(rng, (2, 2, 49, 12, 16)).to(DEV)
    want = [db.corr_index_forward(gv, gc, 3)[0], db.corr_index_backward(gv, gc, cg, 3)[0], db.altcorr_forward(*ga, 3)[0],
            db.altcorr_backward(*ga, acg, 3)[0]]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = [db.corr_index_forward(gv, gc, 3)[0], db.corr_index_backward(gv, gc, cg, 3)[0], db.altcorr_forward(*ga, 3)[0],
               db.altcorr_backward(*ga, acg, 3)[0]]
    s.synchronize()
    for w, g in zip(want, got):
        assert torch.equal(w, g)
    for dtype in (torch.float16, torch.float32):
        v0, c0 = torch.zeros(0, 4, 5, 3, 6, dtype=dtype, device=DEV), torch.zeros(0, 2, 4, 5, device=DEV)
        out, = db.corr_index_forward(v0, c0, 3)
        assert tuple(out.shape) == (0, 7, 7, 4, 5) and out.dtype == dtype
        out, = db.corr_index_backward(v0, c0, out, 3)
        assert tuple(out.shape) == (0, 4, 5, 3, 6) and out.dtype == dtype
    e1, e2, ec = torch.zeros(0, 4, 5, 8, device=DEV), torch.zeros(0, 2, 3, 8, device=DEV), torch.zeros(0, 3, 4, 5, 2, device=DEV)
    out, = db.altcorr_forward(e1, e2, ec, 2)
    assert tuple(out.shape) == (0, 3, 25, 4, 5)
    g1, g2, gc = db.altcorr_backward(e1, e2, ec, out, 2)
    assert g1.shape == e1.shape and g2.shape == e2.shape and gc.shape == ec.shape
    n0 = torch.zeros(2, 0, 4, 5, 2, device=DEV)         # no coordinate sets: gradients are zeros of the maps' shapes
    f = torch.ones(2, 4, 5, 8, device=DEV)
    out, = db.altcorr_forward(f, f, n0, 1)
    g1, g2, gc = db.altcorr_backward(f, f, n0, out, 1)
    assert tuple(out.shape) == (2, 0, 9, 4, 5) and not g1.any() and not g2.any() and g1.shape == f.shape
