"""-m gpu: splat_slam_amd.lpips on the MI355X.  The convolution, the pool, the pack and the distance at their edges against the fp64
statements of tests/lpips_ref.py, with bounds derived from the operands and from the kernels' roundings; the whole metric and
eval_rendering(lpips=...) under the project's criterion (vit_ref.check_against_oracle): the error against fp64 is measured against that
of the torch composition of the same weights.  Bitwise claims are torch.equal."""
import contextlib
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as LR
import vit_ref as VR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 3
U16, U32 = 2.0 ** -11, 2.0 ** -24               # unit roundoffs of fp16 and fp32


def rand(*shape, seed, scale=1.0):
    return ((2 * torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) - 1) * scale).to(DEV)


@contextlib.contextmanager
def vendor_reference():
    """The state the torch fp16 composition is computed in.  By default torch lets the vendor library time its convolution algorithms
    at the first call of a shape in a process and keeps the fastest (its find mode), so the bits of F.conv2d in fp16 differ from
    process to process: measured on the 1 x 31 x 31 case, 1.9e-6, 2.5e-6, 5.0e-6 and 6.5e-6 from the oracle in four processes, the same
    bits within each.  In immediate mode (torch.backends.miopen.flags(immediate=True)) nothing is timed: the algorithm is a function
    of the shape and of the library's find database, the same bits in every process, alone and inside the suite (3.4e-6 on that case).
    Only a find-mode run of these very shapes, which writes them into that database, changes it; nothing in the suite does one, since
    every reference convolution of this file runs under this context.  The flag is restored on exit."""
    with torch.backends.miopen.flags(immediate=True), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        yield


@pytest.fixture(scope="module")
def metric():
    from splat_slam_amd.lpips import LPIPS, normalize_state_dict, prepare, synthetic_state_dict
    canon = normalize_state_dict(synthetic_state_dict(SEED))
    return LPIPS(canon, DEV), {k: v.to(DEV) for k, v in prepare(canon).items()}


# ---- convolution -----------------------------------------------------------------------------------------------------------------------
def check_conv(layer, h, w, B=3, seed=0):
    """relu(conv + bias) against fp64 on the fp16-rounded operands.  The kernel adds the k_pad products of a pixel in fp32 in some fixed
    order (exact fp16 x fp16 products), adds the bias and rounds once to fp16, so with y the exact sum and S = sum |w| |x| + |b|
        |got - relu(y)| <= e + 2^-11 (|y| + e) + 2^-25,     e = (k_pad + 1) 2^-24 S
    (any order of k_pad + 1 fp32 additions; the fp16 rounding of the computed sum; half the smallest fp16 subnormal; relu is
    1-Lipschitz)."""
    from splat_slam_amd.lpips import CONV_SHAPES, conv_relu_f16
    cout, cin, k, stride, pad = CONV_SHAPES[layer]
    x = rand(B, cin, h, w, seed=seed + 1) * torch.tensor([1.0, 4.0, 0.25][:B], device=DEV).reshape(B, 1, 1, 1)
    wt = rand(cout, cin, k, k, seed=seed + 2, scale=(3.0 / (cin * k * k)) ** 0.5)
    b = rand(cout, seed=seed + 3, scale=0.5)
    got = conv_relu_f16(x, wt, b, stride, pad)
    x64, w64, b64 = (t.to(torch.float16).double() for t in (x, wt, b))
    y = F.conv2d(x64, w64, b64, stride=stride, padding=pad)
    S = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=stride, padding=pad)
    assert got.dtype == torch.float16 and got.shape == y.shape, (got.shape, y.shape)
    k_pad = (k * k * ((cin + 7) // 8 * 8) + 31) // 32 * 32
    e = (k_pad + 1) * U32 * S
    bound = e + U16 * (y.abs() + e) + 2.0 ** -25
    err = (got.double() - torch.relu(y)).abs()
    ratio = float((err / bound).max())
    print(f"conv{layer + 1} {h}x{w}: {B * y.shape[2] * y.shape[3]} pixels, max err {float(err.max()):.3e}, max err/bound {ratio:.3f}, "
          f"positive outputs {float((y > 0).double().mean()):.2f}")
    assert ratio <= 1.0
    assert float((y > 0).double().mean()) > 0.2 and float((y < 0).double().mean()) > 0.2         # both sides of the relu are there


@pytest.mark.parametrize("h,w", [(31, 31), (32, 33), (33, 34), (34, 35)])
def test_conv1_on_every_residue_of_the_stride(h, w):
    """(H - 7) mod 4 and (W - 7) mod 4 take all four values; three images of 7 x 7 outputs are 147 pixels, across a tile boundary"""
    check_conv(0, h, w, seed=h)


@pytest.mark.parametrize("h,w", [(3, 3), (7, 15)])
def test_conv2(h, w):
    check_conv(1, h, w, seed=10 + h)


@pytest.mark.parametrize("layer", [2, 3, 4])
def test_conv3_to_conv5(layer):
    for h, w in ((1, 1), (1, 2), (2, 3)):
        check_conv(layer, h, w, seed=20 + layer + h + w)
    check_conv(layer, 11, 13, B=1, seed=30 + layer)                 # 143 pixels: one full tile and a tail of 15


def test_conv_rejects_what_it_cannot_do():
    from splat_slam_amd.lpips import conv_relu_f16
    x = rand(1, 8, 5, 5, seed=1)
    with pytest.raises(RuntimeError, match="kernel size"):
        conv_relu_f16(x, rand(64, 8, 7, 7, seed=2), rand(64, seed=3), 1, 3)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        conv_relu_f16(x, rand(32, 8, 3, 3, seed=2), rand(32, seed=3), 1, 1)
    with pytest.raises(RuntimeError, match="no output"):
        conv_relu_f16(x, rand(64, 8, 11, 11, seed=2), rand(64, seed=3), 4, 2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        conv_relu_f16(x.cpu(), rand(64, 8, 3, 3, seed=2), rand(64, seed=3), 1, 1)


# ---- pool ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 192])
@pytest.mark.parametrize("h,w", [(3, 3), (7, 8), (8, 11), (15, 11)])
def test_max_pool_is_bit_equal_to_torch(h, w, C):
    from splat_slam_amd.lpips import max_pool_f16
    x = (rand(2, C, h, w, seed=h * w + C) * 3 - 1).to(torch.float16)              # mostly negative windows among them
    got, want = max_pool_f16(x), F.max_pool2d(x, 3, 2)
    assert got.shape == want.shape == (2, C, (h - 3) // 2 + 1, (w - 3) // 2 + 1) and torch.equal(got, want)
    assert bool((want < 0).any()) and bool((want > 0).any())
    with pytest.raises(RuntimeError, match="h and w >= 3"):
        max_pool_f16(x[:, :, :2])


# ---- pack ------------------------------------------------------------------------------------------------------------------------------
def ulp16(v):
    """the spacing of fp16 at |v| (fp64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.maximum(2.0 ** (e - 10), torch.tensor(2.0 ** -24, dtype=torch.float64, device=v.device))


def test_pack_frames_applies_exposure_clamp_and_scaling():
    from splat_slam_amd.lpips import SCALE, SHIFT, pack_frames
    n, H, W = 3, 31, 37
    renders = [rand(3, H, W, seed=40 + i) * 0.9 + 0.5 for i in range(n)]            # [-0.4, 1.4]: both clamps act
    gts = [rand(3, H, W, seed=50 + i) * 0.7 + 0.5 for i in range(n)]                # the ground truth is taken as it is, also outside [0, 1]
    a = [None, torch.tensor([0.11], device=DEV), torch.tensor([-0.2], device=DEV)]
    b = [None, torch.tensor([-0.05], device=DEV), torch.tensor([0.07], device=DEV)]
    shift, scale = torch.tensor(SHIFT, dtype=torch.float64), torch.tensor(SCALE, dtype=torch.float64)
    for ea, eb in ((a, b), (None, None)):
        got = pack_frames(renders, gts, ea, eb)
        assert got.shape == (2 * n, H, W, 8) and got.dtype == torch.float16
        assert torch.count_nonzero(got[..., 3:]) == 0
        imgs = [LR.exposed(renders[i], None if ea is None else ea[i], None if eb is None else eb[i]) for i in range(n)]
        assert any(bool((im == 0).any()) and bool((im == 1).any()) for im in imgs)
        want = LR.scale_input(torch.stack(imgs + [g.double() for g in gts]), shift, scale).permute(0, 2, 3, 1)
        err = (got[..., :3].double() - want).abs()
        print("pack_frames: max err / ulp", float((err / ulp16(want)).max()))
        assert bool((err <= ulp16(want)).all())


@pytest.mark.parametrize("normalize", [True, False])
def test_pack_pairs(normalize):
    from splat_slam_amd.lpips import SCALE, SHIFT, pack_pairs
    n, H, W = 2, 33, 31
    x0, x1 = rand(n, 3, H, W, seed=60) * 0.8 + 0.4, rand(n, 3, H, W, seed=61) * 0.8 + 0.4       # [-0.4, 1.2]: taken as they are, no clamp
    got = pack_pairs(x0, x1, normalize)
    want = LR.scale_input(torch.cat([x0, x1]), torch.tensor(SHIFT), torch.tensor(SCALE), normalize).permute(0, 2, 3, 1)
    assert got.shape == (2 * n, H, W, 8) and torch.count_nonzero(got[..., 3:]) == 0
    assert bool(((got[..., :3].double() - want).abs() <= ulp16(want)).all())


# ---- distance --------------------------------------------------------------------------------------------------------------------------
def K_of(C):
    return C / 4 + 22


def check_distance(name, f0, f1, w):
    """The kernel's roundings, all fp32 with unit roundoff u = 2^-24, no operation fused; f is exact (fp16), w >= 0:
      1. s = fl(sum f^2): a lane adds its C / 8 rounded products in turn, three butterfly additions follow; every term is >= 0 and
         passes at most 1 + (C / 8 - 1) + 3 roundings:                                      |s^ - s| <= (C / 8 + 3) u s
      2. q = fl(fl(1e-8) + s^):                                                              rel <= (C / 8 + 5) u
      3. r = 1 / sqrt(q), each of the two within 1 ulp = 2 u:                                rel <= (C / 16 + 2.5 + 4) u =: a u
      4. u^ = fl(f r):                                                                       |u^ - u| <= (a + 1) u |u|
      5. t = fl(u^ - v^):                     |t - (u - v)| <= (a + 1) u (|u| + |v|) + u |u^ - v^| <= (a + 2) u (|u| + |v|)
      6. fl(w fl(t^2)): |t^2 - (u - v)^2| <= 2 (a + 2) u (|u| + |v|)^2 to first order, two more roundings:
                                                                                  per term <= (2 a + 6) u w (|u| + |v|)^2
      7. the sum of the C terms, all >= 0, (C / 8 - 1) + 3 additions:                        <= (C / 8 + 2) u sum
    Together |d^_p - d_p| <= (C / 4 + 21) u B_p with B_p = sum_c w_c (|u_c| + |v_c|)^2; one more u for the second-order terms gives
    K(C) = C / 4 + 22.  A product below the normal range adds at most 2^-126 w each: C max(w) 2^-126 per pixel.
    A workgroup's partial sum adds 4 pixels per group and 32 groups in turn (35 additions), the merge is fp64: the tap mean is within
    mean_p (K u B_p) + 36 u mean_p d_p.  Returns the largest err / bound seen."""
    from splat_slam_amd.lpips import distance
    n, P, C = f0.shape
    partials, per_pixel = distance(f0, f1, w)
    assert partials.shape == (n, (P + 127) // 128) and per_pixel.shape == (n, P)
    assert bool(torch.isfinite(per_pixel).all()) and bool(torch.isfinite(partials).all())
    a, b = f0.permute(0, 2, 1), f1.permute(0, 2, 1)                              # [n,C,P] for the restatement
    d, B = LR.pixel_distance(a, b, w), LR.pixel_bound_sum(a, b, w)
    tiny = C * max(float(w.max()), 1.0) * 2.0 ** -126
    bound = K_of(C) * U32 * B + tiny
    err = (per_pixel.double() - d).abs()
    r_pix = float((err / bound).max())
    mean = partials.double().sum(1) / P
    mbound = bound.mean(1) + 36 * U32 * d.mean(1)
    r_mean = float(((mean - d.mean(1)).abs() / mbound).max())
    print(f"distance {name}: C={C} P={P} n={n} per-pixel err/bound {r_pix:.4f}, mean err/bound {r_mean:.4f}")
    assert bool((err <= bound).all()) and r_mean <= 1.0, (name, r_pix, r_mean)
    return partials, per_pixel, max(r_pix, r_mean)


def features(n, P, C, seed, scale=1.0):
    """post-ReLU-like maps: half of the values zero, the rest positive, per-pixel scales over three decades"""
    g = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(n, P, C, generator=g)) * 10.0 ** (torch.rand(n, P, 1, generator=g) * 3 - 2) * scale
    return f.to(DEV).to(torch.float16)


@pytest.mark.parametrize("C", [64, 192, 384, 256])
def test_distance_against_fp64_within_the_derived_bound(C):
    w = (rand(C, seed=C) + 1) / 2
    worst = 0.0
    for n in (1, 3):
        for P in (1, 2, 63, 64, 65, 129):
            f0 = features(n, P, C, seed=C + P + n)
            # a good render: the second map is the first with a small relative change; and an unrelated one
            near = (f0.float() * (1 + 0.01 * rand(n, P, C, seed=C + P + n + 1))).to(torch.float16)
            far = features(n, P, C, seed=C + P + n + 2)
            for name, f1 in (("near", near), ("far", far)):
                worst = max(worst, check_distance(name, f0, f1, w)[2])
    print(f"distance C={C}: worst err/bound {worst:.4f}")


@pytest.mark.parametrize("C", [64, 192, 384, 256])
def test_distance_edges(C):
    n, P = 2, 65
    w = (rand(C, seed=2 * C) + 1) / 2
    f0, f1 = features(n, P, C, seed=C + 7), features(n, P, C, seed=C + 8)
    # equal maps: exactly zero, every pixel and every partial sum
    partials, per_pixel, _ = check_distance("equal", f0, f0.clone(), w)
    assert torch.count_nonzero(partials) == 0 and torch.count_nonzero(per_pixel) == 0
    # swapped arguments: the same bits
    pa, qa, _ = check_distance("xy", f0, f1, w)
    pb, qb, _ = check_distance("yx", f1, f0, w)
    assert torch.equal(pa, pb) and torch.equal(qa, qb) and bool((qa > 0).all())
    # a pixel that is all zero in one map (d = sum w v^2), and in both (0)
    z0, z1 = f0.clone(), f1.clone()
    z0[:, 3] = 0
    z0[:, 64] = 0
    z1[:, 64] = 0
    _, q, _ = check_distance("zero pixels", z0, z1, w)
    assert bool((q[:, 64] == 0).all()) and bool((q[:, 3] > 0).all())
    # values near the fp16 maximum, signs mixed (sum f^2 up to 1.6e12)
    big = ((rand(n, P, C, seed=C + 9) * 5504).abs() + 60000).to(torch.float16)
    assert float(big.max()) <= 65504 and bool(torch.isfinite(big).all())
    sign = torch.where(rand(n, P, C, seed=C + 10) > 0, 1.0, -1.0).to(torch.float16)
    check_distance("fp16 max", big, big * sign, w)
    check_distance("fp16 max against small", big, f1, w)
    # subnormal fp16 values: sum f^2 <= 384 (20 * 2^-24)^2 = 5.5e-10 << 1e-8, so u = 1e4 f
    sub0 = (torch.randint(0, 21, (n, P, C), generator=torch.Generator().manual_seed(C)).to(DEV) * 2.0 ** -24).to(torch.float16)
    sub1 = (torch.randint(0, 21, (n, P, C), generator=torch.Generator().manual_seed(C + 1)).to(DEV) * 2.0 ** -24).to(torch.float16)
    assert float(sub0.max()) == 20 * 2.0 ** -24
    _, q, _ = check_distance("subnormal", sub0, sub1, w)
    assert bool((q > 0).all())
    check_distance("subnormal against normal", sub0, f1, w)
    # zero weights: some, and all (exactly 0)
    w0 = w.clone()
    w0[::3] = 0
    check_distance("some zero weights", f0, f1, w0)
    partials, per_pixel, _ = check_distance("zero weights", f0, f1, torch.zeros_like(w))
    assert torch.count_nonzero(partials) == 0 and torch.count_nonzero(per_pixel) == 0


def test_distance_rejects_other_channel_counts():
    from splat_slam_amd.lpips import distance
    f = features(1, 4, 128, seed=1)
    with pytest.raises(RuntimeError, match="channels"):
        distance(f, f, rand(128, seed=2).abs())


# ---- the whole metric ------------------------------------------------------------------------------------------------------------------
def image_pairs(n, H, W, seed):
    """a smooth image with texture, and a render of it: a small blur-like change plus noise (the case the metric is for)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, max(H // 8, 2), max(W // 8, 2), generator=g)
    x = (F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) + 0.15 * torch.randn(n, 3, H, W, generator=g)).clamp(0, 1)
    y = (0.9 * x + 0.1 * x.mean((2, 3), keepdim=True) + 0.03 * torch.randn(n, 3, H, W, generator=g)).clamp(0, 1)
    return x.to(DEV).contiguous(), y.to(DEV).contiguous()


@pytest.mark.parametrize("n,H,W", [(1, 31, 31), (3, 31, 31), (1, 35, 47), (3, 35, 47), (8, 48, 64), (2, 120, 160)])
def test_network_is_as_close_to_the_fp64_oracle_as_the_torch_composition(metric, n, H, W):
    """The level table [n,5] and the totals [n], each under the criterion: max error <= 2 x and rms <= 1.5 x that of the torch fp16
    composition, both against the fp64 restatement with the same fp16-rounded weights.
    The torch side is computed under vendor_reference(), so its bits and the verdict are the same when this file runs alone and inside
    the suite.  Measured on the MI355X, the same figures in both (max error of hip | torch; the rms figures are in DESIGN.md
    section 3, "LPIPS"):
        1 x 31 x 31     levels 2.70e-6 | 3.25e-6, total 4.93e-6 | 3.44e-6
        3 x 31 x 31     levels 3.59e-6 | 4.67e-6, total 9.45e-6 | 1.09e-5
        1 x 35 x 47     levels 1.67e-6 | 3.28e-6, total 2.16e-7 | 1.30e-5
        3 x 35 x 47     levels 3.42e-6 | 7.57e-6, total 6.50e-6 | 1.55e-5
        8 x 48 x 64     levels 6.69e-6 | 7.42e-6, total 1.12e-5 | 1.44e-5
        2 x 120 x 160   levels 1.37e-6 | 1.38e-6, total 2.53e-6 | 2.07e-6
    With n = 1 the total is one number and its rms is its error: 1 x 31 x 31 stands at 1.44 x where 1.5 x is allowed.  Both sides are
    draws of the rounding noise of the fp16 layouts (the pipeline with every sum exact in fp64 and only the prescribed roundings of
    the input and the taps is 6.75e-6 from the oracle on this pair)."""
    net, P = metric
    x, y = image_pairs(n, H, W, seed=H + W + n)
    levels = net.lpips(x, y, return_levels=True)
    total = net.lpips(x, y)
    assert levels.shape == (n, 5) and total.shape == (n,) and levels.dtype == total.dtype == torch.float32
    with vendor_reference():
        tt, lt = LR.lpips_torch(P, x, y)
    to, lo = LR.lpips_ref(P, x, y)
    assert bool((lo > 0).all())
    VR.check_against_oracle(f"lpips-{n}x{H}x{W}", ("levels", "total"), (levels, total), (lt, tt), (lo, to))
    # the total is the sum of the levels, rounded once
    assert torch.allclose(total.double(), levels.double().sum(1), rtol=3 * U32, atol=0)


def test_network_repeats_and_a_pair_has_the_bits_it_has_alone(metric):
    net, _ = metric
    x, y = image_pairs(18, 35, 47, seed=5)                           # two chunks: 16 + 2
    a, b = net.lpips(x, y, return_levels=True), net.lpips(x, y, return_levels=True)
    assert torch.equal(a, b)
    for i in (0, 7, 15, 16, 17):
        assert torch.equal(net.lpips(x[i:i + 1], y[i:i + 1], return_levels=True)[0], a[i]), i
    assert torch.equal(net.lpips(x[5:9], y[5:9], return_levels=True), a[5:9])
    assert torch.equal(net.lpips(x, y), net(x, y))
    # fp16 and fp64 images are read as fp32
    assert torch.equal(net.lpips(x.double(), y.double()), net.lpips(x, y))


def test_network_is_zero_on_equal_images_and_symmetric(metric):
    net, _ = metric
    x, y = image_pairs(3, 48, 64, seed=6)
    zero = net.lpips(x, x.clone(), return_levels=True)
    assert torch.count_nonzero(zero) == 0 and torch.count_nonzero(net.lpips(x, x)) == 0
    xy, yx = net.lpips(x, y, return_levels=True), net.lpips(y, x, return_levels=True)
    assert torch.equal(xy, yx) and bool((xy > 0).all())
    assert torch.equal(net.lpips(x, y), net.lpips(y, x))
    # normalize=False reads [-1, 1]: 2 x - 1 in fp32 is what the pack computes
    assert torch.equal(net.lpips(2 * x - 1, 2 * y - 1, normalize=False, return_levels=True), xy)


def test_network_rejects_bad_sizes_and_cpu_tensors(metric):
    from splat_slam_amd.lpips import LPIPS, synthetic_state_dict
    net, _ = metric
    for shape in ((1, 3, 30, 31), (1, 3, 31, 30), (1, 4, 40, 40), (3, 40, 40)):
        with pytest.raises(ValueError, match="lpips"):
            net.lpips(torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        net.lpips(torch.zeros(1, 3, 31, 31), torch.zeros(1, 3, 31, 31))
    with pytest.raises(RuntimeError, match="no CPU path"):
        LPIPS.from_state_dict(synthetic_state_dict(SEED), device="cpu")


def test_both_key_layouts_load_the_same_metric(metric):
    from splat_slam_amd.lpips import LPIPS, synthetic_state_dict
    net, _ = metric
    sd = synthetic_state_dict(SEED)
    alex = {f + p: sd[s + p] for s, f in (("net.slice1.0", "features.0"), ("net.slice2.3", "features.3"), ("net.slice3.6", "features.6"),
                                          ("net.slice4.8", "features.8"), ("net.slice5.10", "features.10")) for p in (".weight", ".bias")}
    lin = {k: v for k, v in sd.items() if k.startswith("lin")}
    x, y = image_pairs(2, 31, 40, seed=8)
    want = net.lpips(x, y, return_levels=True)
    assert torch.equal(LPIPS.from_parts(alex, lin, DEV).lpips(x, y, return_levels=True), want)
    assert torch.equal(LPIPS.from_state_dict({"net." + k: v for k, v in sd.items()}, DEV).lpips(x, y, return_levels=True), want)
    assert torch.equal(LPIPS.synthetic(SEED, DEV).lpips(x, y, return_levels=True), want)


# ---- eval_rendering --------------------------------------------------------------------------------------------------------------------
def _eval_scene(views, n, seed):
    """the small synthetic session of tests/test_gpu_ssim.py: optimised exposures on every frame but the first, masked regions"""
    from splat_slam_amd import synthetic as syn
    intr = syn.INTRINSICS["tiny"]
    params = syn.room_parameters(n, seed=seed, device=DEV)
    params["scaling"] = params["scaling"] + 1.2
    cams = syn.make_views(params, views, intr, DEV, seed=seed)
    gm = syn.model_from_parameters(params, device=DEV)
    H, W = intr["H"], intr["W"]
    with torch.no_grad():
        for k, cam in enumerate(cams):
            if k > 0:
                cam.exposure_a.fill_(0.03 * ((k % 5) - 2))
                cam.exposure_b.fill_(0.01 * ((k % 3) - 1))
            cam.original_image[:, : H // 8, : W // 6] = 0.0
            cam.depth[H // 3: H // 2, W // 4: W // 2] = 0.0
    return cams, gm


def test_eval_rendering_with_lpips(metric):
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.eval import eval_rendering
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.renderer import render
    from splat_slam_amd.session import MappingSession
    net, P = metric
    views = 18                                                       # two chunks of the evaluation: 16 + 2
    cams, gm = _eval_scene(views, 4000, seed=7)
    bg = torch.zeros(3, device=DEV)
    plain = eval_rendering(cams, gm, PipelineParams(), bg)
    got = eval_rendering(cams, gm, PipelineParams(), bg, lpips=net)
    assert "lpips" not in plain and "mean_lpips" not in plain
    assert set(got) == set(plain) | {"lpips", "mean_lpips"}
    for key in plain:                                                # every bit of the other figures
        assert got[key] == plain[key] or (isinstance(plain[key], float) and math.isnan(plain[key]) and math.isnan(got[key])), key
    assert len(got["lpips"]) == views and got["mean_lpips"] == float(np.mean(got["lpips"]))
    # the oracle on the clamped, exposure-compensated images (eval_utils.py:96-100)
    with torch.no_grad():
        renders = [render(c, gm, PipelineParams(), bg)["render"] for c in cams]
        img64 = torch.stack([LR.exposed(r, c.exposure_a if k else None, c.exposure_b if k else None) for k, (r, c) in enumerate(zip(renders, cams))])
        img32 = torch.stack([torch.clamp(torch.exp(c.exposure_a) * r + c.exposure_b if k else r, 0.0, 1.0) for k, (r, c) in enumerate(zip(renders, cams))])
        gt = torch.stack([c.original_image for c in cams])
        with vendor_reference():
            tt, _ = LR.lpips_torch(P, img32, gt)
        to, _ = LR.lpips_ref(P, img64, gt)
    hip = torch.tensor(got["lpips"], dtype=torch.float64)
    assert bool((hip > 0).all())
    VR.check_against_oracle("eval_rendering lpips", ("lpips",), (hip,), (tt,), (to,))
    # the session entry point
    loop = types.SimpleNamespace(config=syn.DEFAULT_CONFIG, device=DEV, viewpoints={2 * k: c for k, c in enumerate(cams)}, gaussians=gm,
                                 background=bg)
    sess = MappingSession(loop, syn.INTRINSICS["tiny"])
    assert sess.evaluate(lpips=net) == got and sess.evaluate() == plain


def test_eval_rendering_with_lpips_rejects_small_frames(metric):
    from splat_slam_amd.eval import eval_rendering
    net, _ = metric
    for shape in ((3, 24, 24), (3, 30, 64), (1, 64, 64)):
        frames = [types.SimpleNamespace(original_image=torch.zeros(shape, device=DEV))]
        with pytest.raises(ValueError, match="31 x 31|3 channels"):
            eval_rendering(frames, None, None, None, lpips=net)
