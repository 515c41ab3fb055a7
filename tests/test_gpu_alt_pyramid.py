"""droid_backends.altcorr_pyramid_forward (sgr_corr_alt_pyramid_forward, csrc/sgr_corr.hip) and corr.FusedAltCorrBlock on the MI355X.

Every level of the output is held, element by element and with no element excluded, to tests/corr_ref.py's fp64 altcorr_forward on the
gathered frames at coords / 2^level, within corr_ref.bound(ref, magnitude, C + 8): C roundings for a C-term fp32 sum in any order
(the kernel's is one chain of fused multiply-adds) and 8 for the four-corner sample, the bound tests/test_gpu_corr.py holds
altcorr_forward to.  The levels of a case are independent random maps, so a level read at the wrong scale or from the wrong frame
cannot pass.  Coordinates follow the recipe of that file (tracker_cases.axis_set): interior points, integers, both borders, far outside
and -1e-7."""
import functools

import numpy as np
import pytest
import torch

import corr_ref as C
from tracker_cases import DEV, edge_coords, li, np_

pytestmark = pytest.mark.gpu

F, LEVELS = 5, 4
SRC = [0, 0, 3, 2, 4, 1, 3]                    # repeated sources
DST = [1, 2, 3, 0, 2, 4, 1]                    # edge 2 is the stereo edge (3, 3)
SIZES = [(12, 16), (6, 8), (7, 9)]             # all levels live; level 3 empty; odd, level 3 empty


@functools.lru_cache(maxsize=None)
def case(H, W, ch, half, r, E=len(SRC), seed=0):
    """levels (CPU), src, dst, coords (CPU) and per level the fp64 (value, magnitude) or None for a level without pixels"""
    rng = np.random.default_rng(1000 * H + 10 * ch + 2 * r + half + seed)
    dtype = torch.float16 if half else torch.float32
    levels = [torch.tensor(rng.normal(0, 1, (F, H >> l, W >> l, ch)), dtype=torch.float32).to(dtype) for l in range(LEVELS)]
    src, dst = SRC[:E], DST[:E]
    coords = edge_coords(rng, E, H, W, r)
    return levels, src, dst, coords, reference(levels, src, dst, coords, r)


def reference(levels, src, dst, coords, r):
    refs = []
    for l, maps in enumerate(levels):
        if maps.numel() == 0:
            refs.append(None)
            continue
        at = np_(coords / 2 ** l)                                               # fp32, exact: what AltCorrBlock hands its lookup
        val, mag, _ = C.altcorr_forward(np_(levels[0].float())[src], np_(maps.float())[dst], at[:, None], r)
        refs.append((val[:, 0], mag[:, 0]))
    return refs


def run(levels, src, dst, coords, r):
    import droid_backends as db
    out, = db.altcorr_pyramid_forward([m.to(DEV) for m in levels], li(src), li(dst), coords.to(DEV), r)
    return out


def check(what, out, refs, ch, r):
    no = (2 * r + 1) ** 2
    out = np_(out).astype(np.float64)
    assert out.shape[1] == len(refs) * no
    for l, ref in enumerate(refs):
        got = out[:, l * no:(l + 1) * no]
        if ref is None:
            assert not got.any(), (what, l, "a level without pixels must give zeros")
            continue
        val, mag = ref
        err, lim = np.abs(got - val), C.bound(val, mag, ch + 8)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0))
        print(f"{what} level {l}: max |err| {err.max():.3e}, max err/bound {ratio.max():.3f}, {got.size} elements")
        assert np.all(err <= lim), (what, l, float(ratio.max()), int((err > lim).sum()))


# ---- 1. against fp64
@pytest.mark.parametrize("r", [3, 0])
@pytest.mark.parametrize("half", [True, False])
@pytest.mark.parametrize("ch", [128, 20])
@pytest.mark.parametrize("H,W", SIZES)
def test_every_level_is_within_the_fp64_bound(H, W, ch, half, r):
    levels, src, dst, coords, refs = case(H, W, ch, half, r)
    out = run(levels, src, dst, coords, r)
    assert tuple(out.shape) == (len(src), LEVELS * (2 * r + 1) ** 2, H, W) and out.dtype == torch.float32 and out.is_contiguous()
    assert (refs[3] is None) == (H < 8)
    check(f"pyramid {H}x{W} C={ch} half={half} r={r}", out, refs, ch, r)


def test_at_the_tracker_size():
    levels, src, dst, coords, refs = case(48, 64, 128, True, 3, E=3)
    check("pyramid 48x64 C=128 fp16 r=3", run(levels, src, dst, coords, 3), refs, 128, 3)


def test_fewer_levels_and_radius_four():
    levels, src, dst, coords, refs = case(12, 16, 20, False, 3)
    out = run(levels, src, dst, coords, 3)
    for n in (1, 2, 3):
        assert torch.equal(run(levels[:n], src, dst, coords, 3), out[:, :n * 49])
    coords4 = edge_coords(np.random.default_rng(4), len(src), 12, 16, 4)
    check("pyramid r=4", run(levels, src, dst, coords4, 4), reference(levels, src, dst, coords4, 4), 20, 4)
    import droid_backends as db
    with pytest.raises(ValueError, match="radius 5 exceeds"):
        db.altcorr_pyramid_forward([m.to(DEV) for m in levels], li(src), li(dst), coords.to(DEV), 5)


# ---- 2. edges outside the frame range, coordinates that are not finite
def raw_call(levels, src, dst, coords, r, out):
    """the C entry point on a caller's output buffer"""
    from splat_slam_amd import _native as nat
    Fr, H, W, ch = levels[0].shape
    ptrs = [m.data_ptr() if m.numel() else None for m in levels] + [None] * (4 - len(levels))
    kind = nat.SGR_CORR_F16 if levels[0].dtype == torch.float16 else nat.SGR_CORR_F32
    nat.check(nat.lib().sgr_corr_alt_pyramid_forward(*ptrs, src.data_ptr(), dst.data_ptr(), coords.data_ptr(), out.data_ptr(), kind, Fr,
                                                     src.shape[0], H, W, ch, r, len(levels), torch.cuda.current_stream().cuda_stream),
              "sgr_corr_alt_pyramid_forward")
    return out


@pytest.mark.parametrize("half", [True, False])
def test_edges_outside_the_frame_range_give_zeros_and_disturb_nothing(half):
    levels, src, dst, coords, _ = case(12, 16, 20, half, 3)
    good = run(levels, src, dst, coords, 3)
    bad_src, bad_dst = list(src), list(dst)
    bad_src[1], bad_dst[3], bad_src[5], bad_dst[6] = -1, F, F, -1
    bad = [1, 3, 5, 6]
    out = run(levels, bad_src, bad_dst, coords, 3)
    keep = [e for e in range(len(src)) if e not in bad]
    assert not out[bad].any() and torch.equal(out[keep], good[keep]) and good[bad].any()
    dev_levels = [m.to(DEV) for m in levels]
    poisoned = torch.full_like(good, float("nan"))
    raw_call(dev_levels, li(bad_src), li(bad_dst), coords.to(DEV), 3, poisoned)
    assert torch.equal(poisoned, out)                                           # every element written, the bad edges with zeros
    far = [2 ** 40, -2 ** 40, 2 ** 62, -2 ** 63, 5, F + 2 ** 32, -1 - 2 ** 32]  # indices that only 64-bit compares reject
    assert not run(levels, far, dst, coords, 3)[[0, 1, 2, 3, 5, 6]].any()


def test_nan_and_inf_coordinates_give_zeros():
    levels, src, dst, coords, _ = case(12, 16, 128, True, 3)
    good = run(levels, src, dst, coords, 3)
    c = coords.clone()
    c[0, 2, 3, 0], c[1, 4, 5, 1], c[2, 0, 0, 0], c[3, 11, 15, 1] = float("nan"), float("inf"), float("-inf"), float("nan")
    c[4, 6, 7] = torch.tensor([float("inf"), float("nan")])
    out = run(levels, src, dst, c, 3)
    dead = torch.zeros(good.shape[0], 12, 16, dtype=torch.bool)
    for e, y, x in ((0, 2, 3), (1, 4, 5), (2, 0, 0), (3, 11, 15), (4, 6, 7)):
        dead[e, y, x] = True
        assert not out[e, :, y, x].any()
    assert good[dead.to(DEV)[:, None].expand_as(good)].any()
    alive = ~dead.to(DEV)[:, None].expand_as(out)
    assert torch.equal(out[alive], good[alive]) and torch.isfinite(out).all()


# ---- 3. batch independence
@pytest.mark.parametrize("half,ch", [(True, 128), (False, 20)])
def test_an_edge_gives_the_same_bits_alone_and_in_any_batch(half, ch):
    levels, src, dst, coords, _ = case(12, 16, ch, half, 3)
    whole = run(levels, src, dst, coords, 3)
    assert torch.equal(whole, run(levels, src, dst, coords, 3))                 # two identical calls
    for e in range(len(src)):
        alone = run(levels, [src[e]], [dst[e]], coords[e:e + 1], 3)
        assert torch.equal(alone[0], whole[e]), e
    perm = [4, 6, 0, 5, 2, 1, 3]
    shuffled = run(levels, [src[p] for p in perm], [dst[p] for p in perm], coords[perm], 3)
    assert torch.equal(shuffled, whole[perm])


# ---- 4. the block
@pytest.mark.parametrize("half", [True, False])
def test_fused_block_agrees_with_alt_corr_block(half):
    """Both blocks keep the same pyramid (checked bit for bit), so both are within one bound of (1) of the same fp64 value: they may
    differ by the sum of the two."""
    from splat_slam_amd.corr import AltCorrBlock, FusedAltCorrBlock
    rng = np.random.default_rng(77 + half)
    N, ch, H, W, r = 6, 128, 12, 16, 3
    fmaps = torch.tensor(rng.normal(0, 1, (1, N, ch, H, W)), dtype=torch.float32).to(torch.float16 if half else torch.float32).to(DEV)
    ii, jj = li([0, 5, 2, 2, 4]), li([1, 3, 2, 0, 5])
    coords = edge_coords(rng, 5, H, W, r)[None].to(DEV)
    alt, fused = AltCorrBlock(fmaps), FusedAltCorrBlock(fmaps)
    assert len(alt.pyramid) == len(fused.pyramid) == 4
    for a, b in zip(alt.pyramid, fused.pyramid):
        assert a.dtype == b.dtype == fmaps.dtype and torch.equal(a, b)
    want, got = alt(coords, ii, jj), fused(coords, ii, jj)
    assert got.shape == want.shape == (1, 5, 4 * 49, H, W) and got.dtype == want.dtype == torch.float32 and got.is_contiguous()
    refs = reference([p[0].cpu() for p in fused.pyramid], ii.tolist(), jj.tolist(), coords[0].cpu(), r)
    check(f"FusedAltCorrBlock half={half}", got[0], refs, ch, r)
    diff = np.abs(np_(got[0]).astype(np.float64) - np_(want[0]).astype(np.float64))
    for l, (val, mag) in enumerate(refs):
        lim = 2.0 * C.bound(val, mag, ch + 8)
        d = diff[:, l * 49:(l + 1) * 49]
        print(f"fused against alt, level {l}: max |difference| {d.max():.3e}, max difference/allowance "
              f"{np.where(lim > 0, d / np.where(lim > 0, lim, 1.0), np.where(d > 0, np.inf, 0.0)).max():.3f}")
        assert np.all(d <= lim), l
    with pytest.raises(ValueError, match="AltCorrBlock"):
        fused(coords.unsqueeze(-2), ii, jj)
    assert tuple(alt(coords.unsqueeze(-2), ii, jj).shape) == (1, 5, 4 * 49, H, W, 1)


# ---- 5. synchronisation, streams, empty batches
def test_no_host_synchronisation_a_side_stream_and_no_edges():
    import droid_backends as db
    from splat_slam_amd.corr import FusedAltCorrBlock
    levels, src, dst, coords, _ = case(12, 16, 128, True, 3)
    want = run(levels, src, dst, coords, 3)
    dev_levels, s, d, c = [m.to(DEV) for m in levels], li(src), li(dst), coords.to(DEV)
    fmaps = torch.randn(1, F, 128, 12, 16, device=DEV).half()
    block = FusedAltCorrBlock(fmaps)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, = db.altcorr_pyramid_forward(dev_levels, s, d, c, 3)
        blk = block(c[None], s, d)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(out, want) and tuple(blk.shape) == (1, len(src), 196, 12, 16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        moved = [m * 2 for m in dev_levels]                                     # produced on the side stream, consumed right behind it
        out2, = db.altcorr_pyramid_forward(moved, s, d, c, 3)
    side.synchronize()
    assert torch.equal(out2, 4 * want)                                          # scaling by two is exact in both inputs
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    empty, = db.altcorr_pyramid_forward(dev_levels, none, none, torch.zeros(0, 12, 16, 2, device=DEV), 3)
    assert tuple(empty.shape) == (0, 196, 12, 16) and empty.dtype == torch.float32
    assert tuple(block(torch.zeros(1, 0, 12, 16, 2, device=DEV), none, none).shape) == (1, 0, 196, 12, 16)


def test_arguments_are_checked():
    import droid_backends as db
    levels, src, dst, coords, _ = case(12, 16, 20, False, 3)
    dev_levels, s, d, c = [m.to(DEV) for m in levels], li(src), li(dst), coords.to(DEV)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        db.altcorr_pyramid_forward(levels, s, d, c, 3)
    with pytest.raises(ValueError, match=r"levels\[1\] must be"):
        db.altcorr_pyramid_forward([dev_levels[0], dev_levels[2]], s, d, c, 3)
    with pytest.raises(TypeError, match=r"levels\[1\] must be torch.float32"):
        db.altcorr_pyramid_forward([dev_levels[0], dev_levels[1].half()], s, d, c, 3)
    with pytest.raises(ValueError, match="contiguous"):
        db.altcorr_pyramid_forward([dev_levels[0].transpose(1, 2).contiguous().transpose(1, 2)], s, d, c[:, :, :16], 3)
    with pytest.raises(ValueError, match="coords must be"):
        db.altcorr_pyramid_forward(dev_levels, s, d, c[:, :5].contiguous(), 3)
    with pytest.raises(TypeError, match="ii must be torch.int64"):
        db.altcorr_pyramid_forward(dev_levels, s.int(), d, c, 3)
    with pytest.raises(ValueError, match="multiple of 4"):
        db.altcorr_pyramid_forward([m[..., :18].contiguous() for m in dev_levels], s, d, c, 3)
    with pytest.raises(ValueError, match="1 to 4 tensors"):
        db.altcorr_pyramid_forward(dev_levels + [dev_levels[3]], s, d, c, 3)
