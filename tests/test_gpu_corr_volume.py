"""droid_backends.corr_volume_pyramid / corr_index_pyramid_forward (sgr_corr_volume.hip, sgr_corr.hip), splat_slam_amd.corr.FusedCorrBlock
and FactorGraph(corr_impl="volume_fused") on the MI355X, against tests/corr_volume_ref.py and the existing corr_index_forward.

Bounds.  Exact data (multiples of 1/8): every product is a multiple of 1/64 and every sum the kernel forms is exact in fp32 in any
order, so each level must equal the fp64 oracle rounded once to fp16.  Normal data: corr_ref.bound(ref, mag, 2 C + 16, half=True),
two roundings per product-add (nothing says that the matrix unit rounds its internal adds to nearest), nine adds of the three poolings
rounded up to 16, and the one fp16 rounding; no element is excluded."""
import functools

import numpy as np
import pytest
import torch

import corr_ref as C
import corr_volume_ref as V
from tracker_cases import edge_coords, make_video, stub

pytestmark = pytest.mark.gpu

DEV = "cuda"
FRAMES, CAMS, LEVELS = 5, 2, 4
II = [0, 0, 3, 2, 4, 1, 0]                       # repeated sources, one stereo edge (2, 2)
JJ = [1, 4, 0, 2, 3, 1 + 1, 0 + 3]
SIZES = [(12, 16), (6, 8), (7, 9), (1, 1), (17, 24)]


def li(a):
    return torch.tensor(np.asarray(a), dtype=torch.int64, device=DEV).reshape(-1)


def np_(t):
    return t.detach().cpu().numpy()


def planes_of(ii, jj):
    ii, jj = np.asarray(ii), np.asarray(jj)
    return ii * CAMS, jj * CAMS + (ii == jj)


@functools.lru_cache(maxsize=None)
def maps_of(h, w, ch, exact):
    rng = np.random.default_rng(1000 * h + 10 * w + ch + exact)
    if exact:
        m = rng.integers(-8, 9, size=(FRAMES, CAMS, ch, h, w)) / 8.0
    else:
        m = rng.normal(size=(FRAMES, CAMS, ch, h, w))
    return torch.tensor(m, dtype=torch.float16, device=DEV)


def store(cap, h, w, levels=LEVELS, fill=None):
    out = [torch.empty((cap, h, w, h >> l, w >> l), dtype=torch.float16, device=DEV) for l in range(levels)]
    if fill is not None:
        for v in out:
            v.fill_(fill)
    return out


def build(maps, src, dst, slots, cap, fill=None):
    import droid_backends as db
    h, w = maps.shape[-2:]
    lv = store(cap, h, w, fill=fill)
    db.corr_volume_pyramid(maps.view(-1, *maps.shape[2:]), li(src), li(dst), lv, li(slots))
    return lv


@functools.lru_cache(maxsize=None)
def case(h, w, ch, exact):
    """the seven edges in slots 6 .. 0 of a store of 8: (GPU levels, oracle [(value, magnitude)] in edge order, slots)"""
    maps = maps_of(h, w, ch, exact)
    src, dst = planes_of(II, JJ)
    slots = list(range(6, -1, -1))
    lv = build(maps, src, dst, slots, 8)
    ref = V.volume_pyramid(np_(maps).reshape(FRAMES * CAMS, ch, h, w), src, dst, LEVELS)
    return lv, ref, slots


@pytest.mark.parametrize("ch", [128, 32])
@pytest.mark.parametrize("h,w", SIZES)
def test_exact_data_gives_the_oracle_rounded_once(h, w, ch):
    lv, ref, slots = case(h, w, ch, True)
    for l in range(LEVELS):
        want = torch.tensor(ref[l][0]).to(torch.float16)                           # one rounding to nearest even
        got = lv[l][li(slots)].cpu()
        assert got.shape == want.shape == (7, h, w, h >> l, w >> l)
        assert torch.equal(got, want), f"level {l}: {(got != want).sum().item()} of {want.numel()} elements differ"
    assert lv[0][li(slots)].any()                                                 # (slot 7 of the store is nobody's: never read)


def worst_ratio(lv, ref, slots, ch):
    worst = 0.0
    for l in range(len(lv)):
        val, mag = ref[l]
        if val.size == 0:
            continue
        err = np.abs(np_(lv[l][li(slots)]).astype(np.float64) - val)
        worst = max(worst, float((err / C.bound(val, mag, 2 * ch + 16, half=True)).max()))
    return worst


@pytest.mark.parametrize("ch", [128, 32])
@pytest.mark.parametrize("h,w", SIZES)
def test_normal_data_is_within_the_bound_everywhere(h, w, ch):
    lv, ref, slots = case(h, w, ch, False)
    worst = worst_ratio(lv, ref, slots, ch)
    print(f"volume pyramid {h}x{w} C={ch}: worst err / bound = {worst:.4f}")
    assert worst <= 1.0


def test_normal_data_at_the_trackers_size():
    h, w, ch = 48, 64, 128
    rng = np.random.default_rng(5)
    maps = torch.tensor(rng.normal(size=(2, 1, ch, h, w)), dtype=torch.float16, device=DEV)
    lv = store(3, h, w)
    import droid_backends as db
    db.corr_volume_pyramid(maps.view(2, ch, h, w), li([0, 1]), li([1, 1]), lv, li([2, 0]))
    m = np_(maps).astype(np.float64).reshape(2, ch, h * w)
    worst = 0.0
    for e, (s, d, slot) in enumerate([(0, 1, 2), (1, 1, 0)]):
        val = (m[s].T @ m[d] / 16.0).reshape(h, w, h, w)
        mag = (np.abs(m[s]).T @ np.abs(m[d]) / 16.0).reshape(h, w, h, w)
        for l in range(LEVELS):
            v, g = V.block_mean(val, l), V.block_mean(mag, l)
            err = np.abs(np_(lv[l][slot]).astype(np.float64) - v)
            worst = max(worst, float((err / C.bound(v, g, 2 * ch + 16, half=True)).max()))
    print(f"volume pyramid 48x64 C=128 E=2: worst err / bound = {worst:.4f}")
    assert worst <= 1.0


def lookup_by_levels(lv, slots, coords, r):
    """corr_index_forward on every gathered level at coords / 2^l, [E, L, rd*rd, h, w]"""
    import droid_backends as db
    E, h, w, _ = coords.shape
    planes = coords.permute(0, 3, 1, 2)
    out = []
    for l, v in enumerate(lv):
        got, = db.corr_index_forward(v[slots].contiguous(), (planes / 2 ** l).float().contiguous(), r)
        out.append(got.view(E, -1, h, w))
    return torch.stack(out, 1)


@pytest.mark.parametrize("r", [3, 0, 4])
@pytest.mark.parametrize("h,w", SIZES)
def test_lookup_equals_corr_index_forward_level_by_level(h, w, r):
    import droid_backends as db
    lv, _, slots = case(h, w, 32, False)
    slots = li(slots)
    rng = np.random.default_rng(h * w + r)
    coords = edge_coords(rng, 7, h, w, r).to(DEV)
    got, = db.corr_index_pyramid_forward(lv, slots, coords, r)
    rd2 = (2 * r + 1) ** 2
    assert got.dtype == torch.float16 and tuple(got.shape) == (7, LEVELS * rd2, h, w)
    want = lookup_by_levels(lv, slots, coords, r)
    for l in range(LEVELS):
        assert torch.equal(got[:, l * rd2:(l + 1) * rd2], want[:, l]), f"level {l}"
        if (h >> l) == 0 or (w >> l) == 0:
            assert not got[:, l * rd2:(l + 1) * rd2].any()
    if h > 1:
        assert got.any()
    again, = db.corr_index_pyramid_forward(lv, slots, coords, r)
    assert torch.equal(got, again)


def test_lookup_radius_nonfinite_coordinates_bad_slots_and_a_poisoned_buffer():
    import droid_backends as db
    from splat_slam_amd import _native as nat
    h, w, r = 12, 16, 3
    lv, _, slots = case(h, w, 32, False)
    slots = li(slots)
    coords = edge_coords(np.random.default_rng(3), 7, h, w, r).to(DEV)
    with pytest.raises(ValueError, match="radius"):
        db.corr_index_pyramid_forward(lv, slots, coords, 5)
    clean, = db.corr_index_pyramid_forward(lv, slots, coords, r)
    bad = coords.clone()
    spots = [(0, 0, 0), (1, 5, 7), (3, 11, 15), (6, 2, 3), (4, 4, 4), (5, 6, 0)]
    vals = [(float("nan"), 1.0), (2.0, float("nan")), (float("inf"), 3.0), (1.0, float("-inf")), (float("nan"), float("inf")), (3e38, -3e38)]
    for (e, y, x), v in zip(spots, vals):
        bad[e, y, x] = torch.tensor(v, device=DEV)
    got, = db.corr_index_pyramid_forward(lv, slots, bad, r)
    mask = torch.zeros((7, h, w), dtype=torch.bool, device=DEV)
    for e, y, x in spots:
        mask[e, y, x] = True
    m = mask[:, None].expand_as(got)
    assert not got[m].any() and torch.equal(got[~m], clean[~m])
    # slots outside the store give zeros, the others are untouched
    odd = slots.clone()
    odd[1], odd[4], odd[6] = -1, 8, 2 ** 40
    got, = db.corr_index_pyramid_forward(lv, odd, coords, r)
    assert not got[[1, 4, 6]].any() and torch.equal(got[[0, 2, 3, 5]], clean[[0, 2, 3, 5]])
    # the C entry writes every element of a buffer it is handed
    out = torch.full_like(clean, float("nan"))
    ptrs = [v.data_ptr() for v in lv]
    nat.check(nat.lib().sgr_corr_index_pyramid_forward(*ptrs, slots.data_ptr(), coords.data_ptr(), out.data_ptr(), 8, 7, h, w, r, LEVELS,
                                                       torch.cuda.current_stream().cuda_stream), "sgr_corr_index_pyramid_forward")
    assert torch.equal(out, clean)
    # (6, 8): level 3 has no pixel and may be NULL
    lv68, _, s68 = case(6, 8, 32, False)
    c68 = edge_coords(np.random.default_rng(4), 7, 6, 8, r).to(DEV)
    out = torch.full((7, LEVELS * 49, 6, 8), float("nan"), dtype=torch.float16, device=DEV)
    ptrs = [v.data_ptr() for v in lv68[:3]] + [None]
    nat.check(nat.lib().sgr_corr_index_pyramid_forward(*ptrs, li(s68).data_ptr(), c68.data_ptr(), out.data_ptr(), 8, 7, 6, 8, r, LEVELS,
                                                       torch.cuda.current_stream().cuda_stream), "sgr_corr_index_pyramid_forward")
    assert not torch.isnan(out).any() and not out[:, 3 * 49:].any() and out[:, :49].any()


@pytest.mark.parametrize("h,w", [(12, 16), (7, 9)])
def test_planes_outside_the_range_zero_their_slot_and_bad_slots_write_nothing(h, w):
    lv, _, slots = case(h, w, 32, False)
    maps = maps_of(h, w, 32, False)
    src, dst = planes_of(II, JJ)
    src, dst = src.copy(), dst.copy()
    src[1], dst[2], src[4], dst[5], dst[6] = -1, FRAMES * CAMS, 2 ** 40, -2 ** 40, 2 ** 62
    dead = [1, 2, 4, 5, 6]
    got = build(maps, src, dst, slots, 8, fill=7.0)
    for l in range(LEVELS):
        for e, s in enumerate(slots):
            if e in dead:
                assert not got[l][s].any(), (l, e)
            else:
                assert torch.equal(got[l][s], lv[l][s]), (l, e)
        assert (got[l][7] == 7.0).all()                                          # the slot nobody named
    # slots outside [0, capacity) write nothing: the canary of every slot but those of edges 0 and 3 is whole
    src, dst = planes_of(II, JJ)
    odd = [3, -1, 8, 5, 2 ** 40, -2 ** 40, 2 ** 62]
    got = build(maps, src, dst, odd, 8, fill=7.0)
    for l in range(LEVELS):
        for s in range(8):
            if s == 3:
                assert torch.equal(got[l][s], lv[l][slots[0]])
            elif s == 5:
                assert torch.equal(got[l][s], lv[l][slots[3]])
            else:
                assert (got[l][s] == 7.0).all(), (l, s)


@pytest.mark.parametrize("h,w,ch", [(12, 16, 128), (17, 24, 32), (7, 9, 32)])
def test_an_edge_gives_the_same_bits_alone_permuted_and_in_another_slot(h, w, ch):
    lv, _, slots = case(h, w, ch, False)
    maps = maps_of(h, w, ch, False)
    src, dst = planes_of(II, JJ)
    perm = [4, 0, 6, 2, 5, 1, 3]
    other = [0, 9, 3, 7, 1, 5, 2]                                                 # other slots, in a store of another size
    got = build(maps, src[perm], dst[perm], [other[e] for e in perm], 10)
    again = build(maps, src, dst, slots, 8)
    for l in range(LEVELS):
        assert torch.equal(again[l][li(slots)], lv[l][li(slots)])                 # two identical calls
        assert torch.equal(got[l][li(other)], lv[l][li(slots)])
    for e in (0, 3, 6):
        alone = build(maps, src[e:e + 1], dst[e:e + 1], [1], 2)
        for l in range(LEVELS):
            assert torch.equal(alone[l][1], lv[l][slots[e]]), (e, l)


def fresh_block(maps, ii, jj, r=3):
    from splat_slam_amd.corr import FusedCorrBlock
    return FusedCorrBlock(maps, radius=r, capacity=max(int(ii.shape[0]), 1)).add(ii, jj)


def test_the_block_through_a_scripted_history():
    from splat_slam_amd.corr import FusedCorrBlock
    h, w = 7, 9
    maps = maps_of(h, w, 32, False)
    rng = np.random.default_rng(9)
    block = FusedCorrBlock(maps, capacity=6)
    empty = block(torch.zeros((1, 0, h, w, 2), device=DEV))
    assert tuple(empty.shape) == (1, 0, LEVELS * 49, h, w) and empty.dtype == torch.float16 and len(block) == 0
    ii, jj = li([]), li([])

    def step(fn, new_ii, new_jj):
        coords = edge_coords(rng, new_ii.shape[0], h, w, 3).to(DEV)[None]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = fn()(coords)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert len(block) == new_ii.shape[0] == block.slots.shape[0] and block.slots.dtype == torch.int64
        assert torch.equal(out, fresh_block(maps, new_ii, new_jj)(coords))
        return new_ii, new_jj

    a_i, a_j = li([0, 1, 2, 2, 4]), li([1, 0, 2, 3, 4])                           # two stereo edges
    ii, jj = step(lambda: block.add(a_i, a_j), a_i, a_j)
    assert sorted(block.slots.tolist()) == [0, 1, 2, 3, 4]
    mask = torch.tensor([True, False, True, False, True], device=DEV)
    ii, jj = step(lambda: block[mask, 3], ii[mask], jj[mask])
    assert block.slots.tolist() == [0, 2, 4]
    b_i, b_j = li([3, 3, 1]), li([0, 3, 4])
    ii, jj = step(lambda: block.add(b_i, b_j), torch.cat([ii, b_i]), torch.cat([jj, b_j]))
    assert block.slots.tolist() == [0, 2, 4, 1, 3, 5] and block.capacity == 6    # the freed slots first, in ascending order
    keep = li([5, 0, 3])
    ii, jj = step(lambda: block[keep], ii[keep], jj[keep])
    assert block.slots.tolist() == [5, 0, 1]
    c_i, c_j = li([4, 0, 1, 2, 3, 0]), li([0, 4, 3, 1, 2, 2])
    ii, jj = step(lambda: block.add(c_i, c_j), torch.cat([ii, c_i]), torch.cat([jj, c_j]))      # 9 edges: the store grows
    assert block.capacity == 12 and block.slots.tolist() == [5, 0, 1, 2, 3, 4, 6, 7, 8] and block.levels[0].shape[0] == 12
    for l in range(LEVELS):
        assert tuple(block.volumes(l).shape) == (9, h, w, h >> l, w >> l)
    ref = V.volume_pyramid(np_(maps).reshape(FRAMES * CAMS, 32, h, w), *planes_of(np_(ii), np_(jj)), LEVELS)
    assert worst_ratio(block.levels, ref, block.slots.tolist(), 32) <= 1.0
    m2 = torch.zeros(9, dtype=torch.bool, device=DEV)
    m2[[1, 8]] = True
    block[m2]                                                                    # a bare mask: one host read, the same result
    assert block.slots.tolist() == [0, 8] and len(block) == 2


def test_the_block_on_a_side_stream_scales_exactly():
    from splat_slam_amd.corr import FusedCorrBlock
    h, w = 12, 16
    maps = maps_of(h, w, 32, True)            # multiples of 1/8: no level value is an fp16 subnormal, where a scaling would not commute
    ii, jj = li([0, 2, 3]), li([1, 2, 0])
    base = FusedCorrBlock(maps, capacity=3).add(ii, jj)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        twice = FusedCorrBlock(maps * 2, capacity=4).add(ii, jj)
        vols = [twice.volumes(l) for l in range(LEVELS)]
    side.synchronize()
    for l in range(LEVELS):
        assert torch.equal(vols[l], base.volumes(l) * 4) and vols[l].any()


def test_the_graph_keeps_one_fused_block_in_step_with_its_edges():
    from splat_slam_amd.corr import CorrBlock, FusedCorrBlock
    from splat_slam_amd.factor_graph import FactorGraph
    v = make_video()
    g = FactorGraph(v, stub, device=DEV, corr_impl="volume_fused", max_factors=30)

    def check():
        assert isinstance(g.corr, FusedCorrBlock) and len(g.corr) == g.ii.shape[0] > 0
        coords = g._motion()[0]
        got = g.corr(coords)
        assert torch.equal(got, fresh_block(v.fmaps, g.ii, g.jj)(coords)) and got.any()
        assert tuple(got.shape) == (1, g.ii.shape[0], 4 * 49, 6, 8)
        assert torch.isfinite(v.poses).all() and torch.isfinite(v.disps).all()

    g.add_neighborhood_factors(0, 6, r=2)
    check()
    assert g.corr.capacity == 46
    g.update(t0=1)
    check()
    g.add_factors([0, 1, 5], [1, 0, 0])                                           # two duplicates and one new edge
    check()
    g.add_proximity_factors(t0=2, t1=0, rad=2, nms=2, beta=0.25, thresh=16.0, remove=True)      # past max_factors: old edges go inactive
    assert g.ii_inac.shape[0] > 0
    check()
    g.update(t0=1)
    check()
    g.rm_factors((g.ii == 4) | (g.jj == 9), store=True)
    check()
    g.add_factors([11, 9], [9, 11])                                              # (dropped where the graph has them already)
    check()
    g.rm_keyframe(10)                                                            # frame 11 takes the place of frame 10
    assert not ((g.ii == 11) | (g.jj == 11)).any() and ((g.ii == 10) | (g.jj == 10)).any()
    check()
    g.update(t0=1)
    check()
    assert g.corr.capacity == 46                                                 # never grown: no volume was ever moved
    g.clear_edges()
    assert g.corr is None
    d = FactorGraph(make_video(), stub, device=DEV)
    d.add_neighborhood_factors(0, 4, r=2)
    assert d.corr_impl == "volume" and isinstance(d.corr, CorrBlock)
