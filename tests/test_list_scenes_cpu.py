"""The scenes of tests/list_scenes.py are what they claim, proven with the fp64 oracle before any GPU run: exact per-8x8-bin list
lengths, no knife edge of any kind, distinct fp32 depths, and (blanket scenes) a walk that either never or always terminates."""
import pytest
import torch

import list_scenes as LS
from oracle import raster_oracle as O

SCENES = [(W, H, L) for W, H in LS.IMAGES for L in LS.BLANKET_LENGTHS]


def _check(inp, s, expect):
    got = LS.bin_list_lengths(inp, s)
    assert torch.equal(got, expect), (got, expect)
    assert LS.depths_distinct_fp32(inp, s), "two visible Gaussians share an fp32 depth"
    d = O.knife_edge_gaussians(inp["means3D"], inp["opacities"], shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"],
                               settings=s, detail=True)
    assert d["alpha"].numel() == 0 and d["geometric"].numel() == 0, d
    k = O.knife_edge_gaussians(inp["means3D"], inp["opacities"], shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"],
                               settings=s)
    assert k.numel() == 0, k


def _final_T(inp, s):
    out = O.rasterize(inp["means3D"], None, inp["opacities"], shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"],
                      settings=s)
    return 1.0 - out[3].reshape(-1), out


@pytest.mark.parametrize("W,H,L", SCENES, ids=["%dx%d-L%d" % t for t in SCENES])
def test_blanket_scene(W, H, L):
    inp, s = LS.blanket_scene(L, W, H)
    assert inp["means3D"].shape[0] == L
    gy, gx = (H + 7) // 8, (W + 7) // 8
    _check(inp, s, torch.full((gy, gx), L, dtype=torch.int64))
    assert bool((inp["opacities"] >= 0.006).all())
    # every splat covers every pixel almost uniformly: all pixels terminate on the same splat or none does
    T, out = _final_T(inp, s)
    stopped = T < 2 * O.T_EPS
    assert bool(stopped.all()) or not bool(stopped.any()), "termination differs between pixels"
    assert bool((out[1] > 0).all())


def test_blanket_lengths_cover_both_sides_of_termination():
    ends = {}
    for L in (256, 257, 512, 513, 4097):
        T, _ = _final_T(*LS.blanket_scene(L, 72, 40))
        ends[L] = bool((T < 2 * O.T_EPS).all())
    assert not ends[256] and not ends[257] and ends[4097], ends


def test_mixed_scene():
    inp, s, expect = LS.mixed_scene()
    _check(inp, s, expect)
    vals = expect.flatten()
    for lo, hi in LS.MIXED_REGIMES:
        assert bool(((vals >= lo) & (vals <= hi)).any()), (lo, hi)
    T, out = _final_T(inp, s)
    assert float(T.min()) > 2 * O.T_EPS          # no walk of this scene terminates
    assert bool((out[1] > 0).all())
