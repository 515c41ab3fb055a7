"""The list hint (SgrWorkspace.max_list_hint) is a performance choice only: every hint gives the same bits.

The hint picks whether K3 scatters or K2 block 0 files the overflow list, launch order vs band mapping of the super
tiles (and so which K2 block zeroes the tile counters), and the light / mid / heavy sort build of the tile kernels.  Each tile's
actual list length then picks its sort mode (registers, register bitonic, LDS, in-HBM) and the backward's pixels per wave.  The scenes
of tests/list_scenes.py pin the list length of every 8x8 tile exactly (proven on the CPU by tests/test_list_scenes_cpu.py), so every
(hint, length) pair below is the one it claims; the header and the tile ranges of each forward confirm it on the GPU.
The hint also picks K1's view parts (k1_parts_for), but only for maps of 768 segments (196 608 Gaussians) and more: these scenes of at
most 4 097 Gaussians always take four parts, so that choice is outside this file's reach
(tests/test_gpu_fused.py::test_two_view_parts_per_segment_on_a_dense_map_give_the_same_bits_as_one covers it).
"""
import pytest
import torch

import list_scenes as LS
from gpu_utils import HintDriver, assert_bitwise, rel_linf, run_hip, run_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every blanket length runs under every one of these, which includes the mismatches named by the design: hint 1 with L = 4097 (light
# build, no K3, band mapping, HBM sort on every tile), hint 257 with L = 1025 (a mid build one class short) and hint 4096 with L = 1
# (the heavy build on one-entry lists)
HINTS = (0, 1, 64, 65, 256, 257, 768, 769, 1536, 1537, 4096, 1 << 20)
REUSE_HINTS = (0, 64, 300, 1, 2000, 0)

BLANKETS = [(W, H, L) for W, H in LS.IMAGES for L in LS.BLANKET_LENGTHS]
_cache = {}


def _weights(H, W, seed=5):
    g = torch.Generator().manual_seed(seed)
    wc = torch.randn(3, H, W, generator=g, dtype=torch.float64).float().double()
    wd = torch.randn(1, H, W, generator=g, dtype=torch.float64).float().double()
    return wc, wd


def _scene(key):
    """(inputs, settings, expected [gy, gx] lengths, driver, H = 0 result) of a blanket (W, H, L) or "mixed"."""
    if key not in _cache:
        if key == "mixed":
            inp, s, expect = LS.mixed_scene()
        else:
            W, H, L = key
            inp, s = LS.blanket_scene(L, W, H)
            expect = torch.full(((H + 7) // 8, (W + 7) // 8), L, dtype=torch.int64)
        wc, wd = _weights(int(s.image_height), int(s.image_width))
        drv = HintDriver(inp, s, wc, wd, capacity=2 * int(expect.sum()) + 4096, dev=DEV)
        base = drv.run(0)
        _check_header(base, expect, "hint 0")
        _cache[key] = (inp, s, expect, drv, base, wc, wd)
    return _cache[key]


def _check_header(res, expect, what):
    w = res["header"]
    assert w[1] == 0, (what, "overflow word", w[1])
    assert w[10] == int(expect.max()), (what, "longest list", w[10], int(expect.max()))
    assert w[9] == int(expect.sum()), (what, "pairs binned", w[9], int(expect.sum()))
    assert torch.equal(res["tile_lengths"], expect), (what, "per-tile lengths", res["tile_lengths"], expect)
    assert w[3] == res["radii"].numel() and bool((res["radii"] > 0).all()), (what, "visible", w[3])


@pytest.mark.parametrize("W,H,L", BLANKETS, ids=["%dx%d-L%d" % t for t in BLANKETS])
def test_every_hint_gives_the_same_bits(W, H, L):
    _, _, expect, drv, base, _, _ = _scene((W, H, L))
    for h in HINTS[1:]:
        r = drv.run(h)
        _check_header(r, expect, "hint %d" % h)
        assert_bitwise(r, base, "L=%d %dx%d hint %d vs 0" % (L, W, H, h))


def test_every_hint_gives_the_same_bits_mixed():
    _, _, expect, drv, base, _, _ = _scene("mixed")
    for h in HINTS[1:]:
        r = drv.run(h)
        _check_header(r, expect, "hint %d" % h)
        assert_bitwise(r, base, "mixed hint %d vs 0" % h)


@pytest.mark.parametrize("key", [(72, 40, 1025), (44, 20, 4097), "mixed"], ids=str)
def test_saved_block_reuse_across_hint_classes(key):
    """One saved block through forwards (each with its backward) whose hints move between classes: counters_clean = 0 on the first
    (the block is fresh), 1 on every later one (the previous forward on this block completed -- the documented contract).  Who zeroes
    the tile counters flips between K2 block 0 (band mapping) and block 3 (launch order) from one forward to the next."""
    _, _, expect, drv, base, _, _ = _scene(key)
    blk = drv.block()
    for i, h in enumerate(REUSE_HINTS):
        r = drv.run(h, block=blk, counters_clean=0 if i == 0 else 1)
        _check_header(r, expect, "re-used block, step %d hint %d" % (i, h))
        fresh = drv.run(h)
        assert_bitwise(r, fresh, "%s: re-used block step %d (hint %d) vs a fresh block" % (key, i, h))
        assert_bitwise(r, base, "%s: re-used block step %d (hint %d) vs hint 0" % (key, i, h))


def test_dropin_stateful_hint_sequence():
    """GaussianRasterizer keeps a process-wide longest-list value that decays by 7/8 per forward: a light scene after a 4097-entry
    one runs on a stale, far too high hint, and a 513-entry one after a light one on a far too low hint."""
    for key in [(72, 40, 16), (72, 40, 4097), (72, 40, 16), (72, 40, 513), (44, 20, 4097), (44, 20, 1)]:
        inp, s, _, drv, _, wc, wd = _scene(key)
        ref = drv.run(0, backward="views")
        out, grads = run_hip(inp, s, wc, wd, dev=DEV)
        got = dict(color=out[0], radii=out[1], depth=out[2], opacity=out[3], n_touched=out[4],
                   d_means3D=grads["means3D"], d_means2D=grads["means2D"], d_opacities=grads["opacities"].reshape(-1),
                   d_shs=grads["shs"], d_scales=grads["scales"], d_rotations=grads["rotations"],
                   d_tau=torch.cat([grads["rho"].reshape(3), grads["theta"].reshape(3)]))
        assert_bitwise(got, ref, "drop-in %s" % (key,))


ANCHOR = BLANKETS + ["mixed"]


@pytest.mark.parametrize("key", ANCHOR, ids=str)
def test_oracle_anchor(key):
    """The hint-0 run (and by the tests above every hint) against the fp64 oracle on the knife-free scenes: radii and n_touched exact,
    images and every gradient within 1e-4 relative L-inf -- no thinning, no nudging, no depth keys handed over."""
    inp, s, _, _, base, wc, wd = _scene(key)
    ref, rg = run_oracle(inp, s, wc, wd)
    assert torch.equal(base["radii"], ref[1]), "radii"
    assert torch.equal(base["n_touched"].long(), ref[4].long()), "n_touched"
    errs = {n: rel_linf(base[n].reshape(-1), ref[i].reshape(-1)) for i, n in ((0, "color"), (2, "depth"), (3, "opacity"))}
    for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
        a, b = base["d_" + k].reshape(-1), rg[k].reshape(-1)
        if k == "means2D":
            a, b = base["d_means2D"][:, :2].reshape(-1), rg[k][:, :2].reshape(-1)
        errs[k] = rel_linf(a, b)
    # the rotation gradient of an isotropic splat is zero by symmetry (fp64: ~1e-30; fp32: rounding noise): relative to ITSELF the
    # measure is meaningless, so it is taken against what the same dL/dSigma gives a scale, dL/dq ~ dL/ds * s
    floor = rg["scales"].abs().max().item() * inp["scales"].abs().max().item()
    errs["rotations"] = (base["d_rotations"].double() - rg["rotations"]).abs().max().item() / max(rg["rotations"].abs().max().item(), floor)
    errs["tau"] = rel_linf(base["d_tau"], torch.cat([rg["rho"].reshape(3), rg["theta"].reshape(3)]))
    bad = {k: v for k, v in errs.items() if not v < 1e-4}
    assert not bad, (key, bad)


# ---- the batched mapping path: FusedMappingLoop (sgr_map_step) with the hint forced ------------------------------------------------
# 64 and 700: the light build, which runs forward + loss + backward of a tile in ONE kernel (blend_can_fuse; 64 also maps the super
# tiles by band), 1200: the mid build, 3000: the heavy build -- both with the separate forward and backward tile kernels
BATCH_HINTS = ((64, 0), (700, 2), (1200, 3), (3000, 4))      # (hint, FusedMappingLoop._build_class())
BATCH_REUSE = (64, 3000, 700, 1200, 64)
BATCH_VIEWS = 3


def _batched_loop(key):
    """A FusedMappingLoop over the scene as a map, with BATCH_VIEWS cameras at the scene's pose (same lists; own ground truth and
    exposure each), and the expected [gy, gx] lengths."""
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.fused import FusedMappingLoop
    inp, s, expect, _, _, _, _ = _scene(key)
    W, H = int(s.image_width), int(s.image_height)
    f = W / (2.0 * s.tanfovx)
    intr = dict(W=W, H=H, fx=f, fy=f, cx=W / 2.0 + 0.25, cy=H / 2.0 + 0.25)
    o = inp["opacities"].reshape(-1, 1)
    params = dict(xyz=inp["means3D"].float().to(DEV), f_dc=inp["shs"].float().to(DEV), opacity=torch.log(o / (1 - o)).float().to(DEV),
                  scaling=torch.log(inp["scales"]).float().to(DEV), rotation=inp["rotations"].float().to(DEV))
    g = torch.Generator().manual_seed(11)
    cams = []
    for k in range(BATCH_VIEWS):
        color = torch.rand(3, H, W, generator=g).to(DEV)
        depth = (3.0 + torch.rand(H, W, generator=g)).to(DEV)
        c = syn.make_camera(k, torch.eye(4), intr, color, depth, DEV)
        c.exposure_a.data.fill_(0.02 * k)
        cams.append(c)
    loop = FusedMappingLoop(syn.DEFAULT_CONFIG, device=DEV)
    loop.gaussians = syn.model_from_parameters(params, device=DEV)
    loop.viewpoints = {c.uid: c for c in cams}
    loop.current_window = list(range(BATCH_VIEWS))
    loop.build_keyframe_optimizers()
    return loop, cams, expect


def _batched_run(loop, cams, hint):
    loop._max_list = lambda: hint          # the instance override: every workspace this loop builds carries `hint`
    loop._hint_changed()                   # ... and so do the launch structs it cached (patched, counters_clean kept)
    loop._ensure_state()
    loop._activate()
    gm = loop.gaussians
    # a views-only pass ADDS to the gradient sinks (like autograd's .grad; an Adam step is what leaves them zero): start every run
    # from the state a fresh loop and every Adam step leave -- zero sinks that the loop knows to be zero -- and zero statistics
    loop._acc["flat"].zero_()
    loop._acc_clean = True
    gm.xyz_gradient_accum.zero_()
    gm.denom.zero_()
    gm.max_radii2D.zero_()
    if loop._exp is not None:
        loop._exp.grad.zero_()
    loop._run_views(cams, stats=True)
    torch.cuda.synchronize()
    return dict(flat=loop._acc["flat"].clone(), loss=torch.cat([loop._views[c.uid].loss for c in cams]).clone(),
                exp=loop._exp.grad[:len(cams)].clone(), nt=torch.stack([loop._views[c.uid].n_touched for c in cams]).clone(),
                accum=gm.xyz_gradient_accum.clone(), denom=gm.denom.clone(), maxr=gm.max_radii2D.clone())


@pytest.mark.parametrize("key", ["mixed", (72, 40, 1025), (72, 40, 513)], ids=str)
def test_batched_mapping_path_every_build_gives_the_same_bits(key):
    """sgr_map_step over BATCH_VIEWS views under the fused light, separate mid and separate heavy builds: per-view losses, exposure
    gradients, n_touched, the accumulated gradient buffer and the densification statistics have the same bits.  Then ONE loop walks
    the hints through the classes on its saved blocks (counters_clean = 1 after the first forward, the hint patched into the cached
    launch structs -- what a session does when its longest list moves) and must give the same bits at every step."""
    ref = None
    for hint, cls in BATCH_HINTS:
        loop, cams, expect = _batched_loop(key)
        r = _batched_run(loop, cams, hint)
        assert loop._build_class() == cls, (hint, loop._build_class())
        assert loop._list_hint and set(loop._list_hint.values()) == {int(expect.max())}, loop._list_hint
        if ref is None:
            ref = r
            assert r["flat"].abs().max() > 0 and r["denom"].min() == BATCH_VIEWS
            continue
        for k in ref:
            assert torch.equal(r[k], ref[k]), (key, "hint %d" % hint, k, (r[k].double() - ref[k].double()).abs().max().item())
    loop, cams, _ = _batched_loop(key)
    for i, hint in enumerate(BATCH_REUSE):
        r = _batched_run(loop, cams, hint)
        for k in ref:
            assert torch.equal(r[k], ref[k]), (key, "re-used loop, step %d hint %d" % (i, hint), k,
                                               (r[k].double() - ref[k].double()).abs().max().item())
