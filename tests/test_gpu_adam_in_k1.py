"""-m gpu: SGR_OPT_ADAM_IN_K1.  Inside sgr_map_run the optimiser step of every iteration but the last is run by the blocks of the NEXT
iteration's forward preprocess (K1) for their own 256 Gaussians instead of being a launch of its own.  Same arithmetic, same order:
a FusedMappingLoop.map() span run from identical state with the switch off and on must end in the same bits, everywhere.

Shapes: `tiny` images (96x64); N = 700 (three segments, the last partial), 200 (one partial segment), 256 (exactly one); 3 window views
+ 2 picks per iteration from a pool of 4 (the picks -- their radii, the exposure row of the first pick's keyframe -- change between
iterations); spans of 1, 2 and 5 iterations (none, one, several carried steps); clean and dirty gradient sinks at the span's start
(gather_adam MODE 2 / MODE 1 in the first step); window view 2 looks away from the room (sees no Gaussian).  Maps this small
take the carried form at level 2 of the option only (level 1, the default, leaves them their K1 view parts); one case runs a map of
2048 segments, where level 1 takes it."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOW, POOL = 3, 4
PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


@functools.lru_cache(maxsize=None)
def _scene(n):
    from splat_slam_amd import synthetic as syn
    params = syn.room_parameters(n, seed=11, device=DEV)
    params["scaling"] = params["scaling"] + 1.2          # make the splats a few pixels wide at 96x64
    cams = syn.make_views(params, WINDOW + POOL, syn.INTRINSICS["tiny"], DEV, seed=11)
    return syn, params, cams


def _fresh_cams(syn, cams):
    out = []
    for c in cams:
        n = syn.make_camera(c.uid, torch.eye(4), syn.INTRINSICS["tiny"], c.original_image.clone(), c.depth.clone(), DEV)
        if c.uid == 2:       # the whole room lies behind this camera
            n.update_RT(torch.eye(3, device=DEV), torch.tensor([0.0, 0.0, -100.0], device=DEV))
        else:
            n.update_RT(c.R, c.T)
        out.append(n)
    return out


def _profile_read(lib, nat):
    ms, cnt = (C.c_float * nat.SGR_PROFILE_KINDS)(), (C.c_int64 * nat.SGR_PROFILE_KINDS)()
    lib.sgr_profile_read(ms, cnt)
    return [int(c) for c in cnt]


def _run(n_gauss, iters, dirty, switch, fused_blend=1, overflow=False):
    """One span of `iters` iterations from a fixed state; returns (every tensor the span leaves behind, profile records per kind,
    replayed transactions)."""
    import numpy as np
    from splat_slam_amd import _native as nat
    from splat_slam_amd.fused import FusedMappingLoop
    syn, params, cams0 = _scene(n_gauss)
    cams = _fresh_cams(syn, cams0)
    lib = nat.lib()
    lib.sgr_set_option(nat.SGR_OPT_ADAM_IN_K1, switch)
    lib.sgr_set_option(nat.SGR_OPT_FUSED_BLEND, fused_blend)
    try:
        assert lib.sgr_get_option(nat.SGR_OPT_ADAM_IN_K1) == switch and switch in (0, 1, 2)
        f = FusedMappingLoop(syn.DEFAULT_CONFIG, device=DEV)
        f.gaussians = syn.model_from_parameters(params, device=DEV)
        f.viewpoints = {c.uid: c for c in cams}
        f.current_window = list(range(WINDOW))
        f.build_keyframe_optimizers()
        f.iteration_count = 50                    # 149 regular iterations follow: map() issues them as ONE sgr_map_run
        torch.manual_seed(3)
        np.random.seed(3)
        for c in cams:                            # (the buffers of a pool camera no iteration picks stay defined)
            f._view(c)._ibuf.zero_()
        if overflow:                              # the pattern of the never-drop tests: measured counts first, then a capacity no view fits
            f.map(f.current_window, iters=2)
            torch.cuda.synchronize()
            assert max(h[0] for h in f._pair_hint.values()) > 256
            for vb in f._views.values():
                vb.pairs = 1
            f.capacity_floor = 256
            f._cap = 256
            f._views_dirty()
        if dirty:                                 # a view rendered without an optimiser step leaves its gradients in the sinks
            f._ensure_state()
            f._activate()
            f._run_views([cams[WINDOW]])
            assert not f._acc_clean
            f._has_stale = lambda: False          # ... and the span starts on them: grads_clean = 0, the first step adds them (MODE 1)
        ev, rp = f.overflow_events, f.replayed_transactions
        torch.cuda.synchronize()
        _profile_read(lib, nat)
        lib.sgr_profile_enable((1 << nat.SGR_PROFILE_KINDS) - 1)
        f.map(f.current_window, iters=iters)
        torch.cuda.synchronize()
        records = _profile_read(lib, nat)
        lib.sgr_profile_enable(0)
        assert f._acc_clean and f.iteration_count == 50 + iters + (2 if overflow else 0)
        if overflow:
            assert f.overflow_events > ev and f.replayed_transactions > rp
        gm = f.gaussians
        out = {k: getattr(gm, k).detach().clone() for k in PARAMS}
        for g in gm.optimizer.param_groups:
            st = gm.optimizer.state.get(g["params"][0])
            if st and g["params"][0].numel():
                out["m_" + g["name"]], out["v_" + g["name"]] = st["exp_avg"].detach().clone(), st["exp_avg_sq"].detach().clone()
                out["step_" + g["name"]] = torch.tensor(float(st["step"]))
        for k in ("act_scale", "act_rot", "act_opac"):
            out[k] = f._acc[k].clone()
        out["accum"], out["denom"], out["maxr"] = gm.xyz_gradient_accum.clone(), gm.denom.clone(), gm.max_radii2D.clone()
        out["exp_param"], out["exp_m"], out["exp_v"], out["exp_step"] = f._exp.param.clone(), f._exp.m.clone(), f._exp.v.clone(), f._exp.step.clone()
        for c in cams:
            vb = f._views[c.uid]
            out["radii_%d" % c.uid], out["loss_%d" % c.uid] = vb.radii.clone(), vb.loss.clone()
            if c.uid < WINDOW:
                out["n_touched_%d" % c.uid] = vb.n_touched.clone()
        out["occ"] = torch.stack([v for _, v in sorted(f.occ_aware_visibility.items())]).clone()
        out["last_used"] = torch.tensor([c.uid for c in f.last_used])
        return out, records, f.replayed_transactions - rp
    finally:
        lib.sgr_profile_enable(0)
        lib.sgr_set_option(nat.SGR_OPT_ADAM_IN_K1, 1)
        lib.sgr_set_option(nat.SGR_OPT_FUSED_BLEND, 1)


def _compare(off, on):
    assert sorted(off) == sorted(on)
    bad = [(k, float((off[k].double() - on[k].double()).abs().max())) for k in off if not torch.equal(off[k], on[k])]
    assert not bad, bad


CASES = [(700, 1, 0), (700, 1, 1), (700, 2, 0), (700, 2, 1), (700, 5, 0), (700, 5, 1), (200, 5, 0), (200, 2, 1), (256, 5, 1), (256, 2, 0)]


@pytest.mark.parametrize("n_gauss,iters,dirty", CASES)
def test_span_ends_in_the_same_bits_with_the_step_in_k1_and_as_its_own_launch(n_gauss, iters, dirty):
    """... and the carried form was really taken: with event pairs armed on every kind a span of n iterations records n launches of
    kind 0 either way (plus one per forward-only probe render that sizes the capacity for a camera new to the loop: those are
    the only launches of kind 4 while the tile kernels run fused); kind 6 records the dense backward of every iteration and every
    optimiser pass that is a launch of its own: 2 n with the switch off, n + 1 with it on (only the last step of the run is launched)."""
    off, rec_off, _ = _run(n_gauss, iters, dirty, 0)
    on, rec_on, _ = _run(n_gauss, iters, dirty, 2)
    _compare(off, on)
    assert off["radii_2"].max().item() == 0 and off["radii_0"].max().item() > 0          # the empty view is empty, the others are not
    assert float(off["exp_step"].max()) > 0 and float(off["accum"].abs().max()) > 0
    assert rec_off[0] - rec_off[4] == iters and rec_on[0] - rec_on[4] == iters and rec_on[3] == iters, (rec_off, rec_on)
    assert rec_off[6] == 2 * iters and rec_on[6] == iters + 1, (rec_off, rec_on)


def test_span_with_the_two_tile_kernels_launched_separately():
    """SGR_OPT_FUSED_BLEND = 0: blend forward, loss and blend backward as separate launches between K1 and the dense backward."""
    off, rec_off, _ = _run(700, 5, 0, 0, fused_blend=0)
    on, rec_on, _ = _run(700, 5, 0, 2, fused_blend=0)
    _compare(off, on)
    # (kind 4: the 5 iterations' blend_fwd + the probe renders; kind 5: blend_bwd of the 5 iterations)
    assert rec_off[6] == 10 and rec_on[6] == 6 and rec_on[0] == rec_on[4] >= 5 and rec_on[5] == 5 and rec_on[3] == 0, (rec_off, rec_on)
    assert rec_off[0] == rec_on[0]


def test_span_whose_forwards_run_out_of_pair_capacity_is_replayed_to_the_same_bits():
    """The capacity estimate is too small: forwards of the span truncate, the views take no part in their steps (header.overflow, which
    the carried step reads as the launched one does: the value its own iteration's K2 wrote), the closing check puts the state back,
    grows the workspace and issues the span again.  The end state is that of the switch-off run."""
    off, _, rp_off = _run(700, 5, 0, 0, overflow=True)
    on, _, rp_on = _run(700, 5, 0, 2, overflow=True)
    assert rp_off >= 1 and rp_on == rp_off
    _compare(off, on)


def test_default_level_takes_the_carried_form_on_a_map_of_2048_segments():
    """Level 1 (the default): K1 of a map of >= 2048 segments has one block per segment whatever its lists, so the carried form is
    taken; N = 2048 * 256 - 100 (the last segment partial).  Same bits as level 0, and 3 + 1 records of kind 6 instead of 6."""
    n = 2048 * 256 - 100
    off, rec_off, _ = _run(n, 3, 0, 0)
    on, rec_on, _ = _run(n, 3, 0, 1)
    _compare(off, on)
    assert rec_off[6] == 6 and rec_on[6] == 4 and rec_on[3] == 3, (rec_off, rec_on)
