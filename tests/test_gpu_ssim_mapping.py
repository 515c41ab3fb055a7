"""-m gpu: the mapping loss with the SSIM term (`ssim_loss: True`, thirdparty/monogs/utils/slam_utils.py:80-105) on the HIP kernels --
the standalone loss (losses.get_loss_mapping_ssim_native, sgr_mapping_loss_ssim) against the reference's golden vectors and fp64
autograd, and FusedMappingLoop(native_ssim=True) (sgr_map_step_ssim / sgr_map_run_ssim) against the autograd MappingLoop, itself
and the default loop."""
import copy
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation")
LR = {"_xyz": 9.6e-4, "_features_dc": 2.5e-3, "_opacity": 0.05, "_scaling": 6e-3, "_rotation": 1e-3}


def _cfg(alpha=0.95, thr=0.01, lam=0.2, ssim=True):
    return {"Training": {"alpha": alpha, "rgb_boundary_threshold": thr, "ssim_loss": ssim}, "opt_params": {"lambda_dssim": lam}}


def _view(gt, gtd, a=None, b=None):
    return types.SimpleNamespace(original_image=gt, depth=gtd, exposure_a=a, exposure_b=b)


def _native(cfg, image, depth, vp, initialization=False, up=1.0):
    from splat_slam_amd.losses import get_loss_mapping_ssim_native
    image = image.detach().clone().requires_grad_(True)
    depth = depth.detach().clone().requires_grad_(True)
    for t in (vp.exposure_a, vp.exposure_b):
        if t is not None:
            t.grad = None
    loss = get_loss_mapping_ssim_native(cfg, image, depth, vp, None, initialization=initialization)
    (loss * up).backward()
    a, b = vp.exposure_a, vp.exposure_b
    return (loss.detach(), image.grad, depth.grad, None if (initialization or a is None) else a.grad.clone(),
            None if (initialization or b is None) else b.grad.clone())


def _fp64(cfg, image, depth, gt, gtd, a, b, initialization=False, up=1.0):
    """slam_utils.py:71-105 (ssim_loss: True) through autograd in fp64, losses.ssim for loss_utils.ssim."""
    from splat_slam_amd.losses import ssim
    tr, lam = cfg["Training"], cfg["opt_params"]["lambda_dssim"]
    image = image.double().requires_grad_(True)
    depth = depth.double().requires_grad_(True)
    gt, gtd = gt.double(), gtd.double()
    a = None if (a is None or initialization) else a.detach().double().requires_grad_(True)
    b = None if (b is None or initialization) else b.detach().double().requires_grad_(True)
    x = image if a is None else torch.exp(a) * image + b
    _, h, w = gt.shape
    m = (gt.sum(dim=0) > tr["rgb_boundary_threshold"]).view(1, h, w)
    rgb = (1 - lam) * torch.abs(x * m - gt * m) + lam * (1 - ssim(x, gt))
    dm = (gtd > 0.01).view(*depth.shape)
    loss = tr["alpha"] * rgb.mean() + (1 - tr["alpha"]) * torch.abs(depth * dm - gtd * dm).mean()
    (loss * up).backward()
    return loss.detach(), image.grad, depth.grad, None if a is None else a.grad, None if b is None else b.grad, x.detach()


def test_reference_golden_vectors():
    """The reference's `ssim_loss: True` mapping loss (tests/golden/reference_ssim.npz) within the bounds the torch formulation meets
    (tests/test_gpu_ssim.py::test_reference_golden_ssim_and_the_ssim_mapping_loss)."""
    S = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_ssim.npz"))
    t = lambda k: torch.from_numpy(np.asarray(S[k])).float().to(DEV)
    a = torch.tensor([0.05], device=DEV, requires_grad=True)
    b = torch.tensor([-0.02], device=DEV, requires_grad=True)
    loss, d_img, d_dep, da, db = _native(_cfg(alpha=0.8, thr=0.01, lam=0.2), t("image"), t("depth"), _view(t("gt"), S["gtd"], a, b))
    assert abs(loss.item() - float(S["loss"])) < 2e-7
    assert torch.allclose(d_img.cpu(), torch.from_numpy(S["dimage"]), rtol=0, atol=2e-8)
    assert torch.allclose(d_dep.cpu(), torch.from_numpy(S["ddepth"]), rtol=0, atol=1e-9)
    assert abs(da.item() - float(S["da"])) < 1e-6 and abs(db.item() - float(S["db"])) < 1e-6


def _inputs(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    gt[:, : H // 5] *= 0.002                                              # a band below the rgb boundary threshold
    image = (0.7 * gt + 0.3 * torch.rand(3, H, W, generator=g)).clamp(0, 1)
    gtd = torch.rand(1, H, W, generator=g) * 4
    gtd[:, :, : W // 6] = 0.0                                             # no depth there
    depth = gtd + 0.2 * torch.randn(1, H, W, generator=g)
    return [t.to(DEV).contiguous() for t in (image, depth, gt, gtd)]


@pytest.mark.parametrize("mode", ["exposure", "identity", "initialization"])
@pytest.mark.parametrize("size", [(37, 53), (480, 640), (7, 5)])
def test_loss_and_gradients_match_fp64_autograd(size, mode):
    H, W = size
    image, depth, gt, gtd = _inputs(H, W, seed=H + W)
    if mode == "identity":
        a, b = torch.zeros(1, device=DEV, requires_grad=True), torch.zeros(1, device=DEV, requires_grad=True)
    else:
        a, b = torch.tensor([0.08], device=DEV, requires_grad=True), torch.tensor([-0.03], device=DEV, requires_grad=True)
    init = mode == "initialization"
    cfg, up = _cfg(), 0.6
    loss, d_img, d_dep, da, db = _native(cfg, image, depth, _view(gt, gtd[0], a, b), initialization=init, up=up)
    rl, r_img, r_dep, ra, rb, x = _fp64(cfg, image, depth, gt, gtd[0][None], a, b, initialization=init, up=up)
    assert abs(loss.double().item() - rl.item()) <= 5e-6, (loss.item(), rl.item())
    # (a residual within fp32 rounding of 0 may take the other sign of the L1 term: those pixels are left out)
    m = (gt.double().sum(0) > 0.01)[None]
    near = (m & ((x - gt.double()).abs() < 1e-5)).expand_as(r_img)
    err = (d_img.double() - r_img).abs()[~near]
    assert err.max().item() <= 2e-3 * r_img.abs().max().item(), (err.max().item(), r_img.abs().max().item())
    dnear = ((gtd > 0.01) & ((depth - gtd).abs() < 1e-5)).view_as(r_dep)
    assert torch.allclose(d_dep.double()[~dnear], r_dep[~dnear], rtol=1e-6, atol=0)
    if init:
        assert da is None and db is None
    else:
        scale = (r_img.abs() * image.abs()).sum().item() + 1e-30
        assert abs(da.item() - ra.item()) <= 2e-3 * scale, (da.item(), ra.item())
        assert abs(db.item() - rb.item()) <= 2e-3 * r_img.abs().sum().item(), (db.item(), rb.item())


def test_equal_images_give_no_ssim_gradient():
    """x == gt: SSIM is 1 and its gradient exactly 0 (the regrouped forms), so only the L1 (sign 0) and depth terms remain."""
    image, depth, gt, gtd = _inputs(48, 80, seed=3)
    a, b = torch.zeros(1, device=DEV, requires_grad=True), torch.zeros(1, device=DEV, requires_grad=True)
    loss, d_img, d_dep, da, db = _native(_cfg(), gt.clone(), depth, _view(gt, gtd[0], a, b))
    assert torch.count_nonzero(d_img).item() == 0 and da.item() == 0.0 and db.item() == 0.0
    dl = 0.05 * ((depth - gtd).abs() * (gtd > 0.01)).mean().item()
    assert abs(loss.item() - dl) <= 1e-5 * dl + 1e-9


def test_standalone_loss_is_bitwise_reproducible():
    image, depth, gt, gtd = _inputs(480, 640, seed=9)
    a, b = torch.tensor([0.1], device=DEV, requires_grad=True), torch.tensor([0.02], device=DEV, requires_grad=True)
    r1 = _native(_cfg(), image, depth, _view(gt, gtd[0], a, b), up=0.3)
    r2 = _native(_cfg(), image, depth, _view(gt, gtd[0], a, b), up=0.3)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ the fused loop
def _scene(n=2500, views=6, seed=11, intr="tiny", add=1.2):
    from splat_slam_amd import synthetic as syn
    params = syn.room_parameters(n, seed=seed, device=DEV)
    params["scaling"] = params["scaling"] + add
    cams = syn.make_views(params, views, syn.INTRINSICS[intr], DEV, seed=seed)
    return syn, params, cams


def _fresh_cams(syn, cams, intr="tiny"):
    out = []
    for c in cams:
        n = syn.make_camera(c.uid, torch.eye(4), syn.INTRINSICS[intr], c.original_image, c.depth, DEV)
        n.update_RT(c.R, c.T)
        out.append(n)
    return out


def _ssim_config(ssim=True):
    from splat_slam_amd import synthetic as syn
    cfg = copy.deepcopy(syn.DEFAULT_CONFIG)
    cfg["mapping"]["Training"]["ssim_loss"] = ssim
    cfg["mapping"].setdefault("opt_params", {})["lambda_dssim"] = 0.2
    return cfg


def _loop(cls, cfg, syn, params, cams, window, **kw):
    loop = cls(cfg, device=DEV, **kw)
    loop.gaussians = syn.model_from_parameters(params, config=cfg, device=DEV)
    loop.viewpoints = {c.uid: c for c in cams}
    loop.current_window = list(window)
    loop.build_keyframe_optimizers()
    return loop


def _state(loop):
    gm = loop.gaussians
    out = {k: getattr(gm, k).detach().clone() for k in PARAMS}
    st = {g["name"]: gm.optimizer.state[g["params"][0]] for g in gm.optimizer.param_groups}
    out.update({"m_" + k: st[k]["exp_avg"].clone() for k in ("xyz", "f_dc", "opacity", "scaling", "rotation")})
    out.update({"accum": gm.xyz_gradient_accum.clone(), "denom": gm.denom.clone(), "maxr": gm.max_radii2D.clone()})
    out["exposure"] = torch.stack([torch.cat([c.exposure_a.detach().reshape(1), c.exposure_b.detach().reshape(1)])
                                   for _, c in sorted(loop.viewpoints.items())])
    return out


def _assert_tracks(a, f, iters):
    """test_gpu_fused.py::test_fused_loop_tracks_autograd_loop's bounds"""
    for name, step in LR.items():
        d = (getattr(a.gaussians, name).detach() - getattr(f.gaussians, name).detach()).abs()
        frac_bad = (d > 0.02 * step).float().mean().item()
        assert frac_bad < 0.01, (name, frac_bad)
        assert d.max().item() <= iters * 2 * step * 1.01, name
    assert torch.equal(a.gaussians.denom, f.gaussians.denom)
    assert torch.equal(a.gaussians.max_radii2D, f.gaussians.max_radii2D)


def test_native_loop_stays_fused_and_tracks_the_autograd_loop():
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.mapper import MappingLoop
    cfg = _ssim_config()
    cfg["mapping"]["Training"]["init_itr_num"] = 5
    cfg["mapping"]["Training"]["init_gaussian_update"] = 1000
    cfg["mapping"]["Training"]["init_gaussian_reset"] = 1000
    cfg["mapping"]["opt_params"]["densify_grad_threshold"] = 1e9           # (iteration 0 prunes only: the same N in both loops)
    syn, params, cams = _scene()
    # map(iters=4) over a window of four keyframes
    a = _loop(MappingLoop, cfg, syn, params, cams, range(4))
    f = _loop(FusedMappingLoop, cfg, syn, params, _fresh_cams(syn, cams), range(4), native_ssim=True)
    assert not f.autograd_fallback and f.native_ssim
    torch.manual_seed(5)
    a.map(a.current_window, iters=4)
    torch.manual_seed(5)
    f.map(f.current_window, iters=4)
    torch.cuda.synchronize()
    assert f._acc is not None and f._ssim_arena is not None                # the fused state ran
    _assert_tracks(a, f, 4)
    for k in range(1, 4):
        assert torch.allclose(a.viewpoints[k].exposure_a, f.viewpoints[k].exposure_a, atol=2e-3)
        assert torch.allclose(a.viewpoints[k].exposure_b, f.viewpoints[k].exposure_b, atol=2e-3)
    # a short final_refine (random views, exposure of the rendered camera)
    a = _loop(MappingLoop, cfg, syn, params, _fresh_cams(syn, cams), range(4))
    f = _loop(FusedMappingLoop, cfg, syn, params, _fresh_cams(syn, cams), range(4), native_ssim=True)
    for lp in (a, f):
        np.random.seed(3)
        lp.final_refine(iters=4)
    torch.cuda.synchronize()
    _assert_tracks(a, f, 4)
    # a short initialize_map (initialization=True: no exposure)
    a = _loop(MappingLoop, cfg, syn, params, _fresh_cams(syn, cams)[:1], [0])
    f = _loop(FusedMappingLoop, cfg, syn, params, _fresh_cams(syn, cams)[:1], [0], native_ssim=True)
    pa = a.initialize_map(0, a.viewpoints[0])
    pf = f.initialize_map(0, f.viewpoints[0])
    torch.cuda.synchronize()
    assert a.gaussians._xyz.shape == f.gaussians._xyz.shape
    _assert_tracks(a, f, 5)
    assert (pa["render"].detach() - pf["render"]).abs().max().item() < 2e-2


def _run_loop(cfg, syn, params, cams, native, span=True, map_iters=(5, 3), refine=4, cap_hook=None):
    from splat_slam_amd.fused import FusedMappingLoop
    loop = _loop(FusedMappingLoop, cfg, syn, params, cams, range(4), native_ssim=native, span_calls=span)
    loop.iteration_count = 50
    torch.manual_seed(5)
    np.random.seed(5)
    for i, it in enumerate(map_iters):
        if cap_hook is not None and i == 1:
            cap_hook(loop)
        loop.map(loop.current_window, iters=it)
    if refine:
        loop.final_refine(iters=refine)
    torch.cuda.synchronize()
    return loop, _state(loop)


def _assert_equal_states(s1, s2):
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k


def test_fused_ssim_loop_is_bitwise_reproducible_and_span_equals_step():
    syn, params, cams = _scene(n=2500, views=7, seed=13)
    cfg = _ssim_config()
    _, s1 = _run_loop(cfg, syn, params, _fresh_cams(syn, cams), True, span=True, map_iters=(7, 3))
    _, s2 = _run_loop(cfg, syn, params, _fresh_cams(syn, cams), True, span=True, map_iters=(7, 3))
    _assert_equal_states(s1, s2)                                          # 10 map iterations + 4 refine, twice
    _, s3 = _run_loop(cfg, syn, params, _fresh_cams(syn, cams), True, span=False, map_iters=(7, 3))
    _assert_equal_states(s1, s3)                                          # sgr_map_run_ssim == one sgr_map_step_ssim per iteration
    _, s4 = _run_loop(cfg, syn, params, _fresh_cams(syn, cams), False, span=True, map_iters=(7, 3))
    assert not torch.equal(s1["_xyz"], s4["_xyz"])                        # (the autograd loop is another computation)


def test_overflow_replay_is_bit_identical():
    """A forced capacity overflow (test_gpu_fused.py: the capacity pushed to the floor) is replayed at the grown capacity: the same
    parameters, moments, statistics and exposures as a run that never overflowed."""
    syn, params, cams = _scene(n=60000, views=4, seed=5, intr="metric", add=2.0)
    cfg = _ssim_config()

    def squeeze(loop):
        for vb in loop._views.values():
            vb.pairs = 1
        loop._cap = 1 << 16
        loop._views_dirty()

    _, ref = _run_loop(cfg, syn, params, _fresh_cams(syn, cams, "metric"), True, map_iters=(2, 3), refine=0)
    loop, got = _run_loop(cfg, syn, params, _fresh_cams(syn, cams, "metric"), True, map_iters=(2, 3), refine=0, cap_hook=squeeze)
    assert loop.replayed_transactions > 0 and loop.overflow_events > 0
    _assert_equal_states(ref, got)


def test_native_ssim_without_the_ssim_loss_is_the_default_loop():
    syn, params, cams = _scene(n=2500, views=6, seed=17)
    cfg = _ssim_config(ssim=False)
    loop, s1 = _run_loop(cfg, syn, params, _fresh_cams(syn, cams), True)
    assert not loop.native_ssim and loop._ssim_arena is None
    _, s2 = _run_loop(cfg, syn, params, _fresh_cams(syn, cams), False)
    _assert_equal_states(s1, s2)


def test_native_ssim_refuses_several_ranks():
    from splat_slam_amd.fused import FusedMappingLoop
    loop = FusedMappingLoop(_ssim_config(), device=DEV, native_ssim=True)
    with pytest.raises(NotImplementedError, match="one GPU"):
        loop.set_parallel(2, 0, comm=object())
