"""droid_backends on the MI355X against the fp64 restatement (tests/dba_ref.py): ba in its three modes, the singular case,
convergence, reproducibility, the absence of host synchronisation, the frame geometry functions and a backend-sized graph."""
import numpy as np
import pytest
import torch

import dba_ref as R

pytestmark = pytest.mark.gpu

SHAPES = {(48, 64): np.array([50.0, 52.0, 31.5, 23.5]), (40, 80): np.array([60.0, 58.0, 39.5, 19.5])}


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def make_scene(ht, wd, n=9, seed=0, near_block=True):
    rng = np.random.default_rng(seed)
    poses = []
    for f in range(n):
        t, q = R.exp_se3(np.concatenate([[0.03 * f, 0.01 * np.sin(f), 0.02 * f], rng.normal(0, 0.02, 3)]))
        poses.append(np.concatenate([t, q]))
    poses = np.stack(poses)
    disps = rng.uniform(0.3, 1.0, (n, ht, wd))
    if near_block:
        disps[:, :6, :10] = -60.0                   # z = 1 + h tz: where tz < 0 these pixels land nearer than MIN_DEPTH
    return rng, poses, disps


def flow_target(poses, disps, intr, i, j):
    """True reprojection of frame i into frame j; a stereo edge (i == j) sees its pixels shifted by the fixed baseline."""
    ht, wd = disps.shape[1:]
    if i != j:
        return R.project(poses[i], poses[j], disps[i], intr).T.reshape(2, ht, wd)
    u, v, _, _ = R.pixel_rays(ht, wd, intr)
    return np.stack([u + intr[0] * R.STEREO_T[0] * disps[i].reshape(-1), v]).reshape(2, ht, wd)


def problem(ht, wd, seed=0, noise=0.5, near_block=True):
    """Window [2, 6) of 9 frames; a stereo edge, edges from and to frames below t0 and at or above t1, sensor disparity on part of
    the pixels."""
    rng, poses, disps = make_scene(ht, wd, seed=seed, near_block=near_block)
    intr = SHAPES[(ht, wd)]
    ii = [2, 3, 3, 4, 4, 5, 5, 2, 3, 0, 1, 6, 7, 4, 3]
    jj = [3, 2, 4, 3, 5, 4, 2, 5, 3, 2, 3, 5, 4, 6, 0]
    tgt = np.stack([flow_target(poses, disps, intr, i, j) for i, j in zip(ii, jj)])
    tgt += rng.normal(0, noise, tgt.shape)
    wgt = rng.uniform(0.2, 1.0, tgt.shape)
    p0 = poses.copy()
    for f in range(1, len(poses)):
        p0[f] = R.retract(poses[f], np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.01, 3)]))
    d0 = np.where(disps < 0, disps, disps * rng.uniform(0.95, 1.05, disps.shape))
    sens = np.where(rng.uniform(size=disps.shape) < 0.3, disps, 0.0)
    t0, t1 = 2, 6
    K = len(set(range(t0, t1)) | set(ii))
    eta = rng.uniform(1e-3, 1e-2, (K, ht, wd))
    return dict(poses=p0, disps=d0, intr=intr, sens=sens, tgt=tgt, wgt=wgt, eta=eta, ii=ii, jj=jj, t0=t0, t1=t1, truth=poses)


def to_gpu(pr):
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda").contiguous()
    li = lambda a: torch.tensor(a, dtype=torch.int64, device="cuda")
    return dict(poses=f(pr["poses"]), disps=f(pr["disps"]), intr=f(pr["intr"]), sens=f(pr["sens"]), tgt=f(pr["tgt"]), wgt=f(pr["wgt"]),
                eta=f(pr["eta"]), ii=li(pr["ii"]), jj=li(pr["jj"]))


def run_gpu(g, pr, iters, lm, ep, motion_only=False, depth_only=False):
    import droid_backends
    dx, dz = droid_backends.ba(g["poses"], g["disps"], g["intr"], g["sens"], g["tgt"], g["wgt"], g["eta"], g["ii"], g["jj"], pr["t0"],
                               pr["t1"], iters, lm, ep, motion_only, depth_only)
    torch.cuda.synchronize()
    return dx, dz


def run_ref(pr, iters, lm, ep, motion_only=False, depth_only=False, poses=None, disps=None):
    # the oracle sees the fp32-rounded inputs the GPU sees
    r32 = lambda a: np.asarray(a, np.float32).astype(float)
    return R.ba(r32(pr["poses"] if poses is None else poses), r32(pr["disps"] if disps is None else disps), r32(pr["intr"]),
                r32(pr["sens"]), r32(pr["tgt"]), r32(pr["wgt"]), r32(pr["eta"]), pr["ii"], pr["jj"], pr["t0"], pr["t1"], iters, lm, ep,
                motion_only, depth_only)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["pose_depth", "motion_only", "depth_only"])
def test_one_iteration_matches_the_fp64_oracle(shape, mode):
    pr = problem(*shape, seed=3)
    g = to_gpu(pr)
    mo, do = mode == "motion_only", mode == "depth_only"
    poses_in, disps_in = g["poses"].clone(), g["disps"].clone()
    dx, dz = run_gpu(g, pr, 1, 1e-4, 0.1, mo, do)
    p_ref, d_ref, dx_ref, dz_ref = run_ref(pr, 1, 1e-4, 0.1, mo, do)
    assert dx.shape == (pr["t1"] - pr["t0"], 6)
    assert np.all(np.isfinite(dx.cpu().numpy()))
    assert rel(dx.cpu().numpy(), dx_ref) < 2e-3, rel(dx.cpu().numpy(), dx_ref)
    out = set(range(len(pr["poses"]))) - set(range(pr["t0"], pr["t1"]))
    for f in out:                                                         # poses outside the window: untouched bits
        assert torch.equal(g["poses"][f], poses_in[f])
    if do:
        assert torch.equal(g["poses"], poses_in)
    else:
        assert np.abs(g["poses"].cpu().numpy() - p_ref).max() < 2e-3 * np.abs(dx_ref).max() + 1e-6
    if mo:
        assert dz is None
        assert torch.equal(g["disps"], disps_in)
    else:
        K, P = pr["eta"].shape[0], shape[0] * shape[1]
        assert dz.shape == (K, P)
        dzn = dz.cpu().numpy()
        assert np.abs(dzn - dz_ref).max() < 2e-3 * np.abs(dz_ref).max() + 1e-6
        assert np.abs(g["disps"].cpu().numpy() - d_ref).max() < 2e-3 * np.abs(dz_ref).max() + 1e-5


def test_singular_system_gives_zero_dx_and_no_nan():
    pr = problem(48, 64, seed=4)
    pr["wgt"] = np.zeros_like(pr["wgt"])
    g = to_gpu(pr)
    poses_in = g["poses"].clone()
    dx, dz = run_gpu(g, pr, 2, 0.0, 0.0)
    assert torch.equal(dx, torch.zeros_like(dx))
    assert torch.isfinite(dz).all() and torch.isfinite(g["disps"]).all()
    assert torch.equal(g["poses"], poses_in)             # exp(0) * pose is the pose itself
    _, d_ref, _, dz_ref = run_ref(pr, 2, 0.0, 0.0)
    assert np.abs(dz.cpu().numpy() - dz_ref).max() < 1e-4 * np.abs(dz_ref).max() + 1e-6


@pytest.mark.parametrize("shape", list(SHAPES))
def test_converges_on_noise_free_data(shape):
    pr = problem(*shape, seed=5, noise=0.0, near_block=False)
    pr["wgt"] = np.ones_like(pr["wgt"])
    outside = [f for f in range(len(pr["poses"])) if not pr["t0"] <= f < pr["t1"]]
    pr["poses"][outside] = pr["truth"][outside]          # the fixed frames hold the true poses
    g = to_gpu(pr)
    iters = 6
    dx, dz = run_gpu(g, pr, iters, 1e-4, 1e-4)
    p_ref, _, _, _ = run_ref(pr, iters, 1e-4, 1e-4)
    truth = pr["truth"]

    def err(p):
        return max(np.linalg.norm(R.relative(truth[0], truth[f])[0] - R.relative(p[0], p[f])[0]) for f in range(pr["t0"], pr["t1"]))

    e0, e_ref, e_gpu = err(pr["poses"]), err(p_ref), err(g["poses"].cpu().numpy().astype(float))
    assert e_ref < 0.2 * e0                              # the oracle itself converges ...
    assert e_gpu < 1.5 * e_ref + 1e-4, (e0, e_ref, e_gpu)    # ... and the GPU as far


def test_two_identical_calls_give_identical_bits():
    pr = problem(40, 80, seed=6)
    outs = []
    for _ in range(2):
        g = to_gpu(pr)
        dx, dz = run_gpu(g, pr, 3, 1e-4, 0.1)
        outs.append((dx, dz, g["poses"], g["disps"]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_ba_issues_no_host_synchronisation():
    import droid_backends
    pr = problem(48, 64, seed=7)
    g = to_gpu(pr)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        droid_backends.ba(g["poses"], g["disps"], g["intr"], g["sens"], g["tgt"], g["wgt"], g["eta"], g["ii"], g["jj"], pr["t0"], pr["t1"],
                          2, 1e-4, 0.1, False, False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(g["poses"]).all()


def test_wrong_number_of_depth_frames_is_reported_as_nan_and_updates_nothing():
    pr = problem(48, 64, seed=8)
    pr["eta"] = pr["eta"][:-1]
    g = to_gpu(pr)
    poses_in, disps_in = g["poses"].clone(), g["disps"].clone()
    dx, dz = run_gpu(g, pr, 1, 1e-4, 0.1)
    assert torch.isnan(dx).all() and torch.isnan(dz).all()
    assert torch.equal(g["poses"], poses_in) and torch.equal(g["disps"], disps_in)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_frame_distance_projmap_iproj_match_the_oracle(shape):
    import droid_backends
    _, poses, disps = make_scene(*shape, seed=9, near_block=False)
    disps[0, :30] = -40.0                                # > 25 % of frame 0 lands nearer than MIN_DEPTH: the 1000 sentinel
    intr = SHAPES[shape]
    ii = [0, 1, 2, 3, 4, 5, 8, 1]
    jj = [1, 0, 4, 3, 7, 2, 0, 8]
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")
    li = lambda a: torch.tensor(a, dtype=torch.int64, device="cuda")
    p32, d32, i32 = (np.asarray(a, np.float32).astype(float) for a in (poses, disps, intr))
    dist = droid_backends.frame_distance(f(poses), f(disps), f(intr), li(ii), li(jj), 0.3).cpu().numpy()
    ref = R.frame_distance(p32, d32, i32, ii, jj, 0.3)
    assert ref[0] == 1000.0 and dist[0] == 1000.0
    np.testing.assert_allclose(dist, ref, rtol=1e-4, atol=1e-4)
    coords, valid = droid_backends.projmap(f(poses), f(disps), f(intr), li(ii), li(jj))
    c_ref, v_ref = R.projmap(p32, d32, i32, ii, jj)
    np.testing.assert_array_equal(valid.cpu().numpy(), v_ref)
    np.testing.assert_allclose(coords.cpu().numpy(), c_ref, rtol=1e-4, atol=2e-3)
    pts = droid_backends.iproj(f(poses), f(disps), f(intr)).cpu().numpy()
    np.testing.assert_allclose(pts, R.iproj(p32, d32, i32), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_depth_filter_counts_match_away_from_the_knife_edge(shape):
    import droid_backends
    rng, poses, disps = make_scene(*shape, n=10, seed=10, near_block=False)
    intr = SHAPES[shape]
    disps = disps * 0 + rng.uniform(0.45, 0.55, disps.shape)          # a nearly planar scene, so neighbours agree often
    inds = [0, 2, 5, 9]
    depths = 1.0 / disps
    thresh = 0.05 * depths[inds].mean(axis=(1, 2))
    p32, d32, i32 = (np.asarray(a, np.float32).astype(float) for a in (poses, disps, intr))
    t32 = np.asarray(thresh, np.float32).astype(float)
    ref, marg = R.depth_filter(p32, d32, i32, inds, t32, margins=True)
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")
    cnt = droid_backends.depth_filter(f(poses), f(disps), f(intr), torch.tensor(inds, device="cuda"), f(thresh)).cpu().numpy()
    safe = marg > 1e-3
    assert safe.mean() > 0.5
    assert 0 < ref[safe].mean() < 6
    np.testing.assert_array_equal(cnt[safe], ref[safe])


def test_backend_sized_graph_matches_the_oracle_dx():
    ht, wd = 48, 64
    n = 100
    rng, poses, disps = make_scene(ht, wd, n=n, seed=11, near_block=False)
    intr = SHAPES[(ht, wd)]
    ii, jj = [], []
    for i in range(n):
        for j in range(max(0, i - 5), min(n, i + 6)):
            if i != j:
                ii.append(i)
                jj.append(j)
    assert 900 <= len(ii) <= 1100
    tgt = np.stack([R.project(poses[i], poses[j], disps[i], intr).T.reshape(2, ht, wd) for i, j in zip(ii, jj)])
    tgt += rng.normal(0, 0.5, tgt.shape)
    pr = dict(poses=poses, disps=disps, intr=intr, sens=np.zeros_like(disps), tgt=tgt, wgt=rng.uniform(0.2, 1.0, tgt.shape),
              eta=rng.uniform(1e-3, 1e-2, (n, ht, wd)), ii=ii, jj=jj, t0=1, t1=n)
    g = to_gpu(pr)
    dx, dz = run_gpu(g, pr, 1, 1e-4, 0.1)
    _, _, dx_ref, dz_ref = run_ref(pr, 1, 1e-4, 0.1)
    assert rel(dx.cpu().numpy(), dx_ref) < 5e-3, rel(dx.cpu().numpy(), dx_ref)
    assert np.abs(dz.cpu().numpy() - dz_ref).max() < 5e-3 * np.abs(dz_ref).max() + 1e-6
