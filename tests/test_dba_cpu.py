"""CPU checks of the dense bundle adjustment restatement (tests/dba_ref.py) and of the droid_backends argument checks.  No GPU."""
import numpy as np
import pytest
import torch

import dba_ref as R

INTR = np.array([40.0, 42.0, 15.5, 11.5])


def random_pose(rng, trans=0.1, ang=0.1):
    t, q = R.exp_se3(np.concatenate([rng.normal(0, trans, 3), rng.normal(0, ang, 3)]))
    return np.concatenate([t, q])


def scene(rng, n=4, ht=12, wd=16):
    """n cameras a few cm apart looking at a surface 1.5-3 m away; disparity maps and noise-free flow targets of every pair."""
    poses = np.stack([random_pose(rng, 0.05, 0.03) for _ in range(n)])
    disps = rng.uniform(1 / 3.0, 1 / 1.5, (n, ht, wd))
    return poses, disps


def targets_for(poses, disps, ii, jj):
    return np.stack([R.project(poses[i], poses[j], disps[i], INTR).T.reshape(2, *disps.shape[1:]) for i, j in zip(ii, jj)])


def test_jacobians_match_central_differences():
    rng = np.random.default_rng(0)
    poses, disps = scene(rng)
    i, j = 1, 3
    target = np.zeros((2,) + disps.shape[1:])
    weight = np.ones_like(target)
    Jp, Ji, Jz, _, _ = R.edge_terms(poses[i], poses[j], disps[i], INTR, target, weight, False)
    eps = 1e-6
    for n in range(6):
        xi = np.zeros(6)
        xi[n] = eps
        dj = (R.project(poses[i], poses[j], disps[i], INTR, xi_j=xi) - R.project(poses[i], poses[j], disps[i], INTR, xi_j=-xi)) / (2 * eps)
        di = (R.project(poses[i], poses[j], disps[i], INTR, xi_i=xi) - R.project(poses[i], poses[j], disps[i], INTR, xi_i=-xi)) / (2 * eps)
        np.testing.assert_allclose(Jp[:, :, n], dj, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(Ji[:, :, n], di, rtol=1e-5, atol=1e-5)
    dz = (R.project(poses[i], poses[j], disps[i], INTR, ddisp=eps) - R.project(poses[i], poses[j], disps[i], INTR, ddisp=-eps)) / (2 * eps)
    np.testing.assert_allclose(Jz, dz, rtol=1e-5, atol=1e-5)


def test_stereo_edges_only_touch_the_disparities():
    rng = np.random.default_rng(1)
    poses, disps = scene(rng, n=2)
    target = rng.normal(10, 3, (2,) + disps.shape[1:])
    Jp, Ji, Jz, r, w = R.edge_terms(poses[0], poses[0], disps[0], INTR, target, np.ones_like(target), True)
    assert np.all(np.abs(Jz[:, 0]) > 0)          # the -0.1 baseline gives the disparity a horizontal lever
    p2, d2, dx, dz = R.ba(poses, disps, INTR, np.zeros_like(disps), target[None], np.ones_like(target)[None],
                          np.full((2,) + disps.shape[1:], 1e-3), [0], [0], 1, 2, 1, 1e-4, 0.1)
    np.testing.assert_array_equal(dx, 0.0)       # no pose term
    assert np.abs(dz[0]).max() > 0 and np.all(dz[1] == 0)


def test_gauss_newton_converges_on_noise_free_data():
    rng = np.random.default_rng(2)
    n, ht, wd = 4, 12, 16
    poses, disps = scene(rng, n, ht, wd)
    ii, jj = zip(*[(a, b) for a in range(n) for b in range(n) if a != b])
    tgt = targets_for(poses, disps, ii, jj)
    wgt = np.ones_like(tgt)
    p0 = poses.copy()
    for f in range(1, n):
        p0[f] = R.retract(poses[f], np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.01, 3)]))
    d0 = disps * rng.uniform(0.97, 1.03, disps.shape)
    sens = disps.copy()                           # a sensor pins the scale
    sens[:, ::2] = 0.0
    eta = np.full(disps.shape, 1e-3)

    def err(p):
        return max(np.linalg.norm(R.relative(p[0], p[f])[0] - R.relative(poses[0], poses[f])[0]) for f in range(1, n))

    e0 = err(p0)
    p, d = p0, d0
    for _ in range(8):
        p, d, dx, dz = R.ba(p, d, INTR, sens, tgt, wgt, eta, ii, jj, 1, n, 1, 1e-4, 1e-6)
    assert err(p) < 1e-3 * e0
    res = max(np.abs(R.project(p[i], p[j], d[i], INTR).T.reshape(2, ht, wd) - tgt[e]).max() for e, (i, j) in enumerate(zip(ii, jj)))
    assert res < 1e-3


def test_depth_filter_neighbour_choice():
    assert R.depth_filter_neighbours(5, 20) == [4, 3, 2, 8, 9, 10]
    assert R.depth_filter_neighbours(0, 4) == [3]


# ---- droid_backends argument checks (no launch happens: every error is raised before the device is touched)
def _args(n=4, e=3, h=6, w=8, k=3):
    return dict(poses=torch.zeros(n, 7), disps=torch.ones(n, h, w), intrinsics=torch.ones(4), disps_sens=torch.zeros(n, h, w),
                targets=torch.zeros(e, 2, h, w), weights=torch.zeros(e, 2, h, w), eta=torch.ones(k, h, w),
                ii=torch.zeros(e, dtype=torch.int64), jj=torch.ones(e, dtype=torch.int64), t0=1, t1=3, iterations=1, lm=1e-4, ep=0.1,
                motion_only=False, depth_only=False)


def _ba(**kw):
    import droid_backends
    a = _args()
    a.update(kw)
    return droid_backends.ba(*a.values())


def test_ba_rejects_cpu_tensors():
    with pytest.raises(RuntimeError, match="GPU tensor"):
        _ba()


@pytest.mark.parametrize("kw,err,msg", [
    (dict(poses=torch.zeros(4, 6)), ValueError, r"poses must be \[N,7\]"),
    (dict(poses=torch.zeros(4, 7, dtype=torch.float64)), TypeError, "poses must be torch.float32"),
    (dict(intrinsics=torch.ones(3)), ValueError, r"intrinsics must be \[4\]"),
    (dict(ii=torch.zeros(3, dtype=torch.int32)), TypeError, "ii must be torch.int64"),
    (dict(jj=torch.ones(2, dtype=torch.int64)), ValueError, "same length"),
    (dict(targets=torch.zeros(3, 2, 6, 9)), ValueError, r"targets must be \[E,2,h,w\]"),
    (dict(weights=torch.zeros(3, 6, 8)), ValueError, "weights must have 4 dimensions"),
    (dict(eta=torch.ones(3, 5, 8)), ValueError, r"eta must be \[K,6,8\]"),
    (dict(disps_sens=torch.zeros(3, 6, 8)), ValueError, "disps_sens must have the shape of disps"),
    (dict(t0=3, t1=3), ValueError, "must be non-empty"),
    (dict(t1=5), ValueError, "inside the 4 frames"),
    (dict(disps=torch.ones(4, 6, 8).transpose(1, 2)), ValueError, "must have 3 dimensions|contiguous"),
])
def test_ba_rejects_bad_arguments(kw, err, msg):
    with pytest.raises(err, match=msg):
        _ba(**kw)


def test_ba_rejects_windows_beyond_the_supported_size():
    n = 600
    with pytest.raises(ValueError, match="exceeds the supported 512"):
        _ba(poses=torch.zeros(n, 7), disps=torch.ones(n, 6, 8), disps_sens=torch.zeros(n, 6, 8), t0=0, t1=513)


def test_geometry_functions_reject_bad_arguments():
    import droid_backends as db
    poses, disps, intr = torch.zeros(4, 7), torch.ones(4, 6, 8), torch.ones(4)
    ii, jj = torch.zeros(2, dtype=torch.int64), torch.ones(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        db.frame_distance(poses, disps, intr, ii, jj, 0.3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        db.projmap(poses, disps, intr, ii, jj)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        db.iproj(poses, disps, intr)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        db.depth_filter(poses, disps, intr, ii, torch.ones(2))
    with pytest.raises(TypeError, match="disps must be torch.float32"):
        db.iproj(poses, disps.double(), intr)
    with pytest.raises(ValueError, match="thresh must have one entry per index"):
        db.depth_filter(poses, disps, intr, ii, torch.ones(3))
    with pytest.raises(ValueError, match="must cover the 4 disparity maps"):
        db.iproj(torch.zeros(3, 7), disps, intr)
    with pytest.raises(TypeError, match="jj must be torch.int64"):
        db.projmap(poses, disps, intr, ii, jj.float())


def test_package_exports_the_reference_names_and_documents_what_it_leaves_out():
    import droid_backends as db
    for name in ("ba", "frame_distance", "projmap", "depth_filter", "iproj"):
        assert callable(getattr(db, name))
    assert "altcorr" in db.__doc__ and "corr_index" in db.__doc__ and "not provided" in db.__doc__


# ---- the oracle with magnitudes and the three criteria of tests/dba_cases.py, proved on the CPU
import dba_cases as DC      # noqa: E402

MUTATIONS = {                                   # planted fault -> the smallest case that can show it
    "drop_last_pixel": "pix:3,5,pose_depth",    # the last pixel of a frame left out of one edge's pose sums
    "dup_skip_E": "dup",                        # the second of two duplicate edges left out of the merged Eij rows
    "dup_skip_C": "dup",                        # ... left out of C and w
    "swap_Hij": "pix:3,5,motion_only",          # Hij and Hji swapped
    "dz_missing_edge": "pix:3,5,pose_depth",    # one outgoing edge missing from one depth row's dz sum
    "no_t0_skip": "pix:3,5,pose_depth",         # the back-substitution does not skip t0
    "clamp_oob": "oob",                         # an out-of-range jj clamped into range instead of dropping the edge
    "chol_skip_tile": "chol:11,motion_only",    # n = 66: the one trailing 64x64 tile update of the factorisation skipped
}


@pytest.fixture(scope="module")
def float32_runs():
    return {name: DC.criteria(name, *DC.emulate(name)) for name in DC.CASES}


def test_every_case_keeps_its_decisions_away_from_fp32_rounding():
    for name in DC.CASES:
        DC.check_scene(name, want_behind=not name.startswith(("chol", "big")))


def test_float32_restatement_is_inside_every_criterion_at_every_case(float32_runs):
    worst = {}
    for name, (ratios, broken) in float32_runs.items():
        assert not broken, (name, broken)
        for k, r in ratios.items():
            assert r <= 1.0, (name, k, r)
            if r > worst.get(k, (0.0, ""))[0]:
                worst[k] = (r, name)
    print("\nlargest err / bound of the float32 restatement (an emulation, not the device):")
    for k in sorted(worst):
        print(f"  criterion {k}: {worst[k][0]:.3f} at {worst[k][1]}")
    assert set(worst) == {"A", "B", "C"}
    singular = float32_runs["win:no_edge_singular"][0]
    assert "A" not in singular                       # held to dx == 0 instead


def test_the_derived_units_are_the_documented_ones():
    """the per-addend counts DESIGN.md section 3 tabulates are what the formulas give (they do not depend on the case)"""
    u = DC.oracle("pix:7,9,pose_depth")["units"]
    P = 63
    got = dict(Hs=u["Hs"] - 2 * P, vs=u["vs"] - 2 * P, E=u["E"], Cii=u["Cii"], bz=u["bz"])
    print("\nper-addend units:", got, "C", u["C"], "w", u["w"], "Q", u["Q"], "F", u["F"], "S", u["S"], "Sg", u["Sg"])
    assert got == DC.DOCUMENTED_UNITS, got


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_planted_fault_fails_a_criterion(mutation):
    name = MUTATIONS[mutation]
    ratios, broken = DC.criteria(name, *DC.emulate(name, mutate=mutation))
    print(mutation, name, ratios, broken)
    assert not DC.passes(ratios, broken)
    ratios, broken = DC.criteria(name, *DC.emulate(name))        # ... and it is the fault, not the case, that fails
    assert DC.passes(ratios, broken)


def test_blocked_cholesky_restatement_factors_what_numpy_factors():
    o = DC.oracle("chol:22,motion_only")
    L = R.blocked_cholesky(o["H"])
    np.testing.assert_allclose(L, np.linalg.cholesky(o["H"]), rtol=1e-12, atol=1e-12 * np.abs(o["H"]).max() ** 0.5)


def test_oracle_solves_its_own_system_to_fp64():
    o = DC.oracle("pix:7,9,pose_depth")
    x = R.solve(o).reshape(-1)
    assert np.all(np.abs(o["H"] @ x - o["g"]) <= R.fp64_solve_term(o, x) + R.bound64(o["H_addends"], o["H_mag"]) @ np.abs(x))


def test_oracle_C_w_F_reproduce_the_dz_of_ba():
    for name in ("pix:7,9,pose_depth", "dup", "oob", "win:both_outside"):
        c, o = DC.case(name), DC.oracle(name)
        _, _, dx, dz = R.ba(c["poses"], c["disps"], c["intr"], c["sens"], c["tgt"], c["wgt"], c["eta"], c["ii"], c["jj"], c["t0"], c["t1"], 1,
                            float(np.float32(c["lm"])), float(np.float32(c["ep"])))
        np.testing.assert_allclose(R.solve(o), dx, rtol=1e-9, atol=1e-12)
        mine = R.back_substitute(o, dx).v
        np.testing.assert_allclose(mine, dz, rtol=1e-9, atol=1e-9 * np.abs(dz).max())


def test_splitting_an_edge_into_two_half_weight_copies_changes_nothing():
    c = DC.case("pix:7,9,pose_depth")
    a = list(DC.lin_args(c))
    e = 2                                                          # 3 -> 4, inside the window
    b = list(a)
    half = c["wgt"].copy()
    half[e] *= 0.5
    b[4] = np.concatenate([c["tgt"], c["tgt"][e:e + 1]])
    b[5] = np.concatenate([half, half[e:e + 1]])
    b[7], b[8] = c["ii"] + [c["ii"][e]], c["jj"] + [c["jj"][e]]
    o1, o2 = R.linearize(*a), R.linearize(*b)
    scale = np.abs(o1["H_mag"]).max()
    np.testing.assert_allclose(o2["H"], o1["H"], rtol=0, atol=1e-13 * scale)
    np.testing.assert_allclose(o2["g"], o1["g"], rtol=0, atol=1e-13 * np.abs(o1["g_mag"]).max())
    np.testing.assert_allclose(o2["C"].v, o1["C"].v, rtol=1e-13)
    np.testing.assert_allclose(R.back_substitute(o2, R.solve(o2)).v, R.back_substitute(o1, R.solve(o1)).v, rtol=1e-9, atol=1e-12)
