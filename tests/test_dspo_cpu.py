"""CPU checks of DSPO stage 2: the library exports and binds sgr_dspo_*, splat_slam_amd.dspo checks its arguments before it touches the
device, and the fp64 restatement (tests/dspo_ref.py) is a sound yardstick: its disparity Jacobian matches finite differences, its
Schur step equals a direct solve of the full normal equations, and a step lowers the cost it works on.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import dba_ref as R
import dspo_ref as D

INTR = np.array([40.0, 42.0, 15.5, 11.5])


def random_pose(rng, trans=0.05, ang=0.03):
    t, q = R.exp_se3(np.concatenate([rng.normal(0, trans, 3), rng.normal(0, ang, 3)]))
    return np.concatenate([t, q])


def scene(rng, n=3, ht=6, wd=8, noise=0.0):
    """n cameras a few cm apart, a surface 1.5-3 m away, noise-free flow targets of every pair and one stereo edge, a mono prior
    m = 1.7 h + 0.05 with some pixels without prior, a valid-depth mask that overlaps them."""
    poses = np.stack([random_pose(rng) for _ in range(n)])
    disps = rng.uniform(1 / 3.0, 1 / 1.5, (n, ht, wd))
    ii, jj = zip(*[(a, b) for a in range(n) for b in range(n) if a != b])
    ii, jj = list(ii) + [1], list(jj) + [1]
    tgt = np.stack([D.project(poses[i], poses[j], disps[i], INTR, i == j).reshape(ht, wd, 2) for i, j in zip(ii, jj)])
    tgt += rng.normal(0, noise, tgt.shape) if noise else 0.0
    wgt = rng.uniform(0.2, 1.0, tgt.shape)
    mono = 1.7 * disps + 0.05
    mono[rng.uniform(size=mono.shape) < 0.15] = 0.0
    vmask = rng.uniform(size=mono.shape) < 0.6
    eta = rng.uniform(1e-3, 1e-2, (len(set(ii)), ht, wd))
    return dict(poses=poses, disps=disps, ii=ii, jj=jj, tgt=tgt, wgt=wgt, mono=mono, vmask=vmask, eta=eta)


# ---- the library and the module
def test_library_exports_and_binds_the_dspo_entry_points():
    from splat_slam_amd.build import build_native
    from splat_slam_amd import _native as nat
    import splat_slam_amd.dspo as dspo
    h = ctypes.CDLL(build_native(verbose=False))
    for name in ("sgr_dspo_align", "sgr_dspo_scratch_bytes", "sgr_dspo_ba"):
        assert hasattr(h, name), name
        assert name in nat.SIGNATURES, name
        assert getattr(nat.lib(), name).argtypes == nat.SIGNATURES[name][1]
    for name in ("align_scale_and_shift", "ba_with_scale_shift", "depth_scale_step"):
        assert callable(getattr(dspo, name))
    assert "not provided" in dspo.__doc__
    lib = nat.lib()
    small, large = lib.sgr_dspo_scratch_bytes(12, 60, 12, 48, 64), lib.sgr_dspo_scratch_bytes(100, 1000, 100, 48, 64)
    assert 12 * 3 * 48 * 64 * 4 <= small < large          # per-pixel state of the depth rows; nothing of size [E, ht*wd]
    assert large < 1000 * 48 * 64 * 4
    assert lib.sgr_dspo_scratch_bytes(12, 0, 12, 48, 64) == 0 and lib.sgr_dspo_scratch_bytes(12, 60, 70000, 48, 64) == 0


def test_problem_struct_matches_the_header_layout():
    from splat_slam_amd import _native as nat
    # pointer, int32 + pad, pointer, 3 x int32 + pad, 11 pointers, 4 x int32, 3 x float + pad, 2 pointers
    assert ctypes.sizeof(nat.SgrDspoProblem) == 8 + 8 + 8 + 16 + 11 * 8 + 16 + 16 + 16
    assert nat.SgrDspoProblem.edge_keep.offset == 8 + 8 + 8 + 16 + 10 * 8
    assert nat.SgrDspoProblem.dwq.offset == ctypes.sizeof(nat.SgrDspoProblem) - 16


def _args(n=4, e=3, h=6, w=8, m=2):
    return dict(target=torch.zeros(e, h, w, 2), weight=torch.zeros(e, h, w, 2), eta=torch.ones(m, h, w), poses=torch.zeros(n, 7),
                disps=torch.ones(n, h, w), intrinsics=torch.ones(4), ii=torch.zeros(e, dtype=torch.int64),
                jj=torch.ones(e, dtype=torch.int64), mono_disps=torch.ones(n, h, w), scales=torch.ones(n), shifts=torch.zeros(n),
                valid_depth_mask=torch.ones(n, h, w, dtype=torch.bool), ignore_frames=0, lm=1e-4, ep=0.1, alpha=1.0, iterations=1,
                edge_keep=None)


def _ba(**kw):
    from splat_slam_amd import dspo
    a = _args()
    a.update(kw)
    return dspo.ba_with_scale_shift(**a)


def test_every_entry_point_rejects_cpu_tensors():
    from splat_slam_amd import dspo
    with pytest.raises(RuntimeError, match="GPU tensor"):
        _ba()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        dspo.align_scale_and_shift(torch.ones(2, 6, 8), torch.ones(2, 6, 8), torch.ones(2, 6, 8, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        dspo.align_scale_and_shift(torch.ones(6, 8), torch.ones(6, 8))
    a = _args()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        dspo.depth_scale_step(a["poses"], a["disps"], a["intrinsics"], a["mono_disps"], a["valid_depth_mask"], a["scales"], a["shifts"], 4,
                              a["target"], a["weight"], a["eta"], a["ii"], a["jj"])


@pytest.mark.parametrize("kw,err,msg", [
    (dict(poses=torch.zeros(4, 7, dtype=torch.float64)), TypeError, "poses must be torch.float32"),
    (dict(mono_disps=torch.ones(4, 6, 8, dtype=torch.float16)), TypeError, "mono_disps must be torch.float32"),
    (dict(valid_depth_mask=torch.ones(4, 6, 8)), TypeError, "valid_depth_mask must be torch.bool or torch.uint8"),
    (dict(ii=torch.zeros(3, dtype=torch.int32)), TypeError, "ii must be torch.int64"),
    (dict(target=torch.zeros(3, 2, 6, 8)), ValueError, r"target must be \[E,h,w,2\] = \(3, 6, 8, 2\), got \(3, 2, 6, 8\)"),
    (dict(weight=torch.zeros(3, 2, 6, 8)), ValueError, r"weight must be \[E,h,w,2\]"),
    (dict(eta=torch.ones(2, 5, 8)), ValueError, r"eta must be \[M,6,8\], got \(2, 5, 8\)"),
    (dict(eta=torch.ones(2, 6, 9)), ValueError, r"eta must be \[M,6,8\], got \(2, 6, 9\)"),
    (dict(jj=torch.ones(2, dtype=torch.int64)), ValueError, "ii and jj must have the same length, got 3 and 2"),
    (dict(iterations=-1), ValueError, "iterations must be >= 0, got -1"),
    (dict(scales=torch.ones(3)), ValueError, r"scales must be \[N\]"),
    (dict(edge_keep=torch.ones(2, dtype=torch.bool)), ValueError, r"edge_keep must be \[E\]"),
    (dict(poses=torch.zeros(4, 6)), ValueError, r"poses must be \[N,7\]"),
])
def test_ba_with_scale_shift_rejects_bad_arguments(kw, err, msg):
    with pytest.raises(err, match=msg):
        _ba(**kw)


def test_align_rejects_bad_arguments():
    from splat_slam_amd import dspo
    with pytest.raises(TypeError, match="prediction must be torch.float32"):
        dspo.align_scale_and_shift(torch.ones(2, 6, 8, dtype=torch.float64), torch.ones(2, 6, 8))
    with pytest.raises(ValueError, match="target must have the shape of prediction"):
        dspo.align_scale_and_shift(torch.ones(2, 6, 8), torch.ones(2, 6, 9))
    with pytest.raises(TypeError, match="weights must be"):
        dspo.align_scale_and_shift(torch.ones(2, 6, 8), torch.ones(2, 6, 8), torch.ones(2, 6, 8, dtype=torch.int64))


# ---- the yardstick
@pytest.mark.parametrize("stereo", [False, True])
def test_oracle_jz_matches_a_central_difference_of_its_own_projection(stereo):
    rng = np.random.default_rng(0)
    s = scene(rng, ht=12, wd=16)
    i, j = (1, 1) if stereo else (0, 2)
    Jz, _, w, z = D.edge_terms(s["poses"][i], s["poses"][j], s["disps"][i], INTR, np.zeros((12, 16, 2)), np.ones((12, 16, 2)), stereo)
    assert np.all(z > D.MIN_DEPTH) and np.all(w == D.WEIGHT_SCALE)
    eps = 1e-6
    fd = (D.project(s["poses"][i], s["poses"][j], s["disps"][i], INTR, stereo, eps)
          - D.project(s["poses"][i], s["poses"][j], s["disps"][i], INTR, stereo, -eps)) / (2 * eps)
    assert np.abs(Jz).max() > 1.0
    assert np.abs(Jz - fd).max() < 1e-6 * np.abs(Jz).max()
    if stereo:
        assert np.all(Jz[:, 1] == 0.0)             # the baseline is horizontal


@pytest.mark.parametrize("alpha", [1.0, 0.01])
def test_oracle_schur_step_equals_the_dense_normal_equation_solve(alpha):
    rng = np.random.default_rng(1)
    s = scene(rng, noise=0.3)
    d0 = s["disps"] * rng.uniform(0.95, 1.05, s["disps"].shape)
    scales, shifts = rng.uniform(0.5, 0.7, 3), rng.uniform(-0.05, 0.05, 3)
    vm, mono = s["vmask"], s["mono"]
    assert all(((mono[:, :, :] < 1e-6) == a)[vm == b].any() for a in (0, 1) for b in (0, 1))      # all four (invalid, vd) cases
    _, _, _, dwq, dz = D.ba_with_scale_shift(s["tgt"], s["wgt"], s["eta"], s["poses"], d0, INTR, s["ii"], s["jj"], mono, scales, shifts,
                                             vm, 0, 1e-4, 0.1, alpha, 1)
    dwq_d, dz_d = D.dense_step(s["tgt"], s["wgt"], s["eta"], s["poses"], d0, INTR, s["ii"], s["jj"], mono, scales, shifts, vm, 0, 1e-4,
                               0.1, alpha)
    assert np.abs(dwq).max() > 1e-4 and np.abs(dz).max() > 1e-4
    assert np.abs(dwq - dwq_d).max() < 1e-9 * max(1.0, np.abs(dwq_d).max())
    assert np.abs(dz - dz_d).max() < 1e-9 * max(1.0, np.abs(dz_d).max())


def test_oracle_step_lowers_the_cost_on_noise_free_data():
    rng = np.random.default_rng(2)
    s = scene(rng, ht=12, wd=16)
    d0 = s["disps"] * rng.uniform(0.95, 1.05, s["disps"].shape)
    sc, sh, _ = D.align_scale_and_shift(s["mono"], d0, s["vmask"].astype(float))
    args = (s["tgt"], s["wgt"], s["poses"])
    rest = (INTR, s["ii"], s["jj"], s["mono"])
    for alpha in (1.0, 0.01):
        c0 = D.cost(*args, d0, *rest, sc, sh, s["vmask"], 0, alpha)
        d1, sc1, sh1, _, _ = D.ba_with_scale_shift(s["tgt"], s["wgt"], s["eta"] * 0, s["poses"], d0, INTR, s["ii"], s["jj"], s["mono"],
                                                   sc, sh, s["vmask"], 0, 0.0, 1e-9, alpha, 1)
        c1 = D.cost(*args, d1, *rest, sc1, sh1, s["vmask"], 0, alpha)
        assert c1 < c0, (alpha, c0, c1)


def test_oracle_alignment_recovers_an_exact_scale_and_shift():
    rng = np.random.default_rng(3)
    pred = rng.uniform(0.2, 2.0, (3, 6, 8))
    w = (rng.uniform(size=pred.shape) < 0.5).astype(float)
    s, q, err = D.align_scale_and_shift(pred, 1.7 * pred + 0.05, w)
    np.testing.assert_allclose(s, 1.7, rtol=1e-12)
    np.testing.assert_allclose(q, 0.05, rtol=1e-10)
    assert err.max() < 1e-12
    s1, q1, _ = D.align_scale_and_shift(pred[0], 1.7 * pred[0] + 0.05)
    assert s1.shape == (1,) and abs(s1[0] - 1.7) < 1e-12 and abs(q1[0] - 0.05) < 1e-12


def test_oracle_edge_mask_equals_removing_the_edges():
    rng = np.random.default_rng(4)
    s = scene(rng, noise=0.3)
    scales, shifts = np.full(3, 0.6), np.zeros(3)
    keep = np.array([not (i == 2 or j == 2) for i, j in zip(s["ii"], s["jj"])])
    a = D.ba_with_scale_shift(s["tgt"], s["wgt"], s["eta"], s["poses"], s["disps"], INTR, s["ii"], s["jj"], s["mono"], scales, shifts,
                              s["vmask"], edge_keep=keep)
    ii2, jj2 = [i for i, k in zip(s["ii"], keep) if k], [j for j, k in zip(s["jj"], keep) if k]
    b = D.ba_with_scale_shift(s["tgt"][keep], s["wgt"][keep], s["eta"][:2], s["poses"], s["disps"], INTR, ii2, jj2, s["mono"], scales,
                              shifts, s["vmask"])
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[3][:2], b[3])
    np.testing.assert_array_equal(a[4][:2], b[4])
    assert np.all(a[3][2] == 0) and np.all(a[4][2] == 0)
    np.testing.assert_array_equal(a[0][2], s["disps"][2])


# ---- the oracle with magnitudes and the criteria of tests/dspo_cases.py, proved on the CPU
import dspo_cases as DC      # noqa: E402

MUTATIONS = {                                   # planted fault -> the smallest case that must show it
    "thresh_025": "pix:7,9,1.0",                # the depth threshold 0.25 of stage 1 instead of 0.2
    "targets_chw": "pix:3,5,1.0",               # targets read as [E,2,h,w]
    "pix_div_ht": "pix:5,13,1.0",               # pixel row and column from p / ht
    "drop_last_pixel": "pix:3,5,1.0",           # the last pixel left out of the frame sums
    "drop_last_edge": "pix:7,9,1.0",            # the last kept edge of a frame's run left out
    "dup_once": "dup",                          # a duplicate edge counted once
    "count_masked": "mask:bool",                # a masked edge counted
    "clamp_oob": "oob",                         # an out-of-range edge clamped into range and counted
    "eta_by_frame": "pix:7,9,1.0",              # eta indexed by frame instead of by depth row
    "scale_by_row": "pix:7,9,1.0",              # scales and shifts indexed by depth row instead of by frame
    "gain_on_rd": "pix:7,9,1.0",                # the gain 10 applied to rd
    "jd_kept": "pix:7,9,1.0",                   # Jd kept where the prior is invalid on a valid-depth pixel
    "ignore_le": "ignore:some",                 # ignore_frames tested with <=
    "lm_from_S": "pix:7,9,1.0",                 # the damping lm taken from the reduced S instead of H_diag
    "sums_fp32": "flat:384,512",                # the seven sums accumulated in fp32: shows where P is far above the units of an addend
    "S_subtracted_fp32": "far:16,16",           # S = H - sum Q E E^T from fp32 sums: the cancellation the kernel avoids, alpha = 1
    "nonpd_zero_all": "singular",               # a frame that is not positive definite zeroes every frame's dwq
    "no_floor": "pix:3,5,1.0",                  # the floor at 0 omitted
    "dz_prev_row": "pix:7,9,1.0",               # dz back-substituted with the dwq of the previous row
}


def scene_wants(name):
    return dict(want_between=name.startswith("pix") or name == MUTATIONS["thresh_025"])


@pytest.fixture(scope="module")
def float32_runs():
    return {name: DC.criteria(name, *DC.emulate(name)) for name in DC.CASES}


def test_every_dspo_case_keeps_its_decisions_away_from_fp32_rounding():
    assert set(MUTATIONS) == set(D.MUTATIONS) and set(MUTATIONS.values()) <= set(DC.CASES)
    for name in DC.CASES + ["iter"]:
        DC.check_scene(name, **scene_wants(name))
    # the edges the cases are there for
    assert [DC.oracle(f"pix:{h},{w},1.0")["P"] for h, w in DC.PIXEL_SHAPES] == [15, 63, 65, 256, 257]
    assert [len(DC.case(f"tile:{E}")["ii"]) for E in DC.TILE_E] == [255, 256, 257, 513]
    for name, nv, M in (("oob", 9, 6), ("oob:long_poses", 9, 6), ("oob:short_poses", 7, 5)):
        c, o = DC.case(name), DC.oracle(name)
        assert o["nv"] == nv and o["M"] == M and 8 not in o["kx"] and 8 in c["ii"]
        assert 0 < len(R.kept_edges(c["ii"], c["jj"], nv)) < len(c["ii"])
    for name in ("mask:bool", "mask:u8"):
        o = DC.oracle(name)
        assert [f for k, f in enumerate(o["kx"]) if not o["active"][k]] == [4, 7]
    assert sorted(set(DC.case("mask:u8")["keep"].tolist())) == [0, 1, 2, 255] and DC.case("mask:bool")["keep"].dtype == bool
    assert DC.oracle("one_edge")["M"] == 1 and DC.oracle("big")["nv"] == 1030 and DC.oracle("big")["kx"][:2] == [3, 7]
    o = DC.oracle("singular")
    assert [f for k, f in enumerate(o["kx"]) if o["fail"][k]] == [5]


def test_float32_restatement_of_dspo_is_inside_every_criterion_at_every_case(float32_runs):
    worst = {}
    for name, (ratios, broken) in float32_runs.items():
        print(f"{name}: err / bound " + " ".join(f"{k}={v:.4f}" for k, v in sorted(ratios.items())), broken)
        assert not broken, (name, broken)
        for k, r in ratios.items():
            assert r <= 1.0, (name, k, r)
            if r > worst.get(k, (0.0, ""))[0]:
                worst[k] = (r, name)
    print("\nlargest err / bound of the float32 restatement (an emulation, not the device):")
    for k in sorted(worst):
        print(f"  criterion {k}: {worst[k][0]:.4f} at {worst[k][1]}")
    assert set(worst) == {"A", "B"}
    # the singular frame is held to dwq == 0 and still steps its disparities by Q b
    c, o = DC.case("singular"), DC.oracle("singular")
    _, _, _, dwq, dz = DC.emulate("singular")
    k = o["kx"].index(5)
    assert not dwq[k].any() and np.abs(dz[k]).max() > 1e-4 and np.abs(np.delete(dwq, k, 0)).min() > 0


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_planted_dspo_fault_fails_a_criterion(mutation):
    """sums_fp32 is the one fault that small shapes cannot show: an fp32 sum of P addends costs at most P units of 2^-24 against
    addends that carry 315 or more of their own, so up to P = 257 it moves criterion A in the fifth digit only.  Its case is the flat
    384 x 512 frame of tests/dspo_cases.py, where every addition rounds the same way and the drift leaves the bound."""
    name = MUTATIONS[mutation]
    ratios, broken = DC.criteria(name, *DC.emulate(name, mutate=mutation))
    print(mutation, name, ratios, broken)
    assert not DC.passes(ratios, broken)
    ratios, broken = DC.criteria(name, *DC.emulate(name))        # ... and it is the fault, not the case, that fails
    assert DC.passes(ratios, broken)


def test_the_derived_dspo_units_are_the_documented_ones():
    """the counts DESIGN.md section 3 tabulates are what the formulas give: those of a frame with one kept edge, and 2 (n - 1) or
    4 (n - 1) more for a frame with n"""
    u1, u4 = DC.oracle("one_edge")["units"], DC.oracle("pix:7,9,1.0")["units"]         # frame 3 of the 13 edges keeps four
    print("\nunits:", u1)
    assert u1 == DC.DOCUMENTED_UNITS, u1
    twice = {"QB0", "v2", "v3", "v4", "v5", "v6"}
    once = {"c", "b", "cpe", "Q", "bb", "QB1", "QB2"}
    assert {k: u4[k] - u1[k] for k in u1} == {k: 12 if k in twice else 6 if k in once else 0 for k in u1}


def _oracle_args(c, alpha=None):
    return (c["tgt"], c["wgt"], c["eta"], c["poses"], c["disps"], c["intr"], c["ii"], c["jj"], c["mono"], c["scales"], c["shifts"],
            c["vmask"], c["ignore_frames"], float(np.float32(c["lm"])), float(np.float32(c["ep"])),
            c["alpha"] if alpha is None else alpha, 1, c["keep"])


@pytest.mark.parametrize("name", ["pix:7,9,1.0", "pix:5,13,0.01", "dup", "oob:short_poses", "mask:u8", "singular", "stereo_only"])
def test_linearize_mag_reproduces_the_dwq_and_dz_of_ba_with_scale_shift(name):
    c, o = DC.case(name), DC.oracle(name)
    sa = float(np.float32(np.sqrt(c["alpha"])))           # the kernel's sqrt_alpha is one fp32 rounding: the oracle gets its square
    _, _, _, dwq, dz = D.ba_with_scale_shift(*_oracle_args(c, sa * sa))
    mine = D.solve_rows(o)
    np.testing.assert_allclose(mine, dwq, rtol=1e-9, atol=1e-9 * np.abs(dwq).max())
    np.testing.assert_allclose(D.back_substitute(o, mine).v, dz, rtol=1e-9, atol=1e-9 * np.abs(dz).max())
    assert np.abs(dz).max() > 1e-4


@pytest.mark.parametrize("name", ["oob", "oob:long_poses", "oob:short_poses"])
def test_oracle_with_out_of_range_edges_equals_the_oracle_on_the_filtered_list(name):
    c = DC.case(name)
    nv = min(len(c["poses"]), len(c["disps"]))
    keep = R.kept_edges(c["ii"], c["jj"], nv)
    a = list(_oracle_args(c))
    b = list(a)
    b[0], b[1], b[6], b[7] = c["tgt"][keep], c["wgt"][keep], [c["ii"][e] for e in keep], [c["jj"][e] for e in keep]
    assert D.depth_frames(c["ii"], c["jj"], nv) == D.depth_frames(b[6]) and len(b[6]) < len(c["ii"])
    for x, y in zip(D.ba_with_scale_shift(*a), D.ba_with_scale_shift(*b)):
        np.testing.assert_array_equal(x, y)
    step = lambda tg, wg, ii, jj: D.depth_scale_step(c["poses"], c["disps"], c["intr"], c["mono"], c["vmask"], c["scales"], c["shifts"],
                                                     nv, tg, wg, c["eta"], ii, jj, itrs=1)
    full, filt = step(c["tgt"], c["wgt"], c["ii"], c["jj"]), step(b[0], b[1], b[6], b[7])
    for x, y in zip(full[:3], filt[:3]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(full[3][keep], filt[3])
    assert not full[3][[e for e in range(len(c["ii"])) if e not in keep]].any() and full[4] == filt[4]
