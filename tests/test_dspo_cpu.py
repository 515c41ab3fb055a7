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
