"""The host half of splat_slam_amd.traj_eval against the restatement of tests/traj_eval_ref.py: umeyama from the 17 sums, ape's
dictionary arithmetic and aligned_c2w, on known answers.  No GPU."""
import types

import numpy as np
import pytest
import torch

import traj_eval_ref as R
from splat_slam_amd import traj_eval as te


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def sums_of(x, y):
    return R.fit_sums(x, y, np.ones(len(x), bool))[0]


def close(got, want, rtol=1e-9):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= rtol * np.abs(want).max()).all())


def test_umeyama_from_the_sums_is_the_restatement_from_the_points():
    rng = np.random.default_rng(0)
    for n in (10, 50, 500):
        x = rng.normal(size=(n, 3)) * [2.0, 1.5, 1.0] + [5.0, -2.0, 1.0]
        y = 1.7 * x @ rotation(rng).T + [0.3, 0.2, -4.0] + 0.05 * rng.normal(size=(n, 3))
        for with_scale in (True, False):
            r, t, s = te.umeyama(sums_of(x, y), with_scale)
            r0, t0, s0, d = R.umeyama(x, y, with_scale)
            assert d[1] / d[0] >= 0.1
            assert close(r, r0) and close(t, t0) and close(s, s0)
            assert with_scale or s == 1.0


def test_an_exact_similarity_is_recovered():
    rng = np.random.default_rng(1)
    x = rng.normal(size=(40, 3))
    r0, t0, s0 = rotation(rng), np.array([1.0, -2.0, 0.5]), 2.5
    r, t, s = te.umeyama(sums_of(x, s0 * x @ r0.T + t0))
    assert close(r, r0, 1e-12) and close(t, t0, 1e-12) and abs(s - s0) <= 1e-12 * s0


def test_a_mirror_image_gives_a_proper_rotation_with_the_last_singular_value_negated():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(60, 3)) * [3.0, 2.0, 1.0]
    y = x * [1.0, 1.0, -1.0]
    sums = sums_of(x, y)
    r, t, s = te.umeyama(sums)
    d = np.linalg.svd(sums[8:17].reshape(3, 3) / sums[0], compute_uv=False)
    assert abs(np.linalg.det(r) - 1.0) < 1e-12
    assert abs(s * sums[7] / sums[0] - (d[0] + d[1] - d[2])) <= 1e-12 * d[0]          # S = diag(1, 1, -1)
    assert s < (d[0] + d[1] + d[2]) / (sums[7] / sums[0]) - 1e-3


def test_a_planar_trajectory_is_accepted():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(size=(30, 2)), np.zeros((30, 1))], 1)
    r0, t0, s0 = rotation(rng), np.array([0.5, 0.25, -1.0]), 0.75
    r, t, s = te.umeyama(sums_of(x, s0 * x @ r0.T + t0))
    assert close(r, r0, 1e-12) and close(t, t0, 1e-12) and abs(s - s0) <= 1e-12


@pytest.mark.parametrize("case", ["collinear", "stationary", "two poses", "no pose", "not finite"])
def test_degenerate_trajectories_raise(case):
    line = np.outer(np.arange(8.0), [1.0, 0.0, 0.0])
    x, y = {"collinear": (line, 2.0 * line + 1.0), "stationary": (np.ones((8, 3)), line), "two poses": (line[:2], line[:2]),
            "no pose": (line[:0], line[:0]), "not finite": (line, line)}[case]
    sums = sums_of(x, y)
    if case == "not finite":
        sums[9] = np.nan
    with pytest.raises(te.TrajectoryDegenerate):
        te.umeyama(sums)
    assert issubclass(te.TrajectoryDegenerate, ValueError)


@pytest.mark.parametrize("n", [1, 2, 7, 8])
def test_ape_statistics_are_evos_for_even_and_odd_counts(n):
    rng = np.random.default_rng(10 + n)
    err = rng.uniform(0.01, 2.0, n)
    got, want = te.ape_statistics(R.stat_sums(err)), R.ape(err)
    assert sorted(got) == ["max", "mean", "median", "min", "rmse", "sse", "std"]
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12 * max(want[k], want["max"]), k
    assert got["median"] == np.median(err) and got["min"] == err.min() and got["max"] == err.max()
    with pytest.raises(te.TrajectoryDegenerate):
        te.ape_statistics(R.stat_sums(err[:0]))


def test_aligned_c2w_scales_the_translations_then_transforms_from_the_left():
    rng = np.random.default_rng(4)
    c2w = np.tile(np.eye(4), (5, 1, 1))
    for k in range(5):
        c2w[k, :3, :3], c2w[k, :3, 3] = rotation(rng), rng.normal(size=3)
    al = te.Alignment(rotation(rng), np.array([0.1, 0.2, 0.3]), 1.3, 5, 0)
    want = R.aligned_c2w(c2w, al.r_a, al.t_a, al.s)
    assert np.abs(te.aligned_c2w(c2w, al) - want).max() < 1e-14
    assert np.abs(te.aligned_c2w(torch.from_numpy(c2w), al) - want).max() < 1e-14
    assert np.abs(te.aligned_c2w([torch.from_numpy(p) for p in c2w], al) - want).max() < 1e-14
    w2c = np.linalg.inv(c2w)
    cams = [types.SimpleNamespace(R=torch.from_numpy(p[:3, :3]), T=torch.from_numpy(p[:3, 3])) for p in w2c]
    assert np.abs(te.aligned_c2w(cams, al) - want).max() < 1e-12
    assert te.aligned_c2w([], al).shape == (0, 4, 4)
    ident = te.aligned_c2w(c2w, te.Alignment.identity())
    assert np.array_equal(ident, c2w)


def test_the_launch_counts_are_declared_and_within_three():
    from splat_slam_amd import _native as nat
    assert te.LAUNCHES == {"accumulate": nat.SGR_TRAJ_ACCUMULATE_LAUNCHES, "errors": nat.SGR_TRAJ_ERRORS_LAUNCHES} == \
        {"accumulate": 2, "errors": 2}
    assert nat.SGR_TRAJ_MAX_POSES == nat.SGR_VIDEO_MAX_FRAMES == 65535


def test_there_is_no_cpu_path():
    with pytest.raises(RuntimeError, match="GPU"):
        te.pair_centres(torch.zeros(4, 7), np.tile(np.eye(4), (4, 1, 1)))
