"""sgr_traj_accumulate / sgr_traj_errors and splat_slam_amd.traj_eval on the MI355X against the restatement and the bounds of
tests/traj_eval_ref.py: the centres bit for bit, the 17 sums and the error sums componentwise, every error per element, the extrema
and the two middle order statistics as exact elements of the kernel's own errors, and align + ape end to end."""
import numpy as np
import pytest
import torch

import traj_eval_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 2049]      # a partial wave, a partial workgroup, more than one workgroup's partials
S0, T0 = 1.6, np.array([0.4, -0.7, 2.0])
_CACHE = {}


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def trajectory(n, offset=0.0):
    """(poses [n,7] fp32 world -> camera, ref [n,4,4] fp32 camera -> world): centres spread over a box of extent about 1 (all three
    axes, so that the two leading singular values are of one order), the reference a similarity of them plus 2 % noise"""
    key = (n, offset)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 + n)
        x = rng.uniform(-0.5, 0.5, (n, 3)) * [1.0, 0.8, 0.7] + offset
        poses = R.w2c_from_centres(x, rng)
        y = S0 * (x - offset) @ rotation(rng).T + T0 + offset + 0.02 * rng.normal(size=(n, 3))
        ref = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
        for k in range(n):
            ref[k, :3, :3] = rotation(rng)
        ref[:, :3, 3] = y
        _CACHE[key] = (poses, ref)
    poses, ref = _CACHE[key]
    return poses.copy(), ref.copy()


def spoil(ref, rows, kind="nan"):
    for k, i in enumerate(rows):
        how = kind if kind != "mixed" else ("nan", "inf", "inf-inf")[k % 3]
        if how == "nan":
            ref[i, 0, 0] = np.nan
        elif how == "inf":
            ref[i, 3, 3] = np.inf                     # the last entry of the last quarter
        else:
            ref[i, 1, 1], ref[i, 2, 2] = np.inf, -np.inf          # finite everywhere else: the sum is inf - inf
    return ref


def extent(a):
    return float(np.abs(a - a.mean(0)).max()) if len(a) else 0.0


def check(poses, ref, inds=None, kind=None, est=None):
    """every assertion of the module on one call of each kernel; returns what the callers compare further"""
    import lietorch
    from splat_slam_amd import traj_eval as te
    kind = te.POSE7_W2C if kind is None else kind
    n = len(ref)
    est = torch.tensor(poses, device=DEV) if est is None else est
    ref_t = torch.tensor(ref, device=DEV)
    pairs = te.pair_centres(est, ref_t, kind, inds)
    again = te.pair_centres(est, ref_t, kind, inds)
    pos, valid = pairs.pos.cpu().numpy(), pairs.valid.cpu().numpy().astype(bool)
    # centres, bit for bit; the skip rule
    rows = est if inds is None else est[torch.as_tensor(inds, device=DEV).long()]
    if kind == te.POSE7_W2C:
        want_x = lietorch.SE3(rows[:n].contiguous()).inv().data[:, :3].double().cpu().numpy()
    else:
        want_x = rows[:n, :3, 3].double().cpu().numpy()
    assert np.array_equal(pos[:, 0], want_x)
    assert np.array_equal(pos[:, 1], ref[:, :3, 3].astype(np.float64), equal_nan=True)
    assert np.array_equal(valid, R.valid_rows(ref))
    # the 17 sums
    want, mag = R.fit_sums(pos[:, 0], pos[:, 1], valid)
    bound, allowed = R.fit_sum_bounds(n, want, mag)
    m = int(want[0])
    print(f"n={n} used={m} sums err/bound max {np.max(np.abs(pairs.sums - want) / np.maximum(bound, 1e-300)):.3f}")
    assert pairs.sums[0] == m == pairs.n_used
    assert (np.abs(pairs.sums - want) <= bound).all(), (pairs.sums - want, bound)
    assert (bound <= allowed).all()
    if m:
        x, y = pos[valid, 0], pos[valid, 1]
        sx, sy = float(np.abs(x).max()), float(np.abs(y).max())       # what the raw sums carry: the distance from the origin
        ex, ey = extent(x), extent(y)                                 # what the centred sums carry: the extent about the mean
        assert (bound[1:4] <= 1e-10 * sx).all() and (bound[4:7] <= 1e-10 * sy).all()
        if m > 1:
            assert bound[7] <= 1e-10 * ex * ex and (bound[8:17] <= 1e-10 * ex * ey).all()
    # the errors under the restatement's similarity (the identity where there is none)
    r, t, s = (np.eye(3), np.zeros(3), 1.0)
    if m >= 3:
        r, t, s, _ = R.umeyama(pos[valid, 0], pos[valid, 1])
    err_t, stats = pairs.errors(r, t, s)
    err_again, stats_again = again.errors(r, t, s)
    err = err_t.cpu().numpy()
    assert np.isnan(err[~valid]).all() and np.isfinite(err[valid]).all()
    e_want = R.errors(pos[valid, 0], pos[valid, 1], r, t, s)
    e_bound = R.error_bounds(pos[valid, 0], pos[valid, 1], r, t, s)
    assert (np.abs(err[valid] - e_want) <= e_bound).all(), np.max(np.abs(err[valid] - e_want) / e_bound)
    own = R.stat_sums(err[valid])                   # of the kernel's own errors: the order statistics are exact, the sums bounded
    s_bound, s_allowed = R.stat_sum_bounds(n, own)
    assert stats[0] == m
    assert np.array_equal(stats[3:7], own[3:7], equal_nan=True), (stats, own)
    assert (np.abs(stats[[1, 2, 7]] - own[[1, 2, 7]]) <= s_bound[[1, 2, 7]]).all(), (stats - own, s_bound)
    assert (s_bound <= s_allowed).all()
    # two calls give identical bits
    assert np.array_equal(again.sums.view(np.int64), pairs.sums.view(np.int64))
    assert torch.equal(again.pos.view(torch.int64), pairs.pos.view(torch.int64)) and torch.equal(again.valid, pairs.valid)
    assert torch.equal(err_again.view(torch.int64), err_t.view(torch.int64))
    assert np.array_equal(stats_again.view(np.int64), stats.view(np.int64))
    return pairs, err_t, stats


@pytest.mark.parametrize("n", SIZES)
def test_every_size_with_a_few_skipped_rows(n):
    poses, ref = trajectory(n)
    check(poses, spoil(ref, range(5, n, 17), "mixed"))


@pytest.mark.parametrize("n", SIZES)
def test_every_size_without_a_skipped_row(n):
    check(*trajectory(n))


@pytest.mark.parametrize("where", ["first", "last", "all but three", "everywhere"])
@pytest.mark.parametrize("kind", ["nan", "inf", "inf-inf"])
def test_skipped_rows_in_the_first_slot_the_last_slot_almost_everywhere_and_everywhere(where, kind):
    n = 257
    poses, ref = trajectory(n)
    rows = {"first": [0], "last": [n - 1], "all but three": [i for i in range(n) if i not in (0, 130, n - 1)], "everywhere": range(n)}[where]
    pairs, _, stats = check(poses, spoil(ref, rows, kind))
    assert pairs.n_used == n - len(rows)
    if where == "everywhere":
        assert (pairs.sums == 0).all() and (stats[:3] == 0).all() and stats[7] == 0 and np.isnan(stats[3:7]).all()


@pytest.mark.parametrize("n", [257, 2049])
def test_a_trajectory_far_from_the_origin(n):
    """offset 1e3, extent 1: without the centred pass the covariance would be the difference of two numbers of 1e6 n"""
    check(*trajectory(n, offset=1000.0))


def test_a_scrambled_row_list_with_a_gap_reads_the_same_rows_as_a_copy():
    from splat_slam_amd import traj_eval as te
    n, rows = 129, 300
    rng = np.random.default_rng(7)
    inds = rng.permutation(np.r_[0:40, 150:rows])[:n]               # no row of [40, 150)
    _, ref = trajectory(n)
    centres = np.zeros((rows, 3))
    centres[inds] = R.centres_w2c(trajectory(n)[0])
    buf = torch.tensor(R.w2c_from_centres(centres, rng), device=DEV)
    spoil(ref, [3, 77], "mixed")
    a, err_a, stats_a = check(None, ref, inds=inds.tolist(), est=buf)
    b, err_b, stats_b = check(None, ref, est=buf[torch.as_tensor(inds, device=DEV)].contiguous())
    assert torch.equal(a.pos.view(torch.int64), b.pos.view(torch.int64)) and np.array_equal(a.sums.view(np.int64), b.sums.view(np.int64))
    assert torch.equal(err_a.view(torch.int64), err_b.view(torch.int64)) and np.array_equal(stats_a.view(np.int64), stats_b.view(np.int64))
    c = te.pair_centres(buf, torch.tensor(ref, device=DEV), te.POSE7_W2C, torch.as_tensor(inds, device=DEV))     # a device list is read back
    assert np.array_equal(c.sums.view(np.int64), a.sums.view(np.int64))


def test_both_input_kinds_on_the_same_poses():
    import lietorch
    from splat_slam_amd import traj_eval as te
    poses, ref = trajectory(257)
    spoil(ref, [0, 100, 256], "mixed")
    a, err_a, stats_a = check(poses, ref)
    c2w = lietorch.SE3(torch.tensor(poses, device=DEV)).inv().matrix()
    b, err_b, stats_b = check(None, ref, kind=te.MAT4_C2W, est=c2w)
    assert torch.equal(a.pos.view(torch.int64), b.pos.view(torch.int64)) and np.array_equal(a.sums.view(np.int64), b.sums.view(np.int64))
    assert torch.equal(err_a.view(torch.int64), err_b.view(torch.int64)) and np.array_equal(stats_a.view(np.int64), stats_b.view(np.int64))


@pytest.mark.parametrize("n,offset", [(63, 0.0), (257, 0.0), (2049, 0.0), (257, 1000.0)])
def test_align_and_ape_end_to_end(n, offset):
    """rtol 1e-9: the sums agree to ~1e-13 and the 3 x 3 SVD amplifies by at most the inverse relative gap of the two leading singular
    values, held to >= 0.1 on the restatement alone: a hundred-fold margin"""
    from splat_slam_amd import traj_eval as te
    poses, ref = trajectory(n, offset)
    spoil(ref, range(4, n, 29), "mixed")
    est = torch.tensor(poses, device=DEV)
    al = te.align(est, torch.tensor(ref, device=DEV))
    got = te.ape(al)
    valid = R.valid_rows(ref)
    x = al.pairs.pos[:, 0].cpu().numpy()              # the kernel's fp32 centres (held bit for bit above), not an fp64 inverse
    y = ref[:, :3, 3].astype(np.float64)
    r, t, s, d = R.umeyama(x[valid], y[valid])
    want = R.ape(R.errors(x[valid], y[valid], r, t, s))
    assert d[1] / d[0] >= 0.1 and want["min"] >= 1e-3 * want["rmse"]
    print(f"n={n} s={al.s} ({s}) rmse={got['rmse']} ({want['rmse']}) d={d}")
    assert al.n_used == int(valid.sum()) and al.n_skipped == n - al.n_used
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))
    assert abs(al.s - s) <= 1e-9 * s and rel(al.r_a, r) <= 1e-9 and rel(al.t_a, t) <= 1e-9
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-9 * want[k], (k, got[k], want[k])
    assert abs(al.s - S0) < 0.05                      # ... and it is the similarity the trajectory was built with
    # no alignment: the pairs as they are
    raw = te.ape(None, al.pairs)
    want_raw = R.ape(R.errors(x[valid], y[valid], np.eye(3), np.zeros(3), 1.0))
    assert all(abs(raw[k] - want_raw[k]) <= 1e-9 * want_raw[k] for k in want_raw)


def test_degenerate_trajectories_and_bad_row_lists_are_refused():
    from splat_slam_amd import _native as nat
    from splat_slam_amd import traj_eval as te
    for n in (1, 2):
        poses, ref = trajectory(n)
        with pytest.raises(te.TrajectoryDegenerate):
            te.align(torch.tensor(poses, device=DEV), torch.tensor(ref, device=DEV))
    poses, ref = trajectory(65)
    with pytest.raises(te.TrajectoryDegenerate):
        te.align(torch.tensor(poses, device=DEV), torch.tensor(spoil(ref.copy(), range(65), "mixed"), device=DEV))
    est, ref_t = torch.tensor(poses, device=DEV), torch.tensor(ref, device=DEV)
    for bad in (65, -1, 2 ** 40):
        inds = list(range(64)) + [bad]
        with pytest.raises(RuntimeError, match="outside"):
            te.pair_centres(est, ref_t, te.POSE7_W2C, inds)
    with pytest.raises(ValueError):
        te.pair_centres(est[:64], ref_t)              # fewer estimated rows than reference poses
    lib = nat.lib()
    assert lib.sgr_traj_scratch_bytes(0) == 0 == lib.sgr_traj_scratch_bytes(65536) and lib.sgr_traj_scratch_bytes(65535) > 0
    assert lib.sgr_traj_scratch_bytes(1) >= 64 + 8
