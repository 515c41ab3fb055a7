"""sgr_traj_associate / sgr_traj_pose_errors and the layers of splat_slam_amd.traj_eval over them on the MI355X, against a numpy fp64
restatement of the equations of DESIGN.md section 3, "Trajectory scoring", written here from the same fp32 inputs (evo is not used).

Integer outputs (match, the compacted lists, the counts, pair_rows) are held exactly.  Every error is held per element to a bound that
is derived, not tuned.  u = 2^-53, gamma_k = k u / (1 - k u).  Every quantity X of the restatement carries a majorant M_X >= |X| (the
same expression with every term replaced by its absolute value) and a count k_X of the roundings on the longest path to it, such that
|fl(X) - X| <= gamma_{k_X} M_X for ANY order of the additions (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1 and
section 3.5); a fused multiply-add only removes roundings.  The rules, from the equations:

    an fp32 input widened to fp64                 k = 0
    a - b                                         k = max(k_a, k_b) + 1, M = M_a + M_b
    a dot product of three terms, sum_k a_k b_k   k = k_a + k_b + 3 (a product, two additions), M = sum_k M_a,k M_b,k
    the unit quaternion q / |q|                   k = 4: |q|^2 is four squares and three additions of positive terms (gamma_4), the square
                                                  root halves that and rounds once (3), the division rounds once
    an entry of R(q)                              k = 11: a product of two components (4 + 4 + 1), one addition, the doubling is exact,
                                                  and on the diagonal the subtraction from 1; M = the entry's formula over |q|, + 1 there
    |v|_2 over m terms of a vector v              |v'|_2 differs from |v|_2 by at most gamma_{k_v} |M_v|_2 (the triangle inequality), and
                                                  forming it costs m squares, m - 1 additions (gamma_m of a sum of positive terms), halved by
                                                  the square root, which rounds once: (m / 2 + 1) u |M_v|_2
    atan2(y, x)                                   |d theta| <= hypot(dx, dy) / (r - dx - dy), r = hypot(x, y) (= 2 for a rotation: nowhere
                                                  ill conditioned), plus the function's own error: 6 ulp on the device (the bound OpenCL
                                                  sets for double atan2, which the device library is written to) and 1 ulp in numpy,
                                                  1 ulp(theta) <= 2 u theta

The kernel and the restatement both satisfy these, so they differ by at most twice the figure of one evaluation (SLACK covers the
terms of second order in u).  The statistics are held as tests/test_gpu_traj_eval.py holds those of sgr_traj_errors: the extrema
and the two middle order statistics are exact elements of the kernel's own err, the three sums lie within the bounds of
tests/traj_eval_ref.py for the addition trees of the same code."""
import math

import numpy as np
import pytest
import torch

import traj_eval_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -53
SLACK = 1.0 + 1e-6
ATAN2_ULPS = 6 + 1
RELS = ["translation_part", "rotation_angle_rad", "rotation_angle_deg", "rotation_part", "full_transformation"]
IDENT = (1.0, np.eye(3), np.zeros(3))


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
class V:
    """values, their majorants and the rounding count of the longest path"""

    def __init__(self, val, mag=None, k=0):
        self.val = np.asarray(val, np.float64)
        self.mag = np.abs(self.val) if mag is None else np.asarray(mag, np.float64)
        self.k = k

    def __getitem__(self, idx):
        return V(self.val[idx], self.mag[idx], self.k)


def sub(a, b):
    return V(a.val - b.val, a.mag + b.mag, max(a.k, b.k) + 1)


def tdot(a, b):
    """a^T b over [.,3,3] x [.,3,3] or [.,3,3] x [.,3]"""
    spec = "nki,nkj->nij" if b.val.ndim == 3 else "nki,nk->ni"
    return V(np.einsum(spec, a.val, b.val), np.einsum(spec, a.mag, b.mag), a.k + b.k + 3)


def inv_mul(a, b):
    """a^-1 b of rigid poses (R, t): [Ra^T Rb | Ra^T (tb - ta)]"""
    return tdot(a[0], b[0]), tdot(a[0], sub(b[1], a[1]))


def quat_c2w_rotation(q):
    """R(q)^T of the normalised quaternion (x, y, z, w) as a V [.,3,3]: the rotation of the camera -> world pose"""
    def entries(x, y, z, w, one):
        return np.stack([one - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
                         2.0 * (x * y + z * w), one - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                         2.0 * (x * z - y * w), 2.0 * (y * z + x * w), one - 2.0 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        qn = q / np.sqrt((q * q).sum(1, keepdims=True))
    x, y, z, w = qn.T
    val = entries(x, y, z, w, 1.0)
    ax, ay, az, aw = np.abs(qn).T
    xy, xz, yz = 2.0 * (ax * ay + az * aw), 2.0 * (ax * az + ay * aw), 2.0 * (ay * az + ax * aw)      # symmetric: as it is for the transpose
    mag = np.stack([1.0 + 2.0 * (ay * ay + az * az), xy, xz, xy, 1.0 + 2.0 * (ax * ax + az * az), yz,
                    xz, yz, 1.0 + 2.0 * (ax * ax + ay * ay)], -1).reshape(-1, 3, 3)
    return V(val.transpose(0, 2, 1), mag, 11)


def poses_of(est, ref, kind_mat4, sim3, est_inds, ref_inds, n):
    """(P, Q, used): the aligned estimate and the reference of every pair as (V R [n,3,3], V t [n,3]), and the used flags"""
    s, r_a, t_a = sim3
    e_rows = np.arange(n) if est_inds is None else np.asarray(est_inds, np.int64)
    q_rows = np.arange(n) if ref_inds is None else np.asarray(ref_inds, np.int64)
    used = (e_rows >= 0) & (e_rows < len(est)) & (q_rows >= 0) & (q_rows < len(ref))
    e = est[np.where(used, e_rows, 0)].astype(np.float64)
    q = ref[np.where(used, q_rows, 0)].astype(np.float64).reshape(n, 4, 4)
    used &= np.isfinite(q.reshape(n, 16)).all(1) & np.isfinite(e.reshape(n, -1)).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind_mat4:
            e = e.reshape(n, 4, 4)
            c_r, c_t = V(e[:, :3, :3]), V(e[:, :3, 3])
        else:
            c_r = quat_c2w_rotation(e[:, 3:7])
            t = V(e[:, :3])
            c_t = V(-np.einsum("nij,nj->ni", c_r.val, t.val), np.einsum("nij,nj->ni", c_r.mag, t.mag), c_r.k + 3)
        ra = np.broadcast_to(np.asarray(r_a, np.float64), (n, 3, 3))
        p_r = V(ra @ c_r.val, np.abs(ra) @ c_r.mag, c_r.k + 3)
        p_t = V(s * np.einsum("nij,nj->ni", ra, c_t.val) + t_a, abs(s) * np.einsum("nij,nj->ni", np.abs(ra), c_t.mag) + np.abs(t_a), c_t.k + 5)
    used &= np.isfinite(p_r.val.reshape(n, 9)).all(1) & np.isfinite(p_t.val).all(1)
    return (p_r, p_t), (V(q[:, :3, :3]), V(q[:, :3, 3])), used


def pairs_of(c, delta, all_pairs):
    if delta is None:
        return [(r, None) for r in range(c)]
    if all_pairs:
        return [(r, r + delta) for r in range(c - delta)]
    return [(k * delta, (k + 1) * delta) for k in range((c - 1) // delta if c >= 1 else 0)]


def norm_bound(v, terms):
    """one evaluation's bound on the 2-norm over the last axis of v"""
    return (gamma(v.k) + (terms / 2.0 + 1.0) * U) * np.sqrt((v.mag * v.mag).sum(-1)) * SLACK


def relation_of(E_r, E_t, relation):
    """(err [m], bound [m]): the relation's error of every E and the bound on |kernel - restatement|"""
    m = len(E_t.val)
    if relation == "translation_part":
        return np.sqrt((E_t.val * E_t.val).sum(1)), 2.0 * norm_bound(E_t, 3)
    if relation in ("rotation_part", "full_transformation"):
        eye = np.broadcast_to(np.eye(3), (m, 3, 3))
        d = sub(E_r, V(eye))
        d = V(d.val.reshape(m, 9), d.mag.reshape(m, 9), d.k)
        if relation == "full_transformation":
            d = V(np.concatenate([d.val, E_t.val], 1), np.concatenate([d.mag, E_t.mag], 1), max(d.k, E_t.k))
        return np.sqrt((d.val * d.val).sum(1)), 2.0 * norm_bound(d, d.val.shape[1])
    pick = lambda a, i, j, k, l: a[:, i, j] - a[:, k, l]
    a = V(np.stack([pick(E_r.val, 2, 1, 1, 2), pick(E_r.val, 0, 2, 2, 0), pick(E_r.val, 1, 0, 0, 1)], -1),
          np.stack([E_r.mag[:, 2, 1] + E_r.mag[:, 1, 2], E_r.mag[:, 0, 2] + E_r.mag[:, 2, 0], E_r.mag[:, 1, 0] + E_r.mag[:, 0, 1]], -1), E_r.k + 1)
    y, dy = np.sqrt((a.val * a.val).sum(1)), norm_bound(a, 3)
    x = E_r.val[:, 0, 0] + E_r.val[:, 1, 1] + E_r.val[:, 2, 2] - 1.0
    dx = gamma(E_r.k + 3) * (E_r.mag[:, 0, 0] + E_r.mag[:, 1, 1] + E_r.mag[:, 2, 2] + 1.0)
    theta, r = np.arctan2(y, x), np.hypot(x, y) - dx - dy
    assert (r > 1.0).all()                                  # 2 for a rotation: the inputs of this module are rotations to fp32
    bound = 2.0 * np.hypot(dx, dy) / r * SLACK + ATAN2_ULPS * 2.0 * U * theta
    if relation == "rotation_angle_deg":
        deg = 180.0 / math.pi
        return theta * deg, bound * deg + 2.0 * U * theta * deg
    return theta, bound


def oracle(est, ref, kind_mat4=False, sim3=IDENT, est_inds=None, ref_inds=None, delta=None, all_pairs=False):
    """what sgr_traj_pose_errors must return but for the relation: the used flags, pair_rows [m,2] and E of every item"""
    given = est_inds if est_inds is not None else ref_inds
    n = len(given) if given is not None else len(ref)
    P, Q, used = poses_of(est, ref, kind_mat4, sim3, est_inds, ref_inds, n)
    rows = np.flatnonzero(used)
    items = pairs_of(len(rows), delta, all_pairs)
    i = rows[[a for a, _ in items]] if items else np.zeros(0, np.int64)
    take = lambda X, idx: (X[0][idx], X[1][idx])
    if delta is None:
        E = inv_mul(take(Q, i), take(P, i))
        pair_rows = np.stack([i, np.full(len(i), -1)], 1)
    else:
        j = rows[[b for _, b in items]] if items else np.zeros(0, np.int64)
        E = inv_mul(inv_mul(take(Q, i), take(Q, j)), inv_mul(take(P, i), take(P, j)))
        pair_rows = np.stack([i, j], 1)
    return dict(n=n, used=used, pair_rows=pair_rows.astype(np.int32).reshape(-1, 2), E=E)


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
def native(est, ref, kind_mat4=False, sim3=IDENT, est_inds=None, ref_inds=None, delta=None, all_pairs=False, relation="translation_part"):
    """sgr_traj_pose_errors as it is: (err [n], pair_rows [n,2], stats [8], header [4]) as numpy"""
    from splat_slam_amd import _native as nat
    from splat_slam_amd import traj_eval as te
    est_t = torch.tensor(np.ascontiguousarray(est, np.float32).reshape(len(est), -1), device=DEV)
    ref_t = torch.tensor(np.ascontiguousarray(ref, np.float32).reshape(len(ref), 16), device=DEV)
    ei = None if est_inds is None else torch.as_tensor(np.asarray(est_inds), dtype=torch.int32, device=DEV)
    ri = None if ref_inds is None else torch.as_tensor(np.asarray(ref_inds), dtype=torch.int32, device=DEV)
    given = ei if ei is not None else ri
    n = int(given.numel()) if given is not None else len(ref)
    lib = nat.lib()
    nbytes = lib.sgr_traj_pose_errors_scratch_bytes(n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    err = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
    pair_rows = torch.full((n, 2), 7, dtype=torch.int32, device=DEV)
    stats = torch.full((8,), 7.0, dtype=torch.float64, device=DEV)
    header = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    s, r_a, t_a = sim3
    c_sim3 = (nat.C.c_double * 13)(float(s), *np.asarray(r_a, np.float64).reshape(9).tolist(), *np.asarray(t_a, np.float64).tolist())
    nat.check(lib.sgr_traj_pose_errors(te.MAT4_C2W if kind_mat4 else te.POSE7_W2C, est_t.data_ptr(), len(est), ref_t.data_ptr(), len(ref),
                                       nat.ptr(ei), nat.ptr(ri), n, c_sim3, nat.SGR_TRAJ_ABSOLUTE if delta is None else nat.SGR_TRAJ_RELATIVE,
                                       1 if delta is None else delta, int(all_pairs), te.RELATIONS[relation], err.data_ptr(),
                                       pair_rows.data_ptr(), stats.data_ptr(), header.data_ptr(), scratch.data_ptr(), nbytes,
                                       torch.cuda.current_stream().cuda_stream), "sgr_traj_pose_errors")
    return err.cpu().numpy(), pair_rows.cpu().numpy(), stats.cpu().numpy(), header.cpu().numpy()


def check(est, ref, relations=RELS, **kw):
    """every assertion of the module on one configuration, under each relation; returns {relation: err [m]}"""
    want = oracle(est, ref, **kw)
    n, m, c = want["n"], len(want["pair_rows"]), int(want["used"].sum())
    out = {}
    for relation in relations:
        err, pair_rows, stats, header = native(est, ref, relation=relation, **kw)
        assert header.tolist() == [m, c, n - c, 0], (relation, header, m, c)
        assert np.array_equal(pair_rows[:m], want["pair_rows"]) and (pair_rows[m:] == -1).all()
        assert np.isnan(err[m:]).all() and np.isfinite(err[:m]).all()
        e_want, bound = relation_of(*want["E"], relation)
        ratio = np.abs(err[:m] - e_want) / np.maximum(bound, 1e-300)
        print(f"{relation} n={n} c={c} m={m} err/bound max {ratio.max() if m else 0.0:.3f}, bound max {bound.max() if m else 0.0:.3g}")
        assert (np.abs(err[:m] - e_want) <= bound).all(), (relation, ratio.max())
        own = R.stat_sums(err[:m])
        s_bound, s_allowed = R.stat_sum_bounds(n, own)
        assert stats[0] == m
        assert np.array_equal(stats[3:7], own[3:7], equal_nan=True), (stats, own)
        assert (np.abs(stats[[1, 2, 7]] - own[[1, 2, 7]]) <= s_bound[[1, 2, 7]]).all() and (s_bound <= s_allowed).all()
        if m:
            assert stats[5] in err[:m] and stats[6] in err[:m] and 0.5 * (stats[5] + stats[6]) == np.median(err[:m])
        else:
            assert (stats[:3] == 0).all() and stats[7] == 0 and np.isnan(stats[3:7]).all()
        again = native(est, ref, relation=relation, **kw)               # the same bits twice
        for a, b in zip((err, pair_rows, stats, header), again):
            assert a.tobytes() == b.tobytes()
        out[relation] = err[:m]
    return out


# ---- trajectories --------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def small_rotation(rng, angle):
    w = rng.normal(size=3)
    w *= angle / np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(angle) / angle * K + (1 - np.cos(angle)) / angle ** 2 * K @ K


def trajectory(n):
    """(poses [n,7] fp32 world -> camera, est_c2w [n,4,4] fp64 of the same poses, ref [n,4,4] fp32): a random walk, the reference the
    estimate scaled by 1.3 with 2 % noise of the centres and 3 degrees of the rotations"""
    if n not in _CACHE:
        rng = np.random.default_rng(2000 + n)
        x = np.cumsum(rng.normal(scale=0.05, size=(n, 3)), 0)
        poses = R.w2c_from_centres(x, rng)
        q = poses[:, 3:].astype(np.float64)
        rot = quat_c2w_rotation(q).val
        c2w = np.tile(np.eye(4), (n, 1, 1))
        c2w[:, :3, :3], c2w[:, :3, 3] = rot, R.centres_w2c(poses)
        ref = c2w.copy()
        for k in range(n):
            ref[k, :3, :3] = rot[k] @ small_rotation(rng, 0.05)
        ref[:, :3, 3] = 1.3 * x + 0.02 * rng.normal(size=(n, 3))
        _CACHE[n] = (poses, c2w, ref.astype(np.float32))
    poses, c2w, ref = _CACHE[n]
    return poses.copy(), c2w.copy(), ref.copy()


def spoil(ref, rows):
    for k, i in enumerate(rows):
        if k % 3 == 0:
            ref[i, 0, 0] = np.nan
        elif k % 3 == 1:
            ref[i, 3, 3] = np.inf
        else:
            ref[i, 1, 1], ref[i, 2, 2] = np.inf, -np.inf
    return ref


SIM3 = (1.7, rotation(np.random.default_rng(5)), np.array([0.3, -0.2, 0.9]))


# ---- pose errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 1025])
def test_every_relation_absolute_and_relative_with_skipped_poses_in_every_position(n):
    poses, _, ref = trajectory(n)
    run = list(range(250, 262)) if n > 262 else list(range(n - 9, n - 2))        # a run across the workgroup boundary at 256
    spoil(ref, [0, n - 1] + run + list(range(40, n, 53)))
    poses[17, 4] = np.nan                                                        # an estimate that is not finite
    poses[18, 3:] = 0.0                                                          # a zero quaternion
    check(poses, ref, sim3=SIM3)
    check(poses, ref, sim3=SIM3, delta=1)
    check(poses, ref, sim3=SIM3, delta=7, relations=RELS[:2])
    check(poses, ref, sim3=SIM3, delta=7, all_pairs=True, relations=RELS[:2])


@pytest.mark.parametrize("n", [255, 256, 257, 1025])
def test_matrix_estimates_and_all_poses_skipped(n):
    _, c2w, ref = trajectory(n)
    check(c2w.astype(np.float32), ref, kind_mat4=True, sim3=SIM3, delta=3, relations=RELS[:1] + RELS[3:])
    bad = spoil(ref.copy(), range(n))
    for delta in (None, 1):
        check(c2w.astype(np.float32), bad, kind_mat4=True, delta=delta, relations=RELS[:2])


def test_the_smallest_trajectories_and_deltas_at_and_beyond_their_length():
    from splat_slam_amd import traj_eval as te
    poses, _, ref = trajectory(9)
    for n, delta in ((1, 1), (4, 4), (5, 4), (4, 5), (9, 4), (9, 2)):
        for all_pairs in (False, True):
            got = check(poses[:n], ref[:n], delta=delta, all_pairs=all_pairs, relations=RELS[:2])
            assert len(got["translation_part"]) == len(te.item_pairs(n, delta, all_pairs))
    check(poses[:1], ref[:1])
    est, ref_t = torch.tensor(poses, device=DEV), torch.tensor(ref, device=DEV)
    with pytest.raises(te.TrajectoryDegenerate):
        te.rpe(est[:1], ref_t[:1], delta=1)
    with pytest.raises(te.TrajectoryDegenerate):
        te.rpe(est[:4], ref_t[:4], delta=5)
    one = te.ape_pose(est[:1], ref_t[:1])
    assert one.n_items == 1 and one.stats["median"] == one.stats["max"] == float(one.err[0])


def test_index_lists_with_gaps_straight_from_associate():
    from splat_slam_amd import traj_eval as te
    n = 300
    poses, _, ref = trajectory(n)
    rng = np.random.default_rng(11)
    stamps_ref = np.arange(n) * 0.01 + 1000.0
    keep = np.sort(rng.choice(n, 140, replace=False))
    stamps_est = stamps_ref[keep] + rng.uniform(-0.002, 0.002, len(keep))
    stamps_est[::9] += 0.005                                                     # between two stamps, 0.003 from either: -1 in match
    est = poses[keep]
    lib_match = associate_native(stamps_est, stamps_ref, 0.0, 0.0025)
    want_match = argmin_match(stamps_est, stamps_ref, 0.0, 0.0025)
    assert np.array_equal(lib_match["match"], want_match) and (want_match < 0).sum() >= 10
    # the raw match list, -1 entries included, as ref_inds
    check(est, ref, ref_inds=want_match, sim3=SIM3, delta=2, relations=RELS[:2])
    check(est, ref, ref_inds=want_match, sim3=SIM3, relations=RELS[:1])
    # the wrapper on the compacted lists gives the same items
    a = te.associate(stamps_est, stamps_ref, max_diff=0.0025)
    assert a.n_matched == int((want_match >= 0).sum())
    assert np.array_equal(a.est_inds.cpu().numpy(), np.flatnonzero(want_match >= 0))
    assert np.array_equal(a.ref_inds.cpu().numpy(), want_match[want_match >= 0])
    al = te.Alignment(SIM3[1], SIM3[2], SIM3[0], 0, 0)
    pe = te.rpe(torch.tensor(est, device=DEV), torch.tensor(ref, device=DEV), al, delta=2, est_inds=a.est_inds, ref_inds=a.ref_inds)
    raw = native(est, ref, sim3=SIM3, ref_inds=want_match, delta=2)
    assert pe.n_items == raw[3][0] and pe.n_used == a.n_matched and pe.n_skipped == 0
    assert pe.err.cpu().numpy().tobytes() == raw[0][:pe.n_items].tobytes()
    assert np.array_equal(np.flatnonzero(want_match >= 0)[pe.pair_rows.cpu().numpy()], raw[1][:pe.n_items])
    assert pe.stats == te.ape_statistics(raw[2]) and sorted(pe.stats) == ["max", "mean", "median", "min", "rmse", "sse", "std"]


def exact_trajectory(n):
    """poses whose rotations are signed permutation matrices (unit quaternions with entries 0, +-1/2, +-1): R^T R = I holds exactly,
    which no rounded general rotation gives in any arithmetic; the translations are arbitrary fp32"""
    rng = np.random.default_rng(3)
    quats = np.array([[0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [.5, .5, .5, .5], [.5, -.5, .5, .5], [-.5, .5, .5, -.5]])
    q = quats[rng.integers(0, len(quats), n)]
    t = rng.normal(size=(n, 3)).astype(np.float32)
    poses = np.concatenate([t, q.astype(np.float32)], 1)
    rot = quat_c2w_rotation(q).val
    c2w = np.tile(np.eye(4), (n, 1, 1))
    c2w[:, :3, :3] = rot
    c2w[:, :3, 3] = -np.einsum("nij,nj->ni", rot, t.astype(np.float64))          # exact: every product is by 0 or +-1
    assert np.array_equal(c2w.astype(np.float32).astype(np.float64), c2w)
    return poses, c2w.astype(np.float32)


def test_identical_trajectories_give_exactly_zero_under_every_relation():
    poses, c2w = exact_trajectory(300)
    for kw in (dict(), dict(delta=1), dict(delta=4, all_pairs=True)):
        for est, mat4 in ((poses, False), (c2w, True)):
            for relation, err in check(est, c2w, kind_mat4=mat4, **kw).items():
                assert (err == 0.0).all() and len(err) > 0, relation
    # general rotations: zero to the bound (R^T R is I only to fp32 there), exactly zero for the translation part of matrices
    _, c2w, _ = trajectory(257)
    c2w = c2w.astype(np.float32)
    assert (check(c2w, c2w, kind_mat4=True)["translation_part"] == 0.0).all()
    check(c2w, c2w, kind_mat4=True, delta=2)


def test_relative_rotations_of_1e_8_of_pi_minus_1e_8_and_of_exactly_pi():
    axis_x = lambda a: np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    n = 8
    est = np.tile(np.eye(4), (n, 1, 1))
    ref = est.copy()
    est[:, :3, 3] = ref[:, :3, 3] = np.arange(n)[:, None] * [0.1, 0.0, 0.2]
    # the estimate turns by `a` between poses 2k and 2k + 1, the reference does not: the relative rotation error is `a`
    angles = [1e-8, np.pi - 1e-8, np.pi, 0.0]
    for k, a in enumerate(angles):
        est[2 * k + 1, :3, :3] = axis_x(a) if a != np.pi else np.diag([1.0, -1.0, -1.0])
    # fp32 cannot hold cos(1e-8) or sin(pi - 1e-8): the estimate is handed over as fp64-exact products of fp32 matrices, i.e. the
    # relative rotation is checked where the kernel forms it, from rotations that fp32 holds (1e-8 rad is sin = 1e-8, cos = 1)
    est32 = est.astype(np.float32)
    got = check(est32, ref.astype(np.float32), kind_mat4=True, delta=1, relations=RELS[1:3])["rotation_angle_rad"]
    assert abs(got[4] - np.pi) <= ATAN2_ULPS * 2.0 * U * np.pi and got[6] == 0.0      # items (4, 5): atan2(0, -2), and (6, 7): atan2(0, 2)
    assert abs(got[0] - 1e-8) <= 1e-8 * 2.0 ** -22                               # fp32 holds sin(1e-8) to 2^-24; atan2 keeps it
    assert abs(got[2] - (np.pi - float(np.float32(np.sin(1e-8))))) <= 1e-12


def test_an_alignment_with_a_scale_scales_the_translation_rpe_and_leaves_the_rotation_relations():
    poses, _, ref = trajectory(257)
    spoil(ref, [3, 100])
    base = check(poses, ref, delta=3)
    doubled = check(poses, ref, delta=3, sim3=(2.0, np.eye(3), np.zeros(3)))
    moved = check(poses, ref, delta=3, sim3=(1.7, np.eye(3), np.array([5.0, -6.0, 7.0])))
    for relation in RELS[1:4]:                                                   # r_a = I leaves every rotation's bits as they are
        assert base[relation].tobytes() == doubled[relation].tobytes() == moved[relation].tobytes()
    # P_i^-1 P_j of the estimate alone (a reference of identities): its translation is s times that of the unscaled estimate
    ident = np.tile(np.eye(4, dtype=np.float32), (257, 1, 1))
    one = check(poses, ident, delta=3, relations=RELS[:1])["translation_part"]
    two = check(poses, ident, delta=3, sim3=(2.0, np.eye(3), np.zeros(3)), relations=RELS[:1])["translation_part"]
    assert np.array_equal(two, 2.0 * one)                                        # a power of two: exactly
    s = check(poses, ident, delta=3, sim3=(1.7, np.eye(3), np.zeros(3)), relations=RELS[:1])["translation_part"]
    assert np.allclose(s, 1.7 * one, rtol=1e-12, atol=0.0)


def test_the_absolute_translation_error_agrees_with_align_and_ape():
    """e_i here is |Rq^T (s r x + t - y)| with the centre x from the fp64 inverse of the normalised pose; ape() scores |s r x32 + t - y|
    with x32 from the fp32 arithmetic of se3_inv on the pose as it is.  Per pose they differ by at most
        s |x32 - x|  +  eta |d|  +  the two fp64 evaluations,
    eta = |Rq Rq^T - I|_F (the reference's rotation is a rotation to fp32 only: | |Rq^T d| - |d| | <= eta |d|), and
    |x32 - x| <= 8 * 2^-24 |M| + | |q|^2 - 1 | (|x| + |t|): se3_inv's t + 2 (w c + d) passes every term through at most 8 fp32 roundings
    (M: the same expression over absolute values), and for q = rho q^ it returns R^ t + (rho^2 - 1)(R^ t - t).  mean, rmse, median,
    min and max move by at most the largest per-pose difference, std by at most twice that."""
    from splat_slam_amd import traj_eval as te
    n = 257
    poses, _, ref = trajectory(n)
    spoil(ref, [0, 77, n - 1])
    est, ref_t = torch.tensor(poses, device=DEV), torch.tensor(ref, device=DEV)
    al = te.align(est, ref_t)
    old = te.ape(al)
    new = te.ape_pose(est, ref_t, al)
    assert new.n_used == al.n_used and new.n_skipped == al.n_skipped == 3 and new.n_items == al.n_used
    valid = R.valid_rows(ref)
    p = poses.astype(np.float64)[valid]
    t, q = np.abs(p[:, :3]), np.abs(p[:, 3:])
    cross = lambda a, b: np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)
    c = cross(q[:, :3], t)
    M = t + 2.0 * (q[:, 3:4] * c + cross(q[:, :3], c))
    x = R.centres_w2c(poses)[valid]
    rho2 = (p[:, 3:] ** 2).sum(1)
    dx = 8.0 * 2.0 ** -24 * np.linalg.norm(M, axis=1) + np.abs(rho2 - 1.0) * (np.linalg.norm(x, axis=1) + np.linalg.norm(p[:, :3], axis=1))
    rq = ref[valid, :3, :3].astype(np.float64)
    eta = np.linalg.norm(rq @ rq.transpose(0, 2, 1) - np.eye(3), axis=(1, 2))
    e_old = al.pairs.errors(al.r_a, al.t_a, al.s)[0].cpu().numpy()[valid]
    want = oracle(poses, ref, sim3=(al.s, al.r_a, al.t_a))
    fp64 = relation_of(*want["E"], "translation_part")[1] + R.error_bounds(x, ref[valid, :3, 3], al.r_a, al.t_a, al.s)
    bound = (al.s * dx + eta * (e_old + al.s * dx)) * SLACK + fp64
    diff = np.abs(new.err.cpu().numpy() - e_old)
    print(f"per-pose difference / bound max {np.max(diff / bound):.3f}, bound max {bound.max():.3g}, error median {old['median']:.3g}")
    assert (diff <= bound).all() and bound.max() < 1e-3 * old["median"]         # ... and the bound is far below what is measured
    for k in ("mean", "rmse", "median", "min", "max"):
        assert abs(new.stats[k] - old[k]) <= bound.max(), k
    assert abs(new.stats["std"] - old["std"]) <= 2.0 * bound.max()


# ---- association ---------------------------------------------------------------------------------------------------------------------
def argmin_match(a, b, offset, max_diff):
    """evo's matching_time_indices: np.argmin takes the lowest index among equal distances"""
    out = np.full(len(a), -1, np.int32)
    for i, t in enumerate(np.asarray(a, np.float64)):
        d = np.abs(np.asarray(b, np.float64) + offset - t)
        j = int(np.argmin(d))
        if d[j] <= max_diff:
            out[i] = j
    return out


def associate_native(a, b, offset, max_diff):
    from splat_slam_amd import _native as nat
    a_t, b_t = torch.tensor(np.asarray(a, np.float64), device=DEV), torch.tensor(np.asarray(b, np.float64), device=DEV)
    na, nb = len(a), len(b)
    lib = nat.lib()
    nbytes = lib.sgr_traj_associate_scratch_bytes(na, nb)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((3, na), 7, dtype=torch.int32, device=DEV)
    header = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    nat.check(lib.sgr_traj_associate(a_t.data_ptr(), na, b_t.data_ptr(), nb, float(offset), float(max_diff), out[0].data_ptr(),
                                     out[1].data_ptr(), out[2].data_ptr(), header.data_ptr(), scratch.data_ptr(), nbytes,
                                     torch.cuda.current_stream().cuda_stream), "sgr_traj_associate")
    o = out.cpu().numpy()
    return dict(match=o[0], a_inds=o[1], b_inds=o[2], header=header.cpu().numpy())


def check_association(a, b, offset=0.0, max_diff=0.01):
    got, again = associate_native(a, b, offset, max_diff), associate_native(a, b, offset, max_diff)
    want = argmin_match(a, b, offset, max_diff)
    m = int((want >= 0).sum())
    assert np.array_equal(got["match"], want), (got["match"], want)
    assert got["header"].tolist() == [m, 0, 0, 0]
    assert np.array_equal(got["a_inds"][:m], np.flatnonzero(want >= 0)) and np.array_equal(got["b_inds"][:m], want[want >= 0])
    assert (got["a_inds"][m:] == -1).all() and (got["b_inds"][m:] == -1).all()
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    return want


def test_association_edge_cases():
    up = lambda v: np.nextafter(v, np.inf)
    assert check_association([5.0], [5.004]).tolist() == [0]                     # na = nb = 1
    assert check_association([5.0], [5.02]).tolist() == [-1]
    b = np.array([1.0, 2.0, 2.0, 2.0, 3.0, 4.0, 4.0, 6.0])
    # before the first and after the last, within and beyond max_diff; halfway between two (the lower wins); duplicates in b
    a = np.array([0.75, 0.25, 6.25, 9.0, 2.5, 3.5, 5.0, 2.0, 4.0, 2.25, 3.75])
    want = check_association(a, b, max_diff=0.5)
    assert want.tolist() == [0, -1, 7, -1, 1, 4, -1, 1, 5, 1, 5]
    # a distance exactly max_diff is a match, the next double above it is not (0.25, 0.5 and their sums are exact)
    assert check_association([2.25, 0.75, 6.5], b, max_diff=0.25).tolist() == [1, 0, -1]
    assert check_association([3.25], b, max_diff=0.25).tolist() == [4]
    assert check_association([up(3.25)], b, max_diff=0.25).tolist() == [-1]
    assert check_association([3.25], b, max_diff=np.nextafter(0.25, 0.0)).tolist() == [-1]
    # an offset of either sign
    assert check_association([11.0, 13.5], b, offset=10.0, max_diff=0.5).tolist() == [0, 4]
    assert check_association([-9.0, -6.5], b, offset=-10.0, max_diff=0.5).tolist() == [0, 4]
    # a NaN stamp in a matches nothing
    assert check_association([np.nan, 2.0], b).tolist() == [-1, 1]


@pytest.mark.parametrize("na", [256, 257, 1025])
@pytest.mark.parametrize("nb", [300, 70001])
def test_association_across_workgroups_on_two_clocks(na, nb):
    rng = np.random.default_rng(na + nb)
    b = np.cumsum(rng.choice([0.0, 0.01, 0.01, 0.02], nb)) + 1.3e9                # a 100 Hz clock with repeated stamps and gaps
    a = np.sort(rng.uniform(b[0] - 0.05, b[-1] + 0.05, na))
    a[::5] = b[rng.integers(0, nb, len(a[::5]))]                                 # exact hits, also on duplicates
    a[1::7] = 0.5 * (b[:-1] + b[1:])[rng.integers(0, nb - 1, len(a[1::7]))]       # (nearly) halfway stamps
    want = check_association(a, b, offset=0.0, max_diff=0.006)
    assert 0 < (want >= 0).sum() < na
    check_association(a, b, offset=0.004, max_diff=0.006)


def test_the_wrapper_searches_from_the_shorter_list_and_flips_the_offset():
    from splat_slam_amd import traj_eval as te
    rng = np.random.default_rng(4)
    long = np.arange(400) * 0.01
    short = np.sort(rng.choice(long, 90, replace=False)) + 0.25 + rng.uniform(-0.003, 0.003, 90)
    short[5] = long[200] + 0.25 + 0.005                                          # halfway between two stamps: 0.005 from either
    # est shorter: offset is added to the reference's stamps
    a = te.associate(short, long, max_diff=0.004, offset=0.25)
    want = argmin_match(short, long, 0.25, 0.004)
    assert a.n_matched == (want >= 0).sum() and a.est_inds.dtype == torch.int32 and a.est_inds.is_cuda
    assert np.array_equal(a.est_inds.cpu().numpy(), np.flatnonzero(want >= 0)) and np.array_equal(a.ref_inds.cpu().numpy(), want[want >= 0])
    # est longer: the search runs from the reference into the estimate, which takes -offset
    b = te.associate(long, short, max_diff=0.004, offset=-0.25)
    want = argmin_match(short, long, 0.25, 0.004)
    assert np.array_equal(b.ref_inds.cpu().numpy(), np.flatnonzero(want >= 0)) and np.array_equal(b.est_inds.cpu().numpy(), want[want >= 0])
    # GPU tensors are taken as they are
    c = te.associate(torch.tensor(short, device=DEV), torch.tensor(long, device=DEV), max_diff=0.004, offset=0.25)
    assert torch.equal(c.est_inds, a.est_inds) and torch.equal(c.ref_inds, a.ref_inds)
    with pytest.raises(te.TrajectoryDegenerate):
        te.associate(short, long + 100.0)


@pytest.mark.parametrize("where", [0, 1, 255, 256, 69998])
def test_unsorted_or_nan_stamps_of_the_longer_list_raise(where):
    from splat_slam_amd import traj_eval as te
    b = np.arange(70000) * 0.01
    a = np.array([1.0, 2.0, 3.0])
    te.associate(a, b)
    bad = b.copy()
    bad[where + 1] = bad[where] - 0.005
    assert associate_native(a, bad, 0.0, 0.01)["header"][1] == 1
    with pytest.raises(ValueError, match="order"):
        te.associate(a, bad)
    bad = b.copy()
    bad[where] = np.nan
    with pytest.raises(ValueError, match="order"):
        te.associate(a, bad)
    assert associate_native([1.0], [np.nan], 0.0, 0.01)["header"].tolist() == [0, 1, 0, 0]


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_the_command_line_on_two_tum_files_on_different_clocks(tmp_path, capsys):
    from splat_slam_amd import traj_eval as te
    n = 120
    _, c2w, ref = trajectory(300)
    rng = np.random.default_rng(9)
    stamps_ref = 1.3e9 + np.arange(300) * 0.01                                    # a 100 Hz reference clock
    keep = np.sort(rng.choice(300, n, replace=False))
    stamps_est = stamps_ref[keep] - 2.5 + rng.uniform(-0.002, 0.002, n)           # the estimate's clock runs 2.5 s behind
    te.write_tum_trajectory(tmp_path / "est.txt", stamps_est, c2w[keep])
    te.write_tum_trajectory(tmp_path / "ref.txt", stamps_ref, ref.astype(np.float64))
    argv = [str(tmp_path / "est.txt"), str(tmp_path / "ref.txt"), "--offset", "-2.5", "--max-diff", "0.005", "--rpe-delta", "2",
            "--relation", "rotation_angle_deg", "--out", str(tmp_path / "out")]
    assert te.main(argv) == 0
    text = capsys.readouterr().out
    assert "scale:" in text and "rpe_rotation_angle_deg_d2" in text
    assert open(tmp_path / "out" / "metrics_traj.txt").read().strip() == text.strip()
    got = te.evaluate_files(argv[0], argv[1], max_diff=0.005, offset=-2.5, rpe_delta=2, relation="rotation_angle_deg")
    # the restatement, from the files as the function reads them
    ts_e, est_f = te.read_tum_trajectory(argv[0])
    ts_r, ref_f = te.read_tum_trajectory(argv[1])
    assert np.array_equal(ts_e, stamps_est) and np.array_equal(ts_r, stamps_ref)
    match = argmin_match(ts_e, ts_r, -2.5, 0.005)
    assert got["n_matched"] == (match >= 0).sum() == n and np.array_equal(match, keep)
    est32, ref32 = est_f.astype(np.float32), ref_f.astype(np.float32)
    x, y = est32[:, :3, 3].astype(np.float64), ref32[match, :3, 3].astype(np.float64)
    r, t, s, d = R.umeyama(x, y)
    assert d[1] / d[0] >= 0.01
    ate = R.ape(R.errors(x, y, r, t, s))
    for k in ate:                                                                # rtol 1e-9, as test_gpu_traj_eval.py derives it
        assert abs(got["ate"][k] - ate[k]) <= 1e-9 * ate[k], k
    al = got["alignment"]
    want = oracle(est32, ref32, kind_mat4=True, sim3=(al.s, al.r_a, al.t_a), ref_inds=match, delta=2)
    e_want, bound = relation_of(*want["E"], "rotation_angle_deg")
    stats = R.ape(e_want)
    assert len(e_want) == (n - 1) // 2
    for k in ("mean", "rmse", "median", "min", "max"):
        assert abs(got["errors"][k] - stats[k]) <= bound.max(), k


def test_the_existing_entry_points_return_what_they_did_without_the_new_keywords():
    import inspect
    from splat_slam_amd import traj_eval as te
    from splat_slam_amd.depth_video import DepthVideo
    from splat_slam_amd.slam import Slam
    n = 40
    poses, _, ref = trajectory(n)
    video = DepthVideo(8, 8, buffer=n, device=DEV)
    video.poses[:] = torch.tensor(poses, device=DEV)
    video.timestamp[:] = torch.arange(n, device=DEV, dtype=torch.float32)
    video.counter.value = n
    plain = te.kf_traj_eval(video, ref)
    assert len(plain) == 4 and sorted(plain[0]) == ["max", "mean", "median", "min", "rmse", "sse", "std"]
    extra = [("translation_part", 3, False), ("rotation_angle_deg", None, False)]
    more = te.kf_traj_eval(video, ref, extra=extra)
    assert len(more) == 5 and more[0] == plain[0] and more[1] == plain[1]
    assert sorted(more[4]) == ["ape_rotation_angle_deg", "rpe_translation_part_d3"]
    al = te.Alignment(plain[2], plain[3], plain[1], 0, 0)
    est, ref_t = torch.tensor(poses, device=DEV), torch.tensor(ref, device=DEV)
    assert more[4]["rpe_translation_part_d3"] == te.rpe(est, ref_t, al, delta=3).stats
    assert more[4]["ape_rotation_angle_deg"] == te.ape_pose(est, ref_t, al, "rotation_angle_deg").stats
    assert 1.0 < more[4]["ape_rotation_angle_deg"]["mean"] < 5.0                 # the trajectory was built with 0.05 rad = 2.9 degrees

    class Filler:                                                                # the trajectory filler's interface: poses of every frame
        def __init__(self, video):
            self.video = video

        def __call__(self, stream):
            return self.video.poses[:n].clone()
    full = te.full_traj_eval(Filler(video), None, ref)
    assert len(full) == 3 and full[1] == plain[0] and tuple(full[0].shape) == (n, 4, 4)
    full_more = te.full_traj_eval(Filler(video), None, ref, extra=extra)
    assert len(full_more) == 4 and full_more[1] == full[1] and full_more[3] == more[4]
    # Slam.evaluate over the same video, with no map (the rendering block is skipped) and the filler above in the tracker's place
    import types
    import splat_slam_amd.trajectory_filler as tf
    slam = Slam.__new__(Slam)
    slam.video, slam.net, slam.stream = video, None, types.SimpleNamespace(poses=list(ref))
    slam.session = types.SimpleNamespace(init=True)
    real, tf.PoseTrajectoryFiller = tf.PoseTrajectoryFiller, lambda net, video, device=None: Filler(video)
    try:
        out = slam.evaluate()
        asked = slam.evaluate(rpe_delta=3, rotation_errors=True)
        only_rot = slam.evaluate(rotation_errors=True)
    finally:
        tf.PoseTrajectoryFiller = real
    assert sorted(out) == sorted(["kf_traj", "global_scale", "r_a", "t_a", "rendering", "depth_l1", "full_traj", "full_traj_alignment",
                                  "traj_est"]) and out["kf_traj"] == plain[0] and out["full_traj"] == plain[0]
    assert sorted(set(asked) - set(out)) == ["full_rot", "full_rpe", "kf_rot", "kf_rpe"] and asked["kf_traj"] == out["kf_traj"]
    assert asked["kf_rpe"] == asked["full_rpe"] == more[4]["rpe_translation_part_d3"]
    assert asked["kf_rot"] == asked["full_rot"] == more[4]["ape_rotation_angle_deg"]
    assert sorted(set(only_rot) - set(out)) == ["full_rot", "kf_rot"] and only_rot["kf_rot"] == asked["kf_rot"]
    sig = inspect.signature(Slam.evaluate).parameters
    assert sig["rpe_delta"].default is None and sig["rotation_errors"].default is False
    assert list(inspect.signature(te.kf_traj_eval).parameters)[:5] == ["video", "gt_poses", "out_dir", "npz_path", "plot"]
