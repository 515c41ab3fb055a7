"""No GPU: the fp64 SE3 oracle (tests/se3_ref.py) is right independently of its own formulas -- matrix exponential, round trips,
double cover, group identities -- its bound is sharp enough to catch the cancelling coefficient formulas `se3_exp` used to
have (restated here in numpy float32; this is a statement about the bound and the cases, not a test of the kernel), the bound stays
below 1e-5 on every input family of tests/test_gpu_se3.py, and the `lietorch` wrapper's device-free behaviour."""
import numpy as np
import pytest
import torch

import se3_cases as K
import se3_ref as R

F = np.float32


def _hat(v):
    z = np.zeros(v.shape[0])
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1), np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def _mat(pose):
    return R.matrix(pose)[0]


def _poses(n=200, seed=3):
    return K.random_poses(n, seed).astype(np.float64)


def test_series_coefficients_and_branch_continuity():
    assert np.allclose(R.C_SERIES[:3], [1 / 6, -1 / 120, 1 / 5040], rtol=1e-15)
    assert np.allclose(R.D_SERIES[:5], [1 / 12, 1 / 720, 1 / 30240, 1 / 1209600, 1 / 47900160], rtol=1e-15)
    lo, hi = np.array([[np.nextafter(R.SERIES_BELOW, 0)]]), np.array([[R.SERIES_BELOW]])
    for f in (R.coef_C, R.coef_D):
        for k in (0, 1):                                  # the value and a f'(a): series and closed form meet
            assert abs(f(lo)[k] - f(hi)[k]) <= 1e-13 * abs(f(hi)[k]) + (1e-11 if k else 0)
    a = np.array([[0.05], [0.2], [1.0], [3.0]])
    for f in (R.coef_B, R.coef_C, R.coef_D):              # a f'(a) against a central difference
        e = 1e-6
        num = a * (f(a * (1 + e))[0] - f(a * (1 - e))[0]) / (2 * e * a)
        assert np.allclose(f(a)[1], num, rtol=1e-6, atol=1e-10)


def test_exp_matches_the_matrix_exponential():
    tau, _, ang = K.exp_inputs(K.ANGLES, seed=11)
    tau = tau.astype(np.float64)
    tw = np.zeros((tau.shape[0], 4, 4))
    tw[:, :3, :3], tw[:, :3, 3] = _hat(tau[:, 3:]), tau[:, :3]
    ref = torch.linalg.matrix_exp(torch.from_numpy(tw)).numpy()
    err = np.abs(_mat(R.exp(tau)[0]) - ref).reshape(len(tau), -1).max(1)
    assert (err <= 1e-12 * (1 + np.linalg.norm(tau[:, :3], axis=1))).all(), (err.max(), ang[err.argmax()])


def test_log_round_trips():
    tau = K.exp_inputs([a for a in K.ANGLES + K.SWEEP if a < np.pi], seed=12)[0].astype(np.float64)
    back = R.log(R.exp(tau)[0])[0]
    assert np.abs(back - tau).max() <= 1e-12 * 4, np.abs(back - tau).max()                        # |tau| < 4
    X = np.concatenate([K.log_inputs(True).astype(np.float64), _poses(),
                        [[0.3, -1, 2, 0, 0, 0, -1], [0.3, -1, 2, 0.6, 0, 0.8, 0], [0, 0, 0, 0, 0, 0, 1]]], 0)
    X[:, 3:] /= np.linalg.norm(X[:, 3:], axis=1, keepdims=True)           # exp returns unit quaternions: compare on the group
    assert (X[:, 6] < 0).any() and (X[:, 6] == 0).any()
    tl = R.log(X)[0]
    assert (np.linalg.norm(tl[:, 3:], axis=1) <= np.pi + 1e-12).all()
    assert np.abs(_mat(R.exp(tl)[0]) - _mat(X)).max() <= 1e-12 * 3


def test_double_cover():
    X = _poses()
    Y = X.copy()
    Y[:, 3:] *= -1
    assert np.abs(_mat(X) - _mat(Y)).max() == 0.0
    assert np.abs(R.act(X, X[:, :3])[0] - R.act(Y, X[:, :3])[0]).max() == 0.0


def test_group_identities():
    X, Y = _poses(seed=4), _poses(seed=5)
    X[:, 3:] /= np.linalg.norm(X[:, 3:], axis=1, keepdims=True)
    Y[:, 3:] /= np.linalg.norm(Y[:, 3:], axis=1, keepdims=True)
    I = np.tile(np.eye(4), (len(X), 1, 1))
    assert np.abs(_mat(R.mul(R.inv(X)[0], X)[0]) - I).max() <= 1e-14 * 3
    assert np.abs(_mat(R.mul(X, R.inv(X)[0])[0]) - I).max() <= 1e-14 * 3
    MX, MY = _mat(X), _mat(Y)
    assert np.abs(MX[:, :3, :3] @ MX[:, :3, :3].transpose(0, 2, 1) - I[:, :3, :3]).max() <= 1e-14
    assert np.abs(_mat(R.mul(X, Y)[0]) - MX @ MY).max() <= 1e-14 * 5
    p = K.random_vectors(len(X), 3, 6).astype(np.float64)
    assert np.abs(R.act(X, p)[0] - ((MX[:, :3, :3] @ p[:, :, None])[:, :, 0] + MX[:, :3, 3])).max() <= 1e-14 * 5
    a, b = K.random_vectors(len(X), 6, 7).astype(np.float64), K.random_vectors(len(X), 6, 8).astype(np.float64)
    Rm, T = MX[:, :3, :3], _hat(MX[:, :3, 3])
    Ad = np.zeros((len(X), 6, 6))
    Ad[:, :3, :3], Ad[:, :3, 3:], Ad[:, 3:, 3:] = Rm, T @ Rm, Rm
    lhs = (R.adjT(X, a)[0] * b).sum(1)
    rhs = (a * (Ad @ b[:, :, None])[:, :, 0]).sum(1)
    assert np.abs(lhs - rhs).max() <= 1e-13
    # Ad is the adjoint of THIS exp: X exp(b) X^-1 = exp(Ad_X b)
    b *= 0.3
    lhs = _mat(R.mul(R.mul(X, R.exp(b)[0])[0], R.inv(X)[0])[0])
    assert np.abs(lhs - _mat(R.exp((Ad @ b[:, :, None])[:, :, 0])[0])).max() <= 1e-13


def test_magnitudes_dominate_values_and_units_respect_the_cap():
    X, Y = _poses(seed=4), _poses(seed=5)
    tau = K.exp_inputs(K.ANGLES + K.SWEEP)[0]
    for val, mag, units in (R.exp(tau), R.log(X), R.inv(X), R.mul(X, Y), R.act(X, Y[:, :3]), R.adjT(X, Y[:, :6]), R.matrix(X)):
        assert (np.abs(val) <= mag * (1 + 1e-12)).all()
        assert units.max() <= 32 and units.min() >= 0


def test_bounds_stay_below_1e5_on_the_inputs_of_the_gpu_tests():
    X, Y = K.random_poses(1000, 21), K.random_poses(1000, 22)
    P0, d = K.filler_inputs()
    outs = {"exp": R.exp(K.exp_inputs(K.ANGLES + K.THRESHOLD + K.SWEEP)[0]), "exp filler": R.exp(d),
            "log0": R.log(K.log_inputs(False)), "log1": R.log(K.log_inputs(True)), "inv": R.inv(X),
            "mul": R.mul(X, Y), "act": R.act(X, K.random_vectors(1000, 3, 23)), "adjT": R.adjT(X, K.random_vectors(1000, 6, 24)),
            "matrix": R.matrix(X)}
    for name, (val, mag, units) in outs.items():
        assert R.bound(mag, units).max() <= 1e-5, (name, R.bound(mag, units).max())


# ---------------------------------------------------------------------------------------------- fp32 emulation of se3_exp's translation
def _coef_cancelling(ang, t2):
    """what se3_exp formed until this test existed: 1 - cos and a - sin in fp32 above the series branch"""
    s, c = np.sin(ang), np.cos(ang)
    ser = ang < F(1e-4)
    safe_t2, safe_a = np.where(ser, F(1), t2), np.where(ser, F(1), ang)
    B = np.where(ser, F(0.5) - t2 / F(24), (F(1) - c) / safe_t2)
    C = np.where(ser, F(1) / F(6) - t2 / F(120), (safe_a - np.where(ser, F(0), s)) / (safe_t2 * safe_a))
    return B.astype(F), C.astype(F)


def _coef_stable(ang, t2):
    """what it forms now: B = (sin(a/2) / (a/2))^2 / 2, C by its series below a = 1"""
    ser = ang < F(1e-4)
    h = F(0.5) * np.where(ser, F(1), ang)
    r = np.sin(h) / h
    B = np.where(ser, F(0.5) - t2 / F(24), F(0.5) * r * r)
    c = [F(x) for x in R.C_SERIES[:5]]
    Cs = c[0] + t2 * (c[1] + t2 * (c[2] + t2 * (c[3] + t2 * c[4])))
    big = np.where(ang < F(1), F(2), ang)
    C = np.where(ang < F(1), Cs, (big - np.sin(big)) / (big * big * big))
    return B.astype(F), C.astype(F)


def _exp_translation_f32(tau, coef):
    tau = tau.astype(F)
    rho, th = tau[:, :3], tau[:, 3:]
    t2 = (th[:, 0] * th[:, 0] + th[:, 1] * th[:, 1] + th[:, 2] * th[:, 2])[:, None]
    B, C = coef(np.sqrt(t2), t2)
    cr = lambda a, b: np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    c1 = cr(th, rho)
    out = rho + B * c1 + C * cr(th, c1)
    assert out.dtype == F
    return out


def _exp_ratio(angles, coef):
    """worst |err| / bound of the emulated translation per angle, rho perpendicular to the axis with unit length, 16 axes each"""
    worst = []
    for a in angles:
        tau, kind, _ = K.exp_inputs([a] * 16, seed=5)
        tau = tau[kind == 2]
        val, mag, units = R.exp(tau)
        worst.append(R.worst_ratio(_exp_translation_f32(tau, coef), val[:, :3], mag[:, :3], units[:3]))
    return np.array(worst)


def test_bound_catches_the_cancelling_coefficients_and_passes_the_stable_ones():
    bad = _exp_ratio(K.DEFECT_ANGLES, _coef_cancelling)
    assert (bad > 1.0).all(), bad                                   # every one of the issue's angles violates the bound
    assert bad.max() > 10.0, bad
    fine = [0.0, 1e-9, 1e-6, 5e-5, 0.1, 1.0, 3.0, np.pi - 1e-6, np.pi + 0.5, 6.0]
    assert (_exp_ratio(fine, _coef_cancelling) <= 1.0).all()         # series branch and large angles were never wrong
    everything = K.DEFECT_ANGLES + fine + K.THRESHOLD + K.SWEEP + [0.999, 1.0, 1.001, 2.0]
    good = _exp_ratio(everything, _coef_stable)
    assert (good <= 1.0).all(), (good.max(), everything[int(good.argmax())])


def _round(out):
    return out[0].astype(F)


def _filler_g1_ratio(coef):
    """the trajectory-filler chain with every stage correctly rounded from the oracle except the translation of exp(v), which is the
    float32 emulation with the given coefficients: worst |matrix(G(1)) - matrix(P1)| / end-to-end bound"""
    P0, d = K.filler_inputs()
    P1 = _round(R.mul(_round(R.exp(d)), P0))
    P0i = _round(R.inv(P0))
    rel = _round(R.mul(P1, P0i))
    v = _round(R.log(rel))
    Es = _round(R.exp(v))
    Es[:, :3] = _exp_translation_f32(v, coef)
    G = _round(R.mul(Es, P0))
    bound, target = K.filler_end_to_end(P0, P1, P0i, rel, v, Es, G)
    return float((np.abs(_round(R.matrix(G)).astype(np.float64) - target) / bound).max()), float(bound[:, :3, :].max())


def test_end_to_end_filler_bound_catches_the_cancelling_coefficients():
    bad, _ = _filler_g1_ratio(_coef_cancelling)
    good, widest = _filler_g1_ratio(_coef_stable)
    assert bad > 1.0 and good <= 1.0, (bad, good)
    assert widest <= 5e-5, widest                       # entries are up to 2.5: a propagated bound, not a vacuous one


def test_effective_units_of_the_sensitivity_terms_are_what_se3_ref_reports():
    """the magnitudes of exp and log carry argument-sensitivity terms beyond the plain sum of terms (se3_ref docstring): pin how many
    roundings of the PLAIN magnitude the bounds amount to, so that the departure cannot grow unnoticed"""
    tau, _, ang = K.exp_inputs(K.ANGLES + K.THRESHOLD + K.SWEEP)
    e = R.effective_units(R.exp(tau), R.exp(tau, sensitivity=False))
    assert e[ang <= 0.1][:, :3].max() <= 26.1 and e[ang <= 0.1][:, 3:].max() <= 5.01
    assert e[ang <= 3.1][:, :3].max() <= 30.2 and e[ang <= 3.1][:, 3:6].max() <= 8.5 and e[:, :3].max() <= 36 and e[:, 3:6].max() <= 83
    for X in (K.log_inputs(False), K.log_inputs(True), K.random_poses(1000, 31, 1.0)):
        e = R.effective_units(R.log(X), R.log(X, sensitivity=False))
        assert e[:, 3:].max() <= 12.5 + 1e-9 and e[:, :3].max() <= 53
    e = R.effective_units(R.log(_round(R.exp(K.filler_inputs()[1]))), R.log(_round(R.exp(K.filler_inputs()[1])), sensitivity=False))
    assert e[:, :3].max() <= 35
    X = K.random_poses(50, 3)
    m = R.matrix(X)
    assert (m[2][3] == 0).all() and (m[2][:3, 3] == 0).all() and (R.inv(X)[2][3:] == 0).all()        # copies and constants: 0 units


# ---------------------------------------------------------------------------------------------- the wrapper, without a device
def test_wrapper_refuses_cpu_tensors_in_every_method():
    import lietorch
    X = lietorch.SE3.Identity(3, device="cpu")
    tau, pts = torch.zeros(3, 6), torch.zeros(3, 3)
    calls = [lambda: lietorch.SE3.exp(tau), X.log, X.inv, X.matrix, lambda: X * X, lambda: X * pts, lambda: X.act(pts),
             lambda: X.adjT(tau), lambda: X.retr(tau)]
    for call in calls:
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            call()


def test_wrapper_identity_and_indexing():
    import lietorch
    I = lietorch.SE3.Identity(2, 5, device="cpu")
    assert I.data.shape == (2, 5, 7) and I.data.dtype == torch.float32
    assert torch.equal(I.data, torch.tensor([0, 0, 0, 0, 0, 0, 1.0]).expand(2, 5, 7))
    assert lietorch.SE3.Identity(4, device="cpu", dtype=torch.float64).data.dtype == torch.float64
    assert lietorch.SE3.Identity(device="cpu").data.shape == (7,)
    assert lietorch.SE3.manifold_dim == 6 and lietorch.SE3.embedded_dim == 7
    d = torch.arange(6 * 7, dtype=torch.float32).reshape(6, 7)
    X = lietorch.SE3(d)
    assert X.vec() is d
    for idx, rows in ((2, d[2]), (slice(1, 4), d[1:4]), (torch.tensor([4, 0, 4]), d[[4, 0, 4]])):
        Y = X[idx]
        assert isinstance(Y, lietorch.SE3) and torch.equal(Y.data, rows)
