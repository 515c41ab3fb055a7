"""-m gpu: the SE3 kernels (`se3_kernel<OP>`, csrc/sgr_aux.hip) and the `lietorch` wrapper over them against the fp64 oracle of
tests/se3_ref.py, element by element to |got - ref| <= C_op * 2^-24 * M (derived there, from the formulas): small angles and the
series thresholds of `exp` and `log`, w < 0, angles at and beyond pi, more than one workgroup and block boundaries through the C
ABI with guarded buffers, streams, broadcasting, views, dtypes, and the trajectory filler's interpolation pattern stage by stage.
Every case reports its worst |err| / bound; inputs come from the seeded generators of tests/se3_cases.py."""
import numpy as np
import pytest
import torch

import se3_cases as K
import se3_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FC5A5A5            # a NaN payload no kernel produces


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def ratio(name, got, ref, cols=slice(None)):
    """worst |err| / bound over the chosen columns of the last axis; printed so that a run records it"""
    val, mag, units = ref
    got = np.asarray(got, np.float64).reshape(val.shape)
    units = np.broadcast_to(units, val.shape)
    r = R.worst_ratio(got[..., cols], val[..., cols], mag[..., cols], units[..., cols])
    print(f"se3 ratio {name}: {r:.3f}")
    return r


def held(cases):
    """cases: {name: ratio}; every one must be <= 1"""
    bad = {k: round(v, 2) for k, v in cases.items() if not v <= 1.0}
    assert not bad, f"worst |err| / bound beyond 1: {bad}"


def SE3(x):
    import lietorch
    return lietorch.SE3(dev(x) if isinstance(x, np.ndarray) else x)


# ------------------------------------------------------------------------------------------------------------------ exp and log
def test_exp_across_angles_and_thresholds():
    import lietorch
    tau, kind, ang = K.exp_inputs(K.ANGLES + K.THRESHOLD + K.SWEEP)
    got = host(lietorch.SE3.exp(dev(tau)).data)
    cases = {}
    for k, name in enumerate(("rho=0", "rho parallel", "rho perpendicular")):
        rows = kind == k
        ref = R.exp(tau[rows])
        small = ang[rows] < 3e-2
        for sel, tag in ((small, "a<3e-2"), (~small, "a>=3e-2")):
            sub = tuple(x[sel] if x.ndim == 2 else x for x in ref)
            cases[f"exp t {name} {tag}"] = ratio(f"exp t {name} {tag}", got[rows][sel], sub, slice(0, 3))
            cases[f"exp q {name} {tag}"] = ratio(f"exp q {name} {tag}", got[rows][sel], sub, slice(3, 7))
    held(cases)
    zero = got[kind == 0][ang[kind == 0] == 0.0]
    assert np.array_equal(zero, np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32))            # exp(0) is the exact identity


@pytest.mark.parametrize("perpendicular", [False, True])
def test_log_across_its_branches(perpendicular):
    X = K.log_inputs(perpendicular)
    assert (X[:, 6] < 0).any() and (X[:, 6] == 0).any()
    n = np.linalg.norm(X[:, 3:6].astype(np.float64), axis=1)
    assert (n[n > 0] < 1e-6).any() and ((n > 1e-6) & (n < 1.1e-6)).any()                    # both sides of the nn branch
    got = host(SE3(X).log())
    ref = R.log(X)
    tag = "t perpendicular" if perpendicular else "t=0"
    held({"theta": ratio(f"log theta {tag}", got, ref, slice(3, 6)), "rho": ratio(f"log rho {tag}", got, ref, slice(0, 3))})
    assert (np.linalg.norm(got[:, 3:].astype(np.float64), axis=1) <= np.pi * (1 + 1e-6)).all()


def test_log_of_general_poses():
    """translation neither zero nor perpendicular to the axis: D (theta x (theta x t)) has elements that |t_k| does not cover"""
    X = np.concatenate([K.random_poses(500, 31, tmax=1.0), K.filler_inputs(200, 32)[0]], 0)
    _, d = K.filler_inputs(200, 33)
    small = R.exp(d)[0].astype(np.float32)                                                  # rotations of 1e-4 .. 3e-2
    got = host(SE3(np.concatenate([X, small], 0)).log())
    ref = R.log(np.concatenate([X, small], 0))
    held({"theta": ratio("log theta general", got, ref, slice(3, 6)), "rho": ratio("log rho general", got, ref, slice(0, 3))})


# ------------------------------------------------------------------------------------------------------------------ group ops
@pytest.fixture(scope="module")
def poses():
    X, Y, Z = (K.random_poses(1000, s) for s in (21, 22, 25))
    assert (X[:, 6] < 0).sum() > 100 and np.array_equal(X[0], np.array([0, 0, 0, 0, 0, 0, 1], np.float32))
    return X, Y, Z


def test_inv_mul_act_adjT_matrix(poses):
    X, Y, _ = poses
    pts, a6 = K.random_vectors(1000, 3, 23), K.random_vectors(1000, 6, 24)
    gi = host(SE3(X).inv().data)
    gm = host((SE3(X) * SE3(Y)).data)
    cases = {"inv t": ratio("inv t", gi, R.inv(X), slice(0, 3)), "inv q": ratio("inv q", gi, R.inv(X), slice(3, 7)),
             "mul t": ratio("mul t", gm, R.mul(X, Y), slice(0, 3)), "mul q": ratio("mul q", gm, R.mul(X, Y), slice(3, 7)),
             "act": ratio("act", host(SE3(X).act(dev(pts))), R.act(X, pts)),
             "adjT": ratio("adjT", host(SE3(X).adjT(dev(a6))), R.adjT(X, a6)),
             "matrix": ratio("matrix", host(SE3(X).matrix()), R.matrix(X))}
    held(cases)
    assert np.array_equal(gi[:, 3:], X[:, 3:] * np.array([-1, -1, -1, 1], np.float32))      # the conjugate is exact


def _end_to_end(name, got, target, exact, last, earlier, tmax):
    """|got - target| against the propagated bound (se3_ref.chain_bound: last stage + every earlier one carried once, to first
    order) plus the oracle's own fp64 defect |exact chain - target| of the identity on these fp32 inputs"""
    b = R.chain_bound(last, earlier, tmax) + np.abs(exact - target)
    r = float((np.abs(np.asarray(got, np.float64) - target) / b).max())
    print(f"se3 ratio {name}: {r:.3f}   (widest bound {b.max():.2e})")
    return r


def test_round_trips_on_the_device(poses):
    import lietorch
    X, Y, Z = (p[:256].copy() for p in poses)
    for p in (X, Y, Z):
        p[:, :3] *= 0.5                                                                      # |t| <= 1
    B = lambda out: R.bound(out[1], out[2])
    car, tn = R.carried, K._tn
    cases = {}
    # exp(log(X)) against X, by matrix: every stage against the oracle fed the stage before, then end to end
    tau = host(SE3(X).log())
    P = host(lietorch.SE3.exp(dev(tau)).data)
    M = host(SE3(P).matrix())
    cases["log"], cases["exp(log)"], cases["matrix"] = ratio("rt log", tau, R.log(X)), ratio("rt exp", P, R.exp(tau)), ratio("rt matrix", M, R.matrix(P))
    exact = R.matrix(R.exp(R.log(X)[0])[0])[0]
    rho = np.linalg.norm(tau[:, :3].astype(np.float64), axis=1)
    cases["exp(log(X)) = X"] = _end_to_end("rt exp(log(X)) = X", M, R.matrix(X)[0], exact, B(R.matrix(P)),
                                           [car(B(R.log(X)), tangent=True, rho=rho), car(B(R.exp(tau)))], tn(X))
    # inverses
    Xi = host(SE3(X).inv().data)
    eye = np.tile(np.eye(4), (256, 1, 1))
    for name, (a, b) in {"inv(X) X": (Xi, X), "X inv(X)": (X, Xi)}.items():
        prod = host((SE3(a) * SE3(b)).data)
        M = host(SE3(prod).matrix())
        cases[name + " stage"] = max(ratio(f"rt {name} mul", prod, R.mul(a, b)), ratio(f"rt {name} matrix", M, R.matrix(prod)))
        ex = R.matrix(R.mul(R.inv(X)[0], X)[0] if a is Xi else R.mul(X, R.inv(X)[0])[0])[0]
        cases[name + " = I"] = _end_to_end(f"rt {name} = I", M, eye, ex, B(R.matrix(prod)), [car(B(R.inv(X))), car(B(R.mul(a, b)))], tn(X, Xi))
    # associativity
    XY, YZ = host((SE3(X) * SE3(Y)).data), host((SE3(Y) * SE3(Z)).data)
    L, Rr = host((SE3(XY) * SE3(Z)).data), host((SE3(X) * SE3(YZ)).data)
    ML, MR = host(SE3(L).matrix()), host(SE3(Rr).matrix())
    exL, exR = R.matrix(R.mul(R.mul(X, Y)[0], Z)[0])[0], R.matrix(R.mul(X, R.mul(Y, Z)[0])[0])[0]
    T = tn(X, Y, Z, XY, YZ, L)
    bL = R.chain_bound(B(R.matrix(L)), [car(B(R.mul(X, Y))), car(B(R.mul(XY, Z)))], T)
    bR = R.chain_bound(B(R.matrix(Rr)), [car(B(R.mul(Y, Z))), car(B(R.mul(X, YZ)))], T)
    cases["(XY)Z"] = float((np.abs(ML - exL) / bL).max())
    cases["X(YZ)"] = float((np.abs(MR - exR) / bR).max())
    cases["(XY)Z = X(YZ)"] = float((np.abs(ML.astype(np.float64) - MR) / (bL + bR + np.abs(exL - exR))).max())
    for k in ("(XY)Z", "X(YZ)", "(XY)Z = X(YZ)"):
        print(f"se3 ratio rt {k}: {cases[k]:.3f}   (widest bound {(bL + bR).max():.2e})")
    held(cases)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
OPS = {   # name: (widths of the inputs, width of the output, oracle)
    "se3_exp": ((6,), 7, R.exp), "se3_log": ((7,), 6, R.log), "se3_inv": ((7,), 7, R.inv), "se3_mul": ((7, 7), 7, R.mul),
    "se3_act": ((7, 3), 3, R.act), "se3_adjT": ((7, 6), 6, R.adjT), "se3_matrix": ((7,), 16, R.matrix)}


def _abi_inputs(op, n):
    widths = OPS[op][0]
    if op == "se3_exp":
        rng = np.random.default_rng(41)
        tau, _, _ = K.exp_inputs(np.exp(rng.uniform(np.log(1e-6), np.log(3.0), 1000)), seed=42)
        return [tau[2000:2000 + n]]                                   # rho perpendicular
    ins = [K.random_poses(1001, 43, tmax=1.0)[1:n + 1]]
    if len(widths) == 2:
        ins.append(K.random_poses(1001, 44)[1:n + 1] if widths[1] == 7 else K.random_vectors(1000, widths[1], 45)[:n])
    return ins


def _abi_call(op, ins, n, out, stream=None):
    from splat_slam_amd import _native as nat
    return getattr(nat.lib(), op)(*[None if t is None else t.data_ptr() for t in ins], n, None if out is None else out.data_ptr(), stream)


@pytest.mark.parametrize("op", list(OPS))
def test_sizes_guard_rows_inputs_and_reproducibility(op):
    widths, wo, oracle = OPS[op]
    cases = {}
    for n in (0, 1, 255, 256, 257, 1000):
        ins_np = _abi_inputs(op, n)
        ins = [dev(x) for x in ins_np]
        outs = []
        for _ in range(2):
            guard = torch.full((n + 64, wo), SENTINEL, dtype=torch.int32, device=DEV)
            assert _abi_call(op, ins, n, guard.view(torch.float32)) == 0
            torch.cuda.synchronize()
            assert bool((guard[n:] == SENTINEL).all()), f"{op} n={n}: wrote past row n"
            outs.append(guard[:n].clone())
        assert torch.equal(outs[0], outs[1]), f"{op} n={n}: two calls differ"                 # bit reproducible
        for t, x in zip(ins, ins_np):
            assert np.array_equal(host(t).view(np.int32), x.view(np.int32)), f"{op} n={n}: an input was written"
        if n:
            assert not bool((outs[0] == SENTINEL).any()), f"{op} n={n}: a row was not written"
            cases[f"n={n}"] = ratio(f"{op} n={n}", host(outs[0].view(torch.float32)), oracle(*ins_np))
    held(cases)


@pytest.mark.parametrize("op", list(OPS))
def test_null_and_negative_arguments_are_refused_without_a_launch(op):
    from splat_slam_amd import _native as nat
    widths, wo, _ = OPS[op]
    assert _abi_call(op, [None] * len(widths), 0, None) == nat.SGR_OK
    ins = [dev(x) for x in _abi_inputs(op, 4)]
    guard = torch.full((4, wo), SENTINEL, dtype=torch.int32, device=DEV)
    out = guard.view(torch.float32)
    assert _abi_call(op, ins, -1, out) == nat.SGR_ERR_INVALID
    assert "null argument" in nat.last_error()
    for k in range(len(ins)):
        assert _abi_call(op, [None if j == k else t for j, t in enumerate(ins)], 4, out) == nat.SGR_ERR_INVALID
    assert _abi_call(op, ins, 4, None) == nat.SGR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((guard == SENTINEL).all())


def test_on_a_side_stream_after_a_producer():
    import lietorch
    src = dev(K.exp_inputs(np.full(300, 0.2), seed=51)[0][600:])                               # rho perpendicular
    A = torch.randn(1024, 1024, device=DEV)
    Y = SE3(K.random_poses(300, 52))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        w = (A @ A).abs().sum() * 0.0 + 0.5                       # a producer that keeps the stream busy before tau exists
        tau = src * w
        X = lietorch.SE3.exp(tau)
        P = X * Y
        M = P.matrix()
    s.synchronize()
    tau, X, P, M = host(tau), host(X.data), host(P.data), host(M)
    assert np.array_equal(tau, host(src) * np.float32(0.5))
    held({"exp": ratio("stream exp", X, R.exp(tau)), "mul": ratio("stream mul", P, R.mul(X, host(Y.data))),
          "matrix": ratio("stream matrix", M, R.matrix(P))})


# ------------------------------------------------------------------------------------------------------------------ the wrapper
def test_wrapper_broadcasting(poses):
    X, Y, _ = poses
    N, Bn, P = 5, 3, 4
    one, many = X[7:8], Y[:N]
    got = (SE3(one) * SE3(many)).data
    assert got.shape == (N, 7)
    cases = {"[1,7]x[N,7]": ratio("bc mul 1xN", host(got), R.mul(np.repeat(one, N, 0), many))}
    a, b = X[10:10 + Bn].reshape(Bn, 1, 7), Y[20:20 + N].reshape(1, N, 7)
    got = (SE3(a) * SE3(b)).data
    assert got.shape == (Bn, N, 7)
    fa, fb = np.broadcast_to(a, (Bn, N, 7)).reshape(-1, 7), np.broadcast_to(b, (Bn, N, 7)).reshape(-1, 7)
    cases["[B,1,7]x[1,N,7]"] = ratio("bc mul Bx1 x 1xN", host(got).reshape(-1, 7), R.mul(fa, fb))
    pts, a6 = K.random_vectors(N * P, 3, 61).reshape(N, P, 3), K.random_vectors(N * P, 6, 62).reshape(N, P, 6)
    pose = X[30:30 + N].reshape(N, 1, 7)
    flat = np.broadcast_to(pose, (N, P, 7)).reshape(-1, 7)
    got = SE3(pose).act(dev(pts))
    assert got.shape == (N, P, 3)
    cases["act [N,1,7]x[N,P,3]"] = ratio("bc act", host(got).reshape(-1, 3), R.act(flat, pts.reshape(-1, 3)))
    assert torch.equal(SE3(pose) * dev(pts), got)                                            # `*` with points is `act`
    got = SE3(pose).adjT(dev(a6))
    assert got.shape == (N, P, 6)
    cases["adjT [N,1,7]x[N,P,6]"] = ratio("bc adjT", host(got).reshape(-1, 6), R.adjT(flat, a6.reshape(-1, 6)))
    single = X[40]
    got = SE3(single).act(dev(pts[0]))
    assert got.shape == (P, 3)
    cases["act [7]x[P,3]"] = ratio("bc act single", host(got), R.act(np.repeat(single[None], P, 0), pts[0]))
    got = SE3(single).adjT(dev(a6[0]))
    assert got.shape == (P, 6)
    cases["adjT [7]x[P,6]"] = ratio("bc adjT single", host(got), R.adjT(np.repeat(single[None], P, 0), a6[0]))
    assert SE3(single).matrix().shape == (4, 4) and SE3(a).inv().data.shape == (Bn, 1, 7) and SE3(a).log().shape == (Bn, 1, 6)
    held(cases)


def test_views_give_the_bits_of_their_contiguous_copies(poses):
    import lietorch
    X = dev(poses[0][:64])
    for view in (X[::2], dev(poses[0][:64].T.copy()).T):
        assert not view.is_contiguous()
        c = view.contiguous()
        a, b = lietorch.SE3(view), lietorch.SE3(c)
        other = lietorch.SE3(dev(poses[1][:view.shape[0]]))
        pts, a6 = dev(K.random_vectors(view.shape[0], 3, 71)), dev(K.random_vectors(view.shape[0], 6, 72))
        for f in (lambda s: s.inv().data, lambda s: s.log(), lambda s: s.matrix(), lambda s: (s * other).data, lambda s: (other * s).data,
                  lambda s: s.act(pts), lambda s: s.adjT(a6)):
            assert torch.equal(f(a), f(b))
    tau = dev(K.exp_inputs(np.full(64, 0.3))[0])
    assert torch.equal(lietorch.SE3.exp(tau[::3]).data, lietorch.SE3.exp(tau[::3].contiguous()).data)


def test_fp64_inputs_are_computed_and_returned_in_fp32(poses):
    import lietorch
    X32 = dev(poses[0][:50])
    X64 = X32.double() * (1 + 1e-10)                                     # not representable in fp32: rounded on the way in
    tau32 = dev(K.exp_inputs(np.full(50, 0.3))[0][:50])
    for out64, out32 in ((lietorch.SE3(X64).inv().data, lietorch.SE3(X32).inv().data), (lietorch.SE3(X64).log(), lietorch.SE3(X32).log()),
                         (lietorch.SE3(X64).matrix(), lietorch.SE3(X32).matrix()), (lietorch.SE3.exp(tau32.double()).data, lietorch.SE3.exp(tau32).data),
                         ((lietorch.SE3(X64) * lietorch.SE3(X32)).data, (lietorch.SE3(X32) * lietorch.SE3(X32)).data),
                         (lietorch.SE3(X64).act(tau32[:, :3].double()), lietorch.SE3(X32).act(tau32[:, :3])),
                         (lietorch.SE3(X64).adjT(tau32.double()), lietorch.SE3(X32).adjT(tau32))):
        assert out64.dtype == torch.float32 and torch.equal(out64, out32)


@pytest.mark.parametrize("size", [1e-6, 1e-4, 1e-2])
def test_retr_is_exp_times_pose(poses, size):
    import lietorch
    X = poses[0][:200]
    dx = (K.unit(np.random.default_rng(81).normal(size=(200, 6))) * size).astype(np.float32)
    got = lietorch.SE3(dev(X)).retr(dev(dx))
    E = lietorch.SE3.exp(dev(dx))
    assert torch.equal(got.data, (E * lietorch.SE3(dev(X))).data)
    held({"exp": ratio(f"retr exp |dx|={size:g}", host(E.data), R.exp(dx)),
          "mul": ratio(f"retr mul |dx|={size:g}", host(got.data), R.mul(host(E.data), X))})


# ------------------------------------------------------------------------------------------------------------------ trajectory filler
def test_trajectory_filler_interpolation_stage_by_stage():
    """P1 = exp(d) P0;  v = log(P1 P0^-1);  G(s) = exp(s v) P0  (the reference's trajectory_filler between two keyframes): every
    stage against the oracle fed the fp32 output of the stage before"""
    import lietorch
    P0, d = K.filler_inputs()
    cases = {}
    E = host(lietorch.SE3.exp(dev(d)).data)
    cases["exp(d)"] = ratio("filler exp(d)", E, R.exp(d))
    P1 = host((SE3(E) * SE3(P0)).data)
    cases["P1"] = ratio("filler P1 = exp(d) P0", P1, R.mul(E, P0))
    P0i = host(SE3(P0).inv().data)
    cases["inv"] = ratio("filler inv(P0)", P0i, R.inv(P0))
    rel = host((SE3(P1) * SE3(P0i)).data)
    cases["rel"] = ratio("filler P1 inv(P0)", rel, R.mul(P1, P0i))
    v = SE3(rel).log()
    cases["log t"] = ratio("filler log rho", host(v), R.log(rel), slice(0, 3))
    cases["log th"] = ratio("filler log theta", host(v), R.log(rel), slice(3, 6))
    for s in (0.0, 0.25, 0.5, 1.0):
        sv = v * s
        Es = host(lietorch.SE3.exp(sv).data)
        cases[f"exp({s} v) t"] = ratio(f"filler exp({s} v) t", Es, R.exp(host(sv)), slice(0, 3))
        cases[f"exp({s} v) q"] = ratio(f"filler exp({s} v) q", Es, R.exp(host(sv)), slice(3, 7))
        G = host((SE3(Es) * SE3(P0)).data)
        cases[f"G({s})"] = ratio(f"filler G({s})", G, R.mul(Es, P0))
        if s == 0.0:
            assert np.array_equal(G.view(np.int32), P0.view(np.int32)), "G(0) is not P0 bit for bit"
        if s == 1.0:
            MG = host(SE3(G).matrix())
            bound, target = K.filler_end_to_end(P0, P1, P0i, rel, host(sv), Es, G)
            cases["G(1) = P1"] = float((np.abs(MG.astype(np.float64) - target) / bound).max())
            print(f"se3 ratio filler G(1) = P1: {cases['G(1) = P1']:.3f}   (widest bound {bound.max():.2e})")
    held(cases)
