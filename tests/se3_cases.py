"""Seeded inputs of the SE3 tests, shared by tests/test_se3_cpu.py (which checks that the bounds stay below 1e-5 on them and that
they catch the cancelling coefficient formulas) and tests/test_gpu_se3.py.  Everything is built in fp64 and rounded to fp32 once."""
import numpy as np

import se3_ref as R

ANGLES = [0.0, 1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 1e-2, 0.1, 1.0, 3.0, np.pi - 1e-6, np.pi + 0.5, 6.0]
_T = np.float32(1e-4)                                            # the kernels' series threshold and its fp32 neighbours
THRESHOLD = [float(np.nextafter(_T, np.float32(0))), float(_T), float(np.nextafter(_T, np.float32(1)))]
SWEEP = list(np.logspace(-6, -1, 64))
DEFECT_ANGLES = [1e-4 * (1 + 2.0 ** -20), 1.5e-4, 3e-4, 1e-3, 3e-3]


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def axes(n, seed):
    """n random unit axes and, for each, a unit vector perpendicular to it"""
    rng = np.random.default_rng(seed)
    ax = unit(rng.normal(size=(n, 3)))
    perp = unit(np.cross(ax, rng.normal(size=(n, 3))))
    return ax, perp


def exp_inputs(angles, seed=0):
    """per angle three tangents: rho = 0, rho parallel to the axis (length 1), rho perpendicular to it (length 1) -> fp32 [3n,6],
    the kind of every row (0, 1, 2) and its angle"""
    ang = np.asarray(angles, np.float64)
    ax, perp = axes(ang.size, seed)
    th = ang[:, None] * ax
    tau = np.concatenate([np.concatenate([r, th], 1) for r in (np.zeros_like(ax), ax, perp)], 0)
    return tau.astype(np.float32), np.repeat(np.arange(3), ang.size), np.tile(ang, 3)


def quat(angle, ax):
    angle = np.asarray(angle, np.float64).reshape(-1, 1)
    return np.concatenate([np.sin(0.5 * angle) * ax, np.cos(0.5 * angle)], 1)


def log_inputs(perpendicular, seed=1):
    """quaternions across the branches of `log`: the angle list and sweep, angles whose |(x,y,z)| straddles 1e-6, angles within 1e-3
    of pi on both sides, the -q copy of every one of them (w < 0), and w in {0, +-1e-13, +-1e-11} at |(x,y,z)| = 1 -> fp32 [N,7]"""
    nn = [2.0 * np.arcsin(s) for s in (0.5e-6, 0.999e-6, 1.001e-6, 2e-6)]
    near_pi = [np.pi - 1e-3, np.pi - 1e-5, np.pi + 1e-5, np.pi + 1e-3]
    ang = np.array(ANGLES + THRESHOLD + SWEEP + nn + near_pi)
    ax, perp = axes(ang.size + 5, seed)
    q = quat(ang, ax[:ang.size])
    q = np.concatenate([q, -q], 0)
    wq = np.concatenate([ax[ang.size:], np.array([0.0, 1e-13, -1e-13, 1e-11, -1e-11])[:, None]], 1)
    q = np.concatenate([q, wq], 0)
    p = np.concatenate([perp[:ang.size], perp[:ang.size], perp[ang.size:]], 0)
    t = p if perpendicular else np.zeros_like(p)
    return np.concatenate([t, q], 1).astype(np.float32)


def random_poses(n, seed, tmax=2.0):
    """rotation angles uniform in [0, 2 pi) (so w < 0 for half of them), |t| uniform in [0, tmax]; row 0 is the identity"""
    rng = np.random.default_rng(seed)
    ax, _ = axes(n, seed + 1000)
    q = quat(rng.uniform(0.0, 2.0 * np.pi, n), ax)
    t = unit(rng.normal(size=(n, 3))) * rng.uniform(0.0, tmax, (n, 1))
    pose = np.concatenate([t, q], 1)
    pose[0] = [0, 0, 0, 0, 0, 0, 1]
    return pose.astype(np.float32)


def random_vectors(n, width, seed, vmax=2.0):
    """points (width 3) or cotangents (width 6) of norm uniform in [0, vmax]"""
    rng = np.random.default_rng(seed)
    return (unit(rng.normal(size=(n, width))) * rng.uniform(0.0, vmax, (n, 1))).astype(np.float32)


def filler_inputs(n=64, seed=7):
    """trajectory filler: P0 random with |t| <= 2; d with rotation 1e-4 .. 3e-2 (log-uniform) and translation 0.01 .. 0.5"""
    rng = np.random.default_rng(seed)
    P0 = random_poses(n + 1, seed)[1:]
    ax, _ = axes(n, seed + 1)
    th = ax * np.exp(rng.uniform(np.log(1e-4), np.log(3e-2), (n, 1)))
    rho = unit(rng.normal(size=(n, 3))) * rng.uniform(0.01, 0.5, (n, 1))
    return P0, np.concatenate([rho, th], 1).astype(np.float32)


def _b(out):
    return R.bound(out[1], out[2])


def _tn(*poses):
    return np.max([np.linalg.norm(np.asarray(p, np.float64)[:, :3], axis=1) for p in poses], 0)


def filler_end_to_end(P0, P1, P0i, rel, v, Es, G):
    """G(1) = P1 by matrix, from the fp32 outputs of the stages inv(P0) -> P0i, P1 P0i -> rel, log -> v, exp -> Es, Es P0 -> G:
    (bound [N,4,4], target [N,4,4]).  The bound is se3_ref.chain_bound over the five stages before `matrix`, plus the fp64 defect of the
    identity exp(log(P1 P0^-1)) P0 = P1 on these fp32 poses (their quaternions are unit to 1e-7 only)."""
    v = np.asarray(v, np.float64)
    stages = [R.carried(_b(R.inv(P0))), R.carried(_b(R.mul(P1, P0i))),
              R.carried(_b(R.log(rel)), tangent=True, rho=np.linalg.norm(v[:, :3], axis=1)),
              R.carried(_b(R.exp(v))), R.carried(_b(R.mul(Es, P0)))]
    exact = R.matrix(R.mul(R.exp(R.log(R.mul(P1, R.inv(P0)[0])[0])[0])[0], P0)[0])[0]
    target = R.matrix(P1)[0]
    return R.chain_bound(_b(R.matrix(G)), stages, _tn(P0, P1, P0i, rel)) + np.abs(exact - target), target
