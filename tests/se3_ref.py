"""fp64 numpy restatement of the seven SE3 operations behind the `lietorch` drop-in (`se3_kernel<OP>`, csrc/sgr_aux.hip), with the
semantics of the kernels, which follow upstream lietorch: pose = (tx,ty,tz,qx,qy,qz,qw), tangent = (rho, theta); quaternions are
NOT renormalised; `inv` conjugates; `log` takes theta = 2 atan(n / w) / n * (x,y,z) with n = |(x,y,z)| (n = 0: 2 / w; w = 0:
+pi / n), so the rotation comes back in (-pi, pi].  Inputs are the kernel's fp32 inputs promoted to fp64, never re-rounded.

Every function returns (value, magnitude, units), elementwise over the output:

    value      the result in fp64, every coefficient evaluated without cancellation (below)
    magnitude  M: the sum of the absolute values of the terms that are added to form the element, cross products expanded
    units      C_op: the number of fp32 roundings (2^-24 relative each) on the longest path to the element

and the bound of a test is |got - value| <= units * 2^-24 * magnitude + one fp32 denormal (`bound`).

Counting.  + - * : 1 unit (an FMA only removes one).  sinf, cosf, sqrtf, a division: 1 ulp in the HIP math tables = 2 units
(division and sqrtf are correctly rounded in the default build; the documented figure is what is counted).  atanf: 2 ulp = 4 units.

Rounded arguments.  sin, cos, atan and the coefficients B, C, D are taken at an argument that is itself rounded: the angle
a = sqrt(x^2 + y^2 + z^2) carries 3 roundings under the root (halved by it) and the root's 2 units, E_ANG = 3.5 units.  One unit
of relative error of the argument moves f(a) by |a f'(a)|, which no "sum of terms" contains and which does not vanish where f
does (cos(a/2) at a = pi, sin(a/2) at a = 2 pi).  So wherever f enters a magnitude it enters as

    |f(a)| + (E / C_op) |a f'(a)|          E = the units of the argument, C_op = the units of the element,

so that C_op * 2^-24 * M charges the argument exactly its E units and the value its C_op.  The derivative is the TOTAL one of
the expression the kernel evaluates with one and the same rounded angle (sin(h)/h hardly moves with h at small h, and M says so):
a sloppy coefficient cannot hide behind it -- at a -> 0 the extra term of B is a^2/12, of C a^2/60, of D a^2/360.

THIS DEPARTS from "M = the sum of the terms added, C_op <= 32 of it", and is a finding about the formulas, not a way round the cap:
measured against the plain M (`exp(..., sensitivity=False)`, `log(..., sensitivity=False)`), what is held amounts to more roundings
than C_op wherever an operation is ill conditioned in its angle -- `effective_units` gives the figure, tests/test_se3_cpu.py pins it:
    exp t       <= 36 at a = 6 (C and B swing with the angle near 2 pi), 30.2 up to pi; 26.0 to 26.1 for a <= 0.1
    exp q xyz   <= 82 at a = 6 (sin(a/2) -> 0 at 2 pi), 8.5 up to pi;  exp q w: unbounded at a = pi (cos(a/2) = 0: plain M vanishes, the error
                of the rounded angle, 3.5 * 2^-24 * pi/2, does not); 5.0 for a <= 0.1 for both
    log theta   <= 9 + 3.5 = 12.5 (n k'/k -> -1 at pi)
    log rho     <= 28 + 2 * 11.5 + ... = 53 of the D term at a = pi, 40 of the (theta x t)/2 term; 44 of the D term and 36 of the
                other at small angles (measured on the tests' inputs: <= 49, and <= 35 on the trajectory-filler pattern).  This is the conditioning problem of forming rho from the COMPUTED theta: theta enters the D
                term squared and carries atanf's 4 units and two divisions (8 units) before it does.  No derivation within 32 units of
                the plain M exists for this formula; an implementation would have to carry theta in higher precision.
inv, mul, act, adjT and matrix use the plain M.

Coefficients without cancellation (fp64):
    B(a) = (1 - cos a)/a^2            = 2 sin^2(a/2) / a^2                                       no sum at all
    C(a) = (a - sin a)/a^3            = sum_j (-1)^j a^2j / (2j+3)!                              for a < SERIES_BELOW
    D(a) = (1 - (a/2) cot(a/2))/a^2   = sum_{n>=1} |B_2n| a^(2n-2) / (2n)!   (Bernoulli numbers)  for a < SERIES_BELOW
SERIES_BELOW = 0.3.  Above it the closed forms lose, relative to the result: C: sin a is within 1.1e-16 a of the truth and the
difference is a^3/6 (1 - a^2/20), so 2 * 1.1e-16 * 6 / a^2 <= 1.5e-14; D: (a/2) cot(a/2) ~ 1 carries three roundings, 3.3e-16,
and 1 minus it is >= a^2/12, so 3.3e-16 * 12 / a^2 <= 4.4e-14.  Below it the series are cut after SERIES_TERMS = 10 terms: the
ratio of consecutive terms is < a^2/20 <= 4.5e-3 (C) and < a^2/(4 pi^2) (1 + 2^-9) <= 2.3e-3 (D: the radius of convergence is
2 pi), so the first term left out is below (4.5e-3)^10 = 3.4e-24 of the sum.  Both errors stay under 1e-13 relative.

Chains (round trips on the device).  When stage s+1 is fed the fp32 output of stage s, the end-to-end error against the exact
chain is at most the last stage's own bound plus every earlier stage's bound carried forward to first order, ONCE, without
compounding: the stages after it are exact group operations (`inv`, `mul`, `exp` after `log`), and those carry a perturbation of a
pose as a perturbation of the group element.  A stage's bound is read as (rot, tr):
    pose output     rot = GAIN_Q |b_q|_2,    tr = |b_t|_2          GAIN_Q = 2 sqrt 5 >= 2 (|w| + 2 |u|): what one unit of |dq|_2 moves an
                                                                    entry of the (unnormalised) rotation matrix by, at most
    tangent output  rot = |b_theta|_2,       tr = |b_rho|_2 + |b_theta|_2 |rho|      (|V| <= 1, |dV/dtheta| <= 1/2)
A later rotation leaves |tr|_2 and rot as they are; a later translation t turns rot into rot |t| more translation.  So with T the
largest |t| of any pose the later stages hold, a rotation entry of the final matrix is off by at most its own bound + sum rot_s and
a translation entry by its own bound + sum (tr_s + T rot_s): the gain of a later stage on an earlier error is at most 1 + |t|,
applied once (`chain_bound`).  Second-order terms and the 1e-7 by which an fp32 quaternion misses unit length are left out of the
carried part; where the identity that is tested holds only for unit quaternions, the test adds the oracle's own fp64 defect of it."""
from fractions import Fraction
from math import factorial

import numpy as np

U32 = 2.0 ** -24
DENORMAL = 2.0 ** -149
E_ANG = 3.5
SERIES_BELOW = 0.3
SERIES_TERMS = 10
GAIN_Q = 2.0 * 5.0 ** 0.5


def _bernoulli(m):
    """B_0 .. B_m (B_1 = -1/2) by the defining recurrence, exactly"""
    B = [Fraction(1)]
    for n in range(1, m + 1):
        B.append(-sum(Fraction(factorial(n + 1), factorial(k) * factorial(n + 1 - k)) * B[k] for k in range(n)) / (n + 1))
    return B


_BERN = _bernoulli(2 * SERIES_TERMS)
C_SERIES = [float(Fraction((-1) ** j, factorial(2 * j + 3))) for j in range(SERIES_TERMS)]               # a^(2j)
D_SERIES = [float(abs(_BERN[2 * n]) / factorial(2 * n)) for n in range(1, SERIES_TERMS + 1)]              # a^(2n-2)


def _series(coef, a2, derivative=False):
    """sum_j c_j a^2j, or a d/da of it = sum_j 2j c_j a^2j"""
    out = np.zeros_like(a2)
    for j in reversed(range(len(coef))):
        out = out * a2 + coef[j] * (2 * j if derivative else 1)
    return out


def _safe(a):
    return np.where(a == 0, 1.0, a)


def coef_B(a):
    """(1 - cos a)/a^2 and a B'(a) = sin(a)/a - 2 B"""
    s = _safe(a)
    B = np.where(a == 0, 0.5, 2.0 * np.sin(0.5 * s) ** 2 / s ** 2)
    return B, np.where(a == 0, 0.0, np.sin(s) / s - 2.0 * B)


def coef_C(a):
    """(a - sin a)/a^3 and a C'(a) = B - 3 C"""
    small, s = a < SERIES_BELOW, np.where(a < SERIES_BELOW, 1.0, a)
    C = np.where(small, _series(C_SERIES, a * a), (s - np.sin(s)) / s ** 3)
    return C, np.where(small, _series(C_SERIES, a * a, True), coef_B(s)[0] - 3.0 * C)


def coef_D(a):
    """(1 - (a/2) cot(a/2))/a^2 and a D'(a) = (h / sin^2 h - cot h) / (2a) - 2 D,  h = a/2"""
    small, s = a < SERIES_BELOW, np.where(a < SERIES_BELOW, 1.0, a)
    h = 0.5 * s
    D = np.where(small, _series(D_SERIES, a * a), (1.0 - h * np.cos(h) / np.sin(h)) / s ** 2)
    aD1 = (h / np.sin(h) ** 2 - np.cos(h) / np.sin(h)) / (2.0 * s) - 2.0 * D
    return D, np.where(small, _series(D_SERIES, a * a, True), aD1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _cross_mag(a, b):
    """the same two products per element, added in absolute value (a, b >= 0)"""
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)


def _rotate(q, v):
    """v + 2 w (u x v) + 2 u x (u x v), u = (x,y,z): the rotation for a unit q, and what the kernels compute for any q"""
    u, w = q[:, :3], q[:, 3:4]
    c = _cross(u, v)
    return v + 2.0 * (w * c + _cross(u, c))


def _rotate_mag(q, vabs):
    u, w = np.abs(q[:, :3]), np.abs(q[:, 3:4])
    c = _cross_mag(u, vabs)
    return vabs + 2.0 * (w * c + _cross_mag(u, c))


# products of the first cross product 1, its difference 1, the second cross product 2 more, w c 1 (the longest path runs through
# u x (u x v): 4), the sum w c + d 1, the final sum 1; times 2 is exact
C_ROTATE = 6


def _f64(x, width):
    x = np.asarray(x, np.float64)
    assert x.ndim == 2 and x.shape[1] == width, x.shape
    return x


# the C term: C itself 19 (series branch: 3; closed form from a = 1 on: sinf 2 |sin a| / (a - sin a) <= 10.7 at a = 1 and
# falling, the difference 1, t2 * a 1, t2 against a^2 4, the division 2), (theta x (theta x rho)) 4, the product 1, two sums 2.
# (the B term: (sin h / h)^2 / 2 = (sinf 2 + division 2) * 2 + the square 1 = 9, theta x rho 2, the product 1, two sums 2 = 14.)
C_EXP_T = 26
# xyz: sinf 2, the division by a 2, times theta_k 1.  w: cosf 2.  One figure for the four of them.
C_EXP_Q = 5


def exp(tau, sensitivity=True):
    """[N,6] -> pose [N,7].  sensitivity=False: the plain M (the terms added alone), to report how far the one that is held departs from it"""
    tau = _f64(tau, 6)
    rho, th = tau[:, :3], tau[:, 3:]
    a = np.sqrt((th * th).sum(1))[:, None]
    h = 0.5 * a
    B, aB1 = coef_B(a)
    C, aC1 = coef_C(a)
    imag = np.where(a == 0, 0.5, np.sin(h) / _safe(a))                       # sin(a/2) / a
    a_imag1 = np.where(a == 0, 0.0, 0.5 * np.cos(h) - imag)                  # a d/da of it
    c1 = _cross(th, rho)
    c2 = _cross(th, c1)
    m1 = _cross_mag(np.abs(th), np.abs(rho))
    m2 = _cross_mag(np.abs(th), m1)
    t = rho + B * c1 + C * c2
    wt = E_ANG / C_EXP_T * sensitivity
    Mt = np.abs(rho) + (np.abs(B) + wt * np.abs(aB1)) * m1 + (np.abs(C) + wt * np.abs(aC1)) * m2
    wq = E_ANG / C_EXP_Q * sensitivity
    q = np.concatenate([imag * th, np.cos(h)], 1)
    Mq = np.concatenate([(np.abs(imag) + wq * np.abs(a_imag1)) * np.abs(th), np.abs(np.cos(h)) + wq * np.abs(h * np.sin(h))], 1)
    units = np.array([C_EXP_T] * 3 + [C_EXP_Q] * 4, np.float64)
    return np.concatenate([t, q], 1), np.concatenate([Mt, Mq], 1), units


# theta_k = k q_k, k = 2 atan(n / w) / n: the division n / w 2, atanf 4 (its own condition |r atan'(r) / atan r| <= 1), the
# division by n 2, times q_k 1; times 2 is exact.  The argument n carries E_ANG, charged on |n k'(n)| = |2 w / (w^2 + n^2) - k|.
C_LOG_TH = 9
# rho_k = t_k - (theta x t)_k / 2 + D (theta x (theta x t))_k.  theta reaches the cross products with a relative error COMMON to its
# three components: that of k, 8 units (the component's own product is counted below), plus E_ANG |n k'/k| (<= 1: 0 at small angles,
# 1 at pi): S = 8 + 3.5 |n k'/k| <= 11.5 units of ONE perturbation theta -> theta (1 + e), which moves rho by
# e (-(theta x t)/2 + (2 D + a D') theta x (theta x t)); the angle D is taken at adds its own E_ANG on a D' alone.  Charged there.
# Independent roundings on the longest path, the D term: the component's own product 1, theta x t 2, theta x (theta x t) 2,
# D 20 (series branch below a = 2: 3; closed form from a = 2 on, g = h cosf h / sinf h: 2 + 2 + 1 + 2 = 7 units of g, magnified by
# g / (1 - g) <= 1.8 at a = 2 and falling to 0 at pi: 12.6; the difference 1, t2 against a^2 4, the division 2), the product 1,
# two sums 2.
S_LOG_K = 8.0
C_LOG_RHO = 28


def log(pose, sensitivity=True):
    """[N,7] -> tangent [N,6]"""
    pose = _f64(pose, 7)
    t, u, w = pose[:, :3], pose[:, 3:6], pose[:, 6:7]
    n = np.sqrt((u * u).sum(1))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        half = np.where(w == 0, 0.5 * np.pi, np.arctan(n / np.where(w == 0, 1.0, w)))
        k = np.where(n == 0, 2.0 / w, 2.0 * half / _safe(n))
        nk1 = np.where(n == 0, 0.0, 2.0 * w / (w * w + n * n) - k)
    th = k * u
    a = np.sqrt((th * th).sum(1))[:, None]
    D, aD1 = coef_D(a)
    c1 = _cross(th, t)
    c2 = _cross(th, c1)
    m1 = _cross_mag(np.abs(th), np.abs(t))
    m2 = _cross_mag(np.abs(th), m1)
    rho = t - 0.5 * c1 + D * c2
    with np.errstate(divide="ignore", invalid="ignore"):
        S = S_LOG_K + E_ANG * np.where(k == 0, 0.0, np.abs(nk1 / np.where(k == 0, 1.0, k)))
    ws, wa = S / C_LOG_RHO * sensitivity, (S + E_ANG) / C_LOG_RHO * sensitivity
    Mrho = np.abs(t) + 0.5 * (1.0 + ws) * m1 + (np.abs(D) * (1.0 + 2.0 * ws) + wa * np.abs(aD1)) * m2
    Mth = (np.abs(k) + E_ANG / C_LOG_TH * sensitivity * np.abs(nk1)) * np.abs(u)
    units = np.array([C_LOG_RHO] * 3 + [C_LOG_TH] * 3, np.float64)
    return np.concatenate([rho, th], 1), np.concatenate([Mrho, Mth], 1), units


# the conjugate is exact (0 units: the bound is the denormal alone); t' = -(rotation of t by the conjugate): C_ROTATE
C_INV_T = C_ROTATE


def inv(pose):
    pose = _f64(pose, 7)
    qc = pose[:, 3:] * np.array([-1.0, -1.0, -1.0, 1.0])
    val = np.concatenate([-_rotate(qc, pose[:, :3]), qc], 1)
    mag = np.concatenate([_rotate_mag(qc, np.abs(pose[:, :3])), np.abs(qc)], 1)
    return val, mag, np.array([C_INV_T] * 3 + [0] * 4, np.float64)


# quaternion: four products, three sums: 1 + 3.  translation: the rotation of y.t by x.q, plus x.t: C_ROTATE + 1
C_MUL_Q = 4
C_MUL_T = C_ROTATE + 1


def mul(x, y):
    x, y = _f64(x, 7), _f64(y, 7)
    a, b = x[:, 3:], y[:, 3:]
    P = [[(3, 0, 1), (0, 3, 1), (1, 2, 1), (2, 1, -1)], [(3, 1, 1), (0, 2, -1), (1, 3, 1), (2, 0, 1)],
         [(3, 2, 1), (0, 1, 1), (1, 0, -1), (2, 3, 1)], [(3, 3, 1), (0, 0, -1), (1, 1, -1), (2, 2, -1)]]
    q = np.stack([sum(s * a[:, i] * b[:, j] for i, j, s in row) for row in P], 1)
    Mq = np.stack([sum(np.abs(a[:, i] * b[:, j]) for i, j, s in row) for row in P], 1)
    t = x[:, :3] + _rotate(a, y[:, :3])
    Mt = np.abs(x[:, :3]) + _rotate_mag(a, np.abs(y[:, :3]))
    return np.concatenate([t, q], 1), np.concatenate([Mt, Mq], 1), np.array([C_MUL_T] * 3 + [C_MUL_Q] * 4, np.float64)


C_ACT = C_ROTATE + 1


def act(pose, pts):
    pose, pts = _f64(pose, 7), _f64(pts, 3)
    val = _rotate(pose[:, 3:], pts) + pose[:, :3]
    return val, _rotate_mag(pose[:, 3:], np.abs(pts)) + np.abs(pose[:, :3]), np.full(3, float(C_ACT))


# Ad_X^T (a_rho, a_theta) = (R^T a_rho, R^T (a_theta - t x a_rho)).  First half: C_ROTATE.  Second: the vector that is rotated is
# itself a sum: (t x a_rho)_k product 1, difference 1, a_theta - it 1: C_ROTATE + 3
C_ADJT_1 = C_ROTATE
C_ADJT_2 = C_ROTATE + 3


def adjT(pose, a6):
    pose, a6 = _f64(pose, 7), _f64(a6, 6)
    t, qc = pose[:, :3], pose[:, 3:] * np.array([-1.0, -1.0, -1.0, 1.0])
    ar, at = a6[:, :3], a6[:, 3:]
    m = at - _cross(t, ar)
    mm = np.abs(at) + _cross_mag(np.abs(t), np.abs(ar))
    val = np.concatenate([_rotate(qc, ar), _rotate(qc, m)], 1)
    mag = np.concatenate([_rotate_mag(qc, np.abs(ar)), _rotate_mag(qc, mm)], 1)
    return val, mag, np.array([C_ADJT_1] * 3 + [C_ADJT_2] * 3, np.float64)


# a column of R is the rotation of a unit vector: C_ROTATE; the translation column and the last row are copies or constants: 0 units
C_MATRIX = C_ROTATE


def matrix(pose):
    """[N,7] -> [N,4,4]"""
    pose = _f64(pose, 7)
    N = pose.shape[0]
    val, mag = np.zeros((N, 4, 4)), np.zeros((N, 4, 4))
    for j in range(3):
        e = np.zeros((N, 3))
        e[:, j] = 1.0
        val[:, :3, j], mag[:, :3, j] = _rotate(pose[:, 3:], e), _rotate_mag(pose[:, 3:], e)
    val[:, :3, 3], mag[:, :3, 3] = pose[:, :3], np.abs(pose[:, :3])
    val[:, 3, 3] = mag[:, 3, 3] = 1.0
    units = np.zeros((4, 4))
    units[:3, :3] = C_MATRIX
    return val, mag, units


def effective_units(held, plain):
    """(val, M, units) with and without the sensitivity terms -> per element units * M / M_plain: the roundings of the PLAIN sum of
    terms that the bound amounts to (inf where the plain M vanishes and the held one does not)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(held[1] == 0, 0.0, held[2] * held[1] / plain[1])


def bound(mag, units):
    """per element: units * 2^-24 * magnitude, plus one fp32 denormal for the exact zeros"""
    return units * U32 * mag + DENORMAL


def worst_ratio(got, ref, mag, units):
    """max |got - ref| / bound: what a failing case reports, and what DESIGN.md records per op"""
    r = np.abs(np.asarray(got, np.float64) - ref) / bound(mag, units)
    return float(r.max()) if r.size else 0.0


def carried(b, tangent=False, rho=None):
    """(rot, tr) per pose of one stage's bound b [N,7] (pose) or [N,6] (tangent, with its |rho| [N]); module docstring"""
    n2 = lambda x: np.sqrt((x * x).sum(1))
    if tangent:
        return n2(b[:, 3:]), n2(b[:, :3]) + n2(b[:, 3:]) * rho
    return GAIN_Q * n2(b[:, 3:]), n2(b[:, :3])


def chain_bound(last, earlier, tmax):
    """last: the bound of the final `matrix` stage [N,4,4]; earlier: the (rot, tr) of every stage before it; tmax [N]: the largest
    |t| of any pose the later stages hold.  First order, every earlier stage carried once."""
    rot, tr = sum(e[0] for e in earlier), sum(e[1] for e in earlier)
    out = last.copy()
    out[:, :3, :3] += rot[:, None, None]
    out[:, :3, 3] += (tr + np.asarray(tmax, np.float64) * rot)[:, None]
    return out
