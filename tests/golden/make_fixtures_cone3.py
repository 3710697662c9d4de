"""Generates tests/golden/cone3_reference.npz: inputs in named families for the projections onto ExponentialCone, PowerCone and their duals, the
projection of every input from its DEFINITION (mpmath, 100 digits, certified by the optimality conditions), and the distance of the reference
algorithm run on the CPU from it.  tests/cone3_cases.py describes the contents and reads them.

The reference does not restate the loops of cone3.h:
  * K_exp: p = t (r, 1, e^r) on the boundary and p - v = mu (-e^r, -(1 - r) e^r, 1) on the boundary of K* give t = ((r - 1) x + y) / (r^2 - r + 1),
    mu = (x - r y) e^-r / (r^2 - r + 1) and one equation in r,
        h(r) = ((r - 1) x + y) e^r - (x - r y) e^-r - (r^2 - r + 1) z = 0,
    on the interval where t > 0 and mu > 0 (unbounded for x < 0 < y -> 0: no scan of r can replace the bracket); bisection in 100 digits.
  * K_pow(a): p = (phi_x(r), phi_y(r), sign(z) r) with phi_c(r) = (c + sqrt(c^2 + 4 a_c r (|z| - r))) / 2, r the root of phi_x^a phi_y^(1 - a) - r
    on (0, |z|); bisection in 100 digits, alpha an mpf made from the stored float.
  * a dual cone: v + P_K(-v).
A result is accepted only if p in K, p - v in K* and <p, p - v> = 0 hold to 1e-30 relative to max(1, ||v||_inf) (squared for the last): a point that
does not certify stops the generator.  Points built as (boundary point) + (multiple of its outward normal) are also compared with the boundary point
they were built from.

Deterministic: seeded draws, a zip written with fixed time stamps -- two runs give the same bytes.  About two minutes.
Usage:  python tests/golden/make_fixtures_cone3.py"""
import io
import math
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import cone3_cases as C3           # noqa: E402
from tests import projection_cases as S       # noqa: E402

PER_FAMILY = 30
ALPHA_GROUP = 6                               # points that share one alpha: two round-robin triples, so that +-pairs share it too
CERT_TOL = "1e-30"
DPS = 100
EXP_FAMILIES = ["uniform", "scale_1e-6", "scale_1e-3", "scale_1e3", "scale_1e6", "branch_interior", "branch_edge", "branch_edge_polar", "y_small", "ratio_large"]
POW_FAMILIES = ["uniform", "scale_1e-6", "scale_1e-3", "scale_1e3", "scale_1e6", "branch_interior", "branch_edge", "branch_edge_polar", "alpha_0.01", "alpha_0.5",
                "alpha_0.99", "xy_zero", "z_tiny", "z_sign"]
DELTAS = [1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e-8, 1e-6, 1e-4, 1e-2, 1e-7, 1e-5, 1e-3]     # relative distances of the branch_edge pairs
SAMPLE = [0, 7, 13, 22, 29]                   # the points of every family the host test regenerates


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


# ---- membership and the certificate, in mpmath ---------------------------------------------------------------------------------------------------------
def in_exp(p, tol):
    mp = _mp()
    x, y, z = p
    if y > 0:
        return y * mp.exp(x / y) <= z + tol
    return x <= tol and abs(y) <= tol and z >= -tol


def in_exp_dual(p, tol):
    mp = _mp()
    u, v, w = p
    if u < 0:
        return -u * mp.exp(v / u) <= mp.e * w + tol
    return abs(u) <= tol and v >= -tol and w >= -tol


def in_pow(p, a, tol):
    x, y, z = p
    return x >= -tol and y >= -tol and max(x, 0) ** a * max(y, 0) ** (1 - a) >= abs(z) - tol


def in_pow_dual(p, a, tol):
    u, v, w = p
    return u >= -tol and v >= -tol and (max(u, 0) / a) ** a * (max(v, 0) / (1 - a)) ** (1 - a) >= abs(w) - tol


def certified(primal, v, p, a, q=None):
    """p = Proj_K(v) for K = K_exp or K_pow(a) iff p in K, q = p - v in K*, <p, q> = 0.  Where q is given (computed without cancellation: membership
    of K_pow(a)* is not Lipschitz at its faces), p - v = q is one more condition."""
    mp = _mp()
    tol = mp.mpf(CERT_TOL)
    sc = max(mp.mpf(1), max(abs(t) for t in v))
    if q is None:
        q = [s - t for s, t in zip(p, v)]
    elif max(abs(s - t - u) for s, t, u in zip(p, v, q)) > tol * sc:
        return False
    if primal == S.EXP:
        ok = in_exp(p, tol * sc) and in_exp_dual(q, tol * sc)
    else:
        ok = in_pow(p, a, tol * sc) and in_pow_dual(q, a, tol * sc)
    return bool(ok and abs(sum(s * t for s, t in zip(p, q))) <= tol * sc * sc)


# ---- the projections from their definitions ------------------------------------------------------------------------------------------------------------
def _bisect(f, lo, hi, steps=350):
    """f(lo) < 0 < f(hi)"""
    for _ in range(steps):
        mid = (lo + hi) / 2
        if f(mid) > 0:
            hi = mid
        else:
            lo = mid
    return (lo + hi) / 2


def ref_exp(v):
    """(projection onto K_exp, the case of exp_project in exact arithmetic)"""
    mp = _mp()
    x, y, z = v
    zero = mp.mpf(0)
    if in_exp(v, 0):
        return list(v), 1
    if in_exp_dual([-t for t in v], 0):
        return [zero] * 3, 2
    if x <= 0 and y <= 0:
        return [x, zero, max(z, zero)], (3 if x < 0 and y < 0 else 4)

    def h_of(r, A, B):
        return A * mp.exp(r) - B * mp.exp(-r) - (r * r - r + 1) * z

    # t > 0: A = (r - 1) x + y > 0;  mu > 0: B = x - r y > 0.  Each end of the interval of r is the zero of A or of B, and the root can sit closer
    # to it than any fixed number of digits resolves (mu ~ exp(-|r|) for x < 0 < y -> 0).  So r = end +- exp(u): the factor that vanishes at the end
    # is a multiple of exp(u) without cancellation, and the bisection runs on u.  h increases with r on the interval.
    ends = []                                                                 # (end, +1: lower end / -1: upper end, (A, B) at r = end +- s)
    if x > 0:
        ends.append((1 - y / x, 1, lambda r, s: (x * s, x - r * y)))
    elif x < 0:
        ends.append((1 - y / x, -1, lambda r, s: (-x * s, x - r * y)))
    if y > 0:
        ends.append((x / y, -1, lambda r, s: ((r - 1) * x + y, y * s)))
    elif y < 0:
        ends.append((x / y, 1, lambda r, s: ((r - 1) * x + y, -y * s)))
    lows, highs = [e for e in ends if e[1] == 1], [e for e in ends if e[1] == -1]
    lo_end = max(lows, key=lambda e: e[0]) if lows else None
    hi_end = min(highs, key=lambda e: e[0]) if highs else None
    width = hi_end[0] - lo_end[0] if lo_end and hi_end else None
    assert width is None or width > 0, v

    def root_from(e, u_max):
        """(r, A) of the root at distance exp(u) <= exp(u_max) from the end e, None if h does not change sign there"""
        end, sgn, near = e

        def g(u):                                                              # increasing in u
            s = mp.exp(u)
            r = end + sgn * s
            return sgn * h_of(r, *near(r, s))

        u_hi = mp.mpf(0) if u_max is None else min(mp.mpf(0), u_max)
        step = mp.mpf(1)
        while g(u_hi) <= 0:
            if u_max is not None and u_hi >= u_max:
                return None
            u_hi = u_hi + step if u_max is None else min(u_hi + step, u_max)
            step *= 2
            assert step < mp.mpf(10) ** 15, v
        u_lo, step = u_hi - 1, mp.mpf(1)
        while g(u_lo) >= 0:
            step *= 2
            u_lo = u_hi - step
            assert step < mp.mpf(10) ** 15, v
        s = mp.exp(_bisect(g, u_lo, u_hi))
        r = end + sgn * s
        return r, near(r, s)[0]

    first, second = (lo_end, hi_end) if lo_end else (hi_end, None)
    got = root_from(first, None if second is None else mp.log(width) + mp.log1p(-mp.mpf("1e-30")))
    if second is not None and (got is None or abs(got[0] - second[0]) <= mp.mpf("1e-25") * max(1, abs(second[0]))):
        got = root_from(second, mp.log(width / 2))
    assert got is not None, v
    r, A = got
    t = A / (r * r - r + 1)
    return [t * r, t, t * mp.exp(r)], 4


def ref_pow(v, a, tol_z):
    """(projection onto K_pow(a), the case of pow_project in exact arithmetic with its |z| <= tol_z shortcut)"""
    mp = _mp()
    x, y, z = v
    zero = mp.mpf(0)
    az = abs(z)
    if in_pow(v, a, 0):
        return list(v), 1, None
    if in_pow_dual([-t for t in v], a, 0):
        return [zero] * 3, 2, None
    br = 3 if az <= tol_z else 4
    if z == 0:
        return [max(x, zero), max(y, zero), zero], br, None

    def phi_c(c, r, w, al):                                                     # w = |z| - r
        k = al * r * w
        root = mp.sqrt(c * c + 4 * k)
        return (c + root) / 2 if c >= 0 else 2 * k / (root - c)               # the same number; no cancellation for c < 0

    def f(r, w):                                                               # < 0 near r = 0, > 0 at r = |z| (v is not in K)
        return r - phi_c(x, r, w, a) ** a * phi_c(y, r, w, 1 - a) ** (1 - a)

    # with x <= 0 or y <= 0 the root can sit at 1e-130 |z| from either end (alpha next to 0 or 1): bisect on the logarithm of the distance from the
    # nearer end, r and |z| - r both without cancellation
    half = mp.log(az / 2)
    low = f(az / 2, az / 2) > 0
    if low:                                                                    # the root is in (0, |z| / 2): r = exp(u)
        def g(u):
            return f(mp.exp(u), az - mp.exp(u))
    else:                                                                      # in [|z| / 2, |z|): |z| - r = exp(u)
        def g(u):
            return -f(az - mp.exp(u), mp.exp(u))
    step = mp.mpf(1)                                                           # both forms: g < 0 for u -> -inf, g >= 0 at u = log(|z| / 2)
    while g(half - step) >= 0:
        step *= 2
        assert step < mp.mpf(10) ** 15, v
    s = mp.exp(_bisect(g, half - step, half))
    r, w = (s, az - s) if low else (az - s, s)
    px, py = phi_c(x, r, w, a), phi_c(y, r, w, 1 - a)
    # phi_c^2 - c phi_c = a_c r w: the residual p - v without the cancellation of the subtraction (certified() checks that it is p - v)
    return [px, py, mp.sign(z) * r], br, [a * r * w / px, (1 - a) * r * w / py, -mp.sign(z) * w]


def reference(kind, v, alpha, tol_z):
    """certified projection of the float vector v onto the cone `kind`: (float64 (3,), case).  alpha and v enter as exact mpf."""
    mp = _mp()
    primal = C3.PRIMAL[kind]
    vm = [mp.mpf(float(t)) for t in v]
    a = mp.mpf(float(alpha))
    w = vm if kind == primal else [-t for t in vm]
    p, br, q = ref_exp(w) + (None,) if primal == S.EXP else ref_pow(w, a, mp.mpf(float(tol_z)))
    if not certified(primal, w, p, a, q):
        raise RuntimeError("the reference of %s %r alpha %r does not certify" % (kind, list(map(float, v)), float(alpha)))
    if kind != primal:                                                         # Moreau: v + Proj_K(-v), the residual of the primal projection
        p = q if q is not None else [s + t for s, t in zip(p, vm)]
    return np.array([float(t) for t in p]), br


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------------------------
def _unit(n):
    return n / np.linalg.norm(n)


def _exp_ray(r):
    """boundary ray d(r) of K_exp and the outward normal n(r) there (n is itself a boundary ray of -K*, with outward normal d)"""
    return np.array([r, 1.0, math.exp(r)]), np.array([math.exp(r), (1.0 - r) * math.exp(r), -1.0])


def exp_inputs():
    """family name -> (points (30, 3), pair (30, 2), built-from boundary point or None per point)"""
    n = PER_FAMILY
    fam = {}
    rng = np.random.default_rng(4100)
    fam["uniform"] = (-25.0 + 50.0 * rng.random((n, 3)), None, None)
    for k, s in enumerate(("1e-6", "1e-3", "1e3", "1e6")):
        fam["scale_" + s] = (float(s) * (-1.0 + 2.0 * np.random.default_rng(4110 + k).random((n, 3))), None, None)
    # branch_interior: 8 + 7 + 7 + 8 points clearly inside the cases 1, 2, 3, 4
    rng = np.random.default_rng(4120)
    pts, known = [], []
    for i in range(n):
        br = (1, 2, 3, 4)[i % 4]
        r, t, c = -2.0 + 4.0 * rng.random(), 10.0 ** (-1.0 + 2.0 * rng.random()), 0.2 + 1.8 * rng.random()
        d, nrm = _exp_ray(r)
        if br == 1:                                                           # above the boundary ray
            pts.append(np.array([t * r, t, t * math.exp(r) * (1.0 + c)])); known.append(None)
        elif br == 2:                                                         # v = mu n(r), pushed into the polar cone: (u, v, w) = -v, w raised
            pts.append(t * nrm * np.array([1.0, 1.0, 1.0 + c])); known.append(None)
        elif br == 3:
            pts.append(np.array([-(0.3 + 5.0 * rng.random()), -(0.3 + 5.0 * rng.random()), -5.0 + 10.0 * rng.random()])); known.append(None)
        else:                                                                 # t d + mu n projects onto t d
            mu = t * (0.3 + 2.7 * rng.random()) * np.linalg.norm(d) / np.linalg.norm(nrm)
            pts.append(t * d + mu * nrm); known.append(t * d)
    fam["branch_interior"] = (np.array(pts), None, known)
    # branch_edge: pairs on both sides of a boundary at relative distance delta
    rng = np.random.default_rng(4130)
    pts, pair = [], []
    for j in range(12):                                                       # the boundary of K: cases 4 (outside) and 1
        r, t = -2.0 + 4.0 * rng.random(), 10.0 ** (-1.0 + 2.0 * rng.random())
        d, nrm = _exp_ray(r)
        for s in (1.0, -1.0):
            pts.append(t * d + s * DELTAS[j] * t * np.linalg.norm(d) * _unit(nrm)); pair.append((4, 1))
    for j, (axis, zsign) in enumerate(((0, -1.0), (0, 1.0), (1, -1.0))):      # the edges x = 0 and y = 0 of case 3
        a, b, zz = 0.5 + 3.0 * rng.random(), 0.5 + 3.0 * rng.random(), zsign * (0.5 + 3.0 * rng.random())
        other = {(0, -1.0): 2, (0, 1.0): 4, (1, -1.0): 4}[(axis, zsign)]
        for s in (-1.0, 1.0):
            p = np.array([-a, -b, zz])
            p[axis] *= -s * (1e-6, 1e-3, 1e-8)[j]
            pts.append(p); pair.append((3, other))
    fam["branch_edge"] = (np.array(pts), np.array(pair), None)
    rng = np.random.default_rng(4135)
    pts, pair = [], []
    for j in range(15):                                                       # the boundary of -K*: cases 4 (outside) and 2
        r, t = -2.0 + 4.0 * rng.random(), 10.0 ** (-1.0 + 2.0 * rng.random())
        d, nrm = _exp_ray(r)
        for s in (1.0, -1.0):
            pts.append(t * nrm + s * DELTAS[j] * t * np.linalg.norm(nrm) * _unit(d)); pair.append((4, 2))
    fam["branch_edge_polar"] = (np.array(pts), np.array(pair), None)
    rng = np.random.default_rng(4140)
    pts = []
    for i in range(n):                                                        # y = +-1e-1 .. +-1e-9, x and z of both signs
        k = 1 + i % 9
        p = -5.0 + 10.0 * rng.random(3)
        p[1] = (1.0 if (i // 9 + i) % 2 == 0 else -1.0) * 10.0 ** -k
        pts.append(p)
    fam["y_small"] = (np.array(pts), None, None)
    rng = np.random.default_rng(4150)
    pts = []
    ratios = [60.0, 85.0, 92.0, 120.0, 300.0, 700.0, 712.0, 750.0, 1000.0, 5000.0]
    for i in range(n):
        y = (1.0, 0.1, 0.01)[i // 10]
        rho = ratios[i % 10] * (1.0 if (i + i // 10) % 2 == 0 else -1.0)
        pts.append(np.array([rho * y, y, -5.0 + 10.0 * rng.random()]))
    fam["ratio_large"] = (np.array(pts), None, None)
    return fam


def _pow_boundary(rng, a):
    """a boundary point p of K_pow(a) with x, y > 0 and the outward normal there (itself on the boundary of -K*, with outward normal p)"""
    x, y, sg = 10.0 ** (-1.0 + 2.0 * rng.random()), 10.0 ** (-1.0 + 2.0 * rng.random()), (1.0 if rng.random() < 0.5 else -1.0)
    p = np.array([x, y, sg * x ** a * y ** (1.0 - a)])
    nrm = np.array([-a * x ** (a - 1.0) * y ** (1.0 - a), -(1.0 - a) * x ** a * y ** -a, sg])
    return p, nrm


def pow_inputs():
    """family name -> (points (30, 3), alpha (30), pair, built-from boundary point or None per point)"""
    n = PER_FAMILY
    fam = {}

    def alphas(seed, fixed=None):
        g = np.random.default_rng(seed)
        return np.repeat([fixed if fixed is not None else 0.1 + 0.85 * g.random() for _ in range(n // ALPHA_GROUP)], ALPHA_GROUP)

    rng = np.random.default_rng(4200)
    fam["uniform"] = (-25.0 + 50.0 * rng.random((n, 3)), alphas(4201), None, None)
    for k, s in enumerate(("1e-6", "1e-3", "1e3", "1e6")):
        fam["scale_" + s] = (float(s) * (-1.0 + 2.0 * np.random.default_rng(4210 + k).random((n, 3))), alphas(4215 + k), None, None)
    rng = np.random.default_rng(4220)
    al = alphas(4221)
    pts, known = [], []
    for i in range(n):
        br = (1, 2, 3, 4)[i % 4]
        a = al[i]
        c = 0.1 + 0.6 * rng.random()
        p, nrm = _pow_boundary(rng, a)
        if br == 1:
            pts.append(p * np.array([1.0, 1.0, c])); known.append(None)
        elif br == 2:
            pts.append(nrm * np.array([1.0, 1.0, c])); known.append(None)
        elif br == 3:                                                         # |z| <= tol, one of x, y negative
            q = np.array([0.3 + 3.0 * rng.random(), 0.3 + 3.0 * rng.random(), (0.0, 5e-9, -5e-9, 1e-9)[(i // 4) % 4]])
            q[(i // 4) % 2] *= -1.0
            pts.append(q); known.append(None)
        else:
            mu = (0.3 + 1.7 * rng.random()) * np.linalg.norm(p) / np.linalg.norm(nrm)
            pts.append(p + mu * nrm); known.append(p)
    fam["branch_interior"] = (np.array(pts), al, None, known)
    rng = np.random.default_rng(4230)
    al = alphas(4231)
    pts, pair = [], []
    for j in range(12):                                                       # the boundary of K: cases 4 (outside) and 1
        p, nrm = _pow_boundary(rng, al[len(pts)])
        for s in (1.0, -1.0):
            pts.append(p + s * DELTAS[j] * np.linalg.norm(p) * _unit(nrm)); pair.append((4, 1))
    for j in range(3):                                                        # |z| = tol (1 +- delta): cases 4 and 3
        q = np.array([-(0.3 + 3.0 * rng.random()), 0.3 + 3.0 * rng.random(), 0.0])
        for s in (1.0, -1.0):
            q2 = q.copy()
            q2[2] = (1.0, -1.0, 1.0)[j] * C3.TOL * (1.0 + s * (1e-6, 1e-3, 1e-1)[j])
            pts.append(q2); pair.append((4, 3))
    fam["branch_edge"] = (np.array(pts), al, np.array(pair), None)
    rng = np.random.default_rng(4235)
    al = alphas(4236)
    pts, pair = [], []
    for j in range(15):                                                       # the boundary of -K*: cases 4 (outside) and 2
        p, nrm = _pow_boundary(rng, al[len(pts)])
        for s in (1.0, -1.0):
            pts.append(nrm + s * DELTAS[j] * np.linalg.norm(nrm) * _unit(p)); pair.append((4, 2))
    fam["branch_edge_polar"] = (np.array(pts), al, np.array(pair), None)
    for k, a in enumerate((0.01, 0.5, 0.99)):
        fam["alpha_%g" % a] = (-25.0 + 50.0 * np.random.default_rng(4240 + k).random((n, 3)), alphas(0, fixed=a), None, None)
    rng = np.random.default_rng(4250)
    X = -5.0 + 10.0 * rng.random((n, 3))
    X[0::2, 0] = 0.0
    X[1::2, 1] = 0.0
    al = alphas(4251)
    X[1], al[:ALPHA_GROUP] = (3.22, 0.0, -1.71), 0.85                         # a point on which the reference algorithm is known to stall
    fam["xy_zero"] = (X, al, None, None)
    rng = np.random.default_rng(4260)
    X = -5.0 + 10.0 * rng.random((n, 3))
    X[:, 2] = 10.0 ** np.linspace(-12.0, -2.0, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    fam["z_tiny"] = (X, alphas(4261), None, None)
    rng = np.random.default_rng(4270)
    X = np.repeat(-25.0 + 50.0 * rng.random((n // 2, 3)), 2, axis=0)
    X[1::2, 2] *= -1.0
    fam["z_sign"] = (X, alphas(4271), None, None)
    return fam


def build_inputs(primal):
    """(names, family (N), v (N, 3) float64, alpha (N), pair (N, 2), known: point index -> the boundary point it was built from)"""
    if primal == S.EXP:
        fam, names = exp_inputs(), EXP_FAMILIES
    else:
        fam, names = pow_inputs(), POW_FAMILIES
    V, A, F, P, known = [], [], [], [], {}
    for k, nm in enumerate(names):
        if primal == S.EXP:
            pts, pair, kn = fam[nm]
            al = np.zeros(PER_FAMILY)
        else:
            pts, al, pair, kn = fam[nm]
        assert pts.shape == (PER_FAMILY, 3) and np.isfinite(pts).all(), nm
        for i, b in enumerate(kn or []):
            if b is not None:
                known[len(V) * PER_FAMILY + i] = b
        V.append(pts); A.append(al); F.append(np.full(PER_FAMILY, k, dtype=np.int16))
        P.append(pair if pair is not None else np.zeros((PER_FAMILY, 2), dtype=np.int64))
    return names, np.concatenate(F), np.concatenate(V), np.concatenate(A), np.concatenate(P).astype(np.int8), known


# ---- the CPU run of the reference algorithm ------------------------------------------------------------------------------------------------------------
def cpu_run(kind, prec, v, alpha):
    """f64: the oracle's project_cone; f32: cone3_cases.project_cpu with np.float32 scalars.  Returned as float64."""
    if prec == "f64":
        from oracle import cosmo_oracle as O
        okind = {S.EXP: O.EXP, S.DUAL_EXP: O.DUAL_EXP, S.POW: O.POW, S.DUAL_POW: O.DUAL_POW}[kind]
        is_exp = C3.PRIMAL[kind] == S.EXP
        out = np.array(v, dtype=np.float64)
        O.project_cone(out, O.Cone(okind, 3, alpha=float(alpha), max_iter=C3.MAX_ITER_EXP if is_exp else C3.MAX_ITER_POW, tol=C3.TOL))
        return out
    return C3.project_cpu(v, kind, alpha, np.float32)[0].astype(np.float64)


def rows_of(kind, prec, v64, alpha64, idx):
    """the stored columns of the points idx of one (kind, precision)"""
    sign = 1.0 if kind == C3.PRIMAL[kind] else -1.0
    dt = C3.DTYPES[prec]
    v = (sign * v64[idx]).astype(dt).astype(np.float64)
    al = alpha64[idx].astype(dt).astype(np.float64)
    tol_z = float(dt(C3.TOL))
    ref, br, cpu = np.empty_like(v), np.empty(len(idx), dtype=np.int8), np.empty_like(v)
    for i in range(len(idx)):
        ref[i], br[i] = reference(kind, v[i], al[i], tol_z)
        cpu[i] = cpu_run(kind, prec, v[i], al[i])
    return dict(v=v, alpha=al, ref=ref, branch=br, cpu=cpu, cpu_err=C3.error(cpu, ref, v))


def family_worst(family, nfam, err):
    return np.array([err[family == k].max() for k in range(nfam)])


def generate():
    out = {}
    for primal in (S.EXP, S.POW):
        names, family, v64, alpha64, pair, known = build_inputs(primal)
        out["%s_names" % primal] = np.array(names)
        out["%s_family" % primal] = family
        out["%s_pair" % primal] = pair
        for kind in (k for k in C3.KINDS if C3.PRIMAL[k] == primal):
            for prec in C3.PRECISIONS:
                cols = rows_of(kind, prec, v64, alpha64, np.arange(len(family)))
                if kind == primal and prec == "f64":
                    for i, b in known.items():                                # the construction is a second, independent reference
                        assert np.max(np.abs(cols["ref"][i] - b)) <= 1e-12 * np.max(np.abs(v64[i])), (primal, i, cols["ref"][i], b)
                    for i in np.flatnonzero(pair[:, 0]):
                        assert cols["branch"][i] in pair[i] and cols["branch"][i ^ 1] in pair[i] and cols["branch"][i] != cols["branch"][i ^ 1], (primal, i)
                cols["worst"] = family_worst(family, len(names), cols["cpu_err"])
                for f, a in cols.items():
                    out["%s_%s_%s" % (kind, prec, f)] = a
                print("%-8s %s: %d points certified" % (kind, prec, len(family)), flush=True)
    return out


def save(path, arrays):
    """an .npz with fixed time stamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def worst_table(arrays):
    lines = []
    for primal in (S.EXP, S.POW):
        names = [str(s) for s in arrays["%s_names" % primal]]
        for kind in (k for k in C3.KINDS if C3.PRIMAL[k] == primal):
            for k, nm in enumerate(names):
                w64, w32 = arrays["%s_f64_worst" % kind][k], arrays["%s_f32_worst" % kind][k]
                lines.append("%-8s %-16s %-5s %.1e  %.1e" % (kind, nm, "WEAK" if w64 > C3.WEAK_ABOVE else "", w64, w32))
    return "\n".join(lines)


if __name__ == "__main__":
    arrays = generate()
    save(C3.FIXTURE, arrays)
    print(worst_table(arrays))
    print("wrote %s, %d bytes" % (C3.FIXTURE, os.path.getsize(C3.FIXTURE)))
