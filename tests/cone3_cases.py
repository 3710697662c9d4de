"""Inputs and a certified reference for the projections onto ExponentialCone, PowerCone and their duals (csrc/cone3.h, called from k_cone3_project in
csrc/cone3.hip and from batch_project_cone3 in csrc/batch.hip).  No test functions, no GPU code: imported by test_cone3_cases_host.py (CPU) and
test_gpu_cone3_reference.py (GPU).  Everything comes from tests/golden/cone3_reference.npz, written by tests/golden/make_fixtures_cone3.py.

Per cone kind (exp, dual_exp, pow, dual_pow) and precision (f64, f32) the fixture holds, one row per point:

  v, alpha   the input and the exponent.  The f32 set is the f64 set rounded to Float32; a dual kind holds the negated points of its primal kind
             (project! of a dual cone runs the primal routine on -v, so both reach the same branches)
  ref        the projection from its definition, by mpmath at 100 digits, accepted only where p in K, p - v in K* and <p, p - v> = 0 hold to 1e-30
             relative to max(1, ||v||_inf) (all points certify); rounded once to float64
  branch     the case 1 .. 4 of project! (cone3.h: exp_project, pow_project) its predicates give in exact arithmetic: 1 v in K, 2 -v in K*,
             3 (exp: x < 0 and y < 0; pow: |z| <= tol), 4 the iteration
  cpu        the reference ALGORITHM run on the CPU in that precision: f64 oracle.cosmo_oracle.project_cone, f32 project_cpu of this file with
             np.float32 scalars (max_iter 100 / 20, tol 1e-8: what cone3.hip and batch.hip pass; x^a in float64 rounded once, as pow_r of
             cone3.h and the reference's Float32 `^` have it)
  cpu_err    max |cpu - ref| / max(1, ||v||_inf), and its worst per family

`error` is that measure, `bound(kind, family, precision)` = max(4 * cpu_err worst, 16 eps) what the device is held to: x2 because the bisection may
end anywhere in its last interval and the device libm differs from the host's in the last place, x2 because a worst over 30 points underestimates
the family's.  A family whose f64 cpu_err worst is above 1e-5 (the project's bound for device against oracle) is `weak`: the reference algorithm
itself is far from the projection there, and the device is held to parity with `cpu` only.

Family -> the lines of cone3.h it is there for -> cpu_err worst in f64 and in f32, of the primal kind (a dual kind has the same to two digits):

  exp  uniform            [-25, 25]^3, the sampling of the other tests: every line once                                7.0e-10  1.9e-07
  exp  scale_1e-6         `tol` is absolute: both loops stop before they have moved a vector of norm 1e-6               2.5e-08  2.5e-08
  exp  scale_1e-3         the same, five digits above tol                                                               5.4e-07  5.4e-07
  exp  scale_1e3          the bracket `while (g > 0) lam *= 2` takes ten and more doublings                             2.2e-11  2.8e-07
  exp  scale_1e6          twenty doublings; u - l < tol is below one ulp of lam                                         2.9e-12  1.4e-01
  exp  branch_interior    the four returns of exp_project far from every predicate's edge; case 4 is t d(r) + mu n(r)   1.8e-09  1.7e-07
  exp  branch_edge        relative distance 1e-8 .. 1e-1 of the boundary of K and of x = 0 / y = 0 (case 3), both sides 1.8e-08  1.8e-02
  exp  branch_edge_polar  the same on both sides of the boundary of -K* (exp_in_dual)                                  6.3e-09  1.9e-07
  exp  y_small            y = +-1e-1 .. +-1e-9: exp(x / y) of exp_in_cone overflows, log(dt / lam) of exp_find_min_t    8.8e-08  3.1e-04
  exp  ratio_large        x / y = +-60 .. +-5000: exp overflows in Float32 (88) and in Float64 (709) or underflows      1.2e-07  8.3e-03
  pow  uniform            [-25, 25]^3, alpha in [0.1, 0.95]                                                             1.3e-10  7.4e-02
  pow  scale_1e-6         |phi| < tol at the first iterate; pow_phic's floor of 1e-10 is 1e-4 of the vector             5.1e-08  5.1e-08
  pow  scale_1e-3         the Newton loop stops five digits above tol                                                   4.7e-08  4.7e-08
  pow  scale_1e3          20 iterations without the help of the absolute stop                                           6.5e-11  3.9e-02
  pow  scale_1e6          the same                                                                                      9.0e-16  7.6e-08
  pow  branch_interior    the four returns of pow_project; case 4 is p + mu n(p)                                        3.1e-09  6.9e-08
  pow  branch_edge        relative distance 1e-8 .. 1e-1 of the boundary of K and of |z| = tol (case 3), both sides      3.8e-09  7.0e-08
  pow  branch_edge_polar  WEAK  the same on both sides of the boundary of -K* (pow_in_dual): r -> 0                     7.1e-05  1.0e-04
  pow  alpha_0.01         pow(x, a) with a next to 0; a^a (1 - a)^(1 - a) of pow_in_dual; dphix                         8.9e-10  5.9e-02
  pow  alpha_0.5          the symmetric cone                                                                            1.4e-09  4.6e-07
  pow  alpha_0.99         a next to 1                                                                                   1.3e-08  4.8e-07
  pow  xy_zero            WEAK  x = 0 or y = 0: phi_x or phi_y on the 1e-10 floor of pow_phic                           1.4e-02  2.0e-02
  pow  z_tiny             |z| = 1e-12 .. 1e-2 across the `fabs(v.z) <= tol` shortcut                                    1.5e-09  2.0e-05
  pow  z_sign             pairs (x, y, +-z): fabs(v.z) and z0 * r / az                                                  9.9e-10  1.2e-06

WEAK families (f64 cpu_err worst above 1e-5), a known property of the reference algorithm and not of the port:
  pow / dual_pow  xy_zero            1.4e-02 (f64), 2.0e-02 (f32): worst point (3.22, 0, -1.71), alpha 0.85, case 4: r runs into its clamp at |z|, where phi_y
                                     is the floor 1e-10 and the Newton step no longer moves
  pow / dual_pow  branch_edge_polar  7.1e-05 (f64), 1.0e-04 (f32): worst point (-0.916, -0.124, -1.0000006), alpha 0.78, 6e-7 outside -K*: the projection has
                                     norm 1e-6, twenty Newton steps from r = |z| / 2 end at 7e-5
In Float32 (tol = 1e-8 is below eps: the loops end at their caps or where a difference rounds to zero) the same stalls reach ordinary inputs: a
power cone with y < 0 < x returns (x, 1e-10, z) where the projection is (18.4, 0.096, 9.76) (uniform, 7.4e-2), an exponential cone at scale 1e6
returns (x, 0, 0) (1.4e-1).  These are what 4 * cpu_err allows the device in those families; in Float64 every family that is not weak is below 6e-7.

The numbers are the generator's (worst_table prints them); test_cone3_cases_host.py holds the fixture to them."""
import os

import numpy as np

from tests import projection_cases as S

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cone3_reference.npz")
KINDS = S.CONE3
PRIMAL = {S.EXP: S.EXP, S.DUAL_EXP: S.EXP, S.POW: S.POW, S.DUAL_POW: S.POW}
PRECISIONS = ("f64", "f32")
DTYPES = {"f64": np.float64, "f32": np.float32}
EPS = {"f64": S.EPS, "f32": S.EPS32}
MAX_ITER_EXP, MAX_ITER_POW, TOL = 100, 20, 1e-8          # k_cone3_project, batch_project_cone3_one
WEAK_ABOVE = 1e-5                                          # the bound of test_projection_matches_oracle, device against oracle
MEMBERS = 3


# ---- the algorithm of cone3.h in the scalar type T ------------------------------------------------------------------------------------------------
def _exp_in_cone(x, y, z, tol, T):
    return bool((y > T(0.0) and y * np.exp(x / y) <= z + tol) or (x <= tol and y == T(0.0) and z >= -tol))


def _exp_in_dual(x, y, z, tol, T):
    return bool((x < T(0.0) and -x * np.exp(y / x) - T(2.718281828459045) * z <= tol) or (abs(x) <= tol and y >= -tol and z >= -tol))


def _exp_find_min_t(lam, s0, t0, tol, T):
    dt = np.fmax(-t0, tol)
    for _ in range(150):
        f = dt * (dt + t0) / (lam * lam) - s0 / lam + np.log(dt / lam) + T(1.0)
        grad_f = (T(2.0) * dt + t0) / (lam * lam) + T(1.0) / dt
        dt = dt - f / grad_f
        if dt <= -t0:
            dt = -t0
            break
        elif dt <= T(0.0):
            dt = T(0.0)
            break
        elif abs(f) < tol:
            break
    return dt + t0


def _exp_grad_dual(lam, v0, tol, T):
    vz = _exp_find_min_t(lam, v0[1], v0[2], tol, T)
    vy = (T(1.0) / lam) * (vz - v0[2]) * vz
    vx = v0[0] - lam
    g = vx if vy == T(0.0) else vx + vy * np.log(vy / vz)
    return g, (vx, vy, vz)


def _exp_project(v, max_iter, tol, T):
    x, y, z = v
    if _exp_in_cone(x, y, z, T(0.0), T):
        return v, 1
    if _exp_in_dual(-x, -y, -z, T(0.0), T):
        return (T(0.0), T(0.0), T(0.0)), 2
    if x < T(0.0) and y < T(0.0):
        return (x, T(0.0), np.fmax(z, T(0.0))), 3
    lo, lam = T(0.0), T(0.125)
    g, out = _exp_grad_dual(lam, v, tol, T)
    guard = 0
    while g > T(0.0) and guard < 2000:
        guard += 1
        lo = lam
        lam = lam * T(2.0)
        g, out = _exp_grad_dual(lam, v, tol, T)
    hi = lam
    for _ in range(max_iter):
        lam = (hi + lo) / T(2.0)
        g, out = _exp_grad_dual(lam, v, tol, T)
        if g > T(0.0):
            lo = lam
        else:
            hi = lam
        if hi - lo < tol:
            break
    return out, 4


def _pow(x, a, T):
    """pow_r of cone3.h: the power in float64, rounded once to T (in float64: np.power)"""
    return T(np.power(np.float64(x), np.float64(a)))


def _pow_in_cone(x, y, z, a, tol, T):
    return bool(x >= T(0.0) and y >= T(0.0) and _pow(x, a, T) * _pow(y, T(1.0) - a, T) >= abs(z) - tol)


def _pow_in_dual(x, y, z, a, tol, T):
    return bool(x >= -tol and y >= -tol
                and _pow(x, a, T) * _pow(y, T(1.0) - a, T) >= abs(z) * _pow(a, a, T) * _pow(T(1.0) - a, T(1.0) - a, T) - tol)


def _pow_project(v, a, max_iter, tol, T):
    x0, y0, z0 = v
    if _pow_in_cone(x0, y0, z0, a, T(0.0), T):
        return v, 1
    if _pow_in_dual(-x0, -y0, -z0, a, T(0.0), T):
        return (T(0.0), T(0.0), T(0.0)), 2
    if abs(z0) <= tol:
        return (np.fmax(x0, T(0.0)), np.fmax(y0, T(0.0)), z0), 3
    az = abs(z0)

    def phic(c0, r_, a_):
        return np.fmax(T(0.5) * (c0 + np.sqrt(c0 * c0 + T(4.0) * a_ * r_ * (az - r_))), T(1e-10))

    r = az / T(2.0)
    phix = phiy = T(0.0)
    for _ in range(max_iter):
        phix = phic(x0, r, a)
        phiy = phic(y0, r, T(1.0) - a)
        prod = _pow(phix, a, T) * _pow(phiy, T(1.0) - a, T)
        phi = prod - r
        if abs(phi) < tol:
            break
        dphix = a / (T(2.0) * phix - x0) * (az - T(2.0) * r)
        dphiy = (T(1.0) - a) / (T(2.0) * phiy - y0) * (az - T(2.0) * r)
        dphi = prod * (a * dphix / phix + (T(1.0) - a) * dphiy / phiy) - T(1.0)
        r = r - phi / dphi
        r = np.fmin(np.fmax(r, T(0.0)), az)
    return (phix, phiy, z0 * r / az), 4


def project_cpu(v, kind, alpha, dtype):
    """(projection, case) of one 3-vector by the algorithm of cone3.h (project_kind with the constants of its two callers), every operation in `dtype`"""
    T = np.dtype(dtype).type
    v = tuple(T(t) for t in v)
    a, tol = T(alpha), T(TOL)
    with np.errstate(all="ignore"):
        if kind == S.EXP:
            out, br = _exp_project(v, MAX_ITER_EXP, tol, T)
        elif kind == S.POW:
            out, br = _pow_project(v, a, MAX_ITER_POW, tol, T)
        else:                                                                 # Moreau: v + Proj_K(-v), the sum as project_kind orders it (t + v0)
            t = tuple(-c for c in v)
            out, br = _exp_project(t, MAX_ITER_EXP, tol, T) if kind == S.DUAL_EXP else _pow_project(t, a, MAX_ITER_POW, tol, T)
            out = tuple(p + c for p, c in zip(out, v))
    return np.array(out, dtype=dtype), br


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------------
class Points:
    """the rows of one (kind, precision): v (N, 3), alpha (N), ref (N, 3), branch (N), cpu (N, 3), cpu_err (N), family (N, index into names), names,
    pair (N, 2: the two cases of a branch_edge pair, 0 elsewhere), worst (per family), weak (per family)"""

    def __init__(self, z, kind, prec):
        self.kind, self.prec = kind, prec
        pk = PRIMAL[kind]
        self.names = [str(s) for s in z["%s_names" % pk]]
        self.family = z["%s_family" % pk]
        self.pair = z["%s_pair" % pk]
        for f in ("v", "alpha", "ref", "branch", "cpu", "cpu_err", "worst"):
            a = z["%s_%s_%s" % (kind, prec, f)]
            a.setflags(write=False)
            setattr(self, f, a)
        w64 = z["%s_f64_worst" % kind]
        self.weak = [bool(w > WEAK_ABOVE) for w in w64]
        self.n = self.v.shape[0]

    def rows_of(self, family):
        return np.flatnonzero(self.family == self.names.index(family))


_points = {}


def points(kind, prec):
    """loaded once, shared, read-only"""
    if not _points:
        with np.load(FIXTURE) as z:
            for k in KINDS:
                for p in PRECISIONS:
                    _points[(k, p)] = Points(z, k, p)
    return _points[(kind, prec)]


def error(out, ref, v):
    """relative infinity-norm error per point: max |out - ref| / max(1, ||v||_inf)"""
    out, ref, v = (np.asarray(t, dtype=np.float64).reshape(-1, 3) for t in (out, ref, v))
    return np.max(np.abs(out - ref), axis=1) / np.maximum(1.0, np.max(np.abs(v), axis=1))


def bound(kind, family, prec):
    """what the device result of a family that is not weak is held to: max(4 * cpu_err worst, 16 eps)"""
    P = points(kind, prec)
    return max(4.0 * float(P.worst[P.names.index(family)]), 16.0 * EPS[prec])


def weak_families(kind):
    P = points(kind, "f64")
    return [nm for nm, w in zip(P.names, P.weak) if w]


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------
def case_name(kind, prec):
    return "cone3ref_%s_%s" % (kind, prec)


def point_index(P, member, cone):
    """points are dealt round-robin: point i is cone i // MEMBERS of member i % MEMBERS, so every member holds a third of every family"""
    return cone * MEMBERS + member


_cases = {}


def case(kind, prec):
    """projection_cases.Case of all points of one kind in one precision: N / 3 cones, three members.  The rows are float64 values (in the f32 set:
    exactly representable in Float32)."""
    key = (kind, prec)
    if key not in _cases:
        P = points(kind, prec)
        assert P.n % MEMBERS == 0
        nc = P.n // MEMBERS
        for k in range(1, MEMBERS):                                           # one alpha per cone of the structure
            assert np.array_equal(P.alpha[0::MEMBERS], P.alpha[k::MEMBERS])
        cones = [S.Cone(kind, 3, alpha=float(P.alpha[point_index(P, 0, j)])) for j in range(nc)]
        members = []
        for k in range(MEMBERS):
            idx = [point_index(P, k, j) for j in range(nc)]
            rows = np.ascontiguousarray(P.v[idx].reshape(-1))
            rows.setflags(write=False)
            members.append(S.Member(rows, ["cone3"] * nc, [int(b) for b in P.branch[idx]], [P.names[f] for f in P.family[idx]]))
        _cases[key] = S.Case(case_name(kind, prec), cones, members, float32=True)
    return _cases[key]


def gather(P, per_member):
    """per-member arrays of length 3 * (N / 3) back into point order: (N, 3)"""
    out = np.empty((P.n, 3), dtype=np.asarray(per_member[0]).dtype)
    for k, a in enumerate(per_member):
        out[k::MEMBERS] = np.asarray(a).reshape(-1, 3)
    return out


def poison_case(prec):
    """exponential and power cones and their duals in one structure: 12 cones of every kind (branch_interior and uniform points), three clean members and
    member 3 = member 1 with a NaN in its first exponential cone and +inf in its first power cone"""
    key = ("poison", prec)
    if key not in _cases:
        cones, rows = [], [[] for _ in range(MEMBERS)]
        for kind in KINDS:
            P = points(kind, prec)
            idx = np.concatenate([P.rows_of("branch_interior")[:18], P.rows_of("uniform")[:18]])
            for j in range(len(idx) // MEMBERS):
                cones.append(S.Cone(kind, 3, alpha=float(P.alpha[idx[MEMBERS * j]])))
                for k in range(MEMBERS):
                    assert P.alpha[idx[MEMBERS * j + k]] == P.alpha[idx[MEMBERS * j]]
                    rows[k].append(P.v[idx[MEMBERS * j + k]])
        rows = [np.concatenate(r) for r in rows]
        bad = rows[1].copy()
        first_exp = 3 * [c.kind for c in cones].index(S.EXP)
        first_pow = 3 * [c.kind for c in cones].index(S.POW)
        bad[first_exp + 1] = np.nan
        bad[first_pow] = np.inf
        nc = len(cones)
        members = [S.Member(r, ["cone3"] * nc, [-1] * nc, [""] * nc) for r in rows + [bad]]
        for mb in members:
            mb.rows.setflags(write=False)
        c = S.Case("cone3ref_poison_" + prec, cones, members, float32=True)
        c.poisoned = (first_exp // 3, first_pow // 3)
        _cases[key] = c
    return _cases[key]
