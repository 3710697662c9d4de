"""Inputs for the infeasibility certificates (csrc/infeas.hip: the five kernels, psd_extreme_eigs in certificate mode, cone3_enqueue_in_dual_neg;
csrc/batch.hip: batch_inf_check_body) and a plain reference written from the definitions (src/infeasibility.jl:1-68, the in_dual / in_pol_recc /
support_function methods of src/convexset.jl).  No test functions, no GPU code, nothing from the oracle: imported by test_certificate_cases_host.py
(CPU) and test_gpu_certificates.py (GPU).

A CASE is one problem structure in the scaled space the loop works in -- P, A, q, b, cones, D, E, c, eps_prim_inf = 2^-10, eps_dual_inf = 2^-8 -- with
MEMBERS (dx, dy, expected status, the comparison that decides it).  A case is built per precision: every number of it is representable in that type,
and "one ulp" is an ulp of that type.  Every member is one of two kinds:

  tie        the deciding quantity is exact in any summation order (terms that are multiples of one power of two, small enough for the mantissa;
             perfect squares under the root) and sits on its threshold or one ulp to either side
  decisive   every inexact quantity the evaluation meets is away from its threshold by at least MARGIN = 1000 times its rounding bound in the type under
             test: (nnz + 2) eps sum|a||x| for row sums and dots, 64 d eps ||X||_F for lambda_min, the bounds written at the 3-d cones below

Float32 runs every case but side 257 (float32_runs); its PSD members of sides above 16 are matrices of small norm (_psd_vector, lean), the only ones
that 64 d eps32 ||X||_F leaves MARGIN bounds away from tol.

evaluate() returns the status and every comparison it went through (value, threshold, rounding bound, 0 where the value is exact);
tests/test_certificate_cases_host.py holds every member to the rule above and to the oracle.

How a chosen vector gets in front of a cone test.  "primal" structures: n = 2, one tiny entry in A, b = 0, a last ZeroSet row that holds dy = 1, so
||E dy||_inf = 1 and the cones see dy itself (in_dual(dy); the Box support function sees -dy).  "dual" structures: A = [I | 0], q = -e_n, dx = [u; 1], so
||D dx||_inf = 1 and the cones see A dx = u (in_pol_recc(u)).  P = 2^-12 I in both.

Which lines a case is there for:

  gates            n = 4, m = 6, powers of two in D, E, c = 8: each of the six scalar comparisons on its threshold and one ulp to either side; both
                   certificates at once (primal wins); the cone test of the primal certificate failing with the dual certificate holding
  scaling          n = 40, m = 60, D, E random powers of two in 2^-6 .. 2^6, c = 8: members whose verdict flips when E and Einv, D and Dinv or the two
                   tolerances are exchanged, or c is replaced by 1 or by 1 / c (Member.flips; evaluate(mutate=...))
  reductions_300   n + m = 300: two workgroups of k_inf_deltas
  reductions_big   n + m = COSMO_BS * COSMO_MAX_PARTIALS + 1000 (handle only): the second grid-stride trip of k_inf_deltas / k_inf_primal_rows /
                   k_inf_dual_rows, host_max / host_sum over 2048 partials, one column of A with 3000 nonzeros (a [P | A'] row longer than
                   COSMO_NNZ_PER_BLOCK); the deciding entry first, last and inside the second trip; integer dot products
  reductions_batch n = 600, m = 4000: several CSR tiles per matrix in the batch kernel, the deciding entry at 0, 255, 256 and last, the same long column
  simple_*         ZeroSet / Nonnegatives / Box rows interleaved; finite, one-sided, two-sided-infinite and equality bounds; the |y| <= tol, y > 0 rule
                   of the Box support function; 0 * -Inf = NaN (no certificate); in_pol_recc on infinite bounds only; one violating row first / last
  soc_*            dims 1, 2, 3, 64, 65, 66, 129, 1000 in one member: on the boundary, one ulp inside, one ulp outside, in both modes
  soc70_*          70 cones per member (more cones than waves of a batch workgroup), the single violator first / last
  soc16400_*       16 400 cones of dim 1 and 2 (handle only: more cones than the 4 * 4096 waves of k_inf_soc's grid), the violator in the last cone
  psd_small9_*     nine cones of side 2, 3, 16, triangle and square (more than four per member: every wave workspace of the batch kernel reused)
  psd_mid3_*       sides 17, 33, 64 in one member (psdwg_*, mid_goff; the second route of psd_extreme_eigs)
  psd_side1_*      1 x 1 cones, triangle and square, on their threshold
  psd_large_*      sides 65 and 130 (handle only: the 16-wave class)
  psd_257_*        side 257 (handle only: the multi-workgroup class and k_psd_eigmin)
  psd_unsym_*      square blocks that are not symmetric: is_pos_def! reads the upper triangle only ([[1, 0], [-10, 1]] passes)
  cone3_<kind>_*   300 cones per member, sampled as projection_cases.cone3_inputs plus the closure branches (|x| <= tol); points within the margin dropped
  poison           NaN / +-Inf in dy or dx; the poisoned members sit between clean ones (Case.clean: the batch without them)
"""
import dataclasses
import functools
import math

import numpy as np
import scipy.sparse as sp

from tests.projection_cases import (BOX, CONE3, DUAL_EXP, DUAL_POW, EPS, EPS32, EXP, LD, NONNEG, POW, PSD, PSD_SQ, PSD_TRI, SOC, ZERO, Cone,
                                    cone3_inputs, psd_rows, smat)

EPS_PRIM_INF, EPS_DUAL_INF = 2.0 ** -10, 2.0 ** -8
UNDETERMINED, PRIMAL, DUAL = 0, 4, 5          # COSMO_HIP_UNDETERMINED / _PRIMAL_INFEASIBLE / _DUAL_INFEASIBLE
MARGIN = 1000.0
TINY = 2.0 ** -12
DTYPES = {"f64": np.float64, "f32": np.float32}
MUTATIONS = ("E", "D", "c1", "cinv", "eps")
GATES = ("norm_dy > eps", "|Dinv A'dy| <= eps norm_dy", "sF <= eps", "norm_dx > eps", "q'dx / (norm_dx c) < -eps", "|Dinv P dx| / (norm_dx c) <= eps")
COSMO_BS, COSMO_MAX_PARTIALS, COSMO_NNZ_PER_BLOCK = 256, 2048, 2048      # csrc/internal.h (asserted by the host test)
CONE3_DROP_CAP = 0.10


@dataclasses.dataclass
class Member:
    name: str
    dx: np.ndarray
    dy: np.ndarray
    expected: int
    deciding: str                # the name of the comparison that decides it (Check.name)
    kind: str                    # "tie" | "decisive"
    flips: tuple = ()            # scaling: the mutations of evaluate() under which the verdict changes
    poisoned: bool = False


@dataclasses.dataclass
class Case:
    name: str
    dtype_id: str
    P: object
    A: object
    q: np.ndarray
    b: np.ndarray
    cones: list
    D: np.ndarray
    E: np.ndarray
    c: float
    members: list
    handle: bool = True
    batch: bool = True
    clean: object = None         # poison: indices of the members that also form the batch without the poisoned ones
    dropped: object = None       # cone3: (points drawn, points dropped)

    @property
    def n(self):
        return self.A.shape[1]

    @property
    def m(self):
        return self.A.shape[0]

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum([c.dim for c in self.cones])]).astype(np.int64)


@dataclasses.dataclass
class Check:
    name: str
    value: float
    op: str                      # ">", "<", "<=", ">="
    threshold: float
    bound: float                 # rounding bound of value - threshold in the type under test; 0: exact in any order
    passed: bool
    scale: float = 0.0           # the largest magnitude among the numbers that form value and threshold: "one ulp" of a tie is an ulp of this

    @property
    def ratio(self):
        """|value - threshold| / bound (inf where the value is exact or not finite: a NaN or an infinity decides whatever the rounding)"""
        d = abs(float(self.value) - float(self.threshold))
        if self.bound == 0 or not math.isfinite(d):
            return math.inf
        return d / self.bound


# ---- exactness in the type under test ------------------------------------------------------------------------------------------------------------
def _mant(dtype):
    return 53 if np.dtype(dtype) == np.float64 else 24


def _fits(v, dtype):
    """is the long double v a number of the type?"""
    v = LD(v)
    return bool(not np.isfinite(v) or LD(np.dtype(dtype).type(v)) == v)


def _sum_exact(terms, dtype):
    """Every partial sum of `terms`, in any order, is a number of the type: the terms are multiples of one power of two q and sum|t| < 2^mantissa q."""
    t = np.asarray(terms, dtype=LD).ravel()
    t = t[t != 0]
    if t.size == 0:
        return True
    t64 = t.astype(np.float64)
    if not np.all(np.isfinite(t)) or not np.all(t64.astype(LD) == t):
        return False
    if t.size <= 12:                                           # few terms: every partial sum in any order is a subset sum; look at all of them
        sums = np.zeros(1, dtype=LD)
        for v in t:
            sums = np.concatenate([sums, sums + v])
        return bool(np.all(sums.astype(np.dtype(dtype)).astype(LD) == sums))
    mant, ex = np.frexp(np.abs(t64))
    mi = (mant * 2.0 ** 53).astype(np.int64)                  # t = mi 2^(ex - 53); its lowest set bit: t = odd * 2^low
    low = ex.astype(np.int64) - 53 + np.log2((mi & -mi).astype(np.float64)).astype(np.int64)
    q = LD(2.0) ** int(low.min())
    return bool(np.sum(np.abs(t)) / q < LD(2.0) ** _mant(dtype))


def _dot(a, x, dtype, eps):
    """(sum a_i x_i in long double, its rounding bound (nnz + 2) eps sum|a_i x_i|, 0 if every product and every partial sum is exact)"""
    a = np.asarray(a, dtype=LD)
    x = np.asarray(x, dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        t = a * x
        s = np.sum(t) if t.size else LD(0.0)
    if not np.all(np.isfinite(t)):
        return s, 0.0
    if all(_fits(v, dtype) for v in t[t != 0]) and _sum_exact(t, dtype):
        return s, 0.0
    return s, float((np.count_nonzero(t) + 2) * eps * np.sum(np.abs(t)))


def _maxabs(v):
    """norm(v, Inf) as Julia computes it: a NaN wins"""
    v = np.abs(np.asarray(v, dtype=LD))
    if v.size == 0:
        return LD(0.0)
    return LD(np.nan) if np.isnan(v).any() else np.max(v)


def _cmp(value, op, threshold):
    with np.errstate(invalid="ignore"):
        return bool({">": value > threshold, "<": value < threshold, "<=": value <= threshold, ">=": value >= threshold}[op])


class _Trace:
    def __init__(self):
        self.checks = []

    def test(self, name, value, op, threshold, bound, scale=None):
        ok = _cmp(LD(value), op, LD(threshold))
        if scale is None:
            scale = max(abs(float(value)), abs(float(threshold)))
        self.checks.append(Check(name, float(value), op, float(threshold), float(bound), ok, float(scale)))
        return ok


# ---- the cone tests from the definitions ---------------------------------------------------------------------------------------------------------
def _upper_hermitian(x, cone):
    """Hermitian(X, 'U') of the matrix a PSD cone's rows stand for (src/convexset.jl:324-328, 415-418: populate_upper_triangle!, is_pos_def!)"""
    d = cone.side
    if cone.kind == PSD_TRI:
        return smat(np.asarray(x, dtype=np.float64), d)
    X = np.asarray(x, dtype=np.float64).reshape(d, d, order="F")
    return np.triu(X) + np.triu(X, 1).T


def _psd_in_dual(tr, x, cone, tol, eps, where):
    """is_pos_def!(X + tol I) (src/algebra.jl:226-233) <=> lambda_min(Hermitian(X, 'U')) > -tol"""
    if cone.dim == 1:                                          # Cholesky of the 1 x 1 matrix x + tol succeeds iff x + tol > 0: one exact comparison
        return tr.test(where + " psd 1x1 x > -tol", x[0], ">", -tol, 0.0)
    if np.isnan(np.asarray(x, dtype=np.float64)).any():
        return tr.test(where + " psd lambda_min > -tol", np.nan, ">", -tol, 0.0)
    U = _upper_hermitian(x, cone)
    lam = float(np.linalg.eigvalsh(U).min())
    return tr.test(where + " psd lambda_min > -tol", lam, ">", -tol, 64.0 * cone.side * eps * float(np.linalg.norm(U)))


def _soc_in_dual(tr, x, tol, dtype, eps, where):
    """norm(x[2:]) <= tol + x[1]  (src/convexset.jl:116-118)"""
    x = np.asarray(x, dtype=LD)
    sq = x[1:] * x[1:]
    with np.errstate(invalid="ignore", over="ignore"):
        ss = np.sum(sq) if sq.size else LD(0.0)
        nx = np.sqrt(ss)
        thr = LD(tol) + x[0]
    exact = bool(np.all(np.isfinite(x))) and all(_fits(v, dtype) for v in sq[sq != 0]) and _sum_exact(sq, dtype) and nx * nx == ss and _fits(nx, dtype) \
        and _fits(thr, dtype)
    bound = 0.0 if exact or not np.isfinite(nx) else float((x.size + 2) * eps * nx + eps * abs(thr))
    return tr.test(where + " soc |x[2:]| <= tol + x[1]", nx, "<=", thr, bound, scale=max(float(abs(tol)), float(abs(x[0])), float(nx)) if x.size else None)


def _cone3_in_dual(tr, kind, v, alpha, tol, eps, where):
    """in_dual of the 3-d cones (src/convexset.jl:609-614 exponential, :732-738 power; the dual cones' in_dual is the primal in_cone, :589-594, :707-713,
    :770-772).  The comparisons of an input with +-tol or 0 are exact.  Rounding bounds of the two expressions, each with a factor 8 for the libm calls:
    x exp(y / x): the quotient's rounding is amplified by |y / x|, so 8 eps |x| exp(y / x) (1 + |y / x|), plus 8 eps e |z|;
    s^a t^(1-a): relative error (1 + |a ln s| + |(1-a) ln t|) eps per power, plus 8 eps |w| a^a (1-a)^(1-a)."""
    x, y, z = (LD(t) for t in v)
    tolL = LD(tol)
    with np.errstate(all="ignore"):
        if kind in (EXP, DUAL_EXP):
            if kind == EXP:                                    # in_dual(ExponentialCone)
                ok = False
                if x < 0:
                    ex = -x * np.exp(y / x)
                    ok = tr.test(where + " exp -x exp(y/x) - e z <= tol", ex - LD(math.e) * z, "<=", tolL,
                                 8 * eps * float(ex * (1 + abs(y / x)) + LD(math.e) * abs(z)) if np.isfinite(ex) else 0.0)
                return bool(ok or (abs(x) <= tolL and y >= -tolL and z >= -tolL))
            ok = False                                         # in_dual(DualExponentialCone) = in_cone(ExponentialCone)
            if y > 0:
                ex = y * np.exp(x / y)
                ok = tr.test(where + " exp y exp(x/y) <= z + tol", ex - z, "<=", tolL, 8 * eps * float(ex * (1 + abs(x / y)) + abs(z)) if np.isfinite(ex) else 0.0)
            return bool(ok or (x <= tolL and y == 0 and z >= -tolL))
        a = LD(alpha)
        if kind == POW:                                        # in_dual(PowerCone)
            if not (x >= -tolL and y >= -tolL):
                return False
            if x < 0 or y < 0:                                 # a negative base: NaN, the comparison is false
                return False
            lhs = x ** a * y ** (1 - a)
            rhs = abs(z) * a ** a * (1 - a) ** (1 - a)
        else:                                                  # in_dual(DualPowerCone) = in_cone(PowerCone)
            if not (x >= 0 and y >= 0):
                return False
            lhs = x ** a * y ** (1 - a)
            rhs = abs(z)
        amp = 1 + (abs(a * np.log(x)) if x > 0 else 0) + (abs((1 - a) * np.log(y)) if y > 0 else 0)
        return tr.test(where + " pow s^a t^(1-a) >= |w| k - tol", lhs - rhs, ">=", -tolL, 8 * eps * float(lhs * amp + rhs))


def _in_dual(tr, x, cone, tol, dtype, eps, where):
    """in_dual(x, cone, tol) for the cones support_function! reaches"""
    if cone.kind == ZERO:
        return True
    if cone.kind == NONNEG:                                    # !any(x < -tol) (:76-78): comparisons of inputs
        xs = np.asarray(x, dtype=LD)
        bad = xs < -LD(tol)
        if xs.size:
            k = int(np.argmin(xs)) if not np.isnan(xs).any() else int(np.argmax(np.isnan(xs)))
            tr.test(where + " nonneg min x >= -tol", xs[k], ">=", -tol, 0.0)
        return not bool(bad.any())
    if cone.kind == SOC:
        return _soc_in_dual(tr, x, tol, dtype, eps, where)
    if cone.kind in PSD:
        return _psd_in_dual(tr, x, cone, tol, eps, where)
    seen = len(tr.checks)
    ok = _cone3_in_dual(tr, cone.kind, x, cone.alpha, tol, eps, where)
    if len(tr.checks) == seen:                                 # decided by comparisons of the inputs with 0 and +-tol alone: exact
        tr.checks.append(Check(where + (" exp " if cone.kind in (EXP, DUAL_EXP) else " pow ") + "exact comparisons", float(ok), ">=", 0.5, 0.0, ok))
    return ok


def _in_pol_recc(tr, x, cone, tol, dtype, eps, where):
    xs = np.asarray(x, dtype=LD)
    tolL = LD(tol)
    with np.errstate(invalid="ignore"):
        if cone.kind == ZERO:                                  # !any(|x| > tol) (:34-36)
            if xs.size:
                tr.test(where + " zero max|x| <= tol", _maxabs(xs), "<=", tol, 0.0)
            return not bool((np.abs(xs) > tolL).any())
        if cone.kind == NONNEG:                                # !any(x > tol) (:80-82)
            if xs.size:
                tr.test(where + " nonneg max x <= tol", np.nan if np.isnan(xs).any() else np.max(xs), "<=", tol, 0.0)
            return not bool((xs > tolL).any())
        if cone.kind == BOX:                                   # (:859-861): the infinite bounds only
            u, l = np.asarray(cone.u, dtype=LD), np.asarray(cone.l, dtype=LD)
            if (u == np.inf).any():
                tr.test(where + " box recc max x <= tol where u = Inf", np.max(xs[u == np.inf]), "<=", tol, 0.0)
            if (l == -np.inf).any():
                tr.test(where + " box recc min x >= -tol where l = -Inf", np.min(xs[l == -np.inf]), ">=", -tol, 0.0)
            return not bool(((u == np.inf) & (xs > tolL)).any()) and not bool(((l == -np.inf) & (xs < -tolL)).any())
    if cone.kind == SOC:                                       # norm(x[2:]) <= tol - x[1] (:120-122)
        return _soc_in_dual(tr, -xs, tol, dtype, eps, where)
    if cone.kind in PSD:                                       # is_neg_def!(X, tol) = is_pos_def!(-X, tol) (:421-424, algebra.jl:235-238)
        return _psd_in_dual(tr, -np.asarray(x, dtype=np.float64), cone, tol, eps, where)
    return _in_dual(tr, -xs, cone, tol, dtype, eps, where)    # (:616-618, 740-742)


# ---- the two certificates (src/infeasibility.jl:1-68) -------------------------------------------------------------------------------------------
def _columns(M, dtype):
    M = sp.coo_matrix(M)
    return M.row, M.col, np.asarray(M.data, dtype=dtype).astype(LD)


def _matvec(rows, cols, vals, x, nout, dtype, eps):
    """(y = M x in long double, per-row rounding bound (nnz + 2) eps sum|a||x|, 0 for a row whose products and partial sums are exact)"""
    y = np.zeros(nout, dtype=LD)
    ab = np.zeros(nout, dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        t = vals * x[cols]
    np.add.at(y, rows, t)
    np.add.at(ab, rows, np.abs(t))
    nz = t != 0
    cnt = np.bincount(rows[nz], minlength=nout)
    bound = ((cnt + 2) * LD(eps) * ab).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fits = (t.astype(np.dtype(dtype)).astype(LD) == t) | ~np.isfinite(t)
    rowfits = np.ones(nout, dtype=bool)
    np.logical_and.at(rowfits, rows, fits)
    bound[rowfits & (cnt <= 1)] = 0.0
    bound[~np.isfinite(bound)] = 0.0                          # a NaN or an infinity decides whatever the rounding
    for r in np.flatnonzero(rowfits & (cnt > 1)):
        if _sum_exact(t[rows == r], dtype):
            bound[r] = 0.0
    return y, bound


def evaluate(case, dx, dy, mutate=()):
    """(status, checks): is_primal_infeasible! then is_dual_infeasible! as check_termination! calls them (src/solver.jl:336-347), every scalar in long
    double on the case's numbers rounded to its type.  mutate: names of MUTATIONS -- the wrong formulas the scaling case tells apart."""
    dtype = DTYPES[case.dtype_id]
    eps = EPS if case.dtype_id == "f64" else EPS32
    rd = lambda a: np.asarray(a, dtype=dtype).astype(LD)
    epi, edi = LD(EPS_PRIM_INF), LD(EPS_DUAL_INF)
    if "eps" in mutate:
        epi, edi = edi, epi
    D, E = rd(case.D), rd(case.E)
    Dinv, Einv = 1 / D, 1 / E
    if "E" in mutate:
        E, Einv = Einv, E
    if "D" in mutate:
        D, Dinv = Dinv, D
    c = LD(case.c)
    if "c1" in mutate:
        c = LD(1.0)
    if "cinv" in mutate:
        c = 1 / c
    dx, dy, q, b = rd(dx), rd(dy), rd(case.q), rd(case.b)
    n, m = case.n, case.m
    ar, ac, av = _columns(case.A, dtype)
    pr, pc, pv = _columns(case.P, dtype)
    tr = _Trace()
    off = case.offsets
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        # ---- is_primal_infeasible! ----
        norm_dy = _maxabs(E * dy)                                                                   # :5
        if tr.test(GATES[0], norm_dy, ">", epi, 0.0 if _fits(norm_dy, dtype) else eps * float(norm_dy)):
            aty, bnd = _matvec(ac, ar, av, dy, n, dtype, eps)                                       # :12-14
            r = np.abs(Dinv * aty)
            k = int(np.argmax(np.where(np.isnan(r), np.inf, r))) if n else 0
            thr = epi * norm_dy
            if tr.test(GATES[1], _maxabs(r), "<=", thr, float(np.max(bnd * Dinv)) + (0.0 if _fits(thr, dtype) else eps * float(thr))):   # :17
                scale = -1 / norm_dy
                dyn = dy * scale                                                                    # :19
                ynoise = 0.0 if (_fits(scale, dtype) and all(_fits(v, dtype) for v in dyn[dyn != 0][:4096])) else 2 * eps
                dtb, dtb_bound = _dot(dyn, b, dtype, eps)                                           # :20
                sF, sF_bound, in_dual_all = LD(0.0), dtb_bound, True
                terms = [np.abs(dyn * b)]                                                           # the numbers that form sF: a tie's ulp is an ulp of the largest
                for i, cone in enumerate(case.cones):
                    y = dyn[off[i]:off[i + 1]]
                    where = "cone %d" % i
                    if cone.kind == BOX:                                                            # support_function(::Box) (convexset.jl:850-856)
                        l, u = rd(cone.l), rd(cone.u)
                        pick_u = (np.abs(y) > epi) & (y > 0)
                        near = np.abs(np.abs(y) - epi)
                        loose = (l != u)
                        if ynoise and loose.any():
                            tr.test(where + " box |y| > tol picks u", float(np.min(near[loose])) + float(epi), ">", epi, ynoise * float(np.max(np.abs(y))))
                        elif loose.any():
                            j = int(np.argmin(np.where(loose, near, np.inf)))
                            tr.test(where + " box |y| > tol picks u", np.abs(y[j]), ">", epi, 0.0)
                        s, sb = _dot(y, np.where(pick_u, u, l), dtype, eps)
                        terms.append(np.abs(y * np.where(pick_u, u, l)))
                        sF = sF + s
                        sF_bound += sb + ynoise * float(np.sum(np.abs(y * np.where(pick_u, u, l)))) if np.isfinite(s) else 0.0
                    else:                                                                           # support_function!: 0 if -y in the dual cone else Inf (:928-936)
                        if not _in_dual(tr, -y, cone, epi, dtype, eps, where):
                            in_dual_all = False
                            sF = sF + LD(np.inf)
                sF = sF - dtb                                                                       # :22
                terms = np.concatenate(terms)
                terms = terms[np.isfinite(terms)]
                if tr.test(GATES[2], sF, "<=", epi, sF_bound + ynoise * float(abs(dtb)) if np.isfinite(sF) else 0.0,
                           scale=max(float(epi), float(terms.max()) if terms.size else 0.0)):
                    return PRIMAL, tr.checks
        # ---- is_dual_infeasible! ----
        norm_dx = _maxabs(D * dx)                                                                   # :35
        if tr.test(GATES[3], norm_dx, ">", edi, 0.0 if _fits(norm_dx, dtype) else eps * float(norm_dx)):
            qdx, qb = _dot(q, dx, dtype, eps)
            den = norm_dx * c
            quo = qdx / den
            if tr.test(GATES[4], quo, "<", -edi, (qb / float(den) if np.isfinite(den) and den != 0 else 0.0) + (0.0 if _fits(quo, dtype) else eps * abs(float(quo)))):
                pdx, bnd = _matvec(pr, pc, pv, dx, n, dtype, eps)                                   # :44-47
                r = np.abs(Dinv * pdx)
                val = _maxabs(r) / den
                if tr.test(GATES[5], val, "<=", edi, (float(np.max(bnd * Dinv)) / float(den) if np.isfinite(den) and den != 0 else 0.0) +
                           (0.0 if _fits(val, dtype) else eps * abs(float(val)))):                  # :49
                    adx, bnd = _matvec(ar, ac, av, dx, m, dtype, eps)                               # :53-59
                    inv = 1 / norm_dx
                    adx = (adx * Einv) * inv
                    noise = 0.0 if _fits(inv, dtype) else 2 * eps
                    in_recc = True
                    for i, cone in enumerate(case.cones):
                        x = adx[off[i]:off[i + 1]]
                        rb = bnd[off[i]:off[i + 1]]
                        if (rb > 0).any() or noise:                                                 # inexact rows in front of a cone test: their noise against the margin
                            xb = rb * np.abs(np.asarray(Einv[off[i]:off[i + 1]] * inv, dtype=np.float64)) + noise * np.abs(x.astype(np.float64))
                            dist = np.minimum(np.abs(np.abs(x) - edi), np.abs(x)).astype(np.float64)
                            j = int(np.argmax(np.where(xb > 0, xb / np.maximum(dist, 1e-300), 0)))
                            if xb[j] > 0:
                                tr.test("cone %d input row away from +-tol" % i, dist[j] + float(edi), ">", edi, float(xb[j]))
                        if not _in_pol_recc(tr, x, cone, edi, dtype, eps, "cone %d" % i):
                            in_recc = False
                            break
                    if in_recc:
                        return DUAL, tr.checks
    return UNDETERMINED, tr.checks


# ---- builders -----------------------------------------------------------------------------------------------------------------------------------------
def _rd(a, dtype_id):
    """round to the case's type, keep float64 storage"""
    return np.asarray(a, dtype=DTYPES[dtype_id]).astype(np.float64)


def _ulp(x, dtype_id, direction):
    t = DTYPES[dtype_id]
    return float(np.nextafter(t(x), t(direction)))


def _primal_structure(name, dtype_id, cones, members, **kw):
    """cones + one ZeroSet row that carries dy = 1: the cones see dy (see the module docstring).  members: (name, v, expected, deciding, kind)"""
    cones = list(cones) + [Cone(ZERO, 1)]
    m = sum(c.dim for c in cones)
    A = sp.csc_matrix(([TINY], ([m - 1], [1])), shape=(m, 2))
    P = sp.identity(2, format="csc") * TINY
    ms = [Member(nm, np.zeros(2), np.concatenate([_rd(v, dtype_id), [1.0]]), ex, dec, kind) for nm, v, ex, dec, kind in members]
    return Case(name, dtype_id, P, A, np.zeros(2), np.zeros(m), cones, np.ones(2), np.ones(m), 1.0, ms, **kw)


def _dual_structure(name, dtype_id, cones, members, **kw):
    """A = [I | 0], q = -e_n, dx = [u; 1]: the cones see u.  members: (name, u, expected, deciding, kind)"""
    cones = list(cones)
    m = sum(c.dim for c in cones)
    n = m + 1
    A = sp.csc_matrix((np.ones(m), (np.arange(m), np.arange(m))), shape=(m, n))
    P = sp.identity(n, format="csc") * TINY
    q = np.zeros(n)
    q[-1] = -1.0
    ms = [Member(nm, np.concatenate([_rd(u, dtype_id), [1.0]]), np.zeros(m), ex, dec, kind) for nm, u, ex, dec, kind in members]
    return Case(name, dtype_id, P, A, q, np.zeros(m), cones, np.ones(n), np.ones(m), 1.0, ms, **kw)


def _cone_case(name, dtype_id, mode, cones, specs, **kw):
    """specs: (name, v, inside, deciding, kind) with v the vector whose in_dual decides: primal mode dy = v, dual mode u = -v (in_pol_recc(u) = in_dual(-u))"""
    if mode == "primal":
        return _primal_structure(name, dtype_id, cones, [(nm, v, PRIMAL if ins else UNDETERMINED, dec, kind) for nm, v, ins, dec, kind in specs], **kw)
    return _dual_structure(name, dtype_id, cones, [(nm, -np.asarray(v), DUAL if ins else UNDETERMINED, dec, kind) for nm, v, ins, dec, kind in specs], **kw)


def _tol(mode):
    return EPS_PRIM_INF if mode == "primal" else EPS_DUAL_INF


# ---- gates ----------------------------------------------------------------------------------------------------------------------------------------------
def _gates(dtype_id):
    """rows: 0 sets ||E dy|| (empty in A), 1 has the one entry of column 3, 2 has b = 1, 3 .. 5 Nonnegatives (4, 5 with entries in column 3);
    columns: 0 sets ||D dx||, 1 carries q, 2 carries P, 3 carries A"""
    epi, edi, c = EPS_PRIM_INF, EPS_DUAL_INF, 8.0
    D = np.array([2.0, 1.0, 4.0, 0.125])
    E = np.array([0.25, 2.0, 0.5, 8.0, 1.0, 4.0])
    A = sp.csc_matrix(([1.0, -1.0, -1.0], ([1, 4, 5], [3, 3, 3])), shape=(6, 4))
    P = sp.csc_matrix(([1.0], ([2], [2])), shape=(4, 4))
    q = np.array([0.0, -16.0, 0.0, 0.0])
    b = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    cones = [Cone(ZERO, 3), Cone(NONNEG, 3)]
    up = lambda x: _ulp(x, dtype_id, np.inf)
    dn = lambda x: _ulp(x, dtype_id, -np.inf)
    z4, z6 = np.zeros(4), np.zeros(6)

    def dyv(**kw):
        v = z6.copy()
        for k, x in kw.items():
            v[int(k[1:])] = x
        return v

    def dxv(**kw):
        v = z4.copy()
        for k, x in kw.items():
            v[int(k[1:])] = x
        return v

    ms = []
    # norm_dy > eps: dy = t e_0, E_0 t = eps
    for tag, t, ex in (("tie", 4 * epi, UNDETERMINED), ("above", up(4 * epi), PRIMAL), ("below", dn(4 * epi), UNDETERMINED)):
        ms.append(Member("norm_dy " + tag, z4, dyv(r0=t), ex, GATES[0], "tie"))
    # |Dinv A'dy| <= eps norm_dy: norm_dy = 1, Dinv_3 * 1 * t = 8 t = eps
    for tag, t, ex in (("tie", epi / 8, PRIMAL), ("above", up(epi / 8), UNDETERMINED), ("below", dn(epi / 8), PRIMAL)):
        ms.append(Member("A'dy " + tag, z4, dyv(r0=4.0, r1=t), ex, GATES[1], "tie"))
    # sF <= eps: sF = dy_2 b_2 / norm_dy = t
    for tag, t, ex in (("tie", epi, PRIMAL), ("above", up(epi), UNDETERMINED), ("below", dn(epi), PRIMAL)):
        ms.append(Member("sF " + tag, z4, dyv(r0=4.0, r2=t), ex, GATES[2], "tie"))
    # norm_dx > eps: dx = t e_1 with q_1 t / (D_1 t c) = -2
    for tag, t, ex in (("tie", edi, UNDETERMINED), ("above", up(edi), DUAL), ("below", dn(edi), UNDETERMINED)):
        ms.append(Member("norm_dx " + tag, dxv(c1=t), z6, ex, GATES[3], "tie"))
    # q'dx / (norm_dx c) < -eps: norm_dx = 1, -16 t / 8 = -eps
    for tag, t, ex in (("tie", edi / 2, UNDETERMINED), ("above", dn(edi / 2), UNDETERMINED), ("below", up(edi / 2), DUAL)):
        ms.append(Member("q'dx " + tag, dxv(c0=0.5, c1=t), z6, ex, GATES[4], "tie"))
    # |Dinv P dx| / (norm_dx c) <= eps: (t / 4) / 8 = eps
    for tag, t, ex in (("tie", 32 * edi, DUAL), ("above", up(32 * edi), UNDETERMINED), ("below", dn(32 * edi), DUAL)):
        ms.append(Member("P dx " + tag, dxv(c0=0.5, c1=0.25, c2=t), z6, ex, GATES[5], "tie"))
    ms.append(Member("both certificates hold", dxv(c0=0.5, c1=0.25), dyv(r0=4.0), PRIMAL, GATES[2], "decisive"))
    ms.append(Member("primal gates pass, cone fails, dual holds", dxv(c0=0.5, c1=0.25), dyv(r0=4.0, r3=-0.0625), DUAL, "cone 1 nonneg min x >= -tol", "decisive"))
    # the dual certificate's own cone test: column 3 reaches the ZeroSet row 1 with Einv_1 dx_3 / norm_dx = dx_3 / 2
    ms.append(Member("dual cone on tol", dxv(c0=0.5, c1=0.25, c3=2 * edi), z6, DUAL, "cone 0 zero max|x| <= tol", "tie"))
    ms.append(Member("dual cone one ulp above tol", dxv(c0=0.5, c1=0.25, c3=up(2 * edi)), z6, UNDETERMINED, "cone 0 zero max|x| <= tol", "tie"))
    for mb in ms:
        mb.dx, mb.dy = _rd(mb.dx, dtype_id), _rd(mb.dy, dtype_id)
    return Case("gates", dtype_id, P, A, q, b, cones, D, E, c, ms)


# ---- scaling ---------------------------------------------------------------------------------------------------------------------------------------------
def _scaling(dtype_id):
    """n = 40, m = 60.  A: one entry per row 0 .. 39 (row r, column r), rows 40 .. 59 empty; P: diagonal on columns 0 .. 19.  Every entry is a power of two
    chosen from D, E, c so that a unit step along one column passes the dual gates by a factor 2^4 and the cone test by 2^4, and every quantity is a single
    product: exact.  ZeroSet rows 0 .. 29, Nonnegatives rows 30 .. 59.  The exponents of D and E are random in -6 .. 6 and nonzero where a member needs
    the difference between a scaling and its inverse."""
    rng = np.random.default_rng(4060)
    n, m, c = 40, 60, 8.0
    epi, edi = EPS_PRIM_INF, EPS_DUAL_INF
    eD = rng.integers(-6, 7, n)
    eE = rng.integers(-6, 7, m)
    eD[[0, 1, 2, 3, 31]] = [3, 4, 2, 5, 2]
    eE[[0, 1, 31, 40, 41, 42]] = [3, 2, 4, 4, 3, 5]
    D, E = 2.0 ** eD, 2.0 ** eE
    a = np.where(np.arange(n) < 30, edi / 16, -1.0) * D * E[:n]                # adx_j = Einv_j a_j dx_j / (D_j dx_j): 2^-12 on ZeroSet rows, -1 on Nonnegatives
    A = sp.csc_matrix((a, (np.arange(n), np.arange(n))), shape=(m, n))
    p = (edi / 16) * D[:20] ** 2 * c                                          # Dinv_j p_j dx_j / (D_j dx_j c) = eps / 16 ...
    p[3] = (edi / 2) * D[3] ** 2 * c                                          # ... and eps / 2 on column 3
    P = sp.csc_matrix((p, (np.arange(20), np.arange(20))), shape=(n, n))
    q = -2.0 * D * c                                                          # q_j dx_j / (D_j dx_j c) = -2
    b = np.zeros(m)
    cones = [Cone(ZERO, 30), Cone(NONNEG, 30)]
    zx, zy = np.zeros(n), np.zeros(m)

    def vec(z, **kw):
        v = z.copy()
        for k, x in kw.items():
            v[int(k[1:])] = x
        return v

    ms = []
    M = lambda name, dx, dy, ex, dec, flips: ms.append(Member(name, dx, dy, ex, dec, "decisive", tuple(flips)))
    # E in ||E dy||: E_40 = 2^4, dy_40 = eps: 16 eps > eps, eps / 16 is not
    M("E in norm_dy", zx, vec(zy, r40=epi), PRIMAL, GATES[0], ["E"])
    # E in the normalisation of dy: a Nonnegatives row at -dy_r / norm_dy against -tol.  dy_41 = 1 / E_41 sets the norm with E, (1 / E_41) / E_41 with Einv
    M("E in dy / norm_dy", zx, vec(zy, r41=1.0 / E[41], r42=-epi / 2), PRIMAL, "cone 1 nonneg min x >= -tol", ["E"])
    # Einv in Einv A dx: row 31 (Nonnegatives), a_31 dx_31 / E_31 = -1 with Einv, -E_31^2 with E: both pass; row 0 (ZeroSet): 2^-12 with Einv, 2^-12 E_0^2 = 2^-6 with E
    M("Einv in A dx", vec(zx, c0=1.0 / D[0]), zy, DUAL, "cone 0 zero max|x| <= tol", ["E"])
    # D in ||D dx||: D_1 = 2^4: dx_1 = eps: 16 eps > eps, eps / 16 is not
    M("D in norm_dx", vec(zx, c1=edi), zy, DUAL, GATES[3], ["D"])
    # Dinv in Dinv A'dy: row 31 reaches column 31 with |a| = D E, D_31 = 4: Dinv |a| t = E t = eps / 2 passes, D |a| t = 16 E t does not
    M("Dinv in A'dy", zx, vec(zy, r40=1.0 / E[40], r31=epi / 2 / E[31]), PRIMAL, GATES[1], ["D"])
    # Dinv in Dinv P dx: column 3 (D_3 = 2^5) next to column 0 that sets the norm: p_3 t / 32 / 8 against eps
    M("Dinv in P dx", vec(zx, c0=1.0 / D[0], c3=128 * edi / p[3]), zy, DUAL, GATES[5], ["D"])
    # c in q'dx / (norm_dx c): q_j dx_j / D_j dx_j = -16 -> -2 ; a column with a smaller step: -4 eps / 8 is not below -eps, -4 eps and -32 eps are
    M("c in q'dx", vec(zx, c39=1.0 / D[39], c25=-(4 * edi - 16) / q[25]), zy, UNDETERMINED, GATES[4], ["c1", "cinv"])
    # c in |Dinv P dx| / (norm_dx c): column 3 alone: 4 eps / 8 passes, 4 eps and 32 eps do not
    M("c in P dx", vec(zx, c3=1.0 / D[3]), zy, DUAL, GATES[5], ["c1", "cinv"])
    # the two tolerances
    M("eps in norm_dy", zx, vec(zy, r40=2 * epi / E[40]), PRIMAL, GATES[0], ["eps"])
    M("eps in norm_dx", vec(zx, c39=2 * epi / D[39]), zy, UNDETERMINED, GATES[3], ["eps"])
    M("eps in the primal cone test", zx, vec(zy, r40=1.0 / E[40], r42=-2 * epi), UNDETERMINED, "cone 1 nonneg min x >= -tol", ["eps"])
    M("eps in the dual cone test", vec(zx, c39=1.0 / D[39], c38=-2 * epi / D[38]), zy, DUAL, "cone 1 nonneg max x <= tol", ["eps"])
    M("eps in |A'dy| <= eps norm_dy", zx, vec(zy, r40=1.0 / E[40], r31=2 * epi / E[31]), UNDETERMINED, GATES[1], ["eps"])
    M("eps in sF", zx, vec(zy, r40=1.0 / E[40]), PRIMAL, GATES[2], [])
    for mb in ms:
        mb.dx, mb.dy = _rd(mb.dx, dtype_id), _rd(mb.dy, dtype_id)
    b[43] = 1.0
    ms.append(Member("eps in sF <= eps", zx, _rd(vec(zy, r40=1.0 / E[40], r43=2 * epi), dtype_id), UNDETERMINED, GATES[2], "decisive", ("eps",)))
    return Case("scaling", dtype_id, P, A, q, b, cones, D, E, c, ms)


# ---- reductions ---------------------------------------------------------------------------------------------------------------------------------------
def _reductions(name, dtype_id, n, m, long_col, spots, **kw):
    """One nonzero per row of A: rows 0 .. long_col - 1 in column 0 (one long row of [P | A']), the others spread over columns 1 .. n - 1; every entry 2^-12
    except A[r, .] = 1 on the rows `hot`; P = 2^-12 I; q = -1 on every 64th column and on the last one; b = 1 on the rows `bs`; Nonnegatives only.
    spots: row positions (first, ..., last) at which a deciding entry is placed; hot / bs rows sit next to them."""
    epi, edi, c = EPS_PRIM_INF, EPS_DUAL_INF, 8.0
    rows = np.arange(m)
    cols = np.where(rows < long_col, 0, 1 + rows % (n - 1))
    vals = np.full(m, TINY)
    spots = sorted(set(int(s) for s in spots))
    hot = [s + 20 if s + 20 < m else s - 30 for s in spots]
    bs = [s + 10 if s + 10 < m else s - 15 for s in spots]
    anchor = max(m // 2, long_col) + 7                                        # sets ||E dy|| = 1 where a member needs it: b = 0, a tiny entry outside column 0
    assert not (set(hot) & set(bs)) and not (set(spots) & set(hot + bs)) and anchor not in spots + hot + bs
    vals[hot] = 1.0
    A = sp.csc_matrix((vals, (rows, cols)), shape=(m, n))
    P = sp.identity(n, format="csc") * TINY
    qcols = sorted(set(list(range(1, n, max(n // 9, 1)))[:8] + [n - 1]))      # nine columns across the workgroups that hold dx
    assert len(qcols) == 9
    q = np.zeros(n)
    q[qcols] = -1.0
    b = np.zeros(m)
    b[bs] = 1.0
    cones = [Cone(NONNEG, m)]
    zx, zy = np.zeros(n), np.zeros(m)

    def at(z, idx, val):
        v = z.copy()
        v[idx] = val
        return v

    ms = []
    for s in spots:
        ms.append(Member("norm_dy found at row %d" % s, zx, at(zy, s, 1.0), PRIMAL, GATES[0], "decisive"))
    for s, h_, b_ in zip(spots, hot, bs):
        ms.append(Member("violating row %d" % s, zx, at(at(zy, anchor, 1.0), s, -0.125), UNDETERMINED, "cone 0 nonneg min x >= -tol", "decisive"))
        ms.append(Member("<dy, b> term at row %d" % b_, zx, at(at(zy, anchor, 1.0), b_, 0.125), UNDETERMINED, GATES[2], "decisive"))
    # <dyn, b> over the partials: eight equal terms on the threshold, then one of them doubled
    tie = at(zy, anchor, 1.0)
    spread = bs + [x for x in np.linspace(3, m - 9, 8).astype(int).tolist() if x not in spots + hot + bs + [anchor]]
    spread = spread[:8]
    assert len(spread) == 8
    bb = b.copy()
    bb[spread] = 1.0
    b = bb
    tie[spread] = epi / 8
    over = tie.copy()
    over[spread[-1]] = epi / 4
    over2 = tie.copy()
    over2[spread[0]] = epi / 4
    ms.append(Member("<dy, b> sums to eps", zx, tie, PRIMAL, GATES[2], "tie"))
    ms.append(Member("<dy, b> one term more (last)", zx, over, UNDETERMINED, GATES[2], "decisive"))
    ms.append(Member("<dy, b> one term more (first)", zx, over2, UNDETERMINED, GATES[2], "decisive"))
    # the long row: A'dy at column 0 = 2^-12 sum dy_r: 2048 terms of 2^-9 sum to 4 -> on the threshold; one more term -> above
    if long_col >= 2049:
        lr = at(zy, anchor, 1.0)
        idx = [r for r in range(long_col - 1) if r not in hot + bs + spread][:2047]
        lr[idx] = 2.0 ** -9
        lr[long_col - 1] = 2.0 ** -9
        ms.append(Member("long row sums to eps", zx, lr.copy(), PRIMAL, GATES[1], "tie"))
        lr2 = lr.copy()
        lr2[long_col - 1] = 2.0 ** -8
        ms.append(Member("long row: last entry doubled", zx, lr2, UNDETERMINED, GATES[1], "decisive"))
        lr3 = lr.copy()
        lr3[idx[0]] = 2.0 ** -8
        ms.append(Member("long row: first entry doubled", zx, lr3, UNDETERMINED, GATES[1], "decisive"))
    # dual side
    cool = [j for j in range(n) if j not in set(cols[hot].tolist())]            # columns without a large entry
    for j in (cool[0], cool[len(cool) // 2], cool[-1]):
        dxj = at(zx, j, 1.0)
        if q[j] == 0:
            dxj[qcols[0]] = 0.5
        ms.append(Member("norm_dx found at column %d" % j, dxj, zy, DUAL, GATES[3], "decisive"))
    free = [j for j in range(1, n) if j not in qcols][0]                      # q = 0: sets ||D dx|| = 1
    tie = at(zx, free, 1.0)
    tie[qcols[:8]] = edi                                                      # -8 eps / 8: on the threshold, not below
    ms.append(Member("q'dx sums to -eps c", tie.copy(), zy, UNDETERMINED, GATES[4], "tie"))
    for tag, j in (("last", qcols[7]), ("first", qcols[0])):
        t2 = tie.copy()
        t2[j] = 2 * edi
        ms.append(Member("q'dx one term more (%s)" % tag, t2, zy, DUAL, GATES[4], "decisive"))
    base = at(zx, free, 1.0)
    base[qcols[8]] = 0.5
    for s, h_ in zip(spots, hot):                                             # A[h, col] = 1: adx_h = 0.125 > eps
        v = base.copy()
        v[cols[h_]] = 0.125 if cols[h_] != free else 1.0
        ms.append(Member("dual violation at row %d" % h_, v, zy, UNDETERMINED, "cone 0 nonneg max x <= tol", "decisive"))
    ms.append(Member("dual certificate holds", base, zy, DUAL, "cone 0 nonneg max x <= tol", "decisive"))
    for mb in ms:
        mb.dx, mb.dy = _rd(mb.dx, dtype_id), _rd(mb.dy, dtype_id)
    return Case(name, dtype_id, P, A, q, b, cones, np.ones(n), np.ones(m), c, ms, **kw)


# ---- simple cones ---------------------------------------------------------------------------------------------------------------------------------------
def _simple_cones():
    inf = np.inf
    return [Cone(NONNEG, 290), Cone(BOX, 6, l=np.array([-1.0, -4.0, -inf, -2.0, 1.0, -0.5]), u=np.array([2.0, 8.0, 3.0, inf, 1.0, 0.5])), Cone(ZERO, 3),
            Cone(NONNEG, 5), Cone(BOX, 2, l=np.array([-inf, 0.0]), u=np.array([inf, 0.0])), Cone(ZERO, 2), Cone(NONNEG, 4)]


def _simple(dtype_id, mode):
    cones = _simple_cones()
    off = np.concatenate([[0], np.cumsum([c.dim for c in cones])])
    m = int(off[-1])
    B0, Z0, N1, B1, Z1, N2 = (int(off[i]) for i in (1, 2, 3, 4, 5, 6))
    up = lambda x: _ulp(x, dtype_id, np.inf)
    dn = lambda x: _ulp(x, dtype_id, -np.inf)
    ms = []
    if mode == "primal":
        tol = EPS_PRIM_INF
        # y = -dy is what the Box support function sees.  This structure holds a (-Inf, Inf) row: whatever y it gets, its term is +-Inf or NaN, so the
        # members here are the four infinite outcomes; the finite sums are in simple_finite_primal.
        def y_base():
            y = np.zeros(m)
            y[off[0]:off[1]] = -0.25                           # Nonnegatives: -y = 0.25 >= -tol
            y[B0 + 2], y[B0 + 3], y[B0 + 4] = 2.0 ** -4, -2.0 ** -4, -0.5
            y[Z0:Z0 + 3] = [0.75, -0.75, 0.5]                  # ZeroSet rows: anything
            y[Z1:Z1 + 2] = [-0.875, 0.625]
            y[B1] = 2.0 ** -4                                  # (-Inf, Inf) row: picks u = Inf -> replaced per member
            return y

        def add(name, y, ex, dec, kind):
            ms.append((name, -y, ex, dec, kind))

        # with the (-Inf, Inf) row at y = 2^-4 the support function is +Inf: no certificate
        add("two-sided infinite row, y > tol: +Inf", y_base(), UNDETERMINED, GATES[2], "decisive")
        y = y_base(); y[B1] = -2.0 ** -4
        add("two-sided infinite row, y < 0: +Inf", y, UNDETERMINED, GATES[2], "decisive")
        y = y_base(); y[B1] = 0.0
        add("y = 0 on an infinite bound: NaN", y, UNDETERMINED, GATES[2], "decisive")
        y = y_base(); y[B1] = tol
        add("0 < y <= tol on l = -Inf picks l: -Inf", y, PRIMAL, GATES[2], "decisive")
        return _primal_structure("simple_primal", dtype_id, cones, ms)
    tol = EPS_DUAL_INF

    def u_base():
        u = np.zeros(m)
        u[off[0]:off[1]] = -0.25                               # Nonnegatives: u <= tol
        u[B0:B0 + 6] = [0.5, -0.5, 0.5, -0.5, 0.75, -0.75]     # finite bounds take anything; (-Inf, 3): u >= -tol; (-2, Inf): u <= tol
        u[N1:N1 + 5] = -0.5
        u[B1:B1 + 2] = [0.0, 0.875]
        u[N2:N2 + 4] = [-1.0, 0.0, tol, -tol]
        return u

    def add(name, u, ex, dec, kind):
        ms.append((name, u, ex, dec, kind))

    add("all rows inside", u_base(), DUAL, "cone 6 nonneg max x <= tol", "tie")
    for tag, idx in (("first", 0), ("last", m - 1), ("last of the long cone", 289)):
        u = u_base(); u[idx] = up(tol)
        add("Nonnegatives one ulp above tol, %s row" % tag, u, UNDETERMINED, "cone %d nonneg max x <= tol" % (0 if idx < 290 else 6), "tie")
    for tag, val, ex in (("tie", tol, DUAL), ("above", up(tol), UNDETERMINED), ("negative tie", -tol, DUAL), ("negative below", dn(-tol), UNDETERMINED)):
        u = u_base(); u[Z0 + 1] = val
        add("ZeroSet row %s" % tag, u, ex, "cone 2 zero max|x| <= tol", "tie")
    u = u_base(); u[Z1 + 1] = 0.5
    add("ZeroSet violation in the last ZeroSet", u, UNDETERMINED, "cone 5 zero max|x| <= tol", "decisive")
    for tag, idx, val, ex in (("u = Inf, x = tol", B0 + 3, tol, DUAL), ("u = Inf, x above tol", B0 + 3, up(tol), UNDETERMINED), ("l = -Inf, x = -tol", B0 + 2, -tol, DUAL),
                              ("l = -Inf, x below -tol", B0 + 2, dn(-tol), UNDETERMINED), ("both infinite, x > tol", B1, 0.5, UNDETERMINED),
                              ("both infinite, x < -tol", B1, -0.5, UNDETERMINED), ("both infinite, x = tol", B1, tol, DUAL)):
        u = u_base(); u[idx] = val
        add("Box " + tag, u, ex, "box recc", "tie" if abs(val) < 0.25 else "decisive")
    return _dual_structure("simple_dual", dtype_id, cones, ms)


def _simple_finite(dtype_id):
    """the Box support function on finite sums: no two-sided infinite row; rows (-1, 2), (-4, 8), (-Inf, 3), (-2, Inf), (1, 1), (-0.5, 0.5)"""
    inf = np.inf
    cones = [Cone(NONNEG, 290), Cone(BOX, 6, l=np.array([-1.0, -4.0, -inf, -2.0, 1.0, -0.5]), u=np.array([2.0, 8.0, 3.0, inf, 1.0, 0.5])), Cone(ZERO, 3),
             Cone(NONNEG, 5)]
    tol = EPS_PRIM_INF
    up = lambda x: _ulp(x, dtype_id, np.inf)
    dn = lambda x: _ulp(x, dtype_id, -np.inf)
    B0, Z0, N1, m = 290, 296, 299, 304
    ms = []

    def y_base(eq):
        y = np.zeros(m)
        y[:290] = -0.25
        y[B0 + 2], y[B0 + 3], y[B0 + 4] = 2.0 ** -4, -2.0 ** -4, eq          # 3 * 2^-4 + 2 * 2^-4 + eq = 0.3125 + eq
        y[Z0:Z0 + 3] = [0.75, -0.75, 0.5]
        y[N1:N1 + 5] = [-0.5, 0.0, tol, -0.125, -1.0]                        # -y >= -tol: the third row on the threshold
        return y

    def add(name, y, ex, dec, kind):
        ms.append((name, -y, ex, dec, kind))

    add("finite sum well below eps", y_base(-0.5), PRIMAL, GATES[2], "decisive")
    add("finite sum on eps", y_base(-(0.3125 - tol)), PRIMAL, GATES[2], "tie")
    add("finite sum one ulp above eps", y_base(up(-(0.3125 - tol))), UNDETERMINED, GATES[2], "tie")
    add("finite sum one ulp below eps", y_base(dn(-(0.3125 - tol))), PRIMAL, GATES[2], "tie")
    y = y_base(-0.3125); y[B0 + 1] = tol                                     # |y| <= tol, y > 0: picks l = -4: -4 tol; u = 8 would give 8 tol > eps
    add("0 < y = tol picks l", y, PRIMAL, "box |y| > tol picks u", "tie")
    y = y_base(-0.3125); y[B0 + 1] = up(tol)
    add("y one ulp above tol picks u", y, UNDETERMINED, "box |y| > tol picks u", "tie")
    y = y_base(-0.3125); y[B0 + 1] = -tol                                    # y < 0 picks l: (-tol)(-4) = 4 tol > eps
    add("y < 0 picks l", y, UNDETERMINED, GATES[2], "decisive")
    y = y_base(-0.5); y[B0 + 2] = -2.0 ** -4                                 # y < 0 on l = -Inf: +Inf
    add("y < 0 on l = -Inf: +Inf", y, UNDETERMINED, GATES[2], "decisive")
    y = y_base(-0.5); y[B0 + 3] = 2.0 ** -4                                  # y > tol on u = Inf: +Inf
    add("y > tol on u = Inf: +Inf", y, UNDETERMINED, GATES[2], "decisive")
    y = y_base(-0.5); y[B0 + 3] = 0.0                                        # 0 * -2 = 0 (finite l): fine; on (-Inf, 3): 0 * -Inf = NaN
    add("y = 0 on a finite lower bound", y, PRIMAL, GATES[2], "decisive")
    y = y_base(-0.5); y[B0 + 2] = 0.0
    add("y = 0 on l = -Inf: NaN", y, UNDETERMINED, GATES[2], "decisive")
    for tag, idx in (("first", 0), ("last", m - 1), ("last of the long cone", 289)):
        y = y_base(-0.5); y[idx] = up(tol)
        add("Nonnegatives one ulp below -tol, %s row" % tag, y, UNDETERMINED, "cone %d nonneg min x >= -tol" % (0 if idx < 290 else 3), "tie")
    return _primal_structure("simple_finite_primal", dtype_id, cones, ms)


# ---- second-order cones -----------------------------------------------------------------------------------------------------------------------------
def _square_pattern(L):
    """L nonzero small integers (alternating signs, the largest last) whose squares sum to N^2: exact in any order"""
    if L == 0:
        return np.zeros(0), 0
    if L == 1:
        return np.array([-3.0]), 3
    if L == 2:
        return np.array([3.0, -4.0]), 5
    N = math.isqrt(L) + 1
    while True:
        if N & (N - 1) == 0:                                   # not a power of two: |x[2:]| and |x[2:]| - tol stay in one binade
            N += 1
        extra = N * N - L
        for j in range(extra // 8 + 1):
            rest = extra - 8 * j
            if rest % 3 == 0 and rest // 3 + j <= L:
                i = rest // 3
                v = np.ones(L)
                v[L - j:] = 3.0
                v[L - j - i:L - j] = 2.0
                v[::2] *= -1.0
                assert float(np.sum(v * v)) == N * N
                return v, N
        N += 1


def _soc_vectors(d, tol, dtype_id):
    """(safe, tie, one ulp inside, one ulp outside) for in_dual: |x[2:]| <= tol + x[1], |x[2:]| = N 2^-k in [0.25, 0.5]"""
    v, N = _square_pattern(d - 1)
    k = (math.ceil(math.log2(N)) + 1) if N else 0
    v = v * 2.0 ** -k
    nx = N * 2.0 ** -k
    t = nx - tol
    mk = lambda x0: np.concatenate([[x0], v])
    return mk(0.75), mk(t), mk(_ulp(t, dtype_id, np.inf)), mk(_ulp(t, dtype_id, -np.inf))


SOC_DIMS = [1, 2, 3, 64, 65, 66, 129, 1000]


def _soc(dtype_id, mode):
    tol = _tol(mode)
    cones = [Cone(SOC, d) for d in SOC_DIMS]
    vecs = [_soc_vectors(d, tol, dtype_id) for d in SOC_DIMS]
    name = "soc |x[2:]| <= tol + x[1]"
    specs = [("all inside", np.concatenate([v[0] for v in vecs]), True, "cone 0 " + name, "decisive")]
    for i, d in enumerate(SOC_DIMS):
        for tag, which, ins in (("on the boundary", 1, True), ("one ulp inside", 2, True), ("one ulp outside", 3, False)):
            specs.append(("dim %d %s" % (d, tag), np.concatenate([v[which if j == i else 0] for j, v in enumerate(vecs)]), ins, "cone %d %s" % (i, name), "tie"))
    return _cone_case("soc_" + mode, dtype_id, mode, cones, specs)


def _soc_many(dtype_id, mode, dims, name, **kw):
    tol = _tol(mode)
    cones = [Cone(SOC, d) for d in dims]
    cache = {}
    for d in set(dims):
        cache[d] = _soc_vectors(d, tol, dtype_id)
    cname = "soc |x[2:]| <= tol + x[1]"
    safe = [cache[d][0] for d in dims]
    last, first = len(dims) - 1, 0

    def with_(i, which):
        parts = list(safe)
        parts[i] = cache[dims[i]][which]
        return np.concatenate(parts)

    specs = [("all inside", np.concatenate(safe), True, "cone 0 " + cname, "decisive"),
             ("last cone on the boundary", with_(last, 1), True, "cone %d %s" % (last, cname), "tie"),
             ("last cone one ulp outside", with_(last, 3), False, "cone %d %s" % (last, cname), "tie"),
             ("first cone one ulp outside", with_(first, 3), False, "cone %d %s" % (first, cname), "tie")]
    far = list(safe)
    far[last] = cache[dims[last]][0].copy()
    far[last][0] = -0.75
    specs.append(("last cone far outside", np.concatenate(far), False, "cone %d %s" % (last, cname), "decisive"))
    return _cone_case(name + "_" + mode, dtype_id, mode, cones, specs, **kw)


# ---- PSD cones ----------------------------------------------------------------------------------------------------------------------------------------
def _psd_vector(rng, cone, spectrum, tol, lean=False):
    """rows of a matrix whose in_dual verdict is known from its spectrum.  lean (Float32 with sides above 16): the bound 64 d eps32 ||X||_F leaves room for
    MARGIN only next to matrices of small norm, so every spectrum has one or two nonzero eigenvalues: below -4 tol, above -tol / 2, the filler +tol / 2
    (lambda_min = 0), indefinite -+0.45"""
    d = cone.side
    lam = np.zeros(d)
    if spectrum == "zero":
        return np.zeros(cone.dim)
    if lean == 2:                                              # sides 65 .. 130: a failing matrix has room only as lambda_min / tol grows: -0.9, alone
        lam[0] = {"below": -0.9, "above": -tol / 8, "safe": tol / 8, "indefinite": -0.9}[spectrum]
        if spectrum == "indefinite":
            lam[1] = tol / 8
    elif lean:
        lam[0] = {"below": -4.0 * tol, "above": -0.5 * tol, "safe": 0.5 * tol, "indefinite": -0.45}[spectrum]
        if spectrum == "indefinite":
            lam[1] = 0.45
    elif spectrum == "below":                                    # lambda_min = -tol - tol / 2
        lam[0] = -1.5 * tol
    elif spectrum == "above":                                  # lambda_min = -tol + tol / 2
        lam[0] = -0.5 * tol
    elif spectrum == "indefinite":
        lam = np.linspace(-0.45, 0.45, d) if d > 1 else np.array([-0.45])
    elif spectrum == "safe":
        lam = rng.uniform(0.25, 0.4, d)
    if spectrum in ("below", "above") and d > 1 and not lean:
        lam[1] = 0.5 * tol
    Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    X = (Q * lam) @ Q.T
    return psd_rows((X + X.T) / 2.0, cone)


def _psd_cone(side, kind):
    return Cone(kind, side * (side + 1) // 2 if kind == PSD_TRI else side * side)


def _psd(dtype_id, mode, name, shapes, **kw):
    tol = _tol(mode)
    rng = np.random.default_rng(sum(map(ord, name + mode)))
    cones = [_psd_cone(s, k) for s, k in shapes]
    side = max(s for s, _ in shapes)
    lean = (2 if side > 64 else 1 if side > 16 else 0) if dtype_id == "f32" else 0
    safe = [_psd_vector(rng, c, "safe", tol, lean) for c in cones]
    cname = "psd lambda_min > -tol"
    specs = [("all safe", np.concatenate(safe), True, "cone 0 " + cname, "decisive"),
             ("all zero", np.zeros(sum(c.dim for c in cones)), True, "cone 0 " + cname, "decisive")]
    for i, c in enumerate(cones):
        for spectrum, ins in (("above", True), ("below", False)):
            parts = list(safe)
            parts[i] = _psd_vector(rng, c, spectrum, tol, lean)
            specs.append(("cone %d (side %d) %s" % (i, c.side, spectrum), np.concatenate(parts), ins, "cone %d %s" % (i, cname), "decisive"))
    parts = list(safe)
    parts[-1] = _psd_vector(rng, cones[-1], "indefinite", tol, lean)
    specs.append(("last cone indefinite", np.concatenate(parts), False, "cone %d %s" % (len(cones) - 1, cname), "decisive"))
    return _cone_case(name + "_" + mode, dtype_id, mode, cones, specs, **kw)


def _psd_side1(dtype_id, mode):
    tol = _tol(mode)
    cones = [Cone(PSD_TRI, 1), Cone(PSD_SQ, 1), Cone(PSD_TRI, 6), Cone(PSD_SQ, 1)]
    rng = np.random.default_rng(11)
    mid = _psd_vector(rng, cones[2], "safe", tol)
    specs = [("all safe", np.concatenate([[0.5], [0.25], mid, [0.125]]), True, "cone 0 psd 1x1 x > -tol", "decisive")]
    for i, at in ((0, 0), (1, 1), (3, 8)):
        for tag, val, ins in (("on -tol", -tol, False), ("one ulp above -tol", _ulp(-tol, dtype_id, np.inf), True), ("one ulp below -tol", _ulp(-tol, dtype_id, -np.inf), False)):
            v = np.concatenate([[0.5], [0.25], mid, [0.125]])
            v[at] = val
            specs.append(("cone %d %s" % (i, tag), v, ins, "cone %d psd 1x1 x > -tol" % i, "tie"))
    return _cone_case("psd_side1_" + mode, dtype_id, mode, cones, specs)


def _psd_unsym(dtype_id, mode):
    """square blocks whose lower triangle disagrees with the upper one: is_pos_def! factors Hermitian(X) = the upper triangle"""
    cones = [Cone(PSD_SQ, 4), Cone(PSD_SQ, 9)]
    s = 2.0 ** -4
    a = np.array([1.0, -10.0, 0.0, 1.0]) * s                                  # [[1, 0], [-10, 1]]: upper triangle I, symmetrised lambda_min = -4
    bmat = np.array([[1.0, 0.0, 0.0], [-10.0, 1.0, 0.0], [-10.0, -10.0, 1.0]]) * s
    bad = np.array([1.0, 0.0, -10.0, 1.0]) * s                                # [[1, -10], [0, 1]]: the upper triangle holds the -10: fails
    cname = "psd lambda_min > -tol"
    specs = [("lower triangles ignored", np.concatenate([a, bmat.reshape(-1, order="F")]), True, "cone 0 " + cname, "decisive"),
             ("the upper triangle decides", np.concatenate([bad, bmat.reshape(-1, order="F")]), False, "cone 0 " + cname, "decisive"),
             ("transposed 3 x 3 fails", np.concatenate([a, bmat.T.reshape(-1, order="F")]), False, "cone 1 " + cname, "decisive")]
    return _cone_case("psd_unsym_" + mode, dtype_id, mode, cones, specs)


# ---- 3-d cones ----------------------------------------------------------------------------------------------------------------------------------------
CONE3_NC = 300
CONE3_SINGLE = 24            # violating points that get a member of their own (the ones closest to their threshold, and the last positions)


def _cone3_points(kind, tol, dtype_id):
    """300 points in [-25, 25]^3 2^-5 as cone3_inputs samples them, ten of them replaced by the closure branches of the kind's in_dual"""
    X = cone3_inputs(np.random.default_rng(7100 + 10 * CONE3.index(kind)), CONE3_NC) * 2.0 ** -5
    up = _ulp(tol, dtype_id, np.inf)
    if kind == EXP:                                            # |x| <= tol && y >= -tol && z >= -tol
        X[70:80] = [[0.0, 0.5, 0.5], [tol, 0.5, 0.0], [-tol, -tol, -tol], [up, 0.5, 0.5], [tol, -tol, 0.25], [tol, -up, 0.25], [0.0, 0.0, 0.0], [tol, 0.25, -up],
                    [2 * tol, 0.5, 0.5], [tol, 0.0, -tol]]
    elif kind == DUAL_EXP:                                     # x <= tol && y == 0 && z >= -tol
        X[70:80] = [[0.0, 0.0, 0.5], [tol, 0.0, 0.0], [up, 0.0, 0.5], [-0.5, 0.0, -tol], [-0.5, 0.0, -up], [tol, 0.0, -tol], [0.0, 0.0, 0.0], [-0.75, 0.0, 0.25],
                    [0.5, 0.0, 0.5], [2 * tol, 0.0, 0.0]]
    elif kind == POW:                                          # s >= -tol && t >= -tol, negative bases give NaN
        X[70:80] = [[0.0, 0.0, 0.0], [-tol, 0.5, 0.0], [0.5, -tol, 0.0], [-up, 0.5, 0.0], [0.0, 0.5, tol], [0.0, 0.5, 2 * tol * 4], [0.5, 0.0, tol], [0.5, 0.5, 0.0],
                    [0.0, 0.0, tol], [0.0, 0.0, up * 4]]
    else:                                                      # x >= 0 && y >= 0
        X[70:80] = [[0.0, 0.0, 0.0], [0.0, 0.5, tol], [0.0, 0.5, up], [0.5, 0.0, -tol], [-tol, 0.5, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, tol], [0.0, 0.0, -up],
                    [0.25, 0.25, 0.25], [0.25, 0.25, 0.5]]
    return _rd(X, dtype_id)


def _cone3(dtype_id, mode, kind):
    tol = _tol(mode)
    dtype = DTYPES[dtype_id]
    eps = EPS if dtype_id == "f64" else EPS32
    alphas = _rd(0.1 + 0.85 * np.random.default_rng(600).random(CONE3_NC), dtype_id) if kind in (POW, DUAL_POW) else np.zeros(CONE3_NC)
    cones = [Cone(kind, 3, alpha=float(alphas[i])) for i in range(CONE3_NC)]
    X = _cone3_points(kind, tol, dtype_id)
    inside, ratio = np.zeros(CONE3_NC, dtype=bool), np.full(CONE3_NC, np.inf)
    for i in range(CONE3_NC):
        tr = _Trace()
        inside[i] = _cone3_in_dual(tr, kind, X[i], cones[i].alpha, tol, eps, "")
        ratio[i] = min([ck.ratio for ck in tr.checks] or [np.inf])
    keep = ratio >= MARGIN
    ins_idx = np.flatnonzero(keep & inside)
    out_idx = np.flatnonzero(keep & ~inside)
    assert ins_idx.size and out_idx.size, (kind, mode, dtype_id)
    safe = {EXP: [-0.5, 0.5, 0.5], DUAL_EXP: [-0.5, 0.5, 0.5], POW: [0.5, 0.5, 0.0], DUAL_POW: [0.5, 0.5, 0.0]}[kind]      # inside for every alpha, by far
    base = np.tile(np.array(safe), (CONE3_NC, 1))
    base[ins_idx] = X[ins_idx]                                              # every kept inside point at its own position
    cname = " exp " if kind in (EXP, DUAL_EXP) else " pow "
    specs = [("every kept inside point", base.reshape(-1), True, cname, "decisive")]
    order = out_idx[np.argsort(ratio[out_idx], kind="stable")]
    single = list(order[:CONE3_SINGLE - 4]) + [j for j in out_idx[-4:] if j not in order[:CONE3_SINGLE - 4]]
    for j in single:
        v = base.copy()
        v[j] = X[j]
        specs.append(("outside point at cone %d" % j, v.reshape(-1), False, cname, "decisive"))
    v = base.copy()
    v[out_idx] = X[out_idx]
    specs.append(("every kept outside point", v.reshape(-1), False, cname, "decisive"))
    case = _cone_case("cone3_%s_%s" % (kind, mode), dtype_id, mode, cones, specs)
    case.dropped = (CONE3_NC, int((~keep).sum()), int(ins_idx.size), int(out_idx.size))
    return case


# ---- poison -------------------------------------------------------------------------------------------------------------------------------------------
def _poison(dtype_id):
    """n = 2, A with one tiny entry, q = (-1, 0): dy = (v, 1) is a primal certificate when the cones accept v, dx = (1, 0) a dual one (A dx = 0)"""
    cones = [Cone(ZERO, 2), Cone(NONNEG, 3), Cone(SOC, 3), Cone(ZERO, 1)]
    m = 9
    A = sp.csc_matrix(([TINY], ([m - 1], [1])), shape=(m, 2))
    P = sp.identity(2, format="csc") * TINY
    q = np.array([-1.0, 0.0])
    good_y = np.array([0.5, -0.5, 0.25, 0.0, 0.5, 0.75, 0.25, -0.25, 1.0])
    bad_y = good_y.copy()
    bad_y[3] = -0.5
    good_x, zx, zy = np.array([1.0, 0.0]), np.zeros(2), np.zeros(m)
    nan, inf = np.nan, np.inf

    def put(v, i, val):
        w = v.copy()
        w[i] = val
        return w

    ms = [Member("clean primal", zx, good_y, PRIMAL, GATES[2], "decisive"),
          Member("clean dual", good_x, zy, DUAL, GATES[5], "decisive"),
          Member("NaN in dy, dual holds", good_x, put(good_y, 2, nan), DUAL, GATES[0], "decisive", poisoned=True),
          Member("clean both", good_x, good_y, PRIMAL, GATES[2], "decisive"),
          Member("NaN in dy alone", zx, put(good_y, 6, nan), UNDETERMINED, GATES[0], "decisive", poisoned=True),
          Member("clean, cone fails, dual holds", good_x, bad_y, DUAL, "cone 1 nonneg min x >= -tol", "decisive"),
          Member("NaN in dx alone", put(good_x, 0, nan), zy, UNDETERMINED, GATES[3], "decisive", poisoned=True),
          Member("NaN in dx, primal holds", put(good_x, 1, nan), good_y, PRIMAL, GATES[2], "decisive", poisoned=True),
          Member("NaN in dx and dy", put(good_x, 1, nan), put(good_y, 0, nan), UNDETERMINED, GATES[3], "decisive", poisoned=True),
          Member("clean none", zx, bad_y, UNDETERMINED, GATES[3], "decisive"),
          Member("+Inf in dy, dual holds", good_x, put(good_y, 4, inf), DUAL, GATES[2], "decisive", poisoned=True),
          Member("-Inf in dy alone", zx, put(good_y, 0, -inf), UNDETERMINED, GATES[2], "decisive", poisoned=True),
          Member("+Inf in dx", put(good_x, 0, inf), zy, UNDETERMINED, GATES[4], "decisive", poisoned=True),
          Member("-Inf in dx, primal holds", put(good_x, 1, -inf), good_y, PRIMAL, GATES[2], "decisive", poisoned=True),
          Member("clean primal again", zx, put(good_y, 0, -0.75), PRIMAL, GATES[2], "decisive")]
    clean = [i for i, mb in enumerate(ms) if not mb.poisoned]
    return Case("poison", dtype_id, P, A, q, np.zeros(m), cones, np.ones(2), np.ones(m), 1.0, ms, clean=clean)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------
def _both(fn, *a, **kw):
    return {"primal": lambda d: fn(d, "primal", *a, **kw), "dual": lambda d: fn(d, "dual", *a, **kw)}


T, S = PSD_TRI, PSD_SQ
_BUILDERS = {"gates": _gates, "scaling": _scaling,
             "reductions_300": lambda d: _reductions("reductions_300", d, 40, 260, 30, [0, 255, 256, 259]),
             "reductions_big": lambda d: _reductions("reductions_big", d, 600, COSMO_BS * COSMO_MAX_PARTIALS + 1000 - 600, 3000,
                                                     [0, COSMO_BS * COSMO_MAX_PARTIALS + 12, COSMO_BS * COSMO_MAX_PARTIALS + 1000 - 600 - 1], batch=False),
             "reductions_batch": lambda d: _reductions("reductions_batch", d, 600, 4000, 3000, [0, 255, 256, 3999], handle=False),
             "simple_finite_primal": _simple_finite, "poison": _poison}
for _mode in ("primal", "dual"):
    _BUILDERS["simple_" + _mode] = functools.partial(lambda d, mode: _simple(d, mode), mode=_mode)
    _BUILDERS["soc_" + _mode] = functools.partial(lambda d, mode: _soc(d, mode), mode=_mode)
    _BUILDERS["soc70_" + _mode] = functools.partial(lambda d, mode: _soc_many(d, mode, ([1, 2, 3, 5, 2, 1, 9] * 10)[:69] + [66], "soc70"), mode=_mode)
    _BUILDERS["soc16400_" + _mode] = functools.partial(lambda d, mode: _soc_many(d, mode, [1, 2] * 8200, "soc16400", batch=False), mode=_mode)
    _BUILDERS["psd_small9_" + _mode] = functools.partial(lambda d, mode: _psd(d, mode, "psd_small9", [(2, T), (3, S), (16, T), (2, S), (3, T), (16, S), (2, T), (3, S), (16, T)]), mode=_mode)
    _BUILDERS["psd_mid3_" + _mode] = functools.partial(lambda d, mode: _psd(d, mode, "psd_mid3", [(17, T), (33, S), (64, T)]), mode=_mode)
    _BUILDERS["psd_side1_" + _mode] = functools.partial(lambda d, mode: _psd_side1(d, mode), mode=_mode)
    _BUILDERS["psd_large_" + _mode] = functools.partial(lambda d, mode: _psd(d, mode, "psd_large", [(65, T), (130, S)], batch=False), mode=_mode)
    _BUILDERS["psd_257_" + _mode] = functools.partial(lambda d, mode: _psd(d, mode, "psd_257", [(257, T)], batch=False), mode=_mode)
    _BUILDERS["psd_unsym_" + _mode] = functools.partial(lambda d, mode: _psd_unsym(d, mode), mode=_mode)
    for _kind in CONE3:
        _BUILDERS["cone3_%s_%s" % (_kind, _mode)] = functools.partial(lambda d, mode, kind: _cone3(d, mode, kind), mode=_mode, kind=_kind)
CASES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name, dtype_id="f64"):
    return _BUILDERS[name](dtype_id)


@functools.lru_cache(maxsize=None)
def verdict(name, dtype_id, k):
    """evaluate() of member k, once"""
    cs = case(name, dtype_id)
    mb = cs.members[k]
    return evaluate(cs, mb.dx, mb.dy)


def float32_runs(name):
    """does the Float32 library run the case?  Every case but side 257, where 64 d eps32 ||X||_F times MARGIN leaves no room for a failing matrix
    (test_float32_is_left_out_only_where_it_cannot_be_decisive).  Sides 17 .. 130 run in Float32 on matrices of small norm (_psd_vector, lean)."""
    return not name.startswith("psd_257")
