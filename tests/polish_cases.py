"""Inputs and the numpy restatement of the batch polish (tests/test_polish_cases_host.py, tests/test_gpu_polish.py; no GPU needed here).

FIXTURE: strictly complementary QPs with a KNOWN solution (x*, y*, s*).  Per member P = G'G / n + I with G 30 % dense, A 40 % dense normal, x* normal; every
Nonnegatives row is active with probability 1/2 (s = 0, y in [0.5, 1.5]) or has s in [0.5, 1.5] and y = 0; every Box row (l = -1, u = 1) is at l with y in
[0.5, 1.5], at u with y in [-1.5, -0.5] or interior with s in [-0.5, 0.5], a third each; Zero rows carry a normal y.  b = A x* + s*, q = -P x* - A' y*, so
(x*, y*, s*) satisfies the KKT conditions exactly up to the rounding of these two products, and the gap of 0.5 between "active" and "inactive" is what an
ADMM solution at eps = 1e-3 still resolves.  A BATCH is a list of members on ONE shared sparsity pattern, the union of theirs, stored with explicit zeros.

RESTATEMENT: the active-set rule, the system, the regularised factor with refinement and the candidate of csrc/batch_polish.h in dense numpy, in any
float type (`polish_dense`).  It is the yardstick of the GPU tests: what the kernel computes with a sparse factor in another elimination order."""
import functools

import numpy as np
import scipy.sparse as sp

COSMO_INFTY = 1e20
BIG = 1e16                       # COSMO_INFTY * MIN_SCALING: a bound beyond it is never active
SHAPE = dict(n=30, mz=4, mn=16, mb=12)          # the fixture of the issue: m = 32
SMALL = dict(n=8, mz=1, mn=3, mb=2, density_A=1.0)      # the smallest fixture: m = 6 (A dense, so that no active row of A is empty)
SEEDS = tuple(range(8))


def member(seed, n=30, mz=4, mn=16, mb=12, p_active=0.5, box="mixed", u_inf=False, density_A=0.4):
    """One QP with its solution.  p_active: probability of an active Nonnegatives row; box: "mixed" (a third each), "interior" or "bounds" (lower /
    upper alternately drawn); u_inf: the upper bounds are +COSMO_INFTY (rows then sit at l or inside)."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.3)
    P = G.T @ G / n + np.eye(n)
    m = mz + mn + mb
    A = rng.standard_normal((m, n)) * (rng.random((m, n)) < density_A)
    xs = rng.standard_normal(n)
    s = np.zeros(m); y = np.zeros(m); act = np.zeros(m, bool)
    act[:mz] = True; y[:mz] = rng.standard_normal(mz)
    for i in range(mz, mz + mn):
        if rng.random() < p_active:
            act[i] = True; y[i] = rng.uniform(0.5, 1.5)
        else:
            s[i] = rng.uniform(0.5, 1.5)
    l = -np.ones(mb); u = np.full(mb, COSMO_INFTY) if u_inf else np.ones(mb)
    for j in range(mb):
        i = mz + mn + j; t = int(rng.integers(3))
        if box == "interior":
            t = 2
        elif box == "bounds":
            t = t % 2
        if u_inf and t == 1:
            t = 0
        if t == 0:
            act[i] = True; s[i] = l[j]; y[i] = rng.uniform(0.5, 1.5)
        elif t == 1:
            act[i] = True; s[i] = u[j]; y[i] = -rng.uniform(0.5, 1.5)
        else:
            s[i] = rng.uniform(-0.5, 0.5)
    b = A @ xs + s; q = -P @ xs - A.T @ y
    lo = np.concatenate([np.zeros(mz), np.zeros(mn), l]); hi = np.concatenate([np.zeros(mz), np.full(mn, np.inf), u])
    return dict(P=P, q=q, A=A, b=b, x=xs, s=s, y=y, act=act, lo=lo, hi=hi, l=l, u=u, n=n, m=m, mz=mz, mn=mn, mb=mb)


def on_union_pattern(members):
    """The members' P and A as CSC matrices on ONE pattern, the union of theirs (a member's missing entries are stored zeros)."""
    pp = np.zeros_like(members[0]["P"], dtype=bool); pa = np.zeros_like(members[0]["A"], dtype=bool)
    for c in members:
        pp |= c["P"] != 0; pa |= c["A"] != 0
    out = []
    for c in members:
        d = dict(c)
        for name, pat in (("P", pp), ("A", pa)):
            r, col = np.nonzero(pat)
            M = sp.csc_matrix((c[name][r, col], (r, col)), shape=pat.shape)
            M.sort_indices()
            assert M.nnz == int(pat.sum())                      # (explicit zeros survive)
            d[name + "_csc"] = M
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def batch(seeds=SEEDS, **shape):
    """The members `seeds` of one shape on their union pattern (cached: treat as read-only)."""
    kw = dict(SHAPE); kw.update(shape)
    return on_union_pattern([member(s, **kw) for s in seeds])


def cone_sets(c, mod):
    """The cones of a member from module `mod`: cosmo_jl_amd (ZeroSet, ...) or the oracle (Cone, Box)."""
    sets = []
    if hasattr(mod, "ZeroSet"):
        if c["mz"]: sets.append(mod.ZeroSet(c["mz"]))
        if c["mn"]: sets.append(mod.Nonnegatives(c["mn"]))
        if c["mb"]: sets.append(mod.Box(c["l"], c["u"]))
    else:
        if c["mz"]: sets.append(mod.Cone(mod.ZERO, c["mz"]))
        if c["mn"]: sets.append(mod.Cone(mod.NONNEG, c["mn"], constr_type=np.zeros(c["mn"], bool)))
        if c["mb"]: sets.append(mod.Box(c["l"].copy(), c["u"].copy()))
    return sets


def active_set(s, y, lo, hi, mz, big=BIG):
    """The rule of csrc/batch_polish.h on iterates (s, y) with row bounds lo / hi (Zero rows first): (lower, upper) boolean masks."""
    with np.errstate(invalid="ignore"):
        dl = s - lo; du = hi - s
        low = (np.abs(lo) < big) & (dl < y); upp = (np.abs(hi) < big) & (du < -y)
    both = low & upp
    upp = upp & ~(both & (dl <= du)); low = low & ~(both & (dl > du))
    low[:mz] = True; upp[:mz] = False
    return low, upp


def kkt_matrix(P, A, act):
    M = act.astype(P.dtype)[:, None] * A
    return np.block([[P, M.T], [M, -np.diag((1.0 - act).astype(P.dtype))]])


def polish_dense(P, q, A, b, s, y, lo, hi, mz, delta=1e-6, refine_iter=3, dtype=np.float64, big=BIG):
    """The polish in dense numpy of type `dtype`: returns dict(x, y, s, act, low, upp, cond)."""
    f = lambda v: np.asarray(v, dtype=dtype)
    P, q, A, b, s, y = f(P), f(q), f(A), f(b), f(s), f(y)
    lo_f = f(np.clip(lo, -3e38, 3e38)); hi_f = f(np.clip(hi, -3e38, 3e38))
    m, n = A.shape
    low, upp = active_set(s, y, lo_f, hi_f, mz, big)
    act = low | upp
    zero = np.zeros(m, dtype=dtype)
    sfix = np.where(low, lo_f, np.where(upp, hi_f, zero)); sfix[:mz] = 0
    K = kkt_matrix(P, A, act)
    Kt = K + np.diag(np.concatenate([np.full(n, delta), -delta * act])).astype(dtype)
    rhs = np.concatenate([-q, np.where(act, b - sfix, zero)]).astype(dtype)
    t = np.linalg.solve(Kt, rhs).astype(dtype)
    for _ in range(refine_iter):
        t = (t + np.linalg.solve(Kt, (rhs - K @ t).astype(dtype)).astype(dtype)).astype(dtype)
    xp = t[:n]
    yp = np.where(act, t[n:], zero)
    yp[mz:] = np.where(low[mz:], np.maximum(yp[mz:], 0), np.where(upp[mz:], np.minimum(yp[mz:], 0), zero[mz:]))
    s2 = np.where(act, sfix, np.clip(b - A @ xp, lo_f, hi_f)).astype(dtype)
    return dict(x=xp, y=yp, s=s2, act=act, low=low, upp=upp, cond=float(np.linalg.cond(K.astype(np.float64))))


def polish_unpivoted(c, delta, refine_iter, dtype, rows_first):
    """x of the polish on the CONSTRUCTED active set with an unpivoted dense LDL' in `dtype`, eliminating the x block first or the rows first -- the two
    extremes of what an ordering can do to the factor the kernel builds (it never pivots).  Returns max |x - x*|.  This is the restatement that chose the
    float32 default of delta: with the rows first a pivot -delta puts entries of size |A|^2 / delta into the x block, and delta = 1e-6 loses every digit
    of a float32 factor, while a large delta slows the refinement down; 1e-4 .. 1e-3 reach the float32 floor in both orders."""
    f = lambda v: np.asarray(v, dtype=dtype)
    P, q, A, b = f(c["P"]), f(c["q"]), f(c["A"]), f(c["b"])
    m, n = A.shape
    act = c["act"]
    K = kkt_matrix(P, A, act)
    Kt = (K + np.diag(np.concatenate([np.full(n, delta), -delta * act]))).astype(dtype)
    rhs = np.concatenate([-q, np.where(act, b - f(c["s"]), 0)]).astype(dtype)
    perm = np.concatenate([np.arange(n, n + m), np.arange(n)]) if rows_first else np.arange(n + m)
    W = Kt[np.ix_(perm, perm)].copy(); N = n + m
    L = np.eye(N, dtype=dtype); d = np.zeros(N, dtype=dtype)
    for j in range(N):
        d[j] = W[j, j]
        L[j + 1:, j] = W[j + 1:, j] / d[j]
        W[j + 1:, j + 1:] = (W[j + 1:, j + 1:] - np.outer(L[j + 1:, j], L[j + 1:, j]) * d[j]).astype(dtype)

    def solve(r):
        y = r[perm].astype(dtype).copy()
        for j in range(N):
            y[j + 1:] = (y[j + 1:] - L[j + 1:, j] * y[j]).astype(dtype)
        y = (y / d).astype(dtype)
        for j in range(N - 1, -1, -1):
            y[j] = y[j] - np.dot(L[j + 1:, j], y[j + 1:])
        out = np.zeros(N, dtype=dtype); out[perm] = y
        return out
    t = solve(rhs)
    for _ in range(refine_iter):
        t = (t + solve((rhs - K @ t).astype(dtype))).astype(dtype)
    return float(np.max(np.abs(t[:n].astype(np.float64) - c["x"])))


def residuals(c, x, y, s):
    """r_prim = ||A x + s - b||_inf, r_dual = ||P x + q + A' y||_inf in float64."""
    return (float(np.max(np.abs(c["A"] @ x + s - c["b"]), initial=0.0)), float(np.max(np.abs(c["P"] @ x + c["q"] + c["A"].T @ y), initial=0.0)))


def errors(c, x, y, s):
    """max |x - x*|, |y - y*|, |s - s*| and the bound scale max(1, ||.*||_inf) of each."""
    return [(float(np.max(np.abs(np.asarray(v, dtype=np.float64) - c[k]))), max(1.0, float(np.max(np.abs(c[k]))))) for k, v in (("x", x), ("y", y), ("s", s))]


def models(members, settings, cj, dtype=np.float64):
    """One cosmo_jl_amd Model per member (shared pattern when the members come from `batch`), all with the ONE Settings object."""
    out = []
    for c in members:
        md = cj.Model(dtype=dtype) if dtype != np.float64 else cj.Model()
        md.set(c.get("P_csc", sp.csc_matrix(c["P"])), c["q"], c.get("A_csc", sp.csc_matrix(c["A"])), c["b"], cone_sets(c, cj), settings)
        out.append(md)
    return out


# ---- the edge members of tests/test_gpu_polish.py (every one inside the caps the host test checks: rule exact, restatement <= 1e-13, cond <= 1e3) ----
def no_inequality_active(seed=0):
    return on_union_pattern([member(seed, p_active=0.0, box="interior")])


def every_row_active(seed=0):
    return on_union_pattern([member(seed, n=30, mz=4, mn=8, mb=6, p_active=1.0, box="bounds")])       # 18 active rows <= n


def upper_bounds_infinite(seed=0):
    return on_union_pattern([member(seed, u_inf=True)])


def single_row(seed=0):
    return on_union_pattern([member(seed, n=5, mz=0, mn=1, mb=0, p_active=1.0, density_A=1.0)])


def infeasible(seed=3):
    """A fixture member made primal infeasible: Zero rows 0 and 1 get equal rows of A and different b."""
    c = dict(member(seed))
    A = c["A"].copy(); b = c["b"].copy()
    A[1] = A[0]; b[1] = b[0] + 1.0
    c["A"], c["b"] = A, b
    return c


def duplicated_active_row(seed=0):
    """A fixture member whose first ACTIVE Nonnegatives row appears twice (the copy replaces an inactive Nonnegatives row and shares the multiplier):
    A restricted to the active rows is rank deficient; the solution x*, s* stays, y* is no longer unique."""
    c = dict(member(seed))
    mz, mn = c["mz"], c["mn"]
    ia = next(i for i in range(mz, mz + mn) if c["act"][i]); ii = next(i for i in range(mz, mz + mn) if not c["act"][i])
    A = c["A"].copy(); b = c["b"].copy(); s = c["s"].copy(); y = c["y"].copy(); act = c["act"].copy()
    A[ii] = A[ia]; s[ii] = 0.0; b[ii] = b[ia]; y[ii] = y[ia] = 0.5 * c["y"][ia]; act[ii] = True
    c.update(A=A, b=b, s=s, y=y, act=act)
    assert np.allclose(-c["P"] @ c["x"] - A.T @ y, c["q"])
    return c
