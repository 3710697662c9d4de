"""Structures, a high-precision reference, the bounds and the list of forms for ONE KKT solve at a time through the CG routes of a bare handle
(csrc/cg_fold.hip, csrc/cg_sr.hip and the unassembled recurrences; tests/test_gpu_krylov_forms.py).  Host only: this module does not import the
GPU library; tests/test_krylov_cases_host.py checks on the CPU everything that is claimed here.

The system.  rhs = [rhs_x; rhs_s], the reduced system is  M x = b,  M = P + sigma I + A' diag(rho) A,  b = rhs_x + A'(rho .* rhs_s),  and
nu = rho .* (A x - rhs_s)  (src/linear_solver/kktsolver_indirect.jl:50-88).  Every row of A is a Nonnegatives row, rho is handed over explicitly
(RHO, or RHO_EQ on the rows a case calls equalities), sigma = SIGMA, no scaling.

Reference.  M is accumulated entry by entry in np.longdouble from the sparse entries of P, A and rho (no dense A' rho A product), solved by
float64 np.linalg.solve and refined three times with the residual taken in longdouble; its own relative residual ||b - M x*|| / (||M|| ||x*|| + ||b||)
must stay <= 2^-55 (measured: 3e-20 .. 2e-19).  For the Float32 library the same reference is built from the Float32-rounded P, A, rho, sigma and rhs.

Floor and tolerance.  floor = eps(dtype) (||M||_2 ||x*||_2 + ||b||_2): what one rounding of M x - b costs.  Every case runs with ONE tol_constant T
and tol_exponent 0, so the stopping threshold of a solve is abstol = T / ||b||; T is the smallest value with abstol >= FLOOR_MARGIN (256) floors for
every right-hand side of the case (rhs1, rhs2 under rho; rhs1 under rho').  A threshold below the floor (the 1e-10 of the older tests on these
structures) makes the literal recurrences run to maxiter = n.

Residual bound.  ||b - M x_dev||_2, computed on the host in longdouble, must be <= abstol + C_DRIFT floor.  The recurrence residual that the stopping
rule sees drifts from the true one; the drift (true residual - threshold) / floor is measured with the oracle's cg_v09 / pcg_v09 run to stagnation
(threshold = floor / 1024, at most 4 n iterations) on every case, both rho vectors and right-hand sides, with the recurrences that run on the case:
    measured worst drift 0.23 .. 0.77 (ORACLE_WORST_DRIFT_BY_CASE),   C_DRIFT = max(16, 16 x worst) = 16
(tests/test_krylov_cases_host.py::test_the_drift_constant_is_the_measured_one measures it again and fails when it is exceeded).  The single-reduction
forms have no oracle restatement and use the same C_DRIFT.

nu.  |nu_i - rho_i ((A x_dev)_i - rhs_s_i)| <= gamma_{len_i + 2} rho_i (|A| |x_dev| + |rhs_s|)_i row by row, gamma_k as in tests/anderson_cases.py.

Krylov count.  |k_dev - k_oracle| <= 2 + 0.03 k_oracle (the allowance of tests/test_gpu_cg_sr.py), k_oracle from IndirectReducedKKT ("CG" or
"CG_JACOBI") with the same T, rho and warm starts.  The oracle stops below n in every (case, recurrence) pair that runs, except the one pair listed in
RUNS_TO_MAXITER: the literal recurrence on hub_2304 under rho' (P = 0: the diagonal of M is rho' alone, cond 1e5).  Where the oracle of a listed pair runs to n, the
device must run to n too and its true residual must stay <= 4 x the oracle's; the solves of the pair that do stop below n (rhs1, rhs2 under rho) keep every bound.

The library's rules restated (so that the host test can prove which path a case takes, and the GPU test can compare fold_stats()):
  split_ok      api.hip build_op_split: the operator is split when the single-nonzero rows hold at least half of nnz(A);
  fold_plan     cg_fold.hip fold_build: the cost gate sum len^2 <= 6 (2 nnz(Am) + nnz(P) + n), the rows kept factored, the stored pattern of
                [Ms | Ad' rho] and its tiles;
  row_blocks    api.hip build_row_blocks, for a given tile size.

Cases (the smallest shapes at which the edge still exists):
  one_tile       n = 40, tridiagonal P, A = [-I; 12 rows of 3 nonzeros]: one tile at every SL, one workgroup.
  one_tile_f     the same with 10 rows of 4 nonzeros: rows of 3 can never stay factored (2 (part + 2 dense) <= terms fails for len < 4), and 12 rows of 4
                 fail the split rule at n = 40; this is the one-tile case of the partially assembled forms.
  edge_257       n = 257 (one element past a workgroup), P zero on the last 100 columns, two empty rows of A, coupling rows of 2 .. 6 nonzeros, a
                 bound row on every column.  On the last 100 columns the diagonal of M is rho alone, so under rho' = 10^U(-3, 2) cond(M) = 1e5 and the
                 literal recurrence runs to n: this case is Jacobi only.
  edge_257_pd    the same with a diagonal of P on the last 100 columns: the case of the literal, single-reduction, partially assembled and unassembled forms.
  mixed_700      n = 700, sparse diagonally dominant P, A = [-I; 120 rows of 3 .. 12 nonzeros], 30 equality rows; more than 64 tiles at tile 256.
                 The row lengths lean to the short side: with the mean 7.5 of an even spread nnz(Am) = 900 > 700 and the split rule refuses the operator.
  hub_2304       n = 2304, P = 0, coupling row i < 576 holds the hub column and columns 4i .. 4i+3: row `hub` of M is full (2304 entries, longer than every
                 tile, SL = 8 included: the generic chunked path).  Bounds are [-I; +I]: with [-I] alone the split rule (4608 < 5183) refuses the operator.
                 24 equality rows: with 72 of them the Krylov count of the literal recurrence moves by 5 of the 5 allowed under another rounding alone.
  factored_long  n = 1200, banded P (half width 76, 175 k entries, what the gate needs), A = [-I; +I; one row of 1030 nonzeros; 150 rows of 4 .. 12
                 nonzeros in the first 200 columns]: one Ad tile longer than ADSL * 256 = 1024 (generic path of k_cg_updF*, an image of padding only) and
                 columns in more than two image slots (the overflow list sovf).  No equality rows: with 30 of them the residual of the literal recurrence
                 swings by a factor 5 around the threshold and the count moves by 6 of the 5 allowed under another rounding alone (ROUNDING_SEEDS below).
"""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
SIGMA = 1e-6
RHO, RHO_EQ = 0.1, 100.0
DTYPES = {"f64": np.float64, "f32": np.float32}
FLOOR_MARGIN = 256.0
REFINE_STEPS = 3
REFERENCE_RESIDUAL_LIMIT = 2.0 ** -55

BS, NNZ_PER_BLOCK, MAX_PARTIALS, ADSL = 256, 2048, 2048, 4            # csrc/internal.h, csrc/cg_fold.hip

# ---- the constant of the residual bound -----------------------------------------------------------------------------------------------------------
# worst (true residual - threshold) / floor of the oracle's recurrences at stagnation, per case, over both recurrences, both rho vectors and both
# right-hand sides (measured with measure_drift below)
# (rounded up to two decimals)
ORACLE_WORST_DRIFT_BY_CASE = {"one_tile": 0.66, "one_tile_f": 0.77, "edge_257": 0.47, "edge_257_pd": 0.27, "mixed_700": 0.42, "hub_2304": 0.23,
                              "factored_long": 0.62}      # C_DRIFT = max(16, 16 x 0.77 = 12.3) = 16
ORACLE_WORST_DRIFT = max(ORACLE_WORST_DRIFT_BY_CASE.values())
C_DRIFT = max(16.0, 16.0 * ORACLE_WORST_DRIFT)

# (case, oracle kind) pairs whose oracle runs to maxiter = n at the case's tolerance: they assert k_dev == n and a true residual <= 4 x the oracle's
RUNS_TO_MAXITER = (("hub_2304", "CG"),)
# oracle kinds that run on a case (edge_257: see the table of cases)
ORACLE_KINDS = {"edge_257": ("CG_JACOBI",)}


def oracle_kinds(name):
    return ORACLE_KINDS.get(name, ("CG", "CG_JACOBI"))
assert len(RUNS_TO_MAXITER) <= 1


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def gamma(k, dtype):
    """gamma_k with eps in place of the unit roundoff (tests/anderson_cases.py: gamma)"""
    e = eps_of(dtype)
    return k * e / (1.0 - k * e)


def krylov_allowance(k_oracle):
    return 2 + 0.03 * k_oracle


# ---- structures -----------------------------------------------------------------------------------------------------------------------------------
class Case:
    """P (n x n, full symmetric), A (m x n) as CSC with sorted indices and no stored zeros; eq marks the equality rows; rho / rho2 the two rho
    vectors (rho2 = 10^U(-3, 2), the update_rho step); rhs1 / rhs2 of length n + m."""

    def __init__(self, name, P, A, eq, seed):
        self.name = name
        self.P = sp.csc_matrix(P); self.P.eliminate_zeros(); self.P.sort_indices()
        self.A = sp.csc_matrix(A); self.A.eliminate_zeros(); self.A.sort_indices()
        self.m, self.n = self.A.shape
        self.eq = np.asarray(eq, dtype=bool)
        assert self.eq.shape == (self.m,) and abs(self.P - self.P.T).max() == 0
        rng = np.random.default_rng([seed, 77])
        self.rho = np.where(self.eq, RHO_EQ, RHO)
        self.rho2 = 10.0 ** rng.uniform(-3, 2, self.m)
        self.rhs1 = rng.standard_normal(self.n + self.m)
        self.rhs2 = rng.standard_normal(self.n + self.m)
        self.row_len = np.diff(self.A.tocsr().indptr)

    def rho_of(self, which):
        return self.rho if which == 1 else self.rho2


def _sym_dominant(rng, n, per_row, scale=0.2, cols=None):
    """sparse symmetric P with about `per_row` off-diagonal entries per row and a dominant diagonal; `cols`: only these rows / columns are nonzero"""
    k = n if cols is None else cols
    S = sp.random(k, k, density=min(1.0, per_row / (2.0 * k)), random_state=rng, format="csr", data_rvs=lambda c: scale * rng.standard_normal(c))
    S = sp.triu(S, 1)
    S = (S + S.T).tocsr()
    D = sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + rng.uniform(0.1, 1.0, k))
    Pk = (S + D).tocoo()
    return sp.csc_matrix((Pk.data, (Pk.row, Pk.col)), shape=(n, n))


def _rows(rng, n, lens, cols_of=None):
    """coupling rows: row i has lens[i] distinct columns (0: an empty row) with standard normal values"""
    r, c, v = [], [], []
    for i, ln in enumerate(lens):
        if ln == 0:
            continue
        pool = n if cols_of is None else cols_of
        cc = np.sort(rng.choice(pool, size=ln, replace=False))
        r += [i] * ln; c += list(cc); v += list(rng.standard_normal(ln))
    return sp.csc_matrix((v, (r, c)), shape=(len(lens), n))


def _one_tile(nrows, rowlen, seed):
    rng = np.random.default_rng(seed)
    n = 40
    off = -20.0 + 2.0 * rng.standard_normal(n - 1)                               # a diagonal that dominates rho' = 10^U(-3, 2): the literal recurrence stops below n = 40
    P = sp.diags([off, 100.0 + rng.uniform(0, 50, n), off], [-1, 0, 1], format="csc")
    G = _rows(rng, n, [rowlen] * nrows)
    eq = np.zeros(n + nrows, dtype=bool); eq[n:n + 3] = True
    return P, sp.vstack([-sp.eye(n), G], format="csc"), eq


def _edge_257(seed, tail_diagonal):
    rng = np.random.default_rng(seed)
    n = 257
    P = _sym_dominant(rng, n, 4, cols=157)                                     # zero on the last 100 columns (and rows)
    P = (P + sp.diags(np.concatenate([np.ones(157), tail_diagonal * rng.uniform(1.0, 2.0, 100)]))).tocsc()
    lens = [2 + (i % 5) for i in range(58)]
    lens.insert(7, 0); lens.insert(40, 0)                                        # two empty rows
    G = _rows(rng, n, lens).tolil()
    G[0, 256] = 1.5; G[59, 256] = -0.75; G[59, 0] = 0.5                          # the element past the workgroup is coupled (rows stay within 2 .. 6)
    G = sp.csc_matrix(G)
    eq = np.zeros(n + len(lens), dtype=bool); eq[n + 10:n + 20] = True
    return P, sp.vstack([-sp.eye(n), G], format="csc"), eq


MIXED_LENS = [3, 3, 4, 3, 5, 3, 6, 4, 7, 3, 8, 4, 3, 5, 9, 3, 4, 10, 3, 11, 3, 4, 12, 5] * 5       # 120 rows, 625 nonzeros


def _mixed_700(seed):
    rng = np.random.default_rng(seed)
    n = 700
    P = _sym_dominant(rng, n, 56, scale=0.03)
    G = _rows(rng, n, MIXED_LENS)
    eq = np.zeros(n + len(MIXED_LENS), dtype=bool); eq[n:n + 120:4] = True       # 30 equality rows
    return P, sp.vstack([-sp.eye(n), G], format="csc"), eq


HUB = 1000


def _hub_2304(seed):
    rng = np.random.default_rng(seed)
    n = 2304
    r, c, v = [], [], []
    for i in range(576):
        cc = sorted(set([HUB, 4 * i, 4 * i + 1, 4 * i + 2, 4 * i + 3]))
        r += [i] * len(cc); c += cc; v += list(rng.uniform(0.5, 1.5, len(cc)) * rng.choice([-1.0, 1.0], len(cc)))
    G = sp.csc_matrix((v, (r, c)), shape=(576, n))
    eq = np.zeros(2 * n + 576, dtype=bool); eq[2 * n:2 * n + 576:24] = True
    return sp.csc_matrix((n, n)), sp.vstack([-sp.eye(n), sp.eye(n), G], format="csc"), eq


LONG_ROW, FACTORED_HALF_WIDTH = 1030, 76


def _factored_long(seed):
    rng = np.random.default_rng(seed)
    n = 1200
    w = FACTORED_HALF_WIDTH
    offs = list(range(1, w + 1))
    bands = [0.01 * rng.standard_normal(n - d) for d in offs]
    S = sp.diags(bands + bands, offs + [-d for d in offs], shape=(n, n), format="csr")
    P = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + rng.uniform(0.5, 1.5, n))).tocsc()
    long_row = _rows(rng, n, [LONG_ROW])
    long_row.data *= 0.05
    G = _rows(rng, n, [4 + (i % 9) for i in range(150)], cols_of=200)
    A = sp.vstack([-sp.eye(n), sp.eye(n), long_row, G], format="csc")
    eq = np.zeros(A.shape[0], dtype=bool)
    return P, A, eq


_BUILDERS = {
    "one_tile": lambda: _one_tile(12, 3, 11),
    "one_tile_f": lambda: _one_tile(10, 4, 12),
    "edge_257": lambda: _edge_257(13, 0.0),
    "edge_257_pd": lambda: _edge_257(13, 1.0),
    "mixed_700": lambda: _mixed_700(14),
    "hub_2304": lambda: _hub_2304(15),
    "factored_long": lambda: _factored_long(16),
}
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    P, A, eq = _BUILDERS[name]()
    return Case(name, P, A, eq, CASES.index(name))


# ---- reference --------------------------------------------------------------------------------------------------------------------------------------
class Reference:
    """M of one (case, rho, dtype) in longdouble, and the refined dense solve.  dtype float32: P, A, rho, sigma are rounded to Float32 first (the
    numbers the Float32 library holds); right-hand sides are rounded by the caller."""

    def __init__(self, cs, which, dtype=np.float64):
        self.case, self.dtype = cs, np.dtype(dtype)
        n = cs.n
        self.rho = cs.rho_of(which).astype(dtype).astype(LD)
        self.sigma = LD(np.asarray(SIGMA, dtype=dtype))
        Pc = cs.P.tocoo()
        self.p_row, self.p_col, self.p_val = Pc.row, Pc.col, Pc.data.astype(dtype).astype(LD)
        Ar = cs.A.tocsr(); Ar.sort_indices()
        self.a_ptr, self.a_col, self.a_val = Ar.indptr, Ar.indices, Ar.data.astype(dtype).astype(LD)
        self.a_row = np.repeat(np.arange(cs.m), np.diff(Ar.indptr))
        M = np.zeros((n, n), dtype=LD)
        np.add.at(M, (self.p_row, self.p_col), self.p_val)
        M[np.arange(n), np.arange(n)] += self.sigma
        single = np.flatnonzero(cs.row_len == 1)
        j = self.a_col[self.a_ptr[single]]
        np.add.at(M, (j, j), self.rho[single] * self.a_val[self.a_ptr[single]] ** 2)
        for i in np.flatnonzero(cs.row_len >= 2):
            idx = self.a_col[self.a_ptr[i]:self.a_ptr[i + 1]]
            v = self.a_val[self.a_ptr[i]:self.a_ptr[i + 1]]
            M[np.ix_(idx, idx)] += self.rho[i] * np.outer(v, v)
        self.M = M
        self.M64 = M.astype(np.float64)
        self.norm2 = float(spla.eigsh(sp.csr_matrix(self.M64), k=1, which="LA", v0=np.ones(n), return_eigenvectors=False)[0]) if n > 2 else float(np.linalg.norm(self.M64, 2))

    def mulA(self, x):
        y = np.zeros(self.case.m, dtype=LD)
        np.add.at(y, self.a_row, self.a_val * np.asarray(x, dtype=LD)[self.a_col])
        return y

    def absA(self, x):
        y = np.zeros(self.case.m, dtype=LD)
        np.add.at(y, self.a_row, np.abs(self.a_val) * np.abs(np.asarray(x, dtype=LD))[self.a_col])
        return y

    def reduced_rhs(self, rhs):
        rhs = np.asarray(rhs, dtype=self.dtype).astype(LD)
        n = self.case.n
        b = rhs[:n].copy()
        np.add.at(b, self.a_col, self.a_val * (self.rho * rhs[n:])[self.a_row])
        return b

    def residual(self, x, b):
        """||b - M x||_2 in longdouble"""
        return float(np.linalg.norm(b - self.M @ np.asarray(x, dtype=LD)))

    def solve(self, b):
        x = np.linalg.solve(self.M64, b.astype(np.float64)).astype(LD)
        for _ in range(REFINE_STEPS):
            x = x + np.linalg.solve(self.M64, (b - self.M @ x).astype(np.float64)).astype(LD)
        return x

    def floor(self, b, xstar):
        return eps_of(self.dtype) * (self.norm2 * float(np.linalg.norm(xstar)) + float(np.linalg.norm(b)))

    def nu_violations(self, sol, rhs):
        """rows where nu misses its bound: (row, |error|, bound)"""
        n = self.case.n
        rhs = np.asarray(rhs, dtype=self.dtype).astype(LD)
        x, nu = np.asarray(sol[:n], dtype=LD), np.asarray(sol[n:], dtype=LD)
        err = np.abs(nu - self.rho * (self.mulA(x) - rhs[n:]))
        g = np.array([gamma(int(k) + 2, self.dtype) for k in self.case.row_len], dtype=LD)
        bound = g * self.rho * (self.absA(x) + np.abs(rhs[n:]))
        bad = np.flatnonzero(~(err <= bound))
        return [(int(i), float(err[i]), float(bound[i])) for i in bad[:5]]


class Solve:
    """one right-hand side of the sequence: the reduced b, x*, the floor, and (once T is known) abstol and the residual limit"""

    def __init__(self, ref, rhs):
        self.ref = ref
        self.rhs = np.asarray(rhs, dtype=ref.dtype)
        self.b = ref.reduced_rhs(self.rhs)
        self.bnorm = float(np.linalg.norm(self.b))
        self.xstar = ref.solve(self.b)
        self.floor = ref.floor(self.b, self.xstar)
        self.own_residual = ref.residual(self.xstar, self.b) / (ref.norm2 * float(np.linalg.norm(self.xstar)) + self.bnorm)


class Plan:
    """the three solves of a case in one dtype, its T, and per solve abstol = T / ||b|| and limit = abstol + C_DRIFT floor"""

    def __init__(self, name, dtype):
        cs = case(name)
        self.case, self.dtype = cs, np.dtype(dtype)
        self.ref1, self.ref2 = Reference(cs, 1, dtype), Reference(cs, 2, dtype)
        self.solves = [Solve(self.ref1, cs.rhs1), Solve(self.ref1, cs.rhs2), Solve(self.ref2, cs.rhs1)]
        self.T = max(FLOOR_MARGIN * s.floor * s.bnorm for s in self.solves)
        for s in self.solves:
            s.abstol = self.T / s.bnorm
            s.limit = s.abstol + C_DRIFT * s.floor


@functools.lru_cache(maxsize=None)
def plan(name, dtype_name="f64"):
    return Plan(name, DTYPES[dtype_name])


# ---- the oracle's sequence ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_sequence(name, kind, dtype_name="f64", rounding=None):
    """IndirectReducedKKT through the steps of the GPU test with the plan's T: [(solution, Krylov count)] for rhs1, rhs2 under rho and rhs1, rhs1 under
    rho'.  It runs in the plan's dtype: the Krylov count of a Float32 recurrence at a threshold 256 Float32 floors up is not that of the Float64 recurrence
    (mixed_700: 37 / 41 / 69 in Float32 arithmetic, 34 / 36 / 54 in Float64 -- rounding delays convergence), and the Float32 library is a Float32 recurrence.
    rounding = seed: every operator product is perturbed componentwise by (1 + u N(0, 1)), u = eps / 2 -- another rounding of the same recurrence, as
    a kernel that sums in another order is (the host test asks that the Krylov counts of a case do not depend on it beyond the allowance)."""
    from oracle import cosmo_oracle as O
    pl = plan(name, dtype_name)
    cs, dt = pl.case, pl.dtype
    kk = O.IndirectReducedKKT(O.Operators(sp.csc_matrix(cs.P.astype(dt)), sp.csc_matrix(cs.A.astype(dt))), cs.n, cs.m, float(np.asarray(SIGMA, dtype=dt)),
                              cs.rho.astype(dt), kind, tol_constant=pl.T, tol_exponent=0.0)
    kk.previous_solution = np.zeros(cs.n, dtype=dt)
    if rounding is not None:
        rng, exact_mul = np.random.default_rng([int(rounding), 991]), kk.reduced_mul
        kk.reduced_mul = lambda x: (exact_mul(x) * (1.0 + 0.5 * eps_of(dt) * rng.standard_normal(cs.n))).astype(dt)
    out = []
    for step, rhs in enumerate((cs.rhs1, cs.rhs2, cs.rhs1, cs.rhs1)):
        if step == 2:
            kk.update_rho(cs.rho2.astype(dt))
        sol = kk.solve(rhs.astype(dt))
        assert sol.dtype == dt
        out.append((sol, kk.last_iters))
    return out


def verify(name, dtype_name, oracle_kind, results, label=""):
    """The bounds of one sequence [(solution, Krylov count)] x 4 (rhs1, rhs2 under rho; rhs1, rhs1 again under rho'): prints every figure, then returns
    the list of violations (empty: the sequence is inside every bound)."""
    pl = plan(name, dtype_name)
    cs, n = pl.case, pl.case.n
    seq = oracle_sequence(name, oracle_kind, dtype_name)
    solves = [pl.solves[0], pl.solves[1], pl.solves[2], pl.solves[2]]
    oracle_res = [s.ref.residual(o[0][:n], s.b) for o, s in zip(seq, solves)]
    to_maxiter = (name, oracle_kind) in RUNS_TO_MAXITER
    bad = []
    for step, ((sol, k), s) in enumerate(zip(results, solves)):
        k_or = seq[step][1]
        if not np.isfinite(np.asarray(sol, dtype=np.float64)).all():
            bad.append((step, "not finite"))
            continue
        res = s.ref.residual(sol[:n], s.b)
        print("%s %s %s step %d: k = %d (oracle %d), residual %.3e = abstol %+.2f floors (limit +%.0f; oracle %+.2f), floor %.3e"
              % (name, dtype_name, label, step + 1, k, k_or, res, (res - s.abstol) / s.floor, C_DRIFT, (oracle_res[step] - s.abstol) / s.floor, s.floor))
        if to_maxiter and step >= 2 and seq[2][1] >= n:
            # the listed pair: the oracle ran out of iterations in step 3, so did the device, and it got as far; step 4 restarts from there
            if step == 2 and k != n:
                bad.append((step, "k = %d, the oracle ran to n = %d" % (k, n)))
            lim = 4.0 * oracle_res[2] if step == 2 else max(s.limit, 4.0 * oracle_res[2])
            if not res <= lim:
                bad.append((step, "residual %.3e > %.3e" % (res, lim)))
        else:
            if not res <= s.limit:
                bad.append((step, "residual %.3e > abstol + C floor = %.3e" % (res, s.limit)))
            if step < 3 and not abs(k - k_or) <= krylov_allowance(k_or):
                bad.append((step, "k = %d, oracle %d" % (k, k_or)))
            if step == 3 and not k <= 1:
                bad.append((step, "the same right-hand side again took k = %d" % k))
        nv = s.ref.nu_violations(sol, s.rhs)
        if nv:
            bad.append((step, "nu rows (row, |error|, bound): %s" % (nv,)))
    return bad


ROUNDING_SEEDS = range(8)


def count_spread(name, kind, dtype_name="f64"):
    """(oracle counts, per step the largest change of the count over ROUNDING_SEEDS other roundings of the oracle's sequence, per step the largest count)"""
    base = [k for _, k in oracle_sequence(name, kind, dtype_name)]
    other = [[k for _, k in oracle_sequence(name, kind, dtype_name, seed)] for seed in ROUNDING_SEEDS]
    return base, [max(abs(o[i] - base[i]) for o in other) for i in range(4)], [max(o[i] for o in other) for i in range(4)]


def measure_drift(name):
    """worst (true residual - threshold) / floor of cg_v09 and pcg_v09 run to stagnation: threshold = floor / 1024, at most 4 n iterations, from x = 0"""
    from oracle import cosmo_oracle as O
    pl = plan(name)
    cs = pl.case
    worst = -np.inf
    for s in pl.solves:
        ref = s.ref
        kk = O.IndirectReducedKKT(O.Operators(cs.P, cs.A), cs.n, cs.m, SIGMA, ref.rho.astype(np.float64))
        kk.multiplications.append(0)
        b = s.b.astype(np.float64)
        thr = s.floor / 1024.0
        for kind in oracle_kinds(name):
            x = np.zeros(cs.n)
            if kind == "CG":
                O.cg_v09(x, kk.reduced_mul, b, thr, 4 * cs.n)
            else:
                O.pcg_v09(x, kk.reduced_mul, b, 1.0 / kk.operator_diagonal(), thr, 4 * cs.n)
            worst = max(worst, (ref.residual(x, s.b) - thr) / s.floor)
    return worst


# ---- the library's rules, restated ---------------------------------------------------------------------------------------------------------------------
def row_blocks(rowptr, tile_override):
    """api.hip build_row_blocks: the row boundaries of the CSR-stream tiles"""
    nrows = len(rowptr) - 1
    nnz = int(rowptr[-1]) if nrows > 0 else 0
    tile = NNZ_PER_BLOCK
    if nnz < 512 * NNZ_PER_BLOCK:
        tile = max(256, ((nnz // 512 + 63) // 64) * 64)
    if nnz <= 256 * 768:
        tile = 256
    if tile_override > 0:
        tile = min(tile_override, NNZ_PER_BLOCK)
    rows_max = BS if tile < NNZ_PER_BLOCK else 4 * BS
    rb, r = [0], 0
    while r < nrows:
        r1, cnt = r, 0
        while r1 < nrows:
            rn = int(rowptr[r1 + 1] - rowptr[r1])
            if r1 > r and (cnt + rn > tile or r1 - r >= rows_max):
                break
            cnt += rn
            r1 += 1
            if cnt > tile:
                break
        rb.append(r1)
        r = r1
    return rb


def split_ok(cs):
    """api.hip build_op_split: the single-nonzero rows hold at least half of the nonzeros of A"""
    return 2 * int((cs.row_len == 1).sum()) >= int(cs.A.nnz)


def slots_of(tile):
    return 8 if tile == 0 else 1 if tile <= BS else 2 if tile <= 2 * BS else 3 if tile <= 3 * BS else 4 if tile <= 4 * BS else 8


def fold_plan(cs, tile=None, factor_min=0):
    """cg_fold.hip fold_build: dict(enabled, gate = (terms, limit), factored_rows, stored_entries, tiles, slots, longest_row, tile_fill = nonzeros of
    the fullest tile, ad_tiles, ad_longest_tile, max_slots_per_column = occurrences of the busiest column in the factored rows).  tile None: the default
    rule (768, or the size heuristic above 700 * 2048 entries); factor_min > 0: COSMO_HIP_FOLD_FACTOR=1 with that row-length threshold."""
    n = cs.n
    Ar = cs.A.tocsr()
    multi = np.flatnonzero(cs.row_len >= 2)
    lens = cs.row_len[multi].astype(np.int64)
    nterms = int((lens * lens).sum())
    streamed = 2 * int(lens.sum()) + int(cs.P.nnz) + n
    out = dict(enabled=0, gate=(nterms, 6 * streamed), factored_rows=0)
    if not split_ok(cs) or nterms > 6 * streamed or nterms > (1 << 24):
        return out
    dense = np.zeros(len(multi), dtype=bool)
    if factor_min > 0:
        cand = lens >= factor_min
        part, dense_nnz = int((lens[~cand] ** 2).sum()), int(lens[cand].sum())
        if dense_nnz > 0 and 2 * (part + 2 * dense_nnz) <= nterms:
            dense = cand
    pat = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    Anf, Ad = pat(Ar[multi[~dense]]), pat(Ar[multi[dense]])
    S = pat(cs.P.tocsr()) + sp.eye(n, format="csr") + (Anf.T @ Anf).tocsr()
    S.eliminate_zeros()
    per_col = np.asarray(Ad.sum(axis=0)).ravel().astype(np.int64) if Ad.shape[0] else np.zeros(n, dtype=np.int64)
    row_nnz = np.diff(S.indptr) + per_col
    rowptr = np.concatenate([[0], np.cumsum(row_nnz)])
    if tile is None:
        tile = 0 if int(rowptr[-1]) > 700 * MAX_PARTIALS else 768
    rb = row_blocks(rowptr, tile)
    fills = [int(rowptr[rb[k + 1]] - rowptr[rb[k]]) for k in range(len(rb) - 1)]
    out.update(enabled=1, factored_rows=int(dense.sum()), stored_entries=int(rowptr[-1]), tiles=len(rb) - 1, slots=slots_of(tile),
               longest_row=int(row_nnz.max()), tile_fill=max(fills), ad_tiles=0, ad_longest_tile=0, max_slots_per_column=int(per_col.max()))
    if dense.any():
        adptr = np.concatenate([[0], np.cumsum(lens[dense])])
        rbd = row_blocks(adptr, ADSL * BS)
        out.update(ad_tiles=len(rbd) - 1, ad_longest_tile=max(int(adptr[rbd[k + 1]] - adptr[rbd[k]]) for k in range(len(rbd) - 1)))
    return out


# ---- forms ------------------------------------------------------------------------------------------------------------------------------------------
TILES = {1: 256, 2: 512, 3: 768, 4: 1024, 8: 2048}                       # SL -> COSMO_HIP_FOLD_TILE
SWITCHES = ("COSMO_HIP_OP_SPLIT", "COSMO_HIP_OP_FOLD", "COSMO_HIP_CG_FUSE_DIR", "COSMO_HIP_CG_PERSIST", "COSMO_HIP_FOLD_FACTOR", "COSMO_HIP_FOLD_FACTOR_MIN",
            "COSMO_HIP_FOLD_FACTOR_FILL", "COSMO_HIP_FOLD_PRESCATTER", "COSMO_HIP_FOLD_TILE", "COSMO_HIP_FOLD_PAD", "COSMO_HIP_CG_SR_DEFAULT", "COSMO_HIP_GRID_CAP",
            "COSMO_HIP_XCD_AFFINE", "COSMO_HIP_CG_GRAPH", "COSMO_HIP_CG_GRAPH_LEN")
# recurrence -> (kkt_kind name, oracle kind, switches, route string with %d = SL, factored)
ASSEMBLED = {
    "literal": ("CG", "CG", {},"cg: literal recurrence on the assembled operator, two launches per iteration, k_cg_dirM<%d, false> + k_cg_upd<false>", False),
    "jacobi": ("CG_JACOBI", "CG_JACOBI", {}, "cg: Jacobi-preconditioned recurrence on the assembled operator (opt-in), k_cg_dirM<%d, true> + k_cg_upd<true>", False),
    "sr": ("CG_SR", "CG", {}, "cg: one-launch single-reduction recurrence on the assembled operator (opt-in kkt_kind CG_SR), k_sr_M<%d>", False),
    # k_cg_dirMs<SL, 2> + k_cg_updF<2>
    "partial_ps2": ("CG", "CG", {"COSMO_HIP_FOLD_FACTOR": "1"}, "two launches per iteration, k_cg_dirM<%d, false> + k_cg_updF", True),
    # k_cg_dirMs<SL, 1> + k_cg_updF<1>
    "partial_ps1": ("CG", "CG", {"COSMO_HIP_FOLD_FACTOR": "1", "COSMO_HIP_FOLD_PRESCATTER": "2"},
                    "k_cg_dirM<%d, false> + k_cg_updF (dense-row image without pre-scattered operands, COSMO_HIP_FOLD_PRESCATTER=2)", True),
    # k_cg_dirM<SL, false> + k_cg_updF0
    "partial_csr": ("CG", "CG", {"COSMO_HIP_FOLD_FACTOR": "1", "COSMO_HIP_FOLD_PRESCATTER": "0"},
                    "k_cg_dirM<%d, false> + k_cg_updF (CSR-stream dense rows k_cg_updF0, COSMO_HIP_FOLD_PRESCATTER=0)", True),
}
FULL = ("literal", "jacobi", "sr")
PARTIAL = ("partial_ps2", "partial_ps1", "partial_csr")
ALL_SL = (1, 2, 3, 4, 8)
# (case, recurrence, SL): the full cross product on one_tile (one_tile_f for the partially assembled forms) and mixed_700, the others where their edge is
ASSEMBLED_RUNS = (
    [("one_tile", r, sl) for r in FULL for sl in ALL_SL] + [("one_tile_f", r, sl) for r in PARTIAL for sl in ALL_SL]
    + [("mixed_700", r, sl) for r in FULL + PARTIAL for sl in ALL_SL]
    + [("edge_257", "jacobi", sl) for sl in (1, 3, 8)] + [("edge_257_pd", r, sl) for r in ("literal", "sr") + PARTIAL for sl in (1, 3)]
    + [("hub_2304", r, sl) for r in FULL for sl in (1, 3, 8)]
    + [("factored_long", r, sl) for r in PARTIAL for sl in (3, 8)])
F32_RUNS = [(c, "literal", sl) for c in ("one_tile", "mixed_700") for sl in (1, 3, 8)]
# the unassembled routes: name -> (kkt_kind name, oracle kind, switches, route string)
UNASSEMBLED = {
    "fused": ("CG", "CG", {"COSMO_HIP_OP_FOLD": "0"}, "cg: literal recurrence, three launches per iteration, k_cg_dirA + k_op_apply + k_cg_upd<false>"),
    "plain": ("CG", "CG", {"COSMO_HIP_CG_FUSE_DIR": "0"}, "cg: literal recurrence, four launches per iteration, k_cg_dir + k_spmv_A_rho + k_op_apply + k_cg_upd<false>"),
    "persist": ("CG", "CG", {"COSMO_HIP_CG_PERSIST": "1"}, "cg: literal recurrence in one persistent launch (csrc/cg_persist.hip, opt-in)"),
    "sr_two_launch": ("CG_SR", "CG", {"COSMO_HIP_OP_FOLD": "0"}, "cg: single-reduction recurrence, two launches per iteration (kkt_kind CG_SR), k_sr_update_A + k_sr_op"),
}
UNASSEMBLED_CASES = ("one_tile", "edge_257_pd", "mixed_700")
GRID_CAP = 64


def factor_min_of(recurrence):
    return 4 if recurrence in PARTIAL else 0
