"""Problems and an exact reference for the residuals, the termination decisions and the rho rule (csrc/kernels.hip: k_chk_prim / k_chk_dual / k_chk_final /
k_rho_apply; csrc/batch.hip: the `residuals` lambdas of batch_admm_body and of the register kernels and the code around them).  No test functions, no GPU
code, nothing from the oracle: imported by test_residual_cases_host.py (CPU), test_gpu_residual_checks.py and test_gpu_batch_residual_checks.py (GPU).

The reference restates src/residuals.jl:1-96,143-147 and src/parameters.jl:17-92 on the EXACT values of the Float32 / Float64 inputs: every input is a dyadic
rational, so every sum and product is computed on Python integers with one common power of two (_ints) and returned as a fractions.Fraction; the square
root of the rho rule is taken by mpmath at 200 bits.  Nothing is rounded before the end.

Rounding bounds (gamma_k = k u / (1 - k u), u the unit roundoff of the type; no tuned constants):

  row i of the primal side   gamma_{len_i + 2 + e}  (sum_j |a_ij x_j| + |s_i| + |b_i|) Einv_i          len_i products and len_i - 1 additions in any order,
                                                                                                      + s, - b, and e = 1 rounding for Einv when it is applied
  row j of the dual side     gamma_{len_j + 4 + d}  (sum |p_jk x_k| + sum |a_ij mu_i| + |q_j|) Dinv_j cinv    len_j = entries of row j of [P | A']; mu_i = rho_i (w_prev_i
                                                                                                      - s_i) is recovered in the type: 2 roundings; + q, - A'mu; d = 2 for Dinv, cinv
  an inf-norm                the maximum of its rows' bounds (|max f - max g| <= max |f - g|); the bound of a max-norm is the same number: each of its
                             three terms is a partial expression of the residual's row
  cost                       gamma_{n + maxlen_P + 2} cinv (1/2 sum_j |x_j| sum_k |p_jk x_k| + sum |q_j x_j|)    a row of P (len), the product with x_j (1), n - 1 additions in any
                                                                                                      order (workgroup partials included), the sum of the two dots (1), cinv (1);
                                                                                                      the factor 1/2 is exact
  new rho                    the rule evaluated on the corners of the four intervals, times (1 +- gamma_8) for its own eight operations (rule)

The sums of absolute values inside the bounds are evaluated in long double; their own relative error of 1e-15 is not carried.  Against the formulas
the issue sketches: its dual row is "the primal one with two more roundings for Dinv and cinv", gamma_{len + 5}.  Counted operation by operation
the dual row has len (products and additions of P x and A'mu), + q, - A'mu, Dinv, cinv: len + 4; here two more are added, len + 6, because the
reference recomputes mu exactly from the fetched w_prev, s and rho, so the two roundings of the device's own mu_i = rho_i (w_prev_i - s_i) are part
of the error it is compared with.  The issue's cost bound is gamma_{n + len}; counted, the product with x_j, the sum of the two dots and cinv are
three roundings beyond the row (len) and the n - 1 additions: gamma_{n + len + 2}.

A PROBLEM is given in the working space of the loop (what Julia's setup! hands over): P, q, A, b, Zero / Nonnegatives / Box rows so that the three rho
classes occur, Dinv and Einv random over four decades, cinv = 37.5, and iterates x0, s0, mu0.  `place = (term, position)` makes one of the six terms
(Ax, s, b; Px, q, ATmu) the strict arg-max of its unscaled max-norm at a chosen row: first, last, tile_end (the last row of the first CSR-stream tile),
idx512 (an index >= 512: the second register slot of the batch register kernels) or long (the long row / column).  P and A are never touched for it:
an entry of s, b or q is raised, or the iterate is scaled and the row's own weight Einv_i / Dinv_i is raised.  (Scaling a row or a column of A by the
factor a placement needs, up to 1e7, takes the reduced KKT matrix P + sigma I + A' rho A from a condition number of a few thousand to 1e16, and
conjugate gradients in Float32 on such a matrix return NaN; the problems are meant to test the checks, not the solver.)  A placement holds at the iterates set_iterates loads -- where cosmo_hip_residuals
reads them; after an iteration the loop's own iterates decide.

Shapes (csrc/api.hip: build_row_blocks -- operators of at most 256 * 768 nonzeros are cut into tiles of 256 nonzeros and at most 256 rows, so every shape
here is cut that way; upload_csr: grid = min(tiles, COSMO_HIP_GRID_CAP); device_utils.h: csr_stream_rows_g takes the chunked path above 2048 nonzeros):

  tiny          n = 7, m = 5: one tile, one workgroup, most lanes idle
  one_tile      n = 40, m = 60, P diagonal, fewer than 256 nonzeros in A and in [P | A']: one full-width tile each
  multi_tile    n = 200, m = 300 (about 1500 / 1900 nonzeros): several workgroups emit partials
  wrapped       n = 600, m = 900, 18 000 nonzeros: more than 64 tiles in A and in [P | A'], run with COSMO_HIP_GRID_CAP = 64 so that a workgroup folds several tiles
  long_row      n = 2200, m = 2300, one row and one column of A with 2100 entries: the chunked path
  empty_rows    n = 30, m = 40 with empty rows (first, middle, last) and empty columns (first, last) of A
  no_rows       n = 9, m = 0
  small_norms   tiny with every vector of order 1e-9: the three + 1e-10 of the rho rule carry weight (sensitivity only)
  zero_prim     A = 0, b = 0, ZeroSet rows: r_prim is exactly 0 in the loop, the rule clamps to rho_min
  tiny_dual     P = 0, q = 0, A of order 1e-20: r_dual is tiny, the rule clamps to rho_max

Batch shapes (csrc/batch_image.cpp: choose_form, LONG_ROW = 64): see BATCH_SHAPES."""
import dataclasses
import functools
import math
import zlib
from fractions import Fraction

import mpmath
import numpy as np
import scipy.sparse as sp

from tests.projection_cases import BOX, NONNEG, ZERO, Cone

DTYPES = {"f64": np.float64, "f32": np.float32}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
LD = np.longdouble
TILE, TILE_ROWS, SMALL_OPERATOR = 256, 256, 256 * 768          # csrc/api.hip: build_row_blocks
CHUNKED_ABOVE = 2048                                           # COSMO_NNZ_PER_BLOCK (csrc/internal.h)
LONG_ROW = 64                                                  # csrc/batch_image.h
TERMS_PRIM, TERMS_DUAL = ("Ax", "s", "b"), ("Px", "q", "ATmu")
POSITIONS = ("first", "last", "tile_end", "idx512", "long")
RHO, RHO_MIN, RHO_MAX, RHO_EQ, ADAPT_TOL = 0.1, 1e-6, 1e6, 1e3, 5.0     # cosmo_hip_default_params (asserted by the GPU tests)
CINV = 37.5
MARGIN = 10.0                                                  # thresholds sit this many bounds away from the exact value
MUTATIONS = tuple("drop:" + t for t in TERMS_PRIM + TERMS_DUAL) + ("skip:Einv", "skip:Dinv", "skip:cinv", "apply:Einv", "apply:Dinv", "apply:cinv",
                                                                   "no_eps:prim", "no_eps:dual", "no_eps:ratio", "old_rho_mu", "no_eq", "no_min")


def gamma(k, dtype_id):
    u = UNIT[dtype_id]
    return k * u / (1.0 - k * u)


def rnd(a, dtype_id):
    """round to the type, keep float64 storage"""
    return np.asarray(a, dtype=DTYPES[dtype_id]).astype(np.float64)


def e10(dtype_id):
    """T(1e-10) of parameters.jl:60-63"""
    return float(DTYPES[dtype_id](1e-10))


# ---- problems ---------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Problem:
    name: str
    dtype_id: str
    P: object
    A: object
    q: np.ndarray
    b: np.ndarray
    cones: list
    Dinv: np.ndarray
    Einv: np.ndarray
    cinv: float
    x0: np.ndarray
    s0: np.ndarray
    mu0: np.ndarray
    place: object = None          # (term, position, index)
    long: object = None           # (long row of A, long column of A)

    @property
    def n(self):
        return self.A.shape[1]

    @property
    def m(self):
        return self.A.shape[0]

    @property
    def cls(self):
        """rho class per row: 0 rho, 1 rho * RHO_EQ, 2 RHO_MIN (parameters.jl:17-49 with convexset.jl:62-69, 831-842; COSMO_INFTY * MIN_SCALING = 1e16,
        RHO_TOL = 1e-4)"""
        out, o = np.zeros(self.m, dtype=np.int32), 0
        for c in self.cones:
            if c.kind == ZERO:
                out[o:o + c.dim] = 1
            elif c.kind == NONNEG:
                out[o:o + c.dim][self.b[o:o + c.dim] > 1e16] = 2
            elif c.kind == BOX:
                with np.errstate(invalid="ignore"):
                    eq = (c.u - c.l) < 1e-4
                loose = (c.l < -1e16) & (c.u > 1e16)
                out[o:o + c.dim] = np.where(loose, 2, np.where(eq, 1, 0))
            o += c.dim
        return out

    @functools.cached_property
    def csr(self):
        """(A, P, A') by rows with sorted columns; row j of [P | A'], the operator of the dual pass, is row j of P followed by row j of A'"""
        A = sp.csr_matrix(self.A); A.sort_indices()
        P = sp.csr_matrix(self.P); P.sort_indices()
        AT = sp.csr_matrix(self.A.T); AT.sort_indices()
        return A, P, AT


def row_blocks(lengths):
    """build_row_blocks (csrc/api.hip) for an operator of at most SMALL_OPERATOR nonzeros: the boundaries of the CSR-stream tiles"""
    lengths = [int(v) for v in lengths]
    assert sum(lengths) <= SMALL_OPERATOR
    rb, r, nrows = [0], 0, len(lengths)
    while r < nrows:
        r1, cnt = r, 0
        while r1 < nrows:
            rn = lengths[r1]
            if r1 > r and (cnt + rn > TILE or r1 - r >= TILE_ROWS):
                break
            cnt += rn
            r1 += 1
            if cnt > TILE:
                break
        rb.append(r1)
        r = r1
    return rb


def tiles(pb):
    """(tile boundaries of A, of [P | A'])"""
    A, P, AT = pb.csr
    return row_blocks(np.diff(A.indptr)), row_blocks(np.diff(P.indptr) + np.diff(AT.indptr))


def rho_vec(rho, cls, dtype_id, mutate=()):
    """update_rho_vec! / set_rho_vec! (parameters.jl:3-13, 75-92) in the type: one product per equality row"""
    t = DTYPES[dtype_id]
    v = np.full(cls.size, t(rho), dtype=t)
    if "no_eq" not in mutate:
        v[cls == 1] = t(rho) * t(RHO_EQ)
    if "no_min" not in mutate:
        v[cls == 2] = t(RHO_MIN)
    return v.astype(np.float64)


def _cones_for(m, rng):
    if m == 0:
        return []
    mz = max(1, m // 4)
    mb = max(3, m // 4)
    mn = m - mz - mb
    assert mn >= 1
    l = rng.standard_normal(mb) - 1.0
    u = l + rng.uniform(0.5, 2.0, mb)
    u[0] = l[0]                                                # an equality row: class 1
    l[1], u[1] = -np.inf, np.inf                               # a loose row: class 2
    if mb >= 5:
        l[3], u[3] = -1e30, 1e30                               # loose, finite
        l[4] = -np.inf                                         # one-sided: class 0
    return [Cone(ZERO, mz), Cone(NONNEG, mn), Cone(BOX, mb, l=l, u=u)]


def _index_of(position, size, blocks, long_index):
    if position == "first":
        return 0
    if position == "last":
        return size - 1
    if position == "tile_end":
        assert len(blocks) > 2, "tile_end needs at least two tiles"
        return blocks[1] - 1
    if position == "idx512":
        assert size > 549
        return 549
    assert position == "long" and long_index is not None
    return long_index


def build(name, dtype_id, n, m, row_nnz, seed, place=None, long=False, empty=False, scale=1.0, p_diag=False, long_len=None):
    """One problem (see the module docstring).  The placement is made on the float64 draws, everything is rounded to the type at the end; the host test
    checks that it survived."""
    rng = np.random.default_rng(seed)
    cones = _cones_for(m, rng)
    k = min(row_nnz, n)
    rows = np.repeat(np.arange(m), k)
    cols = rng.integers(0, n, m * k)
    A = sp.coo_matrix((rng.standard_normal(m * k), (rows, cols)), shape=(m, n)).tolil()
    lr = lc = None
    if long:
        lr, lc = (2 * m) // 3, n // 3
        ll = long_len or (CHUNKED_ABOVE + 52)
        A[lr, rng.choice(n, ll, replace=False)] = rng.standard_normal(ll)
        A[rng.choice(m, min(ll, m), replace=False), lc] = rng.standard_normal(min(ll, m)).reshape(-1, 1)
    if empty:
        for r in (0, m // 2, m - 1):
            A[r, :] = 0.0
        for c in (0, n - 1):
            A[:, c] = 0.0
    A = sp.csc_matrix(A); A.eliminate_zeros()
    if p_diag:
        P = sp.diags(rng.uniform(0.5, 2.0, n)).tolil()
    else:
        S = sp.random(n, n, density=min(1.0, 2.0 / n), random_state=rng, format="csc", data_rvs=rng.standard_normal)
        P = (S.T @ S + sp.diags(rng.uniform(0.5, 2.0, n))).tolil()
    q, b = rng.standard_normal(n) * scale, rng.standard_normal(m) * scale
    Dinv, Einv = 10.0 ** rng.uniform(-2, 2, n), 10.0 ** rng.uniform(-2, 2, m)
    x0, s0, mu0 = rng.standard_normal(n) * scale, np.abs(rng.standard_normal(m)) * scale, rng.standard_normal(m) * scale
    placed = None
    if place is not None:
        # P and A stay as drawn (the loop's KKT systems keep their conditioning): a vector entry is raised (s, b, q), or the iterate is scaled until
        # the matrix term wins inside its row (x for Px, mu for A'mu) and the row's weight Einv_i / Dinv_i is raised until the row wins
        term, position = place
        Ac, Pc, ATc = sp.csr_matrix(A), sp.csr_matrix(P), sp.csr_matrix(A.T)
        if term in TERMS_PRIM:
            i = _index_of(position, m, row_blocks(np.diff(Ac.indptr)) if position == "tile_end" else None, lr)
            ax = Ac @ x0
            if term == "Ax":
                s0[i], b[i] = abs(ax[i]) / 4096.0, -abs(ax[i]) / 4096.0
                Einv[i] = 1.0
            top = 64.0 * max(np.max(Einv * np.abs(ax)), np.max(Einv * np.abs(s0)), np.max(Einv * np.abs(b)))
            if term == "b":
                b[i] = -top / Einv[i]
            elif term == "s":
                s0[i] = top / Einv[i]
            else:
                Einv[i] = top / abs(ax[i])
        else:
            i = _index_of(position, n, row_blocks(np.diff(Pc.indptr) + np.diff(ATc.indptr)) if position == "tile_end" else None, lc)
            if term == "Px":
                x0 *= 64.0 * max(abs((ATc @ mu0)[i]), 1e-3 * scale) / abs((Pc @ x0)[i])
            if term == "ATmu":
                mu0 *= 64.0 * max(abs((Pc @ x0)[i]), 1e-3 * scale) / abs((ATc @ mu0)[i])
            px, atm = Pc @ x0, ATc @ mu0
            if term != "q":
                q[i] = (px[i] if term == "Px" else atm[i]) / 4096.0
                Dinv[i] = 1.0
            top = 64.0 * max(np.max(Dinv * np.abs(px)), np.max(Dinv * np.abs(q)), np.max(Dinv * np.abs(atm)))
            if term == "q":
                q[i] = top / Dinv[i]
            else:
                Dinv[i] = top / abs((px if term == "Px" else atm)[i])
        placed = (term, position, int(i))
    for c in cones:
        if c.kind == BOX:
            c.l, c.u = rnd(c.l, dtype_id), rnd(c.u, dtype_id)
    A = sp.csc_matrix(A); A.sort_indices()
    U = sp.triu(sp.csc_matrix(P), format="csc")                # symmetric to the last bit: the upper triangle, rounded, and its mirror
    U.data = rnd(U.data, dtype_id)
    P = sp.csc_matrix(U + sp.triu(U, 1).T); P.sort_indices()
    A.data = rnd(A.data, dtype_id)
    r = lambda a: rnd(a, dtype_id)
    return Problem(name, dtype_id, P, A, r(q), r(b), cones, r(Dinv), r(Einv), CINV, r(x0), r(s0), r(mu0), placed, (lr, lc) if long else None)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# name -> (build arguments, placements); one problem per placement
HANDLE_SHAPES = {
    "tiny": (dict(n=7, m=5, row_nnz=3), [("Ax", "first"), ("s", "last"), ("b", "first"), ("Px", "last"), ("q", "first"), ("ATmu", "last")]),
    "one_tile": (dict(n=40, m=60, row_nnz=2, p_diag=True), [("b", "last"), ("q", "last"), ("Ax", "last"), ("ATmu", "first")]),
    "multi_tile": (dict(n=200, m=300, row_nnz=5), [("Ax", "tile_end"), ("s", "tile_end"), ("b", "tile_end"), ("Px", "tile_end"), ("q", "tile_end"),
                                                   ("ATmu", "tile_end"), ("s", "first"), ("Px", "first")]),
    "wrapped": (dict(n=600, m=900, row_nnz=20), [("b", "idx512"), ("ATmu", "idx512"), ("Ax", "last"), ("q", "tile_end")]),
    "long_row": (dict(n=2200, m=2300, row_nnz=2, long=True), [("Ax", "long"), ("ATmu", "long"), ("s", "long"), ("q", "long")]),
    "empty_rows": (dict(n=30, m=40, row_nnz=3, empty=True), [("b", "first"), ("s", "last"), ("q", "last"), ("Px", "first"), None]),
    "no_rows": (dict(n=9, m=0, row_nnz=0), [("q", "first"), ("Px", "last")]),
}
HANDLE_ENV = {"wrapped": {"COSMO_HIP_GRID_CAP": "64"}}

# name -> (build arguments, the placements of the three problems of the batch); the forms that take each shape: test_gpu_batch_residual_checks.py
BATCH_SHAPES = {
    "small": (dict(n=60, m=80, row_nnz=3), [("Ax", "first"), ("q", "last"), ("s", "last")]),
    "small_pdiag": (dict(n=50, m=80, row_nnz=3, p_diag=True), [("b", "last"), ("Px", "first"), ("ATmu", "last")]),
    "slots": (dict(n=300, m=700, row_nnz=3), [("b", "idx512"), ("s", "idx512"), ("Ax", "idx512")]),                  # m > 512: the second row slot of <512, 1, 2>
    "long64": (dict(n=120, m=200, row_nnz=3, long=True, long_len=70), [("Ax", "long"), ("ATmu", "long"), ("q", "long")]),   # a row and a column of >= LONG_ROW entries
    "reg24_n": (dict(n=600, m=700, row_nnz=3), [("q", "idx512"), ("Px", "idx512"), ("ATmu", "idx512")]),           # n in 513 .. 1024
    "reg24_m": (dict(n=300, m=1100, row_nnz=2, p_diag=True), [("b", "last"), ("s", "idx512"), ("Ax", "last")]),     # m in 1025 .. 2048, not a multiple of 512
}


@functools.lru_cache(maxsize=None)
def handle_problems(name, dtype_id):
    kw, places = HANDLE_SHAPES[name]
    return [build("%s/%d" % (name, j), dtype_id, seed=_seed(name, j), place=pl, **kw) for j, pl in enumerate(places)]


@functools.lru_cache(maxsize=None)
def batch_problems(name, dtype_id):
    """three DIFFERENT problems of one structure (n, m, cones); their data differ by factors of 8 so that one threshold separates them"""
    kw, places = BATCH_SHAPES[name]
    out = []
    for j, pl in enumerate(places):
        pb = build("%s/%d" % (name, j), dtype_id, seed=_seed(name, 0), place=None, **kw)                  # the cones (and the Box bounds) of member 0 ...
        own = build("%s/%d" % (name, j), dtype_id, seed=_seed(name, j), place=pl, scale=8.0 ** j, **kw)   # ... the data of member j
        own.cones = pb.cones
        out.append(own)
    return out


@functools.lru_cache(maxsize=None)
def special(name, dtype_id):
    if name == "small_norms":
        return build(name, dtype_id, n=7, m=5, row_nnz=3, seed=_seed(name), scale=2e-9)
    if name == "huge_cost":                                   # |cost| > 1e20 after one iteration: Unsolved
        pb = build(name, dtype_id, n=40, m=90, row_nnz=2, seed=_seed(name))
        pb.q = rnd(pb.q * 1e13, dtype_id)
        return pb
    if name == "zero_prim":
        pb = build(name, dtype_id, n=12, m=9, row_nnz=2, seed=_seed(name))
        pb.A = sp.csc_matrix((9, 12))
        pb.b = np.zeros(9)
        pb.cones = [Cone(ZERO, 9)]
        pb.s0 = np.zeros(9)
        return pb
    assert name == "tiny_dual"
    pb = build(name, dtype_id, n=12, m=20, row_nnz=3, seed=_seed(name))
    pb.P = sp.csc_matrix((12, 12))
    pb.q = np.zeros(12)
    pb.A = sp.csc_matrix(pb.A * 1e-20); pb.A.data = rnd(pb.A.data, dtype_id)
    return pb


def with_huge_q(pb):
    """the same problem with q of order 1e13: |cost| > 1e20 at the first check"""
    return dataclasses.replace(pb, name=pb.name + "/huge_q", q=rnd(pb.q * 1e13, pb.dtype_id))


@functools.lru_cache(maxsize=None)
def clamp_batch(dtype_id):
    """three problems of one structure (ZeroSet and Nonnegatives rows, n = 12, m = 20) for one batch: everything zero but P and A (r_prim = r_dual = 0
    exactly: the rule asks for 0, rho_min), P and A of order 1e-20 with q = 0 (a tiny r_dual: the rule asks for thousands of rho), an ordinary one"""
    out = []
    for j in range(3):
        pb = build("clamp/%d" % j, dtype_id, n=12, m=20, row_nnz=3, seed=_seed("clamp", j))
        pb.cones = [Cone(ZERO, 5), Cone(NONNEG, 15)]
        if j == 0:
            pb.q, pb.b, pb.x0, pb.s0, pb.mu0 = np.zeros(12), np.zeros(20), np.zeros(12), np.zeros(20), np.zeros(20)
        if j == 1:
            pb.q = np.zeros(12)
            pb.A = sp.csc_matrix(pb.A * 1e-20); pb.A.data = rnd(pb.A.data, dtype_id)
            pb.P = sp.csc_matrix(pb.P * 1e-20); pb.P.data = rnd(pb.P.data, dtype_id)
        out.append(pb)
    return out


# ---- exact arithmetic on dyadic rationals ---------------------------------------------------------------------------------------------------------
def _shift_for(*arrays):
    """K such that v 2^K is an integer for every finite v of the arrays"""
    k = 0
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).ravel()
        a = a[(a != 0) & np.isfinite(a)]
        if a.size:
            k = max(k, 53 - int(np.frexp(np.abs(a))[1].min()))
    return k


def _ints(a, K):
    out = np.zeros(len(a), dtype=object)
    for i, v in enumerate(np.asarray(a, dtype=np.float64)):
        p, q = float(v).as_integer_ratio()
        out[i] = p << (K - (q.bit_length() - 1))
    return out


def _rowsum(indptr, prod):
    out = np.zeros(len(indptr) - 1, dtype=object)
    out[:] = 0
    ne = np.flatnonzero(np.diff(indptr) > 0)
    if ne.size:
        out[ne] = np.add.reduceat(prod, indptr[ne])
    return out


def _absmax(v):
    """(max |v|, its first index) of an object array of integers; (0, -1) for an empty one"""
    best, at = 0, -1
    for i, x in enumerate(v):
        if abs(x) > best:
            best, at = abs(x), i
    return best, at


@dataclasses.dataclass
class Check:
    """one calculate_result_info! + calculate_cost!: exact values (Fraction) and rounding bounds (float)"""
    r_prim: Fraction
    r_dual: Fraction
    max_norm_prim: Fraction
    max_norm_dual: Fraction
    cost: Fraction
    b_prim: float                 # bound of r_prim and of max_norm_prim
    b_dual: float                 # bound of r_dual and of max_norm_dual
    b_cost: float
    norms: dict                   # term -> (its inf-norm, the row that attains it)

    def five(self):
        return [(self.r_prim, self.b_prim), (self.r_dual, self.b_dual), (self.max_norm_prim, self.b_prim), (self.max_norm_dual, self.b_dual),
                (self.cost, self.b_cost)]


FIVE = ("r_prim", "r_dual", "max_norm_prim", "max_norm_dual", "cost")


def check(pb, x, s, wps, rho, use_E=True, use_D=True, use_c=True, drop=None):
    """residuals.jl:30-96 and :143-147 at x = w_prev[1:n], s, mu = rho .* (w_prev[n+1:end] - s) (solver.jl:307), exactly.  use_E / use_D / use_c: whether
    Einv, Dinv, cinv are applied (all three at termination, none in the rho rule); drop: one of the six terms left out of its max-norm (a mutation)."""
    n, m, did = pb.n, pb.m, pb.dtype_id
    A, P, AT = pb.csr
    ones_n, ones_m = np.ones(n), np.ones(m)
    Einv = pb.Einv if use_E else ones_m
    Dinv = pb.Dinv if use_D else ones_n
    cinv = pb.cinv if use_c else 1.0
    K = _shift_for(A.data, P.data, x, s, wps, rho, pb.q, pb.b, Einv, Dinv, [cinv])
    one = 1 << K
    X, S, W, R, Q, B = (_ints(v, K) for v in (x, s, wps, rho, pb.q, pb.b))
    E, D, Cv = _ints(Einv, K), _ints(Dinv, K), _ints([cinv], K)[0]
    MU = R * (W - S) if m else np.zeros(0, dtype=object)                                           # scale 2K
    AX = _rowsum(A.indptr, _ints(A.data, K) * X[A.indices]) if m else np.zeros(0, dtype=object)      # 2K
    PX = _rowsum(P.indptr, _ints(P.data, K) * X[P.indices])                                        # 2K
    ATM = _rowsum(AT.indptr, _ints(AT.data, K) * MU[AT.indices]) if m else PX * 0                  # 3K
    f2, f3, f5 = Fraction(1, 1 << (2 * K)), Fraction(1, 1 << (3 * K)), Fraction(1, 1 << (5 * K))
    tp = {"Ax": AX * E, "s": S * one * E, "b": B * one * E}                                         # 3K
    rp = (AX + (S - B) * one) * E                                                                   # 3K
    DC = D * Cv
    td = {"Px": PX * one * DC, "q": Q * (one * one) * DC, "ATmu": ATM * DC}                         # 5K
    rd = (PX * one + Q * (one * one) - ATM) * DC                                                    # 5K
    norms = {t: (_absmax(v)[0] * f3, _absmax(v)[1]) for t, v in tp.items()}
    norms.update({t: (_absmax(v)[0] * f5, _absmax(v)[1]) for t, v in td.items()})
    mp_ = max([Fraction(0)] + [norms[t][0] for t in TERMS_PRIM if t != drop])
    md_ = max([Fraction(0)] + [norms[t][0] for t in TERMS_DUAL if t != drop])
    cost = (Fraction(int(np.sum(PX * X)) if n else 0) * f3 / 2 + Fraction(int(np.sum(Q * X)) if n else 0) * f2) * Fraction(Cv, one)
    # ---- bounds ----
    absA, absP, absAT = abs(A).astype(LD), abs(P).astype(LD), abs(AT).astype(LD)
    xa, sa, ba, qa = (np.abs(np.asarray(v, dtype=LD)) for v in (x, s, pb.b, pb.q))
    mu_abs = np.abs(np.asarray(rho, dtype=LD) * (np.asarray(wps, dtype=LD) - np.asarray(s, dtype=LD)))
    b_prim = b_dual = 0.0
    if m:
        lenA = np.diff(A.indptr)
        gp = np.array([gamma(int(k) + 2 + (1 if use_E else 0), did) for k in lenA], dtype=LD)
        b_prim = float(np.max(gp * (absA @ xa + sa + ba) * Einv))
    px_abs = absP @ xa
    lenPT = np.diff(P.indptr) + np.diff(AT.indptr)
    gd = np.array([gamma(int(k) + 4 + (2 if (use_D or use_c) else 0), did) for k in lenPT], dtype=LD)
    atm_abs = absAT @ mu_abs if m else 0.0
    b_dual = float(np.max(gd * (px_abs + atm_abs + qa) * Dinv * cinv))
    lenP = int(np.diff(P.indptr).max()) if n else 0
    b_cost = float(gamma(n + lenP + 2, did) * cinv * (0.5 * np.sum(xa * px_abs) + np.sum(qa * xa)))
    return Check(_absmax(rp)[0] * f3, _absmax(rd)[0] * f5, mp_, md_, cost, b_prim, b_dual, b_cost, norms)


def termination(pb, x, s, wps, rho, mutate=()):
    """the check of check_termination! / calculate_result_info!; mutate: "drop:<term>", "skip:Einv" / "skip:Dinv" / "skip:cinv" """
    drop = next((mu_[5:] for mu_ in mutate if mu_.startswith("drop:")), None)
    return check(pb, x, s, wps, rho, "skip:Einv" not in mutate, "skip:Dinv" not in mutate, "skip:cinv" not in mutate, drop)


@dataclasses.dataclass
class Rule:
    exact: Fraction               # the clamped value to 200 bits
    lo: Fraction                  # every evaluation in the type whose operations round correctly lies in [lo, hi] ...
    hi: Fraction
    rel: Fraction                 # ... and within this relative distance of `exact`
    rho0: Fraction
    chk: Check

    @property
    def new_rho(self):
        return float(self.exact)

    @property
    def ratio(self):
        return float(self.exact / self.rho0)


def _mpf(fr):
    return mpmath.mpf(fr.numerator) / mpmath.mpf(fr.denominator)


def _frac(v):
    """the Fraction an mpf stands for"""
    sign, man, exp, _ = v._mpf_
    return (-1) ** sign * Fraction(int(man)) * Fraction(2) ** int(exp)


def rule(pb, x, s, wps, rho0, rho_min=RHO_MIN, rho_max=RHO_MAX, mutate=()):
    """adapt_rho_vec! up to the clamp (parameters.jl:53-65) on the working variables (nothing unscaled), mu recovered with the rho vector of rho0.
    mutate: "apply:Einv" / "apply:Dinv" / "apply:cinv", "no_eps:prim" / "no_eps:dual" / "no_eps:ratio", "drop:<term>" """
    did = pb.dtype_id
    drop = next((mu_[5:] for mu_ in mutate if mu_.startswith("drop:")), None)
    c = check(pb, x, s, wps, rho_vec(rho0, pb.cls, did), "apply:Einv" in mutate, "apply:Dinv" in mutate, "apply:cinv" in mutate, drop)
    with mpmath.workprec(200):
        ep, ed, er = (mpmath.mpf(0) if ("no_eps:" + k) in mutate else mpmath.mpf(e10(did)) for k in ("prim", "dual", "ratio"))
        r0 = mpmath.mpf(float(DTYPES[did](rho0)))
        lo_c, hi_c = mpmath.mpf(float(DTYPES[did](rho_min))), mpmath.mpf(float(DTYPES[did](rho_max)))

        def ev(rp, mp_, rd, md_):
            den = rd / (md_ + ed) + er
            if den == 0:
                return mpmath.inf if rp > 0 else mpmath.nan
            return r0 * mpmath.sqrt((rp / (mp_ + ep)) / den)

        rp, mp_, rd, md_ = (_mpf(v) for v in (c.r_prim, c.max_norm_prim, c.r_dual, c.max_norm_dual))
        bp, bd = mpmath.mpf(c.b_prim), mpmath.mpf(c.b_dual)
        pos = lambda v: v if v > 0 else mpmath.mpf(0)
        g8 = mpmath.mpf(gamma(8, did))
        clamp = lambda v: min(max(v, lo_c), hi_c)
        mid = clamp(ev(rp, mp_, rd, md_))
        hi = clamp(ev(rp + bp, pos(mp_ - bp), pos(rd - bd), md_ + bd) * (1 + g8))
        lo = clamp(ev(pos(rp - bp), mp_ + bp, rd + bd, pos(md_ - bd)) * (1 - g8))
        mid, lo, hi = _frac(mid), _frac(lo), _frac(hi)
        return Rule(mid, lo, hi, max(hi / mid - 1, 1 - lo / mid), _frac(r0), c)


# ---- thresholds on either side of an exact value, and what the reference decides -----------------------------------------------------------------
def _fr(v):
    return v if isinstance(v, Fraction) else Fraction(float(v))


def outward(value, dtype_id, up):
    """the nearest number of the type at or beyond the Fraction `value` in the direction `up`"""
    t = DTYPES[dtype_id]
    v = t(float(value))
    while (Fraction(float(v)) < value) if up else (Fraction(float(v)) > value):
        v = np.nextafter(v, t(np.inf if up else -np.inf))
    return float(v)


def gates(c, dtype_id, eps_abs=0.0, eps_rel=0.0, obj_true=math.nan, obj_true_tol=0.0):
    """has_converged (residuals.jl:98-139) on the exact values: gate -> (passes, |value - threshold| / bound as a Fraction or None where nothing rounds).
    Bound of r < eps_abs + eps_rel max_norm: the residual's, eps_rel times the max-norm's and the rounding of the product, the rounding of the sum when
    both tolerances are set; of |obj_true - cost| <= tol: the cost's and the rounding of the difference."""
    u = _fr(UNIT[dtype_id])
    out = {}
    for g, r, mn, br in (("prim", c.r_prim, c.max_norm_prim, c.b_prim), ("dual", c.r_dual, c.max_norm_dual, c.b_dual)):
        thr = _fr(eps_abs) + _fr(eps_rel) * mn
        bound = _fr(br) + _fr(eps_rel) * (_fr(br) + u * mn) + (u * thr if (eps_abs != 0 and eps_rel != 0) else 0)
        out[g] = (r < thr, abs(r - thr) / bound if bound > 0 else None)
    if obj_true != obj_true:
        out["obj"] = (True, None)
    else:
        d = abs(_fr(obj_true) - c.cost)
        bound = _fr(c.b_cost) + u * d
        out["obj"] = (d <= _fr(obj_true_tol), abs(d - _fr(obj_true_tol)) / bound if bound > 0 else None)
    return out


def decided(g):
    """(Solved?, the margin in bounds the verdict rests on, the gates that fail).  Not Solved rests on the clearest failing gate, Solved on the
    closest of all gates; a verdict with a margin below MARGIN is not one the device has to reproduce."""
    inf = lambda mg: math.inf if mg is None else float(mg)
    failing = [k for k, (ok, _) in g.items() if not ok]
    if failing:
        return False, max(inf(g[k][1]) for k in failing), failing
    return True, min(inf(mg) for _, mg in g.values()), failing


def plan_decisions(c, dtype_id):
    """[(label, the gate the thresholds straddle, parameters on the failing side, on the passing side)]: one threshold MARGIN bounds on either side of
    the exact value -- eps_abs around r_prim and around r_dual (eps_rel = 0), eps_rel around r / max_norm of either side (eps_abs = 0), obj_true at
    +- obj_true_tol around the cost with both residual gates wide open.  The two residual gates share eps_abs and eps_rel, so the passing side ends
    Solved only where the straddled residual (ratio) is the larger of the two; what every run must return is decided by gates()."""
    u, M = _fr(UNIT[dtype_id]), _fr(MARGIN)
    out = []
    sides = (("prim", c.r_prim, c.max_norm_prim, c.b_prim), ("dual", c.r_dual, c.max_norm_dual, c.b_dual))
    for which, r, mn, b in sides:
        if b > 0:
            out.append(("eps_abs", which, dict(eps_abs=outward(r - M * _fr(b), dtype_id, False), eps_rel=0.0),
                        dict(eps_abs=outward(r + M * _fr(b), dtype_id, True), eps_rel=0.0)))
    for which, r, mn, b in sides:
        if b > 0 and mn > 0:
            cc = _fr(b) + u * mn
            d = M * (_fr(b) + (r / mn) * cc) / (mn - M * cc)                 # d mn = M (b + (r / mn + d) cc): the bound at the far threshold
            out.append(("eps_rel", which, dict(eps_abs=0.0, eps_rel=outward(r / mn - d, dtype_id, False)), dict(eps_abs=0.0, eps_rel=outward(r / mn + d, dtype_id, True))))
    wide = outward(2 * max(c.r_prim, c.r_dual) + 1, dtype_id, True)
    T = _fr(2.0 ** (math.frexp(float(abs(c.cost)))[1] - 7) if c.cost != 0 else 2.0 ** -20)
    sgn = 1 if c.cost >= 0 else -1                                         # obj_true beyond the cost, away from zero: no cancellation in the type
    d_in, d_out = T - M * (_fr(c.b_cost) + u * T), (T + M * _fr(c.b_cost)) / (1 - M * u)
    near = outward(c.cost + sgn * d_in, dtype_id, sgn < 0)                    # rounded towards the cost
    far = outward(c.cost + sgn * d_out, dtype_id, sgn > 0)                    # rounded away from it
    out.append(("obj_true", "obj", dict(eps_abs=wide, eps_rel=0.0, obj_true=far, obj_true_tol=float(T)), dict(eps_abs=wide, eps_rel=0.0, obj_true=near, obj_true_tol=float(T))))
    return out


def adapts(rl, dtype_id, tol, rho0=RHO):
    """(adapted?, margin in bounds) of parameters.jl:66 on the exact clamped value: new_rho against tol rho and (1 / tol) rho, each threshold with three
    roundings of its own on top of the rule's relative bound"""
    u = _fr(UNIT[dtype_id])
    up, dn = _fr(tol) * rl.rho0, rl.rho0 / _fr(tol)
    bound = lambda thr: rl.rel * rl.exact + 3 * u * thr
    return (rl.exact > up or rl.exact < dn), float(min(abs(rl.exact - up) / bound(up), abs(rl.exact - dn) / bound(dn)))


def plan_tolerances(rl, dtype_id):
    """(an adaptive_rho_tolerance that adapts, one that does not): MARGIN bounds on either side of new_rho / rho (of its inverse below 1); None where
    new_rho is so close to rho that the near one would not exceed 1 (both comparisons of the rule would then hold at once)"""
    a = _fr(MARGIN) * (rl.rel + 3 * _fr(UNIT[dtype_id]))
    if a >= 1:
        return None
    d = a / (1 - a)                                                          # d / (1 + d) = a: the far threshold of the inverse is the tightest
    ratio = rl.exact / rl.rho0
    ratio = ratio if ratio > 1 else 1 / ratio
    if ratio * (1 - d) <= 1:
        return None
    return outward(ratio * (1 - d), dtype_id, False), outward(ratio * (1 + d), dtype_id, True)
