"""KKT structures that stress the device LDL' (csrc/ldl_dev.h, csrc/ldl.hip, csrc/batch_ldl.h), a plain NumPy reference factorisation and the
derived componentwise backward-error bound they are held to.  No test functions: imported by test_ldl_structures_host.py (CPU) and
test_gpu_ldl_structures.py (GPU).

Conventions: K = [P + sigma I, A'; A, -diag(1 ./ rho)] of order N = n + m; original indices 0 .. n-1 are the x variables, n .. N-1 the rows of A;
perm[k] = original index at position k (cosmo_hip_set_kkt_perm); BS = 256 is the workgroup size of csrc/ldl.hip.

Which structure reaches which loop of the kernels (the host test file asserts the condition named here for every line):

  ldl_factor_sn panel scaling, second trip (r += BS)          dense_block (one supernode of N > BS rows), tall_panel (width 4, > 600 rows)
  ldl_fwd_sn gather second trip, diagonal block r += BS       dense_border(k = 300: every leaf updates 300 > BS columns of the root); dense_block
  ldl_bwd_sn diagonal block c += BS                           dense_block, dense_border(k = 300), default_ordering_large (max_width > BS)
  ldl_bwd_sn wave loop past its first trip (r += 64)          tall_panel (t rows below a 4-wide block), dense_border (k below every leaf)
  ldl_rowpos binary search in a long row list                 tall_panel (leaf v lands in three rows deep in the hub's list of t), default_ordering_large
  descendant loop, a barrier per descendant                   dense_border (root with n = 3000 descendants)
  one launch per level, thousands of levels                   chain (height N - 1 / N - 3)
  one level with >= 1e5 workgroups, atomicAdd of the inertia  flat (600 000 supernodes in one level)
  grid-stride trips of the capped element-wise grids          flat (N = 1 200 000 > 4096 * 256)
  pdiag < 0, P = 0, m = 0, empty rows / columns of A          flat(absent_diag), p_zero, chain(rows = 0), empty_lines
  Float32                                                     every structure, both test files
"""
import atexit
import ctypes
import dataclasses
import os
import shutil
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import cosmo_oracle as O

BS = 256                     # LDL_BS of csrc/ldl.hip
EW_CAP = 4096 * BS           # elements one trip of the capped element-wise grids covers (ew() of csrc/ldl.hip)
SIGMA = 1e-6                 # as in test_gpu_direct_kkt.py (the default of Settings)
LD = np.longdouble


@dataclasses.dataclass
class Structure:
    name: str
    P: sp.csc_matrix
    A: sp.csc_matrix
    perm: object                 # None = the default ordering of the library
    facts: dict                  # what ldl_analyze must report for the structure's own ordering (exact figures)
    eq_rows: np.ndarray          # rows of A that are equality rows (ZeroSet: rho 1e3 times larger)
    closed_form: bool = False    # flat: 2 x 2 blocks, factor known in closed form
    seed: int = 0

    @property
    def n(self):
        return self.P.shape[0]

    @property
    def m(self):
        return self.A.shape[0]

    @property
    def N(self):
        return self.n + self.m


def rho_vector(st, seed):
    """non-uniform rho in [0.05, 20], the equality rows 1e3 times larger"""
    rho = np.random.default_rng(seed).uniform(0.05, 20.0, st.m)
    rho[st.eq_rows] *= 1e3
    return rho


def _eq_rows(rng, m, frac=0.1):
    k = max(int(round(frac * m)), 1 if m >= 2 else 0)
    return np.sort(rng.choice(m, size=k, replace=False)) if k else np.zeros(0, np.int64)


def _csc(M):
    M = sp.csc_matrix(M)
    M.sum_duplicates()
    M.sort_indices()
    return M


# ---- generators ------------------------------------------------------------------------------------------------------------------------------
def dense_block(n, m, seed=1):
    """dense P, dense A, identity permutation: ONE supernode of width N with N rows"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n)) / np.sqrt(n)
    P = B @ B.T + np.eye(n)
    P = 0.5 * (P + P.T)
    A = rng.standard_normal((m, n))
    N = n + m
    return Structure("dense_block_%d" % N, _csc(P), _csc(A), np.arange(N), dict(supernodes=1, max_width=N, height=1, nnz_L=N * (N - 1) // 2),
                     _eq_rows(rng, m), seed=seed)


def dense_border(n, k, seed=2):
    """diagonal P, k dense rows of A ordered last: n - 1 leaves of width 1 whose k tail rows all land in the root; the root holds the k rows and, merged
    with them (maximal supernodes: its column is {the k rows} too), the last x column: width k + 1, n - 1 descendants"""
    rng = np.random.default_rng(seed)
    P = sp.diags(rng.uniform(0.5, 2.0, n))
    A = rng.standard_normal((k, n))
    return Structure("dense_border_%d_%d" % (n, k), _csc(P), _csc(A), np.arange(n + k),
                     dict(supernodes=n, height=2, max_width=k + 1, nnz_L=n * k + k * (k - 1) // 2), _eq_rows(rng, k), seed=seed)


def tall_panel(w, t, seed=3):
    """x = [v, hub_0 .. hub_{w-1}, z], t rows of A, ordered [v, hub, rows, z].  The hub columns couple to all t rows: one supernode of width w with
    t rows below its block.  z couples to the first row only and comes last, so the first row's column has one entry more than the hub's tail and the
    hub does not merge into the dense trailing supernode (rows + z, width t + 1).  The leaf v couples to hub_0 (through P) and to three rows deep in
    the hub's row list (through A): its update of the hub finds them by the binary search of ldl_rowpos."""
    rng = np.random.default_rng(seed)
    n = w + 2
    P = np.zeros((n, n))
    P[1:w + 1, 1:w + 1] = rng.standard_normal((w, w)) * 0.2
    P = P + P.T
    P[0, 1] = P[1, 0] = 0.3
    P += np.diag(np.abs(P).sum(axis=1) + rng.uniform(0.5, 1.5, n))            # diagonally dominant: positive definite
    A = np.zeros((t, n))
    A[:, 1:w + 1] = rng.standard_normal((t, w))
    A[0, n - 1] = 1.5
    deep = [5, t // 2, t - 1]
    A[deep, 0] = rng.standard_normal(3)
    perm = np.concatenate([np.arange(0, w + 1), n + np.arange(t), [n - 1]])
    st = Structure("tall_panel_%d_%d" % (w, t), _csc(P), _csc(A), perm,
                   dict(supernodes=3, height=3, max_width=t + 1, nnz_L=4 + (w * (w - 1) // 2 + w * t) + (t + 1) * t // 2), _eq_rows(rng, t), seed=seed)
    st.deep_rows = deep
    return st


def chain(n, rows=0, seed=4):
    """tridiagonal positive definite P, identity permutation: a tree that is one path.  rows = 0 is the m == 0 case; rows > 0 adds singleton rows of A
    (on x_0, ..., x_{n-1} evenly), whose fill runs down the rest of the chain.

    P = D T D with T = tridiag(-1, 2 + 4e-4, -1) and a random diagonal D in [0.7, 1.4].  The shift is small on purpose: the solution of a unit vector
    decays like exp(-sqrt(4e-4)) = 0.98 per step, 1e-26 over 3000 steps -- inside the NORMAL range of Float32 (with a shift of order one it would run
    into the subnormals after a hundred steps, where the rounding model of the bound, fl(a op b) = (a op b)(1 + delta), does not hold)."""
    rng = np.random.default_rng(seed)
    D = sp.diags(rng.uniform(0.7, 1.4, n))
    T = sp.diags([-np.ones(n - 1), np.full(n, 2.0 + 4e-4), -np.ones(n - 1)], [-1, 0, 1])
    P = D @ T @ D
    cols = np.linspace(0, n - 1, rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    A = sp.csc_matrix((rng.uniform(0.5, 2.0, rows), (np.arange(rows), cols)), shape=(rows, n))
    N = n + rows
    # columns 0 .. n-2 each have {next column} + {the singleton rows met so far} below the diagonal: widths 1; the last x column and the rows merge
    facts = dict(supernodes=n - 1 if rows == 0 else n, height=n - 1 if rows == 0 else n, max_width=2 if rows == 0 else rows + 1)
    return Structure("chain_%d_%d" % (n, rows), _csc(P), _csc(A), np.arange(N), facts, np.arange(min(rows, 1)), seed=seed)


def flat(n, absent_diag=False, seed=5):
    """diagonal P, A a scaled permutation matrix, ordered [x_j, row of x_j] pairwise: K is block diagonal with 2 x 2 blocks
    [[P_jj + sigma, a_j], [a_j, -1 / rho_i]] -- n supernodes of width 2 in ONE level.  absent_diag: every second P_jj is missing from the PATTERN
    (its slot holds sigma alone); |a_j| of those columns is in [32, 64] >= 1 / rho_min = 20, so that the block's eigenvalues are about +-|a_j|."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.5, 2.0, n)
    a = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    row_of = rng.permutation(n)                         # row_of[j]: the row of A that holds x_j
    keep = np.ones(n, bool)
    if absent_diag:
        keep[1::2] = False
        a[~keep] *= 32.0
    P = sp.csc_matrix((p[keep], (np.flatnonzero(keep), np.flatnonzero(keep))), shape=(n, n))
    A = sp.csc_matrix((a, (row_of, np.arange(n))), shape=(n, n))
    perm = np.empty(2 * n, np.int64)
    perm[0::2] = np.arange(n)
    perm[1::2] = n + row_of
    st = Structure("flat_%d%s" % (n, "_absent_diag" if absent_diag else ""), _csc(P), _csc(A), perm,
                   dict(supernodes=n, height=1, max_width=2, nnz_L=n), _eq_rows(rng, n, 0.01), closed_form=True, seed=seed)
    st.row_of = row_of
    return st


def p_zero(n, m, seed=6):
    """an LP: P has no stored entry at all; A sparse with full column rank (a diagonal block on top of a random pattern); default ordering.

    The entries of A are of order 1e-3 = sqrt(sigma).  An x column whose diagonal is sigma alone and that is eliminated before its rows has
    L = a / sigma, and two rows that share it leave the pivot (1/rho_2 + (a_2 / a_1)^2 / rho_1) as the difference of two numbers of size a^2 / sigma:
    with a of order one that is a cancellation of sigma / (rho a^2) = 1e-6 ... 1e-11 -- no-pivot LDL' of such a K breaks down in Float32 (a zero
    pivot in the NumPy reference as well), which says nothing about a kernel.  With a^2 of the order of sigma there is no such growth."""
    rng = np.random.default_rng(seed)
    A = sp.random(m, n, density=4.0 / n, random_state=rng, format="csc", data_rvs=rng.standard_normal)
    A = 1e-3 * (A + sp.csc_matrix((rng.uniform(1.0, 2.0, n), (np.arange(n), np.arange(n))), shape=(m, n)))
    return Structure("p_zero_%d_%d" % (n, m), sp.csc_matrix((n, n)), _csc(A), None, {}, _eq_rows(rng, m), seed=seed)


def empty_lines(n, m, seed=7):
    """random sparse P; every 7th row and every 5th column of A is all zero; default ordering"""
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density=3.0 / n, random_state=rng, format="csc", data_rvs=rng.standard_normal)
    P = S @ S.T + 0.1 * sp.identity(n)
    A = sp.random(m, n, density=4.0 / n, random_state=rng, format="lil", data_rvs=rng.standard_normal)
    A[::7, :] = 0.0
    A[:, ::5] = 0.0
    A = _csc(A)
    A.eliminate_zeros()
    st = Structure("empty_lines_%d_%d" % (n, m), _csc(P), A, None, {}, _eq_rows(rng, m), seed=seed)
    st.empty_rows = np.arange(0, m, 7)
    st.empty_cols = np.arange(0, n, 5)
    return st


def default_ordering_large(n=1500, m_zero=100, m_nonneg=1400, m_box=700, soc_dims=(40, 60, 80), psd_tri_dims=(8, 12), density=0.004, seed=8):
    """the pattern of tests/util.random_qp (Zero, Nonnegatives, Box, SOC and PSD-triangle blocks of rows; A random with a half-unit diagonal; P = S S' +
    shift) at n = 1500, m about 2500, under the DEFAULT ordering"""
    from tests import util
    rng = np.random.default_rng(seed)
    prob = util.random_qp(rng, n, m_zero, m_nonneg, m_box, soc_dims=soc_dims, density=density, psd_tri_dims=psd_tri_dims, p_shift=0.5)
    m = prob["A"].shape[0]
    return Structure("default_ordering_large", _csc(prob["P"]), _csc(prob["A"]), None, {}, np.arange(m_zero), seed=seed)


# ---- assembling K in the working precision ---------------------------------------------------------------------------------------------------
def rounded(st, rho, dtype):
    """P, A, rho rounded to the working dtype and widened again: exactly the data the device holds"""
    r = lambda M: sp.csc_matrix(M, dtype=dtype).astype(np.float64)
    return r(st.P), r(st.A), np.asarray(rho, dtype=dtype).astype(np.float64)


def kkt(st, rho, dtype=np.float64):
    """the unpermuted K in float64 (O.assemble_kkt_full) from the values rounded to the working dtype.  (For Float32 data every entry but P_jj + sigma
    and 1 / rho is exact in float64; those two are what the second term of the bound pays for.)"""
    P, A, r = rounded(st, rho, dtype)
    return O.assemble_kkt_full(P, A, SIGMA, r).tocsr()


def spmv_ld(M, x):
    """M x in long double (M: scipy CSR with float64 values; SciPy has no long double kernels)"""
    M = sp.csr_matrix(M)
    prod = M.data.astype(LD) * np.asarray(x, dtype=LD)[M.indices]
    out = np.zeros(M.shape[0], dtype=LD)
    nonempty = np.diff(M.indptr) > 0
    if prod.size:
        out[nonempty] = np.add.reduceat(prod, M.indptr[:-1][nonempty])
    return out


def permuted_dense(K, perm):
    p = np.asarray(perm)
    return K[p][:, p].toarray()


# ---- the reference factorisation -------------------------------------------------------------------------------------------------------------
def ldl_nopivot(Kp, dtype=np.float64, fault=None):
    """Right-looking LDL' without pivoting of the dense (already permuted) matrix Kp in `dtype`: column loop, rank-1 update of the trailing matrix --
    restricted to the nonzero rows of the column, which is what makes it affordable on the sparse structures.  Returns (L with unit diagonal, d).

    fault (only the host tests pass it) emulates a kernel bug: ("unscaled", r, c): L[r, c] is left undivided by d_c; ("dropped", r, c2, c): the update
    of entry (r, c2) by column c is skipped; ("perturbed", r, c, rel): L[r, c] *= 1 + rel."""
    S = np.array(Kp, dtype=dtype)
    N = S.shape[0]
    L = np.eye(N, dtype=dtype)
    d = np.zeros(N, dtype=dtype)
    for c in range(N):
        d[c] = S[c, c]
        idx = c + 1 + np.flatnonzero(S[c + 1:, c])
        if idx.size == 0:
            continue
        col = S[idx, c]
        l = col / d[c]
        upd = np.outer(l, col)
        if fault is not None and fault[0] == "dropped" and fault[3] == c:
            upd[np.searchsorted(idx, fault[1]), np.searchsorted(idx, fault[2])] = 0
        if idx.size == N - c - 1:
            S[c + 1:, c + 1:] -= upd                                     # (a dense column: plain slices, no gather / scatter)
        else:
            S[np.ix_(idx, idx)] -= upd
        if fault is not None and fault[0] == "unscaled" and fault[2] == c:
            l[np.searchsorted(idx, fault[1])] = col[np.searchsorted(idx, fault[1])]
        if fault is not None and fault[0] == "perturbed" and fault[2] == c:
            l[np.searchsorted(idx, fault[1])] *= dtype(1) + dtype(fault[3])
        L[idx, c] = l
    return L, d


def ldl_solve(L, d, b, order="dot"):
    """L D L' x = b in the dtype of L, row oriented: every component is one inner product, summed by np.dot ("dot") or by np.dot over the reversed
    operands ("reversed": the opposite summation order) -- the bound holds for any order"""
    dt = L.dtype.type
    N = L.shape[0]
    Ls = sp.csr_matrix(L)
    Lt = sp.csr_matrix(L.T)
    y = np.array(b, dtype=dt)

    def inner(v, w):
        return np.dot(v[::-1], w[::-1]) if order == "reversed" else np.dot(v, w)
    for i in range(N):
        lo, hi = Ls.indptr[i], Ls.indptr[i + 1] - 1                     # (the last entry of row i is the unit diagonal)
        if hi > lo:
            y[i] = y[i] - inner(Ls.data[lo:hi], y[Ls.indices[lo:hi]])
    x = y / d
    for i in range(N - 1, -1, -1):
        lo, hi = Lt.indptr[i] + 1, Lt.indptr[i + 1]                     # (the first entry of row i of L' is the unit diagonal)
        if hi > lo:
            x[i] = x[i] - inner(Lt.data[lo:hi], x[Lt.indices[lo:hi]])
    return x


def flat_closed_form(st, rho, dtype, rhs=None, data_dtype=None):
    """flat: the factor of the 2 x 2 blocks [[d1, a], [a, -1/rho]] in `dtype`: l = a / d1, d2 = -1/rho - l a; with rhs also the solution (every
    operation rounded to `dtype`).  The data are first rounded to data_dtype (default: dtype).  Returns (L (sparse, permuted order), d, x in the
    ORIGINAL order or None)."""
    dt = np.dtype(dtype).type
    n = st.n
    P, A, r = rounded(st, rho, data_dtype or dtype)
    pj = np.asarray(P.diagonal(), dtype=dtype)
    a = np.zeros(n, dtype=dtype)
    Ac = sp.csc_matrix(A)
    a[:] = Ac.data.astype(dtype)                                          # one entry per column, columns in order
    row = Ac.indices
    d1 = pj + dt(SIGMA)
    l = a / d1
    d2 = -(dt(1.0) / r[row].astype(dtype)) - l * a
    d = np.empty(2 * n, dtype=dtype)
    d[0::2] = d1
    d[1::2] = d2
    L = sp.identity(2 * n, format="csr") + sp.csr_matrix((l.astype(np.float64), (2 * np.arange(n) + 1, 2 * np.arange(n))), shape=(2 * n, 2 * n))
    x = None
    if rhs is not None:
        b = np.asarray(rhs, dtype=dtype)
        b1, b2 = b[:n], b[n + row]
        y2 = b2 - l * b1
        x2 = y2 / d2
        x1 = b1 / d1 - l * x2
        x = np.empty(2 * n, dtype=dtype)
        x[:n] = x1
        x[n + row] = x2
    return sp.csr_matrix(L), d, x


class Reference:
    """The reference side of the bound for one (structure, rho, working dtype): K from the rounded data, the float64 no-pivot factor of K[perm][:, perm]
    (ldl_nopivot, or the closed form of flat) -- never anything the device computed."""

    def __init__(self, st, rho, dtype, perm):
        self.st, self.dtype, self.perm = st, np.dtype(dtype), np.asarray(perm)
        self.u = LD(2.0) ** (-53 if self.dtype == np.float64 else -24)
        self.K = kkt(st, rho, dtype)
        if st.closed_form:
            assert np.array_equal(self.perm, st.perm)
            L, d, _ = flat_closed_form(st, rho, np.float64, data_dtype=dtype)
            self.absL, self.absD = abs(L).tocsr(), np.abs(d)
        else:
            L, d = ldl_nopivot(permuted_dense(self.K, self.perm))
            self.absL, self.absD = sp.csr_matrix(np.abs(L)), np.abs(d)
        self.absLt = self.absL.T.tocsr()
        self.absK = abs(self.K).tocsr()
        # W: the largest number of terms any one sum of the factorisation and of the two substitutions can have.  Entry (i, j) of L D L' and row i of
        # the forward substitution sum over (at most) the stored entries of row i of L; component c of the backward substitution sums over the stored
        # entries of COLUMN c of L.  So W - 1 = the larger of the largest row count and the largest column count of L (diagonal included).
        self.W = int(max(np.diff(self.absL.indptr).max(), np.diff(self.absLt.indptr).max())) + 1

    # Componentwise backward-error bound (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.).  gamma_k = k u / (1 - k u); by Lemma 3.3
    # gamma_j + gamma_k + gamma_j gamma_k <= gamma_{j+k}, so the steps below simply add up.  Every sum has at most W - 1 terms.
    #   * factorisation (Thm 10.3 carried over to L D L': two products per term instead of one, then the subtraction from the entry of K and the division
    #     by the pivot): |K~ - L D L'| <= gamma_{W+2} |L||D||L'|.  The kernels take the two products from separately stored, already rounded operands
    #     (l_ik (d_k l_jk) across supernodes, s_ik (s_jk / d_k) inside a diagonal block): 2 more roundings per term allowed, gamma_{W+4};
    #   * forward substitution (Lemma 8.5, valid for ANY summation order): (L + dL1) y = b, |dL1| <= gamma_{W-1} |L|;
    #   * the diagonal solve y / d: gamma_1;
    #   * backward substitution (Lemma 8.5 again -- the wave-tree sum of ldl_bwd_sn is one more summation order): |dL2| <= gamma_{W-1} |L|, and one more
    #     rounding for the subtraction fused with the diagonal solve (x_c = y_c / d_c - s): gamma_W.
    #   Multiplied out as in Thm 10.4: (K~ + dK) x = b with |dK| <= gamma_{(W+4) + (W-1) + 1 + W} |L||D||L'| = gamma_{3W+4} |L||D||L'|.  The constant in use,
    #   c = 3 W + 8, has 4 to spare over this count.
    #   * K~ is what the refill stores: fl(P_jj + fl(sigma)) and fl(-fl(1 / rho_i)), each within gamma_2 <= gamma_c of the exact entry of K: the second term.
    # Hence for every component  |b - K x|_i <= gamma_c ( (|L||D||L'|) |x| )_i + gamma_c ( |K| |x| )_i  with c = 3 W + 8.
    def bound(self, x):
        """the right-hand side of the bound, per component (long double), for the solution x in the original order"""
        c = LD(3 * self.W + 8)
        gamma = c * self.u / (LD(1.0) - c * self.u)
        ax = np.abs(np.asarray(x, dtype=LD))
        t = spmv_ld(self.absL, LD(1.0) * self.absD * spmv_ld(self.absLt, ax[self.perm]))
        g = np.zeros(ax.size, dtype=LD)
        g[self.perm] = t
        return gamma * g + gamma * spmv_ld(self.absK, ax)

    def residual(self, x, rhs):
        """rhs - K x in long double; rhs is what the solver was given (already in the working dtype)"""
        return np.asarray(rhs, dtype=LD) - spmv_ld(self.K, np.asarray(x, dtype=LD))

    def violations(self, x, rhs):
        """components where the bound fails: (index, |r_i|, bound_i), worst ratio first; a non-finite x violates everywhere"""
        r = np.abs(self.residual(x, rhs))
        b = self.bound(x)
        bad = np.flatnonzero(~(r <= b))
        order = bad[np.argsort(-(r[bad] / np.maximum(b[bad], np.finfo(LD).tiny)).astype(np.float64))]
        return [(int(i), float(r[i]), float(b[i])) for i in order[:5]], (float(np.max(r / np.maximum(b, np.finfo(LD).tiny))) if r.size else 0.0)

    # ---- the forward check (well-conditioned structures) ----
    def forward(self, rhs):
        """(x_ref, cond_est): splu of the float64 K, two steps of iterative refinement with long double residuals; cond_est = ||K^-1||_1 ||K||_1"""
        if not hasattr(self, "_lu"):
            Kc = self.K.tocsc()
            self._lu = lu = spla.splu(Kc)
            N = Kc.shape[0]
            inv = spla.LinearOperator((N, N), matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T"), dtype=np.float64)
            self._norm1 = float(spla.onenormest(Kc))
            self._cond = float(spla.onenormest(inv)) * self._norm1
        lu = self._lu
        b = np.asarray(rhs, dtype=LD)
        x = lu.solve(np.asarray(rhs, dtype=np.float64)).astype(LD)
        for _ in range(2):
            x = x + lu.solve((b - spmv_ld(self.K, x)).astype(np.float64)).astype(LD)
        return x, self._cond

    def forward_check(self, x, rhs):
        """(||x - x_ref||_inf, its limit).  x - x_ref = K^-1 (K x_ref - K x) = K^-1 r up to the (refined) error of x_ref, so
        ||x - x_ref||_inf <= ||K^-1||_inf ||r||_inf <= (cond_est / ||K||_1) * ||bound||_inf   (K symmetric: its 1- and inf-norms agree)"""
        xr, cond = self.forward(rhs)
        err = float(np.max(np.abs(np.asarray(x, dtype=LD) - xr)))
        return err, cond * float(np.max(self.bound(x))) / self._norm1


def rhs_pair(st, perm, dtype, seed=99):
    """the two right-hand sides of the tests: standard normal, and the unit vector at the LAST permuted position (a trivial forward solve: the backward
    solve alone)"""
    b = np.random.default_rng(seed).standard_normal(st.N).astype(dtype)
    e = np.zeros(st.N, dtype=dtype)
    e[np.asarray(perm)[-1]] = 1
    return [("normal", b), ("unit_last", e)]


def analysis_perm(st):
    """the permutation a test passes to ldl_analyze / set_kkt_perm (None: the default ordering)"""
    return None if st.perm is None else np.asarray(st.perm, dtype=np.int64)


# ---- the elimination order of the library ----------------------------------------------------------------------------------------------------
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_probe_lib = None


def _probe():
    """tests/ldl_analysis_probe.cpp + csrc/ldl_symbolic.cpp as a shared object in a temporary directory (host C++, a second or two, once per process)"""
    global _probe_lib
    if _probe_lib is None:
        csrc = os.path.join(_ROOT, "cosmo.jl_amd", "csrc")
        tmp = tempfile.mkdtemp(prefix="ldl_probe_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "ldl_probe.so")
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + csrc, "-o", so,
                        os.path.join(_ROOT, "tests", "ldl_analysis_probe.cpp"), os.path.join(csrc, "ldl_symbolic.cpp")], check=True)
        lib = ctypes.CDLL(so)
        pi = ctypes.POINTER(ctypes.c_int64)
        lib.ldl_probe.restype = ctypes.c_int
        lib.ldl_probe.argtypes = [ctypes.c_int64, ctypes.c_int64, pi, pi, pi, pi, pi, pi, pi]
        _probe_lib = lib
    return _probe_lib


FIGURES = ["supernodes", "rows_below_block", "descendants", "searched_list", "gather_columns", "widest_first", "widest_rows"]


def library_order(st, perm="own"):
    """(order, figures): the elimination order the analysis of csrc/ldl_symbolic.cpp uses for this pattern and requested permutation (the default
    ordering, or a postorder of the requested one: the same factor up to a relabelling) and the structural figures of ldl_analysis_probe.cpp.
    perm: "own" = st.perm; None = the default ordering; else an explicit permutation."""
    if isinstance(perm, str):
        perm = st.perm
    pi = ctypes.POINTER(ctypes.c_int64)
    P = sp.csc_matrix(st.P); A = sp.csc_matrix(st.A)
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (P.indptr, P.indices, A.indptr, A.indices)]
    pin = None if perm is None else np.ascontiguousarray(perm, dtype=np.int64)
    out = np.zeros(st.N, dtype=np.int64)
    fig = np.zeros(len(FIGURES), dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(pi)
    rc = _probe().ldl_probe(st.n, st.m, *[ptr(a) for a in arrs], None if pin is None else ptr(pin), ptr(out), ptr(fig))
    assert rc == 0
    return out, dict(zip(FIGURES, fig.tolist()))


# ---- the cases of both test files ------------------------------------------------------------------------------------------------------------
def default_ordering_medium():
    """default_ordering_large's generator at n = 600, m about 1000: small enough for the reference factorisation under the IDENTITY ordering as well
    (nearly dense there: N^3 / 3 operations in NumPy; at the size of default_ordering_large that alone takes more than a minute)"""
    st = default_ordering_large(n=600, m_zero=40, m_nonneg=560, m_box=280, soc_dims=(16, 24, 32), psd_tri_dims=(8,), density=0.01, seed=9)
    st.name = "default_ordering_medium"
    return st


CASES = {
    "dense_block_257": lambda: dense_block(129, 128),
    "dense_block_350": lambda: dense_block(200, 150),
    "dense_block_700": lambda: dense_block(400, 300),
    "dense_border_3000_300": lambda: dense_border(3000, 300),
    "dense_border_3000_5": lambda: dense_border(3000, 5),
    "tall_panel_4_640": lambda: tall_panel(4, 640),
    "chain_3000_0": lambda: chain(3000, 0),
    "chain_3000_3": lambda: chain(3000, 3),
    "flat_600000": lambda: flat(600000),
    "flat_600000_absent_diag": lambda: flat(600000, absent_diag=True),
    "p_zero_300_500": lambda: p_zero(300, 500),
    "empty_lines_300_400": lambda: empty_lines(300, 400),
    "default_ordering_medium": default_ordering_medium,
    "default_ordering_large": default_ordering_large,
}
WELL_CONDITIONED = ("dense_block_257", "dense_block_350", "dense_block_700", "flat_600000", "flat_600000_absent_diag")      # the forward check as well
BOTH_ORDERINGS = ("dense_border_3000_300", "dense_border_3000_5", "default_ordering_medium")    # the other of {identity, default} too

_structures = {}


def structure(name):
    if name not in _structures:
        _structures[name] = CASES[name]()
    return _structures[name]


# ---- two of the structures as real problems (the loop and the batch kernels) --------------------------------------------------------------------
def loop_problem(name, member=0, q_scale=1.0):
    """min 1/2 x'Px + q'x  s.t.  A x + s = b, s >= 0 on the pattern (and, member 0, the values) of structure `name`: b = A x0 + s0 with s0 > 0
    (feasible), q random.  member > 0: the same pattern with the values of P, A scaled per row / column and q, b redrawn (a batch of one pattern)."""
    st = structure(name)
    rng = np.random.default_rng(1000 + 17 * member)
    P, A = st.P, st.A
    if member:
        dx = sp.diags(rng.uniform(0.7, 1.4, st.n))
        P = _csc(dx @ P @ dx)                                                  # a congruence: still positive definite
        A = _csc(sp.diags(rng.uniform(0.5, 2.0, st.m)) @ A @ dx)
    x0 = rng.standard_normal(st.n)
    b = A @ x0 + rng.uniform(0.1, 1.0, st.m)
    q = q_scale * rng.standard_normal(st.n)
    return dict(P=P, q=q, A=A, b=b, perm=st.perm)
