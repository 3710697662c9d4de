"""Problems with a prescribed split for the Schur-complement KKT solver (kkt_kind KKT_SCHUR, csrc/schur_plan.cpp / csrc/schur.hip).

build(sizes, nd) returns a conic QP whose reduced matrix M = P + sigma I + A' rho A has, at row threshold 3, exactly `nd` long rows (>= 3 stored
entries) and whose block-diagonal part M_s has exactly the connected components `sizes`:

  * the variables are shuffled, then cut into components; consecutive members of a component are chained by two-entry rows,
  * a share of the variables gets a singleton row, and nd rows of 3 .. 6 entries touch several components,
  * P is a positive diagonal plus a few symmetric off-diagonals inside components (p_zero: P has no entry at all),
  * the cones: ZeroSet (chain rows, singleton rows and up to two long rows: rho * 1e3 on both sides of the split), Nonnegatives, and two
    PsdConeTriangle of side 2 on singleton rows.

b = A x0 + s0 with s0 inside the cones, so the problem is feasible.  Nothing here reads the code under test; `ms_pattern` and `components` restate the
split with SciPy for the tests to compare with."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import cosmo_jl_amd as cj

NB = 64            # block side of the dense Cholesky factorisation (csrc/schur_plan.h: SCHUR_NB)
WAVE_MAX = 64      # blocks up to this side are factored by one wave (SCHUR_WAVE_MAX)
SMALL_MAX = 3      # blocks up to this side are factored by one thread (SCHUR_SMALL_MAX)
BLOCK_MAX = 256    # SCHUR_BLOCK_MAX_DEFAULT
ND_MAX = 16384     # SCHUR_ND_MAX_DEFAULT


def build(sizes, nd, seed=0, p_zero=False, zero_rows=True, single_frac=1.0, long_len=(3, 6)):
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in sizes]
    n = int(sum(sizes))
    order = rng.permutation(n)
    comps, o = [], 0
    for s in sizes:
        comps.append(order[o:o + s]); o += s
    label = np.empty(n, dtype=np.int64)
    for k, c in enumerate(comps):
        label[c] = k
    rows = {"zero": [], "nonneg": [], "psd": []}          # lists of (columns, values)

    def val(k):
        return rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k)
    for c in comps:                                        # chains: every third one an equality row
        for i in range(len(c) - 1):
            kind = "zero" if (zero_rows and i % 3 == 0) else "nonneg"
            rows[kind].append((np.array([c[i], c[i + 1]]), val(2)))
    singles = [j for j in range(n) if rng.random() < single_frac]
    for t, j in enumerate(singles):
        kind = "zero" if (zero_rows and t % 7 == 0) else "nonneg"
        rows[kind].append((np.array([j]), val(1)))
    for t in range(6):                                     # two PsdConeTriangle(3): singleton rows
        rows["psd"].append((np.array([int(rng.integers(n))]), val(1)))
    for t in range(int(nd)):                               # long rows over several components
        assert n >= 3, "a long row needs three distinct variables"
        k = min(int(rng.integers(long_len[0], long_len[1] + 1)), n)
        pick = rng.choice(len(comps), size=min(len(comps), k), replace=False)
        cols = [int(rng.choice(comps[p])) for p in pick]
        rest = [j for j in rng.permutation(n) if j not in cols]
        cols = np.array((cols + rest[:k - len(cols)])[:k])
        kind = "zero" if (zero_rows and t < 2) else "nonneg"
        rows[kind].append((cols, val(len(cols))))
    ri, ci, vv, r = [], [], [], 0
    counts = {}
    for kind in ("zero", "nonneg", "psd"):
        counts[kind] = len(rows[kind])
        for cols, vals in rows[kind]:
            ri += [r] * len(cols); ci += list(cols); vv += list(vals); r += 1
    m = r
    A = sp.csc_matrix((vv, (ri, ci)), shape=(m, n))
    if not p_zero:
        d = rng.uniform(0.5, 2.0, n)
        pi, pj, pv = list(range(n)), list(range(n)), list(d)
        for c in comps:
            for _ in range(len(c) // 4):
                a, b_ = rng.choice(c, 2, replace=False)
                w = 0.1 * rng.standard_normal()
                pi += [a, b_]; pj += [b_, a]; pv += [w, w]
        P = sp.csc_matrix((pv, (pi, pj)), shape=(n, n))
    else:
        P = sp.csc_matrix((n, n))
    sets, s0 = [], []
    if counts["zero"]:
        sets.append(cj.ZeroSet(counts["zero"])); s0.append(np.zeros(counts["zero"]))
    sets.append(cj.Nonnegatives(counts["nonneg"])); s0.append(rng.uniform(0.1, 1.0, counts["nonneg"]))
    for _ in range(2):
        B = rng.standard_normal((2, 2))
        sets.append(cj.PsdConeTriangle(3)); s0.append(cj.problems.svec(B @ B.T / 2 + 0.1 * np.eye(2)))
    x0 = rng.standard_normal(n)
    b = A @ x0 + np.concatenate(s0)
    return dict(P=P, q=rng.standard_normal(n), A=A, b=b, sets=sets, label=label, sizes=sorted(sizes), nd=int(nd), n=n, m=m)


def row_lengths(A):
    return np.diff(sp.csr_matrix(A).indptr)


def ms_pattern(P, A, threshold=3):
    """pattern of M_s = P + sigma I + A_s' rho_s A_s (0/1 CSR with a full diagonal), A_s = the rows of A with fewer than `threshold` stored entries"""
    A = sp.csr_matrix(A); n = A.shape[1]
    keep = np.flatnonzero(row_lengths(A) < threshold)
    As = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)[keep]
    Pp = sp.csr_matrix(P); Pp = sp.csr_matrix((np.ones(Pp.nnz), Pp.indices, Pp.indptr), shape=Pp.shape)
    M = (Pp + Pp.T + As.T @ As + sp.identity(n)).tocsr()
    M.data[:] = 1.0
    return M


def components(P, A, threshold=3):
    """(nd, number of components of M_s, largest, sum of size^2, labels) by scipy.sparse.csgraph"""
    nc, lab = connected_components(ms_pattern(P, A, threshold), directed=False)
    size = np.bincount(lab, minlength=nc)
    return int(np.sum(row_lengths(A) >= threshold)), int(nc), int(size.max()) if nc else 0, int(np.sum(size.astype(np.int64) ** 2)), lab


def nnz_w(P, A, threshold=3):
    """nnz(M_s^-1 A_d'): a long row fills every block it touches"""
    A = sp.csr_matrix(A)
    _, nc, _, _, lab = components(P, A, threshold)
    size = np.bincount(lab, minlength=nc)
    total = 0
    for i in np.flatnonzero(row_lengths(A) >= threshold):
        total += int(size[np.unique(lab[A.indices[A.indptr[i]:A.indptr[i + 1]]])].sum())
    return total
