"""Inputs of the batch matrix-update tests (tests/test_gpu_batch_update_matrices.py, tests/test_gpu_batch_resident_matrices.py,
tests/test_batch_update_matrices_host.py).

A FAMILY is a list of members of one batch: conic QPs (P, q, A, b, sets) that share n, m and the cones but not their sparsity pattern, each with a second
pair (P2, A2) of its own stored pattern and other values.  Every family carries the structures a value map can get wrong, and asserts them here so that
a later edit cannot lose them: two different patterns, an empty row and an empty column of A, a row of P without its diagonal entry, and new values
with stored exact zeros and sign flips."""
import numpy as np
import scipy.sparse as sp

import cosmo_jl_amd as cj
from tests import update_matrix_cases as UC
from tests import util

MEMBERS = 5
P_ONLY, A_ONLY, BOTH = 0, 2, 3              # the staged members and what each gets; members 1 and 4 stay as they are
STAGED = (P_ONLY, A_ONLY, BOTH)


def _csc(M):
    M = sp.csc_matrix(M); M.eliminate_zeros(); M.sort_indices()
    return M


def _member(j, seed, n, m_zero, m_nonneg, m_box, psd, p_kind, dense_row):
    rng = np.random.default_rng(seed + 101 * j)
    pr = util.random_qp(rng, n, m_zero, m_nonneg, m_box, psd_tri_dims=(2,) if psd else (), p_shift=1.0)
    m = pr["A"].shape[0]
    A = pr["A"].tolil()
    empty_row, empty_col = m_zero + 3 + j, (7 + 2 * j) % n
    if dense_row is not None:
        A[dense_row, :] = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    A[empty_row, :] = 0.0
    A[:, empty_col] = 0.0
    A = _csc(A)
    no_diag = (11 + j) % n                                   # row and column no_diag of P are empty: its diagonal entry is missing
    if p_kind == "diag":
        d = rng.uniform(0.5, 2.0, n)
        if j == BOTH:
            d[no_diag] = 0.0
        P = _csc(sp.diags(d))
    else:
        L = sp.tril(pr["P"], k=-1)
        P = (L + L.T + sp.diags(pr["P"].diagonal())).tolil()  # symmetric bit for bit
        P[no_diag, :] = 0.0; P[:, no_diag] = 0.0
        P = _csc(P)
        assert (P - sp.diags(P.diagonal())).nnz > 0
    c = dict(P=P, q=pr["q"], A=A, b=pr["b"], sets=pr["sets"], P2=UC.perturbed_psd(P, rng), A2=UC.perturbed(A, rng))
    if j == BOTH and p_kind == "diag":                        # (G P G of a diagonal P cannot change a sign: a stored zero, the rest positive)
        c["A2"] = UC.perturbed(A, rng, zeros=max(3, A.nnz // 10), flips=max(3, A.nnz // 5))
        d2 = c["P2"].data.copy(); d2[0] = 0.0
        c["P2"] = UC.same_pattern(P, d2)
    elif j == BOTH:
        c = UC.zeros_and_flips(c, seed=3 + seed)
        assert np.any(np.sign(c["P2"].data) * np.sign(P.data) < 0)
    if j == BOTH:
        assert np.any(c["A2"].data == 0.0) and np.any(np.sign(c["A2"].data) * np.sign(A.data) < 0) and np.any(c["P2"].data == 0.0)
    Ar = A.tocsr()
    assert np.diff(Ar.indptr)[empty_row] == 0 and np.diff(A.indptr)[empty_col] == 0
    if p_kind != "diag" or j == BOTH:
        assert P[no_diag, no_diag] == 0.0 and np.diff(P.indptr)[no_diag] == 0
    if dense_row is not None:
        assert np.diff(Ar.indptr)[dense_row] == n - 1 >= 64   # (every column but the empty one)
    for a, b2 in ((c["P"], c["P2"]), (c["A"], c["A2"])):
        assert np.array_equal(a.indptr, b2.indptr) and np.array_equal(a.indices, b2.indices)
    return c


_families = {}

SHAPES = {
    # name: (n, m_zero, m_nonneg, m_box, PsdConeTriangle(3), P, dense row of A)
    "base": (30, 4, 20, 12, False, "full", None),            # n = 30, m = 36
    "psd": (30, 4, 20, 12, True, "full", None),              # one PsdConeTriangle(3) on top: m = 39
    "pdiag": (30, 4, 20, 12, False, "diag", None),           # P diagonal in every member, member BOTH lacks one diagonal entry
    "long": (70, 4, 20, 12, False, "full", 20),              # one row of A with 69 >= 64 entries
    "tall": (30, 4, 1014, 12, False, "full", None),          # m = 1030: past the <512, 1, 2> register kernel
}


def family(name):
    if name not in _families:
        n, mz, mn, mb, psd, p_kind, dense = SHAPES[name]
        fam = [_member(j, 1000 + 17 * len(name), n, mz, mn, mb, psd, p_kind, dense) for j in range(MEMBERS)]
        pats = {(c["A"].indptr.tobytes(), c["A"].indices.tobytes()) for c in fam}
        assert len(pats) >= 2 and len({c["A"].shape for c in fam}) == 1
        if p_kind == "diag":
            assert all((c["P"] - sp.diags(c["P"].diagonal())).nnz == 0 for c in fam) and fam[BOTH]["P"].nnz == n - 1
        _families[name] = fam
    return _families[name]


def scaling_of(fam, k):
    """a random D, E, c of member k (tests/test_gpu_update_matrices._scaling_of)"""
    rng = np.random.default_rng(17 + k)
    m, n = fam[k]["A"].shape
    return rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, m), 0.75


def scaled(M, L, R, c, dtype):
    """M's pattern with the values v * (L_i * R_j), then * c, in the arithmetic of dtype: the association of model._scale_csc and csrc/update.hip"""
    M = sp.csc_matrix(M); M.sort_indices()
    cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
    L = np.asarray(L).astype(dtype); R = np.asarray(R).astype(dtype)
    d = M.data.astype(dtype) * (L[M.indices] * R[cols])
    if c is not None:
        d = d * np.dtype(dtype).type(c)
    assert d.dtype == np.dtype(dtype)
    return UC.same_pattern(M, d.astype(np.float64))


def scaled_PA(fam, k, P, A, dtype):
    D, E, c = scaling_of(fam, k)
    return scaled(P, D, D, c, dtype), scaled(A, E, D, None, dtype)


def resident_family(count=12, seed=7):
    """the 12-member family of tests/test_gpu_batch_resident.py (n = 30, Zero / Nonnegatives / Box rows), P symmetric bit for bit, with new values"""
    out = []
    for j in range(count):
        rng = np.random.default_rng(seed + j)
        pr = util.random_qp(rng, 30, 4, 20, 12, p_shift=1.0)
        L = sp.tril(pr["P"], k=-1)
        pr["P"] = _csc(L + L.T + sp.diags(pr["P"].diagonal())); pr["A"] = _csc(pr["A"])
        pr["P2"] = UC.perturbed_psd(pr["P"], rng); pr["A2"] = UC.perturbed(pr["A"], rng, lo=0.9, hi=1.1)
        out.append(pr)
    return out
