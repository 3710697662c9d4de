"""Inputs of the matrix-value-update tests (tests/test_update_matrices_host.py, tests/test_gpu_update_matrices.py).

A CASE is a conic QP (P, q, A, b, sets) with a second pair (P2, A2) of the SAME stored pattern and other values.  A PATTERN is a pair (P, A) for the
value maps of csrc/value_maps.cpp alone, which `maps_of` builds through tests/value_maps_probe.cpp (g++, its own shared object, nothing preloaded)."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp

import cosmo_jl_amd as cj

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- new values on a fixed pattern ------------------------------------------------------------------------------------------------------------
def same_pattern(M, data):
    out = sp.csc_matrix((np.asarray(data, dtype=np.float64), M.indices.copy(), M.indptr.copy()), shape=M.shape)
    assert out.nnz == M.nnz
    return out


def perturbed_psd(P, rng, lo=0.7, hi=1.3):
    """G P G with a positive diagonal G: the pattern of P, still PSD, symmetric bit for bit (the factor g_i g_j is formed first)"""
    P = sp.csc_matrix(P); P.sort_indices()
    g = rng.uniform(np.sqrt(lo), np.sqrt(hi), P.shape[0])
    cols = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
    return same_pattern(P, P.data * (g[P.indices] * g[cols]))


def perturbed(A, rng, lo=0.7, hi=1.3, zeros=0, flips=0):
    """the pattern of A, values scaled by factors in [lo, hi]; `zeros` entries become exact (stored) zeros, `flips` entries change sign"""
    A = sp.csc_matrix(A); A.sort_indices()
    d = A.data * rng.uniform(lo, hi, A.nnz)
    if zeros or flips:
        pick = rng.permutation(A.nnz)[:zeros + flips]
        d[pick[:zeros]] = 0.0
        d[pick[zeros:]] *= -1.0
    return same_pattern(A, d)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------
def split_case(seed=7, n=40, with_P=True):
    """Structure (i): at least half of nnz(A) in singleton rows (the split operator is active), rows of 2-3 entries, one 12-entry row, one empty row,
    one empty column; two singleton rows hit the same column (a diagonal sum with two terms).  P is not diagonal and lacks one diagonal entry."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    r = 0
    empty_col = n - 1

    def add(cs):
        nonlocal r
        for c in cs:
            rows.append(r); cols.append(int(c)); vals.append(float(rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])))
        r += 1
    for c in list(range(n - 1)) * 2:              # two singleton rows per column but the last ...
        add([c])
    add([3]); add([3]); add([5])                   # ... and more on columns 3 (three terms) and 5
    n_single = r
    for _ in range(10):
        add(rng.choice(n - 1, size=2, replace=False))
    for _ in range(6):
        add(rng.choice(n - 1, size=3, replace=False))
    add(rng.choice(n - 1, size=12, replace=False))
    empty_row = r
    r += 1                                         # a row without entries
    add([0, 7])
    m = r
    A = sp.csc_matrix((vals, (rows, cols)), shape=(m, n)); A.sort_indices()
    Ar = A.tocsr()
    lens = np.diff(Ar.indptr)
    assert 2 * int(np.sum(lens == 1)) >= A.nnz and lens[empty_row] == 0 and np.diff(A.indptr)[empty_col] == 0 and 12 in lens
    if with_P:
        S = sp.random(n, n, density=3.0 / n, random_state=rng, format="csc", data_rvs=rng.standard_normal)
        k0 = 11                                    # variable k0 has no entry in P at all: its diagonal entry is missing
        S = S.tolil(); S[k0, :] = 0.0; S = S.tocsc(); S.eliminate_zeros()
        d = np.full(n, 0.3); d[k0] = 0.0
        P = (S @ S.T + sp.diags(d)).tocsc(); P.eliminate_zeros(); P.sort_indices()
        assert P[k0, k0] == 0.0 and (P - sp.diags(P.diagonal())).nnz > 0 and (abs(P - P.T)).nnz == 0
    else:
        P = sp.csc_matrix((n, n))
    nz = n_single // 2
    sets = [cj.ZeroSet(nz), cj.Nonnegatives(m - nz)]
    x0 = rng.standard_normal(n)
    s0 = np.concatenate([np.zeros(nz), rng.uniform(0.1, 1.0, m - nz)])
    b = A @ x0 + s0
    q = rng.standard_normal(n)
    return dict(P=P, q=q, A=A, b=b, sets=sets, P2=perturbed_psd(P, rng) if with_P else P.copy(), A2=perturbed(A, rng))


def mixed_case(seed=11):
    """Structure (ii): tests/util.random_qp with Zero / Nonnegatives / Box / SOC rows at density 0.1 (the split operator is inactive)"""
    from tests import util
    rng = np.random.default_rng(seed)
    pr = util.random_qp(rng, 60, 8, 40, 30, soc_dims=(6, 11), density=0.1, p_shift=0.5)
    L = sp.tril(pr["P"], k=-1)
    pr["P"] = (L + L.T + sp.diags(pr["P"].diagonal())).tocsc()        # symmetric bit for bit (the device Ruiz scaling asks for it)
    pr["P"].sort_indices(); pr["A"].sort_indices()
    pr["P2"] = perturbed_psd(pr["P"], rng); pr["A2"] = perturbed(pr["A"], rng)
    Ar = pr["A"].tocsr()
    assert 2 * int(np.sum(np.diff(Ar.indptr) == 1)) < pr["A"].nnz
    return pr


def zeros_and_flips(case, seed=3):
    """Structure (v): new values with exact zeros (still stored) and sign flips"""
    rng = np.random.default_rng(seed)
    out = dict(case)
    out["A2"] = perturbed(case["A"], rng, zeros=max(3, case["A"].nnz // 10), flips=max(3, case["A"].nnz // 5))
    P = sp.csc_matrix(case["P"]); P.sort_indices()
    if P.nnz:
        # G P G stays PSD for ANY real diagonal G: g_i = -1 flips the signs of row and column i, g_i = 0 turns them into stored zeros
        n = P.shape[0]
        g = rng.uniform(0.85, 1.15, n)
        busy = np.argsort(-np.diff(P.indptr))[:3]
        g[busy[0]] = 0.0; g[busy[1]] *= -1.0; g[busy[2]] *= -1.0
        cols = np.repeat(np.arange(n), np.diff(P.indptr))
        out["P2"] = same_pattern(P, P.data * (g[P.indices] * g[cols]))
        assert np.any(out["P2"].data == 0.0) and np.any(np.sign(out["P2"].data) * np.sign(P.data) < 0)
    return out


# ---- patterns for the value maps ------------------------------------------------------------------------------------------------------------------
def map_patterns():
    rng = np.random.default_rng(5)

    def rnd(m, n, dens):
        M = sp.random(m, n, density=dens, random_state=rng, format="csc", data_rvs=rng.standard_normal); M.sort_indices()
        return M
    out = []
    A = rnd(17, 9, 0.3).tolil(); A[4, :] = 0.0; A[:, 6] = 0.0; A = A.tocsc(); A.eliminate_zeros()
    P = rnd(9, 9, 0.4).tolil(); P[2, :] = 0.0; P[:, 2] = 0.0; P[5, 5] = 0.0; P = P.tocsc(); P.eliminate_zeros()
    out.append(("empty rows and columns, missing diagonal entries", P, A))
    out.append(("nnz(P) = 0", sp.csc_matrix((9, 9)), rnd(12, 9, 0.4)))
    out.append(("m = 0", rnd(7, 7, 0.5), sp.csc_matrix((0, 7))))
    out.append(("1 x n", rnd(6, 6, 0.5), rnd(1, 6, 0.9)))
    out.append(("m x 1", rnd(1, 1, 1.0), rnd(8, 1, 0.8)))
    c = split_case()
    out.append(("split case", c["P"], c["A"]))
    return out


def raw_duplicate_pattern():
    """Raw CSC arrays (0-based here) with duplicate entries and unsorted row indices inside a column, as the C ABI passes them through:
    returns (n, m, (P_indptr, P_indices), (A_indptr, A_indices))"""
    n, m = 4, 5
    A_indptr = np.array([0, 4, 4, 7, 9]); A_indices = np.array([3, 0, 3, 1, 4, 2, 4, 0, 0])          # column 0: rows 3, 0, 3 (a duplicate), 1 -- unsorted
    P_indptr = np.array([0, 3, 5, 5, 7]); P_indices = np.array([2, 0, 0, 1, 1, 3, 0])                # column 0: 2, 0, 0; column 1: 1, 1
    return n, m, (P_indptr, P_indices), (A_indptr, A_indices)


_lib = None


def _probe():
    global _lib
    if _lib is None:
        csrc = os.path.join(_ROOT, "cosmo.jl_amd", "csrc")
        tmp = tempfile.mkdtemp(prefix="value_maps_probe_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "value_maps_probe.so")
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + csrc, "-o", so,
                        os.path.join(_ROOT, "tests", "value_maps_probe.cpp"), os.path.join(csrc, "value_maps.cpp")], check=True)
        lib = ctypes.CDLL(so)
        p64, p32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
        lib.value_maps_probe.restype = ctypes.c_int
        lib.value_maps_probe.argtypes = [ctypes.c_int64, ctypes.c_int64, p64, p64, p64, p64, p32, p32, p32, p32, p32, p32, p32]
        _lib = lib
    return _lib


def maps_of(n, m, P_indptr, P_indices, A_indptr, A_indices):
    """the value maps of csrc/value_maps.cpp for 0-based CSC patterns: dict(A_rowptr, A_map, P_rowptr, P_map, PT_rowptr, PT_split, PT_map)"""
    p64, p32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    ins = [np.ascontiguousarray(np.asarray(a, dtype=np.int64) + 1) for a in (P_indptr, P_indices, A_indptr, A_indices)]
    nnzP, nnzA = int(P_indptr[-1]), int(A_indptr[-1])
    sizes = dict(A_rowptr=m + 1, A_map=nnzA, P_rowptr=n + 1, P_map=nnzP, PT_rowptr=n + 1, PT_split=n, PT_map=nnzP + nnzA)
    outs = {k: np.full(max(v, 1), -7, dtype=np.int32) for k, v in sizes.items()}
    rc = _probe().value_maps_probe(n, m, *[a.ctypes.data_as(p64) for a in ins], *[outs[k].ctypes.data_as(p32) for k in sizes])
    assert rc == 0, rc
    return {k: outs[k][:v] for k, v in sizes.items()}
