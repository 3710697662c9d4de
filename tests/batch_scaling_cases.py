"""Seeded batches for the device Ruiz equilibration of batches (csrc/batch_ruiz.hip) and their host references.

The shapes are the smallest at which the kernel can go wrong: one variable, an empty P, q = 0 (the two branches of the cost scaling), rows and columns one
past a wave (65 entries: the wave-per-row walk), a column that is empty in P and in A, an empty row, entries beyond MIN_SCALING / MAX_SCALING, infinite Box
bounds, short and long rows in one matrix, a scalar-scaled cone with more rows than the workgroup has threads, members of one structure with different patterns, more members than one
wave of workgroups, and a member whose work vectors cannot live in LDS.

`reference(name, scaling, dtype)` runs the host `scale_ruiz` on copies in the arithmetic of `dtype` three times -- as it is, and with the two
order-dependent means taken sequentially forwards and backwards -- once per process (shared by the host and the GPU tests).  A case whose three results
agree in every bit is in the BITWISE class: nothing in it depends on the order of a sum, so the device must reproduce it to the bit.  The others are held
to `bound(...)`.
"""
import functools

import numpy as np
import scipy.sparse as sp

import cosmo_jl_amd as cj
from cosmo_jl_amd import problems

SCALINGS = (1, 10)
F32_CASES = ("dense_qp_65", "socp_small", "psd_exp_pow", "ragged", "mixed_rows")


def _rand_sparse(rng, m, n, nnz):
    i = rng.integers(0, m, size=nnz); j = rng.integers(0, n, size=nnz)
    M = sp.coo_matrix((rng.standard_normal(nnz), (i, j)), shape=(m, n)).tocsc()
    M.sort_indices()
    return M


def lp_tiny():
    P = sp.csc_matrix((1, 1))
    return [dict(P=P, q=np.array([1.0]), A=sp.csc_matrix(np.array([[1.0], [-1.0]])), b=np.array([1.0, 2.0]), sets=[cj.ZeroSet(1), cj.Nonnegatives(1)])]


def q_zero():
    rng = np.random.default_rng(11)
    P = sp.diags(rng.uniform(0.5, 3.0, 7)).tocsc()
    A = sp.csc_matrix(rng.standard_normal((9, 7)) * (rng.uniform(size=(9, 7)) < 0.6))
    A.sort_indices()
    return [dict(P=P, q=np.zeros(7), A=A, b=rng.standard_normal(9), sets=[cj.ZeroSet(2), cj.Nonnegatives(7)])]


def dense_qp_65(count=1, seed=3):
    return [problems.dense_qp(n=65, half_m=40, seed=seed + k) for k in range(count)]


def clip():
    rng = np.random.default_rng(17)
    n, m = 33, 40
    A = _rand_sparse(rng, m, n, 260).tolil()
    S = _rand_sparse(rng, n, n, 60)
    P = (S + S.T + sp.diags(rng.uniform(1.0, 2.0, n))).tolil()
    A[:, 7] = 0.0; P[:, 7] = 0.0; P[7, :] = 0.0            # an all-zero column of both
    A[12, :] = 0.0                                          # an empty row
    A[3, 2] = 1e7; A[20, 5] = 1e-9                          # above MAX_SCALING, below MIN_SCALING
    A[30, :] = 0.0; A[30, 9] = 3e-7                         # a row whose norm is below MIN_SCALING
    P[4, 4] = 5e6
    A = A.tocsc(); P = P.tocsc(); A.eliminate_zeros(); P.eliminate_zeros(); A.sort_indices(); P.sort_indices()
    l = -np.abs(rng.standard_normal(20)) - 0.1; u = np.abs(rng.standard_normal(20)) + 0.1
    l[0], u[0] = -1e20, 1e20
    l[1], u[1] = -np.inf, np.inf
    l[2] = -np.inf
    u[3] = 1e20
    l[4] = u[4] = 0.25
    return [dict(P=P, q=rng.standard_normal(n), A=A, b=rng.standard_normal(m), sets=[cj.ZeroSet(5), cj.Nonnegatives(15), cj.Box(l, u)])]


def socp_small(count=1, seed=5):
    return [problems.socp(n=70, m=133, ncones=7, nnz=900, seed=seed + k) for k in range(count)]


def _svec_of(M):
    return problems.svec(M)


def conic(seed, n, psd_sides, with_exp_pow, nnz):
    """A strictly feasible problem over PsdConeTriangles (and an exponential, a power and a dual power cone): b = A x0 + s0, q = -P x0 - A' y0 with
    s0 / y0 interior to the cones / their duals."""
    rng = np.random.default_rng(seed)
    sets, s0, y0 = [], [], []
    for d in psd_sides:
        sets.append(cj.PsdConeTriangle(d * (d + 1) // 2))
        for out in (s0, y0):
            W = rng.standard_normal((d, d)) * 0.1
            out.append(_svec_of(2.0 * np.eye(d) + (W + W.T) / 2))
    if with_exp_pow:
        sets += [cj.ExponentialCone(), cj.PowerCone(0.3), cj.DualPowerCone(0.6)]
        s0 += [np.array([0.0, 1.0, 2.0]), np.array([1.0, 1.0, 0.1]), np.array([1.0, 1.0, 0.1])]
        y0 += [np.array([-1.0, 0.0, 1.0]), np.array([1.0, 1.0, 0.1]), np.array([1.0, 1.0, 0.1])]
    s0 = np.concatenate(s0); y0 = np.concatenate(y0)
    m = s0.size
    A = _rand_sparse(rng, m, n, nnz)
    P = sp.diags(0.05 + rng.uniform(size=n)).tocsc()
    x0 = rng.standard_normal(n)
    return dict(P=P, q=-(P @ x0) - A.T @ y0, A=A, b=A @ x0 + s0, sets=sets)


def psd_exp_pow(count=1, seed=23):
    return [conic(seed + k, 40, (24, 1), True, 1500) for k in range(count)]


def psd_side_65(count=1, seed=41):
    """one PsdConeTriangle of side 65: outside the batch kernels, a group solves it on its own handle"""
    return [conic(seed + k, 30, (65,), False, 4000) for k in range(count)]


def ragged():
    out = []
    for k, (nnzA, nnzP) in enumerate(((40, 12), (150, 30), (9, 0), (300, 60), (77, 5))):
        rng = np.random.default_rng(100 + k)
        n, m = 20, 30
        A = _rand_sparse(rng, m, n, nnzA)
        if nnzP:
            S = _rand_sparse(rng, n, n, nnzP)
            P = (S + S.T + sp.diags(rng.uniform(0.5, 1.5, n))).tocsc(); P.sort_indices()
        else:
            P = sp.csc_matrix((n, n))
        out.append(dict(P=P, q=rng.standard_normal(n), A=A, b=rng.standard_normal(m), sets=[cj.ZeroSet(5), cj.Nonnegatives(10), cj.SecondOrderCone(15)]))
    return out


def mixed_rows():
    """short and long rows in the same matrices: a sparse A with three dense rows and two dense columns, a sparse P with one dense row / column --
    the thread-per-row and the wave-per-row walks side by side (the merge of a long A' row into a short P row's norm and the other way round)"""
    rng = np.random.default_rng(29)
    n, m = 90, 110
    A = _rand_sparse(rng, m, n, 500).tolil()
    for i in (4, 57, 109):
        A[i, :] = rng.standard_normal(n)
    for j in (0, 63):
        A[:, j] = rng.standard_normal((m, 1))
    S = _rand_sparse(rng, n, n, 120).tolil()
    S[17, :] = rng.standard_normal(n) * 0.1
    S = S.tocsc()
    P = (S + S.T + sp.diags(rng.uniform(2.0, 3.0, n))).tocsc(); P.sort_indices()
    A = A.tocsc(); A.sort_indices()
    l = -np.abs(rng.standard_normal(30)) - 0.1; u = np.abs(rng.standard_normal(30)) + 0.1
    return [dict(P=P, q=rng.standard_normal(n), A=A, b=rng.standard_normal(m), sets=[cj.ZeroSet(10), cj.Nonnegatives(50), cj.Box(l, u), cj.SecondOrderCone(20)])]


def many():
    return [problems.socp(n=70, m=133, ncones=7, nnz=900, seed=k) for k in range(70)]


def wide():
    return [problems.sparse_box_qp(n=12000, m=16000, nnz=60000)]


CASES = dict(lp_tiny=lp_tiny, q_zero=q_zero, dense_qp_65=dense_qp_65, clip=clip, socp_small=socp_small, psd_exp_pow=psd_exp_pow, ragged=ragged, many=many,
             wide=wide, mixed_rows=mixed_rows)
MUST_BE_BITWISE = ("lp_tiny", "q_zero", "dense_qp_65")


def runs():
    """every (case, scaling, dtype) the tests cover"""
    out = [(name, sc, np.float64) for name in CASES for sc in SCALINGS]
    out += [(name, sc, np.float32) for name in F32_CASES for sc in SCALINGS]
    return out


@functools.lru_cache(maxsize=None)
def batch(name):
    return CASES[name]()


def settings(scaling):
    return cj.Settings(scaling=scaling)


def _mean_forward(v):
    return np.cumsum(v)[-1] / v.dtype.type(v.size)          # cumsum adds sequentially, in the array's type


def _mean_backward(v):
    return np.cumsum(v[::-1])[-1] / v.dtype.type(v.size)


def host_scale(p, scaling, dtype, mean=np.mean):
    """model.scale_ruiz on copies of problem p in the arithmetic of dtype: dict(D, E, c, P, A (CSC values), q, b, box_l, box_u)"""
    T = np.dtype(dtype).type
    P = sp.csc_matrix(p["P"], dtype=T, copy=True); A = sp.csc_matrix(p["A"], dtype=T, copy=True)
    P.sort_indices(); A.sort_indices()
    q = np.array(p["q"], dtype=T); b = np.array(p["b"], dtype=T)
    sets = []
    for K in p["sets"]:
        K2 = cj.model._copy_set(K)
        if K2.kind == cj._ffi.BOX:                        # the bounds the library receives: rounded to T
            K2.l = K2.l.astype(T).astype(np.float64); K2.u = K2.u.astype(T).astype(np.float64)
        sets.append(K2)
    sm = cj.model.scale_ruiz(P, q, A, b, sets, settings(scaling), dtype=T, mean=mean)
    with np.errstate(over="ignore"):
        bl = np.concatenate([K.l for K in sets if K.kind == cj._ffi.BOX] or [np.zeros(0)]).astype(T)
        bu = np.concatenate([K.u for K in sets if K.kind == cj._ffi.BOX] or [np.zeros(0)]).astype(T)
    return dict(D=sm.D, E=sm.E, c=T(sm.c), P=P.data.copy(), A=A.data.copy(), q=q, b=b, box_l=bl, box_u=bu)


FIELDS = ("D", "E", "c", "P", "A", "q", "b", "box_l", "box_u")


def same_bits(r1, r2):
    return all(np.asarray(r1[f]).tobytes() == np.asarray(r2[f]).tobytes() for f in FIELDS)


def bound(p, scaling, dtype):
    """rtol = 4 T (max(n, d_max) + 8) u: a sum of k non-negative terms moves by at most 2 (k - 1) u between two orders, every round adds a handful of
    roundings on top; T rounds, d_max the largest scalar-scaled cone, u the unit roundoff."""
    n = p["A"].shape[1]
    d_max = max([K.dim for K in p["sets"] if K.kind in cj.model._SCALAR_SCALED] or [0])
    u = np.finfo(dtype).eps / 2
    return 4.0 * scaling * (max(n, d_max) + 8) * u


def close(a, b, rtol):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64)); b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return bool(np.all((a == b) | (np.abs(a - b) <= rtol * np.abs(b))))


def spread(r1, r2):
    """largest relative difference between two results, in units of nothing (0 for identical)"""
    worst = 0.0
    for f in FIELDS:
        a = np.atleast_1d(np.asarray(r1[f], dtype=np.float64)); b = np.atleast_1d(np.asarray(r2[f], dtype=np.float64))
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))
        if d.size:
            worst = max(worst, float(np.max(d)))
    return worst


@functools.lru_cache(maxsize=None)
def reference(name, scaling, dtype):
    """(host results of every member with np.mean, the forward and the backward restatements, bitwise class?) -- computed once per process"""
    probs = batch(name)
    ref = [host_scale(p, scaling, dtype) for p in probs]
    fwd = [host_scale(p, scaling, dtype, _mean_forward) for p in probs]
    bwd = [host_scale(p, scaling, dtype, _mean_backward) for p in probs]
    bitwise = all(same_bits(a, b) and same_bits(a, c) for a, b, c in zip(ref, fwd, bwd))
    return ref, fwd, bwd, bitwise


def rho_classes(p, res, st):
    """classify_constraints! on the scaled b and bounds, as cosmo_hip_batch_set_params does it (0 inequality, 1 equality, 2 loose)"""
    big = res["b"].dtype.type(st.COSMO_INFTY * st.MIN_SCALING)
    out, off, bp = [], 0, 0
    for K in p["sets"]:
        cl = np.zeros(K.dim, dtype=np.int32)
        if K.kind == cj._ffi.ZERO:
            cl[:] = 1
        elif K.kind == cj._ffi.NONNEG:
            cl[res["b"][off:off + K.dim] > big] = 2
        elif K.kind == cj._ffi.BOX:
            l = res["box_l"][bp:bp + K.dim]; u = res["box_u"][bp:bp + K.dim]
            with np.errstate(invalid="ignore"):
                cl[:] = np.where((l < -big) & (u > big), 2, np.where((u - l) < res["b"].dtype.type(st.RHO_TOL), 1, 0))
            bp += K.dim
        out.append(cl); off += K.dim
    return np.concatenate(out)
