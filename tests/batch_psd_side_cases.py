"""Cases and drivers for PSD cones of side 65 .. 256 in the batch kernels (Settings.batch_psd_side_max; csrc/psdwg.h: psdwg_jacobi_rounds).  No test
functions: imported by test_batch_psd_side_host.py (CPU) and test_gpu_batch_psd_side*.py (GPU).  The case builders and references are those of
tests/projection_cases.py and tests/certificate_cases.py; project_step and the environment helpers are copies of the small drivers of
test_gpu_batch_projections.py / test_gpu_batch.py with the side limit as a parameter.

The round schedule (rr_pair, step_pairs, wave_visits) restates in Python what the kernel must implement: in every tournament step, and in the diagonal
pass, the nb / 2 block pairs are disjoint, and wave wv of NW visits pairs wv, wv + NW, wv + 2 NW, ... one after the other."""
import contextlib
import os

import numpy as np
import scipy.sparse as sp

import cosmo_jl_amd as cj
from tests import certificate_cases as C
from tests import projection_cases as S
from tests import util

# side -> (nb, block pairs per step) and what it exercises with four waves
SIDES = {65: (10, 5),       # first side beyond the old limit: nb 9 -> 10, a ragged second round
         80: (10, 5),       # ld is a multiple of 16
         128: (16, 8),      # two full rounds
         129: (18, 9),      # nb 17 -> 18, three rounds, the last ragged; ld = 144
         256: (32, 16)}     # the ceiling
SQUARE_SIDES = (65, 129)
LDS_SIDES = (65, 80)        # triangle cones whose problem fits the LDS image
# gapped, clustered, indefinite (+3 / -3 and a gapped rest), all negative (-> the zero matrix), all positive (-> the identity map)
SPECTRA = ["gapped", "clusters", "pair", "negdef", "psd"]
BATCHES = [(0, 1), (2, 3), (4, 0), (1, 0)]      # two members with different data per batch; (0, 1) once more in the other order
DTYPES = {"f64": np.float64, "f32": np.float32}
SWITCHES = ("COSMO_HIP_BATCH_LDS", "COSMO_HIP_BATCH_REG", "COSMO_HIP_BATCH_BS", "COSMO_HIP_BATCH_LDSCG")
SEED_DEFAULT, SEED_TIGHT = 6572, 72130          # whole-solve workloads: every instance solves in the oracle (test_gpu_batch_psd_side_solves.py)
VARIANTS = {"streaming": ({"COSMO_HIP_BATCH_LDS": "0"}, "streaming"), "lds_image": ({"COSMO_HIP_BATCH_REG": "0"}, "lds_image")}


# ---- the round schedule ------------------------------------------------------------------------------------------------------------------------------
def geometry(side):
    """(ld, nb, ncp) of a cone of that side: batch_finalize of csrc/batch.hip"""
    ld = (side + 15) // 16 * 16
    nb = (side + 7) // 8
    nb += nb & 1
    return ld, nb, max(nb * 8, ld)


def rr_pair(nb, st, w):
    """block pair w (0 <= w < nb / 2) of tournament step st (0 <= st < nb - 1): rr_pair of csrc/psdwg.h"""
    m = nb - 1
    if w == 0:
        i, j = st % m, m
    else:
        i, j = (st + w) % m, (st - w + m) % m
    return (i, j) if i < j else (j, i)


def step_pairs(nb, st):
    """the block pairs of step st in pair order; st = -1: the diagonal pass (2 w, 2 w + 1)"""
    return [(2 * w, 2 * w + 1) if st < 0 else rr_pair(nb, st, w) for w in range(nb // 2)]


def wave_visits(nb, nw, wv):
    """the pair indices wave wv of nw visits in one step, in order"""
    return list(range(wv, nb // 2, nw))


# ---- projection cases ----------------------------------------------------------------------------------------------------------------------------------
_cases = {}


def case(side, kind):
    """one cone of that side per member, five members: one spectrum of SPECTRA each.  Built once, shared, never modified."""
    key = (side, kind)
    if key not in _cases:
        name = "psd_side_%d_%s" % (side, "tri" if kind == S.PSD_TRI else "sq")
        c = S.psd_spectra_case(name, [side], kind, SPECTRA, len(SPECTRA), 1300 + 3 * side + (kind == S.PSD_SQ), per_member=1)
        for mb in c.members:
            mb.rows.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def three_paths_case():
    """sides 9 (one wave, psd16.h), 40 (one block pair per wave) and 96 (rounds) in one problem, with simple rows between them: two members"""
    if "three" not in _cases:
        bs = []
        for k in range(2):
            rng = np.random.default_rng(1290 + k)
            b = S._Builder()
            S._add_psd(b, rng, 9, S.PSD_TRI, SPECTRA[k])
            b.add(S.Cone(S.NONNEG, 3), rng.standard_normal(3), "exact")
            S._add_psd(b, rng, 96, S.PSD_TRI, SPECTRA[2 + k])
            S._add_psd(b, rng, 40, S.PSD_SQ, SPECTRA[1 + k])
            bs.append(b)
        c = S._case("psd_side_9_96_40", bs)
        for mb in c.members:
            mb.rows.setflags(write=False)
        _cases["three"] = c
    return _cases["three"]


@contextlib.contextmanager
def switches(env):
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def with_env(env, fn):
    with switches(env):
        return fn()


def project_step(cs, members, dtype, variant, side_max, fetch_reversed=False):
    """One batch of the given members of `cs`: set_iterates(0, rows, 0), iterate(1), get_iterates (member by member, in reversed order on request).
    Returns [(sent rows, fetched w_prev[n:], s)] in member order and the kernel_info of the batch; the form is asserted here."""
    n, m = cs.m // 32 + 2, cs.m
    P = sp.identity(n, format="csc")
    A = sp.csc_matrix((np.ones(m), (np.arange(m), np.arange(m) % n)), shape=(m, n))
    st = cj.Settings(scaling=0, check_infeasibility=10 ** 9, batch_psd_side_max=side_max)
    sets = util.projection_sets(cs.cones)
    models = []
    for _ in members:
        md = cj.Model(dtype=dtype)
        md.set(P, np.zeros(n), A, np.zeros(m), sets, st)
        models.append(md)
    env, form = VARIANTS[variant]
    with switches(env):
        B, _ = cj.model.prepare_batch(models, 0)
    try:
        info = B.kernel_info()
        assert info["form"] == form, (cs.name, variant, info)
        sent = [cs.members[k].rows.astype(dtype) for k in members]
        B.set_iterates(None, np.concatenate(sent), None)
        B.iterate(1)
        out = [None] * len(members)
        for j in (range(len(members))[::-1] if fetch_reversed else range(len(members))):
            _, w_prev, s, _ = B.get_iterates(j)
            assert not w_prev[:n].any()
            out[j] = (sent[j], w_prev[n:].copy(), s.copy())
    finally:
        B.close()
    return out, info


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def check_member(cs, k, dtype_id, variant, sent, got_in, got):
    """the fetched input bit for bit, then every cone against the reference of projection_cases applied to it; returns the worst error / bound of the PSD
    cones.  Simple rows: bit equality.  PSD cones: ||out - ref||_F <= psd_bound = 64 d eps ||X||_F, the square layout an exact mirror, gapped spectra
    with eigvalsh(out) >= -bound."""
    mb = cs.members[k]
    eps = S.EPS if dtype_id == "f64" else S.EPS32
    expect_in = sent.copy()
    expect_in[sent == 0] = 0.0
    assert same_bits(got_in, expect_in), (cs.name, k, variant)
    ref, _ = S.project_reference(cs.cones, got_in)
    worst = 0.0
    for i, (c, a, b) in enumerate(zip(cs.cones, cs.offsets[:-1], cs.offsets[1:])):
        x, r, o, tag = got_in[a:b], ref[a:b], got[a:b], mb.tags[i]
        where = (cs.name, dtype_id, variant, k, i, c.kind, c.dim, tag, mb.note[i])
        if tag == "exact":
            assert same_bits(o, r), where
            continue
        assert c.kind in S.PSD and tag in ("psd", "gapped"), where
        d = c.side
        X = S.psd_matrix(x, c)
        bound = S.psd_bound(X, d, eps)
        if c.kind == S.PSD_SQ:
            M = o.reshape(d, d, order="F")
            assert np.array_equal(M, M.T), where
        Om = S.psd_matrix(o, c)
        ratio = float(np.linalg.norm(Om - S.psd_matrix(r, c)) / bound)
        worst = max(worst, ratio)
        print("%s %s %s member %d cone %d (%s): error / bound = %.3g" % (cs.name, dtype_id, variant, k, i, mb.note[i], ratio))
        assert ratio <= 1.0, where + (ratio,)
        if tag == "gapped":
            assert np.linalg.eigvalsh(Om).min() >= -bound, where
    return worst


# ---- certificate cases ---------------------------------------------------------------------------------------------------------------------------------
def certificate_case(mode, dtype_id):
    """the PSD members of certificate_cases.py ("above" / "below" -tol, indefinite, safe, zero) at sides 65 (triangle) and 129 (square), with that file's own
    expected verdicts and margins"""
    return C._psd(dtype_id, mode, "psd_side_65_129", [(65, S.PSD_TRI), (129, S.PSD_SQ)])


def certificate_batch(cs, nprob, side_max, env=None):
    """make_batch of test_gpu_certificates.py with the side limit set before set_cones"""
    F = cj._ffi
    dtype = C.DTYPES[cs.dtype_id]
    sets = util.projection_sets(cs.cones)
    with switches(env or {}):
        B = F.Batch(nprob, cs.n, cs.m, 0, dtype=dtype)
        for k in range(nprob):
            B.set_problem(k, cs.P, cs.q, cs.A, cs.b)
            B.set_scaling_full(k, cs.D, 1.0 / cs.D, cs.E, 1.0 / cs.E, cs.c, 1.0 / cs.c)
        if side_max is not None:
            B.set_psd_side_max(side_max)
        B.set_cones([K.kind for K in sets], [K.dim for K in sets], None, None, cone_param=[getattr(K, "alpha", 0.0) for K in sets])
        p = F.default_params(dtype)
        p.kkt_kind = F.KKT_CG
        p.eps_prim_inf, p.eps_dual_inf = C.EPS_PRIM_INF, C.EPS_DUAL_INF
        B.set_params(p)
    return B


# ---- whole problems ------------------------------------------------------------------------------------------------------------------------------------
def models(probs, st, dtype=np.float64):
    out = []
    for p in probs:
        md = cj.Model(dtype=dtype)
        md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st)
        out.append(md)
    return out


def sdps_default():
    """eight SDPs with triangle cones of side 24 and 72 and a square cone of side 66 (the workload the default-settings test names)"""
    rng = np.random.default_rng(SEED_DEFAULT)
    return [util.random_qp(rng, 60, 0, 10, 0, psd_tri_dims=(24, 72), psd_sq_dims=(66,), p_shift=1.0, density=0.02) for _ in range(8)]


def sdps_tight():
    """four SDPs with triangle cones of side 72 and 130"""
    rng = np.random.default_rng(SEED_TIGHT)
    return [util.random_qp(rng, 60, 0, 10, 0, psd_tri_dims=(72, 130), p_shift=1.0, density=0.02) for _ in range(4)]

