"""The cone projections of the persistent batch kernels (csrc/batch.hip), one step at a time.

Batch.set_iterates loads w = [0 ; rows]; one Batch.iterate(1) runs admm_z first (w_prev = w, s = Pi(w_s)) and the KKT solve behind it never writes s:
get_iterates then returns the exact input of the projection, w_prev[n:], and its result, s.  The problems are as plain as the step allows: P = I, one
nonzero per row of A, q = b = 0, scaling off, the infeasibility checks far away.

Every case of tests/projection_cases.py runs in every kernel form that can take it (kernel_info()["form"] is asserted: a case that silently falls to
another kernel fails), against the reference of that file applied to the FETCHED w_prev[n:].  tests/test_projection_cases_host.py proves the cases and
the reference on the CPU.  The bounds are the project's own: bit equality for simple cones and exact cases, 8 eps d ||x|| (test_project_soc),
64 d eps ||X||_F (check_projection / SURVEY 8c), the bounds of test_projection_matches_oracle for the 3-d cones.

Which form takes which case (choose_form and plan_batch_images, csrc/batch_image.cpp):
  * register kernel: n <= 512 and m <= 1024 -> <512, 1, 2>, n <= 1024 and m <= 2048 -> <512, 2, 4> ("if (n <= 512 && m <= 1024) pl.reg_mode = 1; else if
    ..."), never with a PSD cone of side 17 .. 64 ("if (in.nmid > 0) pl.reg_mode = 0"): cases with more rows or a mid cone have no register variant;
  * LDS-image kernel: the image and the work vectors must fit the CU's LDS ("if (h.bytes + sizeof(real) * (n + m) + ... > in.max_lds) return"): about 24
    bytes per row in Float64, so every case here (m <= 4700) fits; its workgroup size is a parameter only without extended cones ("if (ext) pl.bs =
    512"), and COSMO_HIP_BATCH_LDSCG changes its code only with extended cones and m <= 2048 (rcg_form, D.regcg);
  * streaming kernel: everything."""
import contextlib
import faulthandler
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cosmo_jl_amd as cj
from oracle import cosmo_oracle as O
from tests import projection_cases as S
from tests import util

pytestmark = pytest.mark.gpu

CASE_LIMIT_S = 120
SWITCHES = ("COSMO_HIP_BATCH_LDS", "COSMO_HIP_BATCH_REG", "COSMO_HIP_BATCH_BS", "COSMO_HIP_BATCH_LDSCG")
VARIANTS = {                                    # name -> (environment, the form kernel_info must report; None: by size, see _register_form)
    "streaming": ({"COSMO_HIP_BATCH_LDS": "0"}, "streaming"),
    "lds_bs256": ({"COSMO_HIP_BATCH_REG": "0", "COSMO_HIP_BATCH_BS": "256"}, "lds_image"),
    "lds_bs512": ({"COSMO_HIP_BATCH_REG": "0", "COSMO_HIP_BATCH_BS": "512"}, "lds_image"),
    "lds_bs1024": ({"COSMO_HIP_BATCH_REG": "0", "COSMO_HIP_BATCH_BS": "1024"}, "lds_image"),
    "lds_ldscg1": ({"COSMO_HIP_BATCH_REG": "0"}, "lds_image"),
    "lds_ldscg0": ({"COSMO_HIP_BATCH_REG": "0", "COSMO_HIP_BATCH_LDSCG": "0"}, "lds_image"),
    "register": ({}, None),
}
DTYPES = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(autouse=True)
def _case_time_limit():
    """a case that hangs takes the whole process down instead of holding the GPU: nothing runs after a hang"""
    faulthandler.dump_traceback_later(CASE_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def n_of(case):
    """columns: one nonzero per row of A, spread so that no column has 64 entries (LONG_ROW: the default register kernel keeps its sliced image)"""
    return case.m // 32 + 2


def has_extended_cones(case):
    return any((c.kind in S.PSD and c.dim > 1) or c.kind in S.CONE3 for c in case.cones)


def variants_of(case):
    """the kernel forms that can take the case (the lines of csrc/batch_image.cpp quoted in the module docstring)"""
    ext = has_extended_cones(case)
    out = ["streaming"]
    if ext:
        out.append("lds_ldscg1")
        if case.m <= 2048:                                                    # above that D.regcg = 0 whatever the switch says: the same code twice
            out.append("lds_ldscg0")
    else:
        out += ["lds_bs256", "lds_bs512", "lds_bs1024"]
    if not case.mid_sides and case.m <= 2048:                                 # mid cones never reach the register kernel; it holds at most 4 * 512 rows
        out.append("register")
    return out


def _register_form(case):
    return "register_1_2" if n_of(case) <= 512 and case.m <= 1024 else "register_2_4"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    """bit equality; two NaNs count as equal whatever their payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


@contextlib.contextmanager
def _switches(env):
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


def project_step(case, members, dtype, variant):
    """One batch of the given members of `case`: set_iterates(0, rows, 0), iterate(1), get_iterates.  Returns (sent rows, fetched w_prev[n:], s) per member
    and the kernel_info of the batch; the form is asserted here."""
    n, m = n_of(case), case.m
    P = sp.identity(n, format="csc")
    A = sp.csc_matrix((np.ones(m), (np.arange(m), np.arange(m) % n)), shape=(m, n))
    st = cj.Settings(scaling=0, check_infeasibility=10 ** 9)
    sets = util.projection_sets(case.cones)
    models = []
    for _ in members:
        md = cj.Model(dtype=dtype)
        md.set(P, np.zeros(n), A, np.zeros(m), sets, st)
        models.append(md)
    env, form = VARIANTS[variant]
    with _switches(env):
        B, _ = cj.model.prepare_batch(models, 0)
    try:
        info = B.kernel_info()
        assert info["form"] == (form or _register_form(case)), (case.name, variant, info)
        sent = [case.members[k].rows.astype(dtype) for k in members]
        B.set_iterates(None, np.concatenate(sent), None)
        B.iterate(1)
        out = []
        for j in range(len(members)):
            _, w_prev, s, _ = B.get_iterates(j)
            assert not w_prev[:n].any()
            out.append((sent[j], w_prev[n:].copy(), s.copy()))
    finally:
        B.close()
    return out, info


_runs = {}


def run(name, dtype_id, variant, members=None):
    """project_step, once per (case, precision, form, members) for all tests of this file"""
    case = S.case(name)
    members = tuple(range(len(case.members))) if members is None else tuple(members)
    key = (name, dtype_id, variant, members)
    if key not in _runs:
        _runs[key] = project_step(case, members, DTYPES[dtype_id], variant)[0]
    return _runs[key]


_oracle3 = {}


def _oracle_cone3(name, k, i, c, x):
    """the oracle's projection of one 3-d cone (float64), computed once"""
    key = (name, k, i, np.asarray(x).dtype.name)
    if key not in _oracle3:
        v = np.array(x, dtype=np.float64)
        O.project_cone(v, util.oracle_cones(util.projection_sets([c]))[0])
        _oracle3[key] = v
    return _oracle3[key]


WORST = {}                                      # (cone kind, variant, precision) -> worst observed error / bound, printed by every test for the summary


def _note(kind, variant, dtype_id, ratio):
    key = (kind, variant, dtype_id)
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def check_member(case, k, dtype_id, variant, sent, got_in, got):
    """every assertion on one member: the fetched input, then cone by cone against the reference applied to it"""
    mb = case.members[k]
    eps = S.EPS if dtype_id == "f64" else S.EPS32
    expect_in = sent.copy()
    expect_in[sent == 0] = 0.0                                                # k_batch_set_w computes (1 / rho) * mu0 + s0 with mu0 = 0: -0.0 arrives as +0.0
    assert same_bits(got_in, expect_in), (case.name, k, variant)
    ref, branches = S.project_reference(case.cones, got_in)
    c3_err = []
    for i, (c, a, b) in enumerate(zip(case.cones, case.offsets[:-1], case.offsets[1:])):
        x, r, o, tag = got_in[a:b], ref[a:b], got[a:b], mb.tags[i]
        where = (case.name, dtype_id, variant, k, i, c.kind, c.dim, tag, mb.note[i])
        if tag == "exact":
            assert same_bits(o, r), where + (x[:8], o[:8], r[:8])
        elif tag == "poison":
            assert np.isnan(o).all(), where
        elif c.kind == S.SOC:
            assert branches[i] == mb.branch[i], where
            ratio = np.linalg.norm(o.astype(np.float64) - r) / (8 * eps * c.dim * max(np.linalg.norm(x.astype(np.float64)), 1e-300))
            _note("soc", variant, dtype_id, ratio)
            assert ratio <= 1.0, where + (ratio,)
        elif c.kind in S.PSD:
            if tag == "zero":
                assert not x.any() and not o.any(), where
                continue
            d = c.side
            X = S.psd_matrix(x, c)
            bound = S.psd_bound(X, d, eps)
            if c.kind == S.PSD_SQ:
                M = o.reshape(d, d, order="F")
                assert np.array_equal(M, M.T), where                          # the lower triangle is an exact mirror (convexset.jl:316-318)
            Om = S.psd_matrix(o, c)
            ratio = np.linalg.norm(Om - S.psd_matrix(r, c)) / bound
            _note("psd_small" if d <= 16 else "psd_mid", variant, dtype_id, ratio)
            assert ratio <= 1.0, where + (ratio,)
            if tag == "gapped":
                assert np.linalg.eigvalsh(Om).min() >= -bound, where
        else:
            assert tag == "cone3" and np.isfinite(o).all(), where
            orc = _oracle_cone3(case.name, k, i, c, x)
            c3_err.append(float(np.max(np.abs(o.astype(np.float64) - orc)) / max(1.0, float(np.max(np.abs(x))))))
            # from the definition: where the oracle's own result satisfies it ten times tighter (everywhere but y = 0 of the power cones, see the host
            # test), the kernel's satisfies it to the 1e-3 of test_projection_matches_oracle
            if not S.cone3_violation(c, x, orc, tol=S.CONE3_TOL / 10):
                assert S.cone3_violation(c, x, o) == [], where + (x, o, orc)
    if c3_err and dtype_id == "f64":                                          # the bounds of test_projection_matches_oracle (same algorithm, device libm)
        err = np.array(c3_err)                                                # (Float32, the mixed cases: the definition above and Handle.project's bits only --
        q99, worst = float(np.quantile(err, 0.99)), float(err.max())          #  the iterations stop at 1e-8, which no Float32 bound of the project speaks about)
        _note("cone3_max/1e-5", variant, dtype_id, worst / 1e-5)
        assert worst < 1e-5, (case.name, variant, k, worst)
        if len(c3_err) >= 100:
            _note("cone3_q99/1e-9", variant, dtype_id, q99 / 1e-9)
            assert q99 < 1e-9, (case.name, variant, k, q99)


def _params():
    out = []
    for name in S.CASES:
        case_f32 = name.startswith(("simple", "soc_", "psd_small", "psd_19", "psd_side_one", "mixed", "poison"))
        for dtype_id in ("f64", "f32") if case_f32 else ("f64",):
            out.append((name, dtype_id))
    return out


PARAMS = _params()


# Handle.project has the same code for every cone but the PSD cones of side 17 .. 64: the cases that hold only those have nothing to compare
PARAMS_SINGLE = [(n, d) for n, d in PARAMS if any(not (c.kind in S.PSD and c.side > 16) for c in S.case(n).cones)]


def _report(name, dtype_id):
    print("worst error / bound so far: %s" % ", ".join("%s %s %s %.3g" % (k + (v,)) for k, v in sorted(WORST.items())))


def test_the_float32_cases_are_the_ones_marked_in_the_case_file():
    for name, dtype_id in PARAMS:
        if dtype_id == "f32":
            assert S.case(name).float32, name
    assert {n for n, d in PARAMS if d == "f32"} == {n for n in S.CASES if S.case(n).float32}


@pytest.mark.parametrize("name,dtype_id", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_every_form_projects_every_member_within_the_bounds(name, dtype_id):
    """each form that can take the case against the reference; then device against device, bit for bit: every form against the streaming kernel"""
    case = S.case(name)
    variants = variants_of(case)
    assert "streaming" in variants and len(variants) >= 2
    for variant in variants:
        for k, (sent, got_in, got) in enumerate(run(name, dtype_id, variant)):
            check_member(case, k, dtype_id, variant, sent, got_in, got)
    # Device against device.  Every form returns the bits of the streaming kernel -- except for PSD cones of side 17 .. 64 between the streaming kernel
    # (256 threads) and the LDS-image kernel (512): psdwg_populate<BS> sums ||X||_F, the shift of the block Jacobi, over BS-strided elements and BS / 64
    # wave partials, so the shift and with it the result differ in the last bits (14 of the 19 mid cases, found by this test).  That pair is held to the
    # bound both already meet against eigh; the LDS-image variants among themselves are the same code with the same BS: bit for bit.
    eps = S.EPS if dtype_id == "f64" else S.EPS32
    base = run(name, dtype_id, "streaming")
    lds = [v for v in variants if v.startswith("lds")]
    for variant in variants[1:]:
        for k, ((_, in0, s0), (_, in1, s1)) in enumerate(zip(base, run(name, dtype_id, variant))):
            assert same_bits(in0, in1)
            for i, (c, a, b) in enumerate(zip(case.cones, case.offsets[:-1], case.offsets[1:])):
                where = (name, dtype_id, variant, "differs from streaming", k, i, c.kind, c.dim, case.members[k].note[i])
                if c.kind in S.PSD and c.side > 16:
                    ratio = np.linalg.norm(S.psd_matrix(s0[a:b], c) - S.psd_matrix(s1[a:b], c)) / max(S.psd_bound(S.psd_matrix(in0[a:b], c), c.side, eps), 1e-300)
                    _note("psd_mid_vs_streaming", variant, dtype_id, ratio)
                    assert ratio <= 1.0 and (case.members[k].tags[i] != "zero" or not s1[a:b].any()), where + (ratio,)
                    s_lds = run(name, dtype_id, lds[0])[k][2]
                    assert same_bits(s_lds[a:b], s1[a:b]), where + ("and from", lds[0])
                else:
                    assert same_bits(s0[a:b], s1[a:b]), where
    _report(name, dtype_id)


@pytest.mark.parametrize("name,dtype_id", PARAMS_SINGLE, ids=["%s-%s" % p for p in PARAMS_SINGLE])
def test_every_form_equals_the_single_problem_projection(name, dtype_id):
    """simple cones, second-order cones, PSD cones of side <= 16 and the 3-d cones: cosmo_hip_project (Handle.project) runs the same operations -- k_soc,
    psd16.h, cone3.h under one set of flags -- so every batch form returns its bits.  (Side 17 .. 64 goes through the matrix-sign iteration there and
    through block Jacobi here: two algorithms, compared with the reference only.)"""
    case = S.case(name)
    dtype = DTYPES[dtype_id]
    h = cj.Handle(0, dtype=dtype)
    sets = util.projection_sets(case.cones)
    h.set_problem(sp.identity(2, format="csc"), np.zeros(2), sp.csc_matrix((case.m, 2)), np.zeros(case.m))
    bl = np.concatenate([K.l for K in sets if K.kind == cj._ffi.BOX] or [np.zeros(0)])
    bu = np.concatenate([K.u for K in sets if K.kind == cj._ffi.BOX] or [np.zeros(0)])
    h.set_cones([K.kind for K in sets], [K.dim for K in sets], bl, bu, cone_param=[getattr(K, "alpha", 0.0) for K in sets])
    try:
        single = None
        for variant in variants_of(case):
            res = run(name, dtype_id, variant)
            if single is None:
                single = [h.project(got_in)[0] for _, got_in, _ in res]
            for k, (_, got_in, got) in enumerate(res):
                for i, (c, a, b) in enumerate(zip(case.cones, case.offsets[:-1], case.offsets[1:])):
                    if c.kind in S.PSD and c.side > 16:
                        continue
                    assert same_bits(got[a:b], single[k][a:b]), (name, dtype_id, variant, "differs from Handle.project", k, i, c.kind, c.dim,
                                                                 case.members[k].note[i])
    finally:
        h.close()


@pytest.mark.parametrize("dtype_id", ["f64", "f32"])
def test_a_poisoned_member_stays_alone(dtype_id):
    """NaN, +-inf and -0.0 in simple rows and one NaN inside one second-order cone of member 2: inside that member only the poisoned cone comes back NaN
    (and the NaNs the simple cones pass through by definition); every other member returns the bits it returns in a batch without member 2."""
    case = S.case("poison")
    assert case.clean == [0, 1, 3]
    for variant in variants_of(case):
        full = run("poison", dtype_id, variant)
        clean = run("poison", dtype_id, variant, members=case.clean)
        for j, k in enumerate(case.clean):
            assert same_bits(full[k][1], clean[j][1]) and same_bits(full[k][2], clean[j][2]), (variant, k)
            assert np.isfinite(full[k][2]).all(), (variant, k)
            check_member(case, k, dtype_id, variant, *clean[j])
        sent, got_in, got = full[2]
        ref, _ = S.project_reference(case.cones, got_in)
        mb = case.members[2]
        for i, (c, a, b) in enumerate(zip(case.cones, case.offsets[:-1], case.offsets[1:])):
            if mb.tags[i] == "poison":
                assert np.isnan(got[a:b]).all(), (variant, i)
            elif c.kind in S.CONE3:
                assert np.isfinite(got[a:b]).all(), (variant, i)
            else:
                assert np.array_equal(np.isnan(got[a:b]), np.isnan(ref[a:b])), (variant, i, c.kind)
                if c.kind not in S.SIMPLE:
                    assert np.isfinite(got[a:b]).all(), (variant, i, c.kind)
        assert np.isnan(got).sum() == np.isnan(ref[[j for c, a, b in zip(case.cones, case.offsets[:-1], case.offsets[1:]) if c.kind not in S.CONE3
                                                    for j in range(a, b)]]).sum()


def test_rows_of_simple_cones_that_project_to_themselves_come_back_untouched():
    """the rows no cone routine owns (ZeroSet, Nonnegatives, Box between the cones of the mixed member): where the projection is the identity the result
    is the input bit for bit, in every form -- a cone routine that writes one row too many would show here"""
    case = S.case("mixed")
    for dtype_id in ("f64", "f32"):
        for variant in variants_of(case):
            for k, (_, got_in, got) in enumerate(run("mixed", dtype_id, variant)):
                ref, _ = S.project_reference(case.cones, got_in)
                kept = 0
                for c, a, b in zip(case.cones, case.offsets[:-1], case.offsets[1:]):
                    if c.kind in S.SIMPLE:
                        keep = bits(ref[a:b]) == bits(got_in[a:b])
                        kept += int(keep.sum())
                        assert np.array_equal(bits(got[a:b])[keep], bits(got_in[a:b])[keep]), (dtype_id, variant, k, c.kind)
                        assert same_bits(got[a:b], ref[a:b]), (dtype_id, variant, k, c.kind)
                assert kept >= 5, (dtype_id, variant, k, kept)
