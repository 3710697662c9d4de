"""CPU tests of the polish fixtures and their numpy restatement (tests/polish_cases.py): everything tests/test_gpu_polish.py assumes about its inputs is
shown here by the reference alone -- the active-set rule recovers the constructed active set from the oracle's ADMM solutions (default settings and
eps = 1e-3, on the unscaled iterates and on the iterates scaled with the oracle's D, E, c), the dense polish reproduces (x*, y*, s*) to <= 1e-13
(measured <= 3.8e-15) and the reduced KKT matrices have cond <= 1e3 (measured <= 1.1e2), which is what makes 1e-10 the GPU tests' bound.  Plus the ABI
side of the feature: the header declares the two entry points, the version script exports them, the ABI version stays 1005."""
import fnmatch
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import cosmo_oracle as O
from tests import polish_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _members():
    out = [("fixture%d" % k, c) for k, c in enumerate(PC.batch())]
    out += [(name, getattr(PC, name)()[0]) for name in ("no_inequality_active", "every_row_active", "upper_bounds_infinite", "single_row")]
    out += [("small%d" % k, c) for k, c in enumerate(PC.batch(seeds=(0, 1, 2, 3), **PC.SMALL))]
    return out


MEMBERS = _members()
_solved = {}


def _oracle(name, c, eps):
    """(result, scale matrices) of oracle.solve on member c, computed once"""
    if (name, eps) not in _solved:
        st = O.Settings() if eps is None else O.Settings(eps_abs=eps, eps_rel=eps)
        ws = O.Workspace(sp.csc_matrix(c["P"]), c["q"], sp.csc_matrix(c["A"]), c["b"], PC.cone_sets(c, O), st)
        _solved[(name, eps)] = (ws.optimize(), ws.sm)
    return _solved[(name, eps)]


@pytest.mark.parametrize("eps", [None, 1e-3], ids=["default", "eps1e-3"])
@pytest.mark.parametrize("name,c", MEMBERS, ids=[m[0] for m in MEMBERS])
def test_the_rule_recovers_the_constructed_active_set(name, c, eps):
    r, sm = _oracle(name, c, eps)
    assert r.status == "Solved"
    low, upp = PC.active_set(r.s, r.y, c["lo"], c["hi"], c["mz"])
    assert np.array_equal(low | upp, c["act"])
    assert np.all(c["s"][low] == c["lo"][low]) and np.all(c["s"][upp] == c["hi"][upp])          # ... and the right side of every Box row
    # the scaled iterates and bounds the device holds: x / D, E s, (y / E) c, E l, E u
    low2, upp2 = PC.active_set(sm.E * r.s, (sm.Einv * r.y) * sm.c, sm.E * c["lo"], sm.E * c["hi"], c["mz"])
    assert np.array_equal(low2, low) and np.array_equal(upp2, upp)


@pytest.mark.parametrize("eps", [None, 1e-3], ids=["default", "eps1e-3"])
@pytest.mark.parametrize("name,c", MEMBERS, ids=[m[0] for m in MEMBERS])
def test_the_restatement_reproduces_the_solution_and_the_system_is_well_conditioned(name, c, eps):
    r, _ = _oracle(name, c, eps)
    p = PC.polish_dense(c["P"], c["q"], c["A"], c["b"], r.s, r.y, c["lo"], c["hi"], c["mz"])
    for err, _scale in PC.errors(c, p["x"], p["y"], p["s"]):
        assert err <= 1e-13
    assert p["cond"] <= 1e3
    assert int(p["act"].sum()) == int(c["act"].sum())


def test_the_300_small_members_stay_inside_the_caps():
    """the batch of tests/test_gpu_polish.py that has more members than the polish grid has workgroups (measured: cond <= 1.2e2, error <= 4.0e-15)"""
    for k, c in enumerate(PC.batch(seeds=tuple(range(300)), **PC.SMALL)):
        r = O.Workspace(sp.csc_matrix(c["P"]), c["q"], sp.csc_matrix(c["A"]), c["b"], PC.cone_sets(c, O), O.Settings()).optimize()
        assert r.status == "Solved", k
        p = PC.polish_dense(c["P"], c["q"], c["A"], c["b"], r.s, r.y, c["lo"], c["hi"], c["mz"])
        assert np.array_equal(p["act"], c["act"]) and p["cond"] <= 1e3, k
        assert max(err for err, _ in PC.errors(c, p["x"], p["y"], p["s"])) <= 1e-13, k


def test_the_fixture_is_what_the_issue_describes():
    B = PC.batch()
    assert len(B) == 8 and all(c["n"] == 30 and (c["mz"], c["mn"], c["mb"]) == (4, 16, 12) for c in B)
    for c in B:
        assert np.array_equal(c["P_csc"].indices, B[0]["P_csc"].indices) and np.array_equal(c["A_csc"].indptr, B[0]["A_csc"].indptr)       # one pattern
        assert np.array_equal(c["A_csc"].toarray(), c["A"]) and np.array_equal(c["P_csc"].toarray(), c["P"])
        ineq = slice(c["mz"], None)
        assert np.all((c["s"][ineq] == c["lo"][ineq]) | (c["s"][ineq] == c["hi"][ineq]) | (c["y"][ineq] == 0))          # complementary ...
        gap = np.where(c["act"][ineq], np.abs(c["y"][ineq]), np.minimum(c["s"][ineq] - c["lo"][ineq], c["hi"][ineq] - c["s"][ineq]))
        assert gap.min() >= 0.5                                                                                          # ... strictly
    assert any(np.any(c["A_csc"].data == 0.0) for c in B)                      # the union pattern stores zeros
    ea, eb = PC.errors(B[5], *(lambda r: (r.x, r.y, r.s))(_oracle("fixture5", B[5], 1e-3)[0]))[:2]
    assert ea[0] > 1e-3                                                        # ADMM at eps = 1e-3 is far from x*: what the polish has to repair


def test_the_singular_guess_members_are_what_they_claim():
    c = PC.duplicated_active_row()
    rows = c["A"][c["act"]]
    assert np.linalg.matrix_rank(rows) == rows.shape[0] - 1
    rp, rd = PC.residuals(c, c["x"], c["y"], c["s"])
    assert rp <= 1e-13 and rd <= 1e-13
    d = PC.infeasible()
    assert np.array_equal(d["A"][0], d["A"][1]) and d["b"][0] != d["b"][1]


def test_float32_delta_comes_from_the_unpivoted_restatement():
    """The float32 default of delta (model.POLISH_DELTA_F32): the unpivoted float32 factor reaches the float32 floor (measured 4e-7 .. 6e-7 over the
    fixture) in BOTH extreme orderings at 1e-4 and 1e-3; 1e-6 loses every digit with the rows first (measured 6e4) and 1e-1 stalls the refinement
    (4e-3).  The default is the upper end of that range, the side on which a misjudgement costs refinement steps instead of the factor."""
    import cosmo_jl_amd as cj
    assert cj.model.POLISH_DELTA_F32 == 1e-3
    B = PC.batch()
    for rows_first in (False, True):
        assert max(PC.polish_unpivoted(c, cj.model.POLISH_DELTA_F32, 3, np.float32, rows_first) for c in B) <= 2e-6
        assert max(PC.polish_unpivoted(c, 1e-6, 3, np.float64, rows_first) for c in B) <= 1e-13           # Float64 at its own default
    assert max(PC.polish_unpivoted(c, 1e-6, 3, np.float32, True) for c in B) > 1e-2
    assert max(PC.polish_unpivoted(c, 1e-1, 3, np.float32, True) for c in B) > 1e-4


def test_the_abi_declares_and_exports_the_polish_entry_points():
    from cosmo_jl_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "cosmo_hip.h")).read()
    ver = open(os.path.join(ROOT, "cosmo.jl_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", ver)
    for name in ("cosmo_hip_batch_polish", "cosmo_hip_batch_polish_info"):
        assert re.search(r"(?m)^COSMO_HIP_API int32_t %s\(" % name, hdr), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in patterns), name
        assert name in _ffi.SIGNATURES
    assert re.search(r"cosmo_hip_batch_polish\(cosmo_hip_batch\* b, double delta, int32_t refine_iter\)", hdr)
    assert _ffi.ABI_VERSION == 1005 and re.search(r"#define COSMO_HIP_ABI_VERSION\s+1005\b", hdr)


def test_settings_and_results_carry_the_polish_fields():
    import cosmo_jl_amd as cj
    st = cj.Settings()
    assert st.polish is False and st.polish_delta == 1e-6 and st.polish_refine_iter == 3
    info = cj.model.ResultInfo(0.0, 0.0, 0.0, 0.0, [])
    assert info.polish_status == 0 and np.isnan(info.polish_res_prim_before) and np.isnan(info.polish_res_dual_before)
