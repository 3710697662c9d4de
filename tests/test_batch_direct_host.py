"""CPU test of the union analysis behind the direct KKT solver in batch mode (csrc/batch_ldl.hip): one symbolic analysis of the union of the members'
K patterns (upper triangle of P, A) serves every member.  Through cosmo_hip_ldl_analyze (host only): under a fixed ordering, adding any member's
entries to the union leaves the symbolic factor unchanged -- every entry of every member has a slot in the union's panels, so a member's refill
only writes slots that exist and its missing entries are explicit zeros -- and the union's factor holds each member's."""
import numpy as np
import scipy.sparse as sp

import cosmo_jl_amd as cj
from tests import util


def _members(count=5, n=30):
    return [util.random_qp(np.random.default_rng(900 + j), n, 3, 15, 8, soc_dims=(4,), psd_tri_dims=(3,)) for j in range(count)]


def _pattern(M):
    M = sp.csc_matrix(abs(M)); M.data[:] = 1.0
    return M


def _union(probs):
    Pu = _pattern(sum(sp.triu(_pattern(p["P"])) for p in probs))
    Au = _pattern(sum(_pattern(p["A"]) for p in probs))
    return Pu, Au


def test_every_member_entry_has_a_slot_in_the_union_factor():
    probs = _members()
    n, m = probs[0]["P"].shape[0], probs[0]["A"].shape[0]
    assert len({tuple(p["A"].indices) for p in probs}) == len(probs)         # the patterns really differ
    Pu, Au = _union(probs)
    rng = np.random.default_rng(7)
    for perm in (None, np.arange(n + m), rng.permutation(n + m)):
        base = cj._ffi.ldl_analyze(n, m, Pu, Au, perm=perm)
        for p in probs:
            if perm is not None:                                          # same ordering: the member's entries add nothing to the union's factor
                P2 = _pattern(Pu + sp.triu(_pattern(p["P"]))); A2 = _pattern(Au + _pattern(p["A"]))
                assert cj._ffi.ldl_analyze(n, m, P2, A2, perm=perm) == base
                own = cj._ffi.ldl_analyze(n, m, sp.triu(_pattern(p["P"])), _pattern(p["A"]), perm=perm)
                assert own["nnz_L"] <= base["nnz_L"]
        assert base["nnz_L"] > 0 and base["panel_size"] >= base["nnz_stored"]


def test_identical_members_analyse_like_one_member():
    p = _members(1)[0]
    n, m = p["P"].shape[0], p["A"].shape[0]
    Pu, Au = _union([p, dict(p), dict(p)])
    assert cj._ffi.ldl_analyze(n, m, Pu, Au) == cj._ffi.ldl_analyze(n, m, sp.triu(_pattern(p["P"])), _pattern(p["A"]))
