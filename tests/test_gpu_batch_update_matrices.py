"""GPU tests of cosmo_hip_batch_stage_matrices / cosmo_hip_batch_apply_updates: new values of P and A for members of a finalised batch.

PURITY: a batch U that was set up with the old values and then updated must hold the bits of a batch F that was set up with the new values.  The bar
is bitwise equality, and it is derived, not measured: the refresh (csrc/batch.hip: k_batch_update_matrices) scales every staged value once with two
multiplications in the association of model._scale_csc and then only copies it into every value array of the member, and every later kernel is the
same code on the same bits.  One case per kernel form; each asserts through kernel_info() that it reached the form it names."""
import numpy as np
import pytest

from cosmo_jl_amd import _ffi
from tests import batch_update_cases as BC

pytestmark = pytest.mark.gpu

SWITCHES = ("COSMO_HIP_BATCH_LDS", "COSMO_HIP_BATCH_REG", "COSMO_HIP_BATCH_BS", "COSMO_HIP_BATCH_EXT", "COSMO_HIP_BATCH_SLICED", "COSMO_HIP_BATCH_LONG",
            "COSMO_HIP_BATCH_LDSCG", "COSMO_HIP_BATCH_LDSCG_SORTED", "COSMO_HIP_BATCH_STORE_SORTED", "COSMO_HIP_BATCH_SORTED", "COSMO_HIP_BATCH_COLOR")
P_ONLY, A_ONLY, BOTH, STAGED = BC.P_ONLY, BC.A_ONLY, BC.BOTH, BC.STAGED


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _new_parts(k):
    """(P is new, A is new) for member k after the update"""
    return k in (P_ONLY, BOTH), k in (A_ONLY, BOTH)


def make_batch(fam, dtype, new, direct=False, finalize=True):
    """set_problem (values scaled in NumPy with the member's D, E, c), set_scaling_full, set_cones, set_params: no solve.  new: the members' new values
    where _new_parts says so (batch F), else the old ones everywhere (batch U)."""
    m, n = fam[0]["A"].shape
    B = _ffi.Batch(len(fam), n, m, 0, dtype=dtype)
    if direct:
        B.set_direct(True)
    bl, bu = [], []
    for k, c in enumerate(fam):
        nP, nA = _new_parts(k) if new else (False, False)
        Ps, As = BC.scaled_PA(fam, k, c["P2"] if nP else c["P"], c["A2"] if nA else c["A"], dtype)
        B.set_problem(k, Ps, c["q"], As, c["b"])
        D, E, cc = BC.scaling_of(fam, k)
        B.set_scaling_full(k, D, 1.0 / D, E, 1.0 / E, cc, 1.0 / cc)
        bl += [K.l for K in c["sets"] if K.kind == _ffi.BOX]; bu += [K.u for K in c["sets"] if K.kind == _ffi.BOX]
    B.set_cones([K.kind for K in fam[0]["sets"]], [K.dim for K in fam[0]["sets"]], np.concatenate(bl) if bl else None, np.concatenate(bu) if bu else None)
    if finalize:
        B.set_params(_params(dtype, direct))
    return B


def _params(dtype, direct):
    p = _ffi.default_params(dtype)
    p.kkt_kind = _ffi.KKT_DIRECT if direct else _ffi.KKT_CG
    p.tol_constant, p.tol_exponent = (1e-4, 0.0) if dtype == np.float32 else (1e-9, 0.0)
    p.adaptive_rho_interval = 10                              # rho adapts inside the 30 iterations below
    return p


def stage(U, fam, k, dtype, P2=None, A2=None):
    """stage member k's new values: P_ONLY raw with apply_scaling = 1, A_ONLY scaled here with apply_scaling = 0, BOTH raw with apply_scaling = 1"""
    c = fam[k]
    nP, nA = _new_parts(k)
    P2 = c["P2"] if P2 is None else P2
    A2 = c["A2"] if A2 is None else A2
    if k == A_ONLY:
        U.stage_matrices(k, None, BC.scaled_PA(fam, k, c["P"], A2, dtype)[1].data, apply_scaling=False)
    else:
        U.stage_matrices(k, P2.data if nP and c["P"].nnz else None, A2.data if nA else None, apply_scaling=True)


def bytes_of(B, k):
    return [B.get_matrix_values(k, w).tobytes() for w in ("A", "AT", "PT")] + [B.get_image(k).tobytes()]


def same_iterates(U, F, seed=23):
    rng = np.random.default_rng(seed)
    x0, s0, mu0 = rng.standard_normal(U.nprob * U.n), rng.standard_normal(U.nprob * U.m), rng.standard_normal(U.nprob * U.m)
    for B in (U, F):
        B.set_iterates(x0, s0, mu0); B.iterate(30, with_init=True)
    for k in range(U.nprob):
        for a, b in zip(U.get_iterates(k), F.get_iterates(k)):
            assert np.all(np.isfinite(a)) and np.array_equal(a, b), (k, float(np.max(np.abs(a - b))))


def purity(fam, dtype, reached, arrays, direct=False):
    U = make_batch(fam, dtype, new=False, direct=direct)
    F = make_batch(fam, dtype, new=True, direct=direct)
    info = U.kernel_info()
    assert reached(info) and reached(F.kernel_info()), info
    old = [bytes_of(U, k) for k in range(U.nprob)]
    counts0 = U.direct_counts() if direct else None
    for k in STAGED:
        stage(U, fam, k, dtype)
    assert [bytes_of(U, k) for k in range(U.nprob)] == old     # staging is host only
    U.apply_updates()
    ui = U.update_matrices_info()
    assert ui["updates"] == 1 and ui["host_rebuilds"] == 0 and ui["arrays_per_update"] == arrays and ui["map_bytes"] > 0, ui
    assert ui["last_bytes"] >= sum(fam[k]["P"].nnz + fam[k]["A"].nnz for k in STAGED) * np.dtype(dtype).itemsize
    assert U.kernel_info() == info
    for k in range(U.nprob):
        got, want = bytes_of(U, k), bytes_of(F, k)
        for name, g, w in zip(("A", "AT", "PT", "image"), got, want):
            assert g == w, (k, name)
        if k not in STAGED:
            assert got == old[k], k
        else:
            assert got != old[k], k
    if direct:
        counts1 = U.direct_counts()
        assert [int(counts1[k] - counts0[k]) for k in range(U.nprob)] == [1 if k in STAGED else 0 for k in range(U.nprob)]
        assert ui["factorizations"] == len(STAGED)
    same_iterates(U, F)
    return U, F


FORMS = {
    # name: (family, switches, dtype, what kernel_info() must say, destination arrays per update)
    "streaming": ("base", {"COSMO_HIP_BATCH_LDS": "0"}, np.float64, lambda i: i["form"] == "streaming", 3),
    "streaming_f32": ("base", {"COSMO_HIP_BATCH_LDS": "0"}, np.float32, lambda i: i["form"] == "streaming", 3),
    "lds_index_order": ("base", {"COSMO_HIP_BATCH_REG": "0"}, np.float64, lambda i: i["form"] == "lds_image" and not i["sorted_assignment"], 5),
    "lds_index_order_f32": ("base", {"COSMO_HIP_BATCH_REG": "0"}, np.float32, lambda i: i["form"] == "lds_image" and not i["sorted_assignment"], 5),
    "lds_sorted_storage": ("psd", {"COSMO_HIP_BATCH_REG": "0"}, np.float64, lambda i: i["form"] == "lds_image" and i["sorted_assignment"], 5),
    "lds_sorted_storage_f32": ("psd", {"COSMO_HIP_BATCH_REG": "0"}, np.float32, lambda i: i["form"] == "lds_image" and i["sorted_assignment"], 5),
    "register_sliced_P_in_image": ("base", {}, np.float64, lambda i: i["form"] == "register_1_2" and i["sliced"] and not i["p_in_registers"], 5),
    "register_sliced_P_in_registers": ("pdiag", {}, np.float64, lambda i: i["form"] == "register_1_2" and i["sliced"] and i["p_in_registers"], 5),
    "register_unsliced_f32": ("base", {}, np.float32, lambda i: i["form"] == "register_1_2" and not i["sliced"], 5),
    "register_long_rows": ("long", {}, np.float64, lambda i: i["form"] == "register_1_2" and i["long_rows"], 5),
    "register_2_4": ("tall", {}, np.float64, lambda i: i["form"] == "register_2_4", 5),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_updated_batch_equals_fresh_batch(monkeypatch, form):
    fam, env, dtype, reached, arrays = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                # read at set_params
    purity(BC.family(fam), dtype, reached, arrays)


def test_direct_batch_refactors_the_staged_members_only_and_reports_a_nonconvex_member():
    fam = BC.family("base")
    dtype = np.float64
    U, F = purity(fam, dtype, lambda i: i["form"] == "streaming", 4, direct=True)
    # P2 = -P on member BOTH: the inertia test of its new factor fails, the call says which member, the others hold F's bits
    counts0 = U.direct_counts()
    neg = fam[BOTH]["P2"].copy(); neg.data *= -1.0
    U.stage_matrices(BOTH, neg.data, None, apply_scaling=True)
    with pytest.raises(_ffi.CosmoHipError) as e:
        U.apply_updates()
    assert _ffi.ERR_NAMES.get(e.value.code) == "INVALID" and "not convex" in str(e.value) and "member %d" % BOTH in str(e.value), str(e.value)
    assert [int(x) for x in U.direct_counts() - counts0] == [1 if k == BOTH else 0 for k in range(U.nprob)]
    for k in range(U.nprob):
        if k != BOTH:
            assert bytes_of(U, k) == bytes_of(F, k), k
    assert bytes_of(U, BOTH) != bytes_of(F, BOTH)
    # a valid update of that member restores it
    U.stage_matrices(BOTH, fam[BOTH]["P2"].data, None, apply_scaling=True)
    U.apply_updates()
    for k in range(U.nprob):
        assert bytes_of(U, k) == bytes_of(F, k), k
    same_iterates(U, F, seed=29)


def test_bad_calls():
    fam = BC.family("base")
    c = fam[0]
    B = make_batch(fam, np.float64, new=False, finalize=False)
    with pytest.raises(_ffi.CosmoHipError) as e:
        B.stage_matrices(0, c["P2"].data, c["A2"].data)            # before set_params
    assert _ffi.ERR_NAMES.get(e.value.code) == "INVALID"
    B.set_params(_params(np.float64, False))
    for k in (-1, len(fam)):
        with pytest.raises(_ffi.CosmoHipError) as e:
            B.stage_matrices(k, c["P2"].data, c["A2"].data, apply_scaling=True)      # k out of range
        assert _ffi.ERR_NAMES.get(e.value.code) == "INVALID"
    old = bytes_of(B, 0)
    B.stage_matrices(0, None, None)                                # NULL for both: a no-op
    B.apply_updates()
    assert B.update_matrices_info()["updates"] == 0 and bytes_of(B, 0) == old
    # update_matrices = stage + apply for a list of members, the value arrays one after the other
    F = make_batch(fam, np.float64, new=True)
    mem = [BOTH, P_ONLY]
    B.update_matrices(mem, np.concatenate([fam[k]["P2"].data for k in mem]), np.concatenate([fam[BOTH]["A2"].data, fam[P_ONLY]["A"].data]), apply_scaling=True)
    for k in mem:
        assert bytes_of(B, k) == bytes_of(F, k), k
    assert B.update_matrices_info()["updates"] == 1
