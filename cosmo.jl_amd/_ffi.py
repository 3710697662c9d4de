"""ctypes binding of libcosmo_hip.so (include/cosmo_hip.h).

This is the same C ABI a Julia `ccall` layer binds (julia/CosmoHIP.jl); the Python binding
exists because Julia is not installed in this image.  There is NO CPU fallback: if the shared library is
missing, or no HIP device is visible, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcosmo_hip.so")            # cosmo_hip_real = double (COSMO.Model{Float64})
LIB_PATH_F32 = os.path.join(_HERE, "libcosmo_hip_f32.so")     # the same sources, cosmo_hip_real = float (COSMO.Model{Float32})

OK = 0
ERR_NAMES = {1: "INVALID", 2: "HIP", 5: "EIG", 6: "UNSUPPORTED", 7: "COMM"}

ZERO, NONNEG, BOX, SOC, PSD_SQUARE, PSD_TRIANGLE = 0, 1, 2, 3, 4, 5
EXP, DUAL_EXP, POW, DUAL_POW = 6, 7, 8, 9
PSD_TRIANGLE_COMPLEX = 10
CUSTOM = 11
KKT_CG, KKT_MINRES_REDUCED, KKT_MINRES, KKT_CG_SR, KKT_CG_JACOBI = 0, 1, 2, 3, 4
KKT_DIRECT = 5          # QdldlKKTSolver: supernodal LDL' of the full KKT matrix on the device (csrc/ldl.hip)
KKT_SCHUR = 6           # exact solve of the reduced system: block-diagonal part + dense capacitance inverse (csrc/schur.hip)
STATUS_NAMES = {0: "Undetermined", 1: "Solved", 2: "Max_iter_reached", 3: "Unsolved", 4: "Primal_infeasible",
                5: "Dual_infeasible", 6: "Time_limit_reached"}
MAT_A, MAT_AT, MAT_P, MAT_OP = 0, 1, 2, 3
MAX_RHO_UPDATES = 64
NUM_KERNEL_CLASSES = 16


from ._abi_structs import ABI_VERSION, AccelParams, Params, ResultStruct   # noqa: E402  generated from include/cosmo_hip.h (tools/gen_abi_structs.py)

ACCEL_EMPTY, ACCEL_ANDERSON = 0, 1
PSD_PROJECTION_SIGN, PSD_PROJECTION_EIGEN = 0, 1
# the non-default variants of docs/src/acceleration.md:23 (include/cosmo_hip.h: COSMO_HIP_ACCEL_ANDERSON_*)
ACCEL_ANDERSON_TYPE1_RESTARTED, ACCEL_ANDERSON_TYPE1_ROLLING, ACCEL_ANDERSON_TYPE2NE_RESTARTED, ACCEL_ANDERSON_TYPE2NE_ROLLING = 2, 3, 4, 5


class CosmoHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libcosmo_hip error %d (%s): %s" % (code, ERR_NAMES.get(code, "?"), msg))
        self.code = code


_libs = {}

_PD = C.POINTER(C.c_double)
_PF = C.POINTER(C.c_float)


class _RealPtr:
    """Placeholder in SIGNATURES for `cosmo_hip_real*` (include/cosmo_hip.h): resolved to double* or float* when a library is loaded."""


_PR = _RealPtr
_PI64 = C.POINTER(C.c_int64)
_PI32 = C.POINTER(C.c_int32)

# name -> (restype, argtypes).  Kept in one table so tests can check it against the header.
PROJECT_FN = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int64, C.c_void_p)                       # cosmo_hip_project_fn
CONE_TEST_FN = C.CFUNCTYPE(C.c_int32, C.POINTER(C.c_double), C.c_int64, C.c_double, C.c_void_p)     # cosmo_hip_cone_test_fn
PROJECT_FN_F32 = C.CFUNCTYPE(None, C.POINTER(C.c_float), C.c_int64, C.c_void_p)
CONE_TEST_FN_F32 = C.CFUNCTYPE(C.c_int32, C.POINTER(C.c_float), C.c_int64, C.c_double, C.c_void_p)

SIGNATURES = {
    "cosmo_hip_version": (C.c_int32, []),
    "cosmo_hip_default_params": (None, [C.POINTER(Params)]),
    "cosmo_hip_create": (C.c_int32, [C.POINTER(C.c_void_p), C.c_int32]),
    "cosmo_hip_destroy": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_last_error": (C.c_char_p, [C.c_void_p]),
    "cosmo_hip_set_problem": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, _PI64, _PI64, _PR, _PI64, _PI64, _PR, _PR, _PR]),
    "cosmo_hip_set_cones": (C.c_int32, [C.c_void_p, C.c_int64, _PI32, _PI64, _PR, _PR]),
    "cosmo_hip_set_cones_ex": (C.c_int32, [C.c_void_p, C.c_int64, _PI32, _PI64, _PR, _PR, _PR]),
    "cosmo_hip_set_custom_cone": (C.c_int32, [C.c_void_p, C.c_int64, PROJECT_FN, CONE_TEST_FN, CONE_TEST_FN, C.c_void_p]),
    "cosmo_hip_set_params": (C.c_int32, [C.c_void_p, C.POINTER(Params), _PR]),
    "cosmo_hip_update_rho": (C.c_int32, [C.c_void_p, _PR]),
    "cosmo_hip_set_scaling": (C.c_int32, [C.c_void_p, _PR, _PR, C.c_double]),
    "cosmo_hip_set_scaling_full": (C.c_int32, [C.c_void_p, _PR, _PR, _PR, _PR, C.c_double, C.c_double]),
    "cosmo_hip_default_accel_params": (None, [C.POINTER(AccelParams)]),
    "cosmo_hip_set_accelerator": (C.c_int32, [C.c_void_p, C.POINTER(AccelParams)]),
    "cosmo_hip_get_accel_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_get_accel_restarts": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_accel_pre": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, _PI64, _PR, _PR, _PR]),
    "cosmo_hip_accel_post": (C.c_int32, [C.c_void_p, _PR, _PR, _PI32, _PR]),
    "cosmo_hip_accel_restart": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_scale_ruiz": (C.c_int32, [C.c_void_p, C.c_int64, C.c_double, C.c_double, _PR, _PR, _PD]),
    "cosmo_hip_update_qb": (C.c_int32, [C.c_void_p, _PR, _PR]),
    "cosmo_hip_update_matrices": (C.c_int32, [C.c_void_p, _PR, _PR, C.c_int32]),
    "cosmo_hip_update_matrices_info": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_get_rho_classes": (C.c_int32, [C.c_void_p, _PI32]),
    "cosmo_hip_get_rho_vec": (C.c_int32, [C.c_void_p, _PR]),
    "cosmo_hip_kkt_solve": (C.c_int32, [C.c_void_p, _PR, _PR, _PI64]),
    "cosmo_hip_project": (C.c_int32, [C.c_void_p, _PR, _PI64, _PI32]),
    "cosmo_hip_spmv": (C.c_int32, [C.c_void_p, C.c_int32, _PR, _PR]),
    "cosmo_hip_set_iterates": (C.c_int32, [C.c_void_p, _PR, _PR, _PR]),
    "cosmo_hip_check_certificates": (C.c_int32, [C.c_void_p, _PR, _PR, _PI32]),
    "cosmo_hip_admm_init": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_admm_iterate": (C.c_int32, [C.c_void_p, C.c_int64]),
    "cosmo_hip_admm_iterate_checked": (C.c_int32, [C.c_void_p, C.c_int64, _PI32]),
    "cosmo_hip_residuals": (C.c_int32, [C.c_void_p, _PD]),
    "cosmo_hip_optimize": (C.c_int32, [C.c_void_p, C.POINTER(ResultStruct)]),
    "cosmo_hip_get_iterates": (C.c_int32, [C.c_void_p, _PR, _PR, _PR, _PR]),
    "cosmo_hip_cg_persist_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_fold_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_kkt_recurrence": (C.c_char_p, [C.c_void_p]),
    "cosmo_hip_ldl_analyze": (C.c_int32, [C.c_int64, C.c_int64, _PI64, _PI64, _PI64, _PI64, _PI64, _PI64]),
    "cosmo_hip_set_kkt_perm": (C.c_int32, [C.c_void_p, C.c_int64, _PI64]),
    "cosmo_hip_direct_info": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_set_schur_options": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32]),
    "cosmo_hip_schur_analyze": (C.c_int32, [C.c_int64, C.c_int64, _PI64, _PI64, _PI64, _PI64, C.c_int32, _PI64]),
    "cosmo_hip_schur_info": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_schur_residual": (C.c_int32, [C.c_void_p, C.POINTER(C.c_double)]),
    "cosmo_hip_polar_dataflow_stats": (C.c_int32, [C.c_void_p, _PD]),
    "cosmo_hip_polar_dataflow_reset_timing": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_get_kkt_solution": (C.c_int32, [C.c_void_p, _PR]),
    "cosmo_hip_get_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_set_setup_time": (C.c_int32, [C.c_void_p, C.c_double]),
    "cosmo_hip_get_rho_interval": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_time_spmv": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _PD, _PD]),
    "cosmo_hip_set_profiling": (C.c_int32, [C.c_void_p, C.c_int32]),
    "cosmo_hip_get_kernel_times": (C.c_int32, [C.c_void_p, _PD, _PI64]),
    "cosmo_hip_kernel_class_name": (C.c_char_p, [C.c_int32]),
    "cosmo_hip_psd_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_set_psd_projection": (C.c_int32, [C.c_void_p, C.c_int32]),
    "cosmo_hip_polar_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_polar_streamk_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_polar_schedule": (C.c_int32, [C.c_int32, _PD, _PI32]),
    "cosmo_hip_time_psd_product": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _PD, _PD]),
    "cosmo_hip_comm_unique_id": (C.c_int32, [C.POINTER(C.c_uint8)]),
    "cosmo_hip_comm_init": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "cosmo_hip_comm_destroy": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_set_cone_shard": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_polar_depth_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_time_krylov": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "cosmo_hip_comm_selftest": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_comm_allreduce_check": (C.c_int32, [C.c_void_p, C.c_int64, _PI64]),
    "cosmo_hip_comm_init_hostshm": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p]),
    "cosmo_hip_comm_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_set_cone_ownership": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64]),
    "cosmo_hip_set_row_shard": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_row_shard_info": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_comm_stats_ex": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_create": (C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int64, C.c_int64]),
    "cosmo_hip_batch_destroy": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_batch_last_error": (C.c_char_p, [C.c_void_p]),
    "cosmo_hip_batch_set_problem": (C.c_int32, [C.c_void_p, C.c_int64, _PI64, _PI64, _PR, _PI64, _PI64, _PR, _PR, _PR]),
    "cosmo_hip_batch_set_cones": (C.c_int32, [C.c_void_p, C.c_int64, _PI32, _PI64, _PR, _PR]),
    "cosmo_hip_batch_set_cones_ex": (C.c_int32, [C.c_void_p, C.c_int64, _PI32, _PI64, _PR, _PR, _PR]),
    "cosmo_hip_batch_set_scaling": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, C.c_double]),
    "cosmo_hip_batch_set_params": (C.c_int32, [C.c_void_p, C.POINTER(Params)]),
    "cosmo_hip_batch_set_accelerator": (C.c_int32, [C.c_void_p, C.POINTER(AccelParams)]),
    "cosmo_hip_batch_get_accel_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_get_rho_classes": (C.c_int32, [C.c_void_p, C.c_int64, _PI32]),
    "cosmo_hip_batch_set_iterates": (C.c_int32, [C.c_void_p, _PR, _PR, _PR]),
    "cosmo_hip_batch_check_certificates": (C.c_int32, [C.c_void_p, _PR, _PR, _PI32]),
    "cosmo_hip_batch_optimize": (C.c_int32, [C.c_void_p, C.POINTER(ResultStruct)]),
    "cosmo_hip_batch_iterate": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32]),
    "cosmo_hip_batch_get_iterates": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, _PR, _PR]),
    "cosmo_hip_batch_get_counters": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_kernel_info": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_set_direct": (C.c_int32, [C.c_void_p, C.c_int32, _PI64]),
    "cosmo_hip_batch_set_psd_side_max": (C.c_int32, [C.c_void_p, C.c_int32]),
    "cosmo_hip_batch_direct_info": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_direct_counts": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_polish": (C.c_int32, [C.c_void_p, C.c_double, C.c_int32]),
    "cosmo_hip_batch_polish_info": (C.c_int32, [C.c_void_p, _PI32, _PD]),
    "cosmo_hip_batch_set_scaling_full": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, _PR, _PR, C.c_double, C.c_double]),
    "cosmo_hip_batch_stage_qb": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR]),
    "cosmo_hip_batch_apply_updates": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_batch_update_qb": (C.c_int32, [C.c_void_p, C.c_int64, _PI64, _PR, _PR]),
    "cosmo_hip_batch_warm_restart": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_batch_get_qb": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR]),
    "cosmo_hip_batch_update_qb_device": (C.c_int32, [C.c_void_p, C.c_int64, _PI64, _PR, _PR, C.c_void_p]),
    "cosmo_hip_batch_set_iterates_device": (C.c_int32, [C.c_void_p, _PR, _PR, _PR, C.c_void_p]),
    "cosmo_hip_batch_get_solution_device": (C.c_int32, [C.c_void_p, _PR, _PR, _PR, C.c_void_p]),
    "cosmo_hip_batch_stage_matrices": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, C.c_int32]),
    "cosmo_hip_batch_update_matrices": (C.c_int32, [C.c_void_p, C.c_int64, _PI64, _PR, _PR, C.c_int32]),
    "cosmo_hip_batch_update_matrices_info": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_get_matrix_values": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32, _PR]),
    "cosmo_hip_batch_get_image": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, _PI64]),
    "cosmo_hip_batch_scale_ruiz": (C.c_int32, [C.c_void_p, C.c_int64, C.c_double, C.c_double]),
    "cosmo_hip_batch_get_scaling": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, _PD]),
    "cosmo_hip_batch_get_scaled_problem": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, _PR, _PR, _PR, _PR]),
    "cosmo_hip_batch_ruiz_info": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_group_create": (C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64]),
    "cosmo_hip_batch_group_destroy": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_batch_group_last_error": (C.c_char_p, [C.c_void_p]),
    "cosmo_hip_batch_group_set_problem": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, _PI64, _PI64, _PR, _PI64, _PI64, _PR, _PR, _PR]),
    "cosmo_hip_batch_group_set_cones": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, _PI32, _PI64, _PR, _PR, _PR]),
    "cosmo_hip_batch_group_set_scaling": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, C.c_double]),
    "cosmo_hip_batch_group_set_scaling_full": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, _PR, _PR, C.c_double, C.c_double]),
    "cosmo_hip_batch_group_set_accelerator": (C.c_int32, [C.c_void_p, C.POINTER(AccelParams)]),
    "cosmo_hip_batch_group_set_direct": (C.c_int32, [C.c_void_p, C.c_int32]),
    "cosmo_hip_batch_group_set_psd_side_max": (C.c_int32, [C.c_void_p, C.c_int32]),
    "cosmo_hip_batch_group_set_schur_options": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32]),
    "cosmo_hip_batch_group_set_device_scaling": (C.c_int32, [C.c_void_p, C.c_int64, C.c_double, C.c_double]),
    "cosmo_hip_batch_group_get_scaling": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, _PD]),
    "cosmo_hip_batch_group_set_params": (C.c_int32, [C.c_void_p, C.POINTER(Params)]),
    "cosmo_hip_batch_group_class_info": (C.c_int32, [C.c_void_p, _PI64, _PI64, _PI64]),
    "cosmo_hip_batch_group_run_info": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_group_get_rho_interval": (C.c_int32, [C.c_void_p, C.c_int64, _PI64]),
    "cosmo_hip_batch_group_set_iterates": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, _PR]),
    "cosmo_hip_batch_group_optimize": (C.c_int32, [C.c_void_p, C.POINTER(ResultStruct)]),
    "cosmo_hip_batch_group_get_iterates": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, _PR, _PR]),
    "cosmo_hip_batch_group_get_counters": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_group_get_accel_stats": (C.c_int32, [C.c_void_p, _PI64]),
    "cosmo_hip_batch_group_stage_qb": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR]),
    "cosmo_hip_batch_group_stage_matrices": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR, C.c_int32]),
    "cosmo_hip_batch_group_apply_updates": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_batch_group_warm_restart": (C.c_int32, [C.c_void_p]),
    "cosmo_hip_batch_group_get_qb": (C.c_int32, [C.c_void_p, C.c_int64, _PR, _PR]),
}


def _is_f32(dtype):
    return np.dtype(dtype) == np.float32


def ldl_analyze(n, m, P, A, perm=None, dtype=np.float64):
    """cosmo_hip_ldl_analyze: symbolic analysis of K = [P + sigma I, A'; A, -diag(1 ./ rho)] on the host (no GPU needed).  P, A: scipy sparse
    (pattern only).  Returns a dict with the eight figures of include/cosmo_hip.h."""
    import scipy.sparse as sp
    lib = load_library(dtype)
    P = sp.csc_matrix(P); A = sp.csc_matrix(A)
    Pp = P.indptr.astype(np.int64); Pi = P.indices.astype(np.int64)
    Ap = A.indptr.astype(np.int64); Ai = A.indices.astype(np.int64)
    pr = None if perm is None else np.ascontiguousarray(perm, dtype=np.int64)
    if pr is not None and pr.size != n + m:
        raise ValueError("perm must have n + m = %d entries" % (n + m))
    out = np.zeros(8, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(_PI64)
    rc = lib.cosmo_hip_ldl_analyze(int(n), int(m), ptr(Pp), ptr(Pi), ptr(Ap), ptr(Ai), None if pr is None else ptr(pr), ptr(out))
    if rc != 0:
        raise CosmoHipError(rc, "cosmo_hip_ldl_analyze failed (bad pattern or permutation)")
    keys = ["nnz_L", "nnz_stored", "supernodes", "height", "max_width", "amalgamation_zeros", "panel_size", "update_pairs"]
    return dict(zip(keys, out.tolist()))


SCHUR_PLAN_KEYS = ["nd", "components", "largest", "sum_size2", "nnz_W"]


def schur_analyze(n, m, P, A, row_threshold=0, dtype=np.float64):
    """cosmo_hip_schur_analyze: the split of the Schur-complement KKT solver on the host (no GPU needed).  P, A: scipy sparse (pattern only; stored
    entries count, also explicit zeros).  Returns a dict with the eight figures of include/cosmo_hip.h."""
    import scipy.sparse as sp
    lib = load_library(dtype)
    P = sp.csc_matrix(P); A = sp.csc_matrix(A)
    Pp = P.indptr.astype(np.int64); Pi = P.indices.astype(np.int64)
    Ap = A.indptr.astype(np.int64); Ai = A.indices.astype(np.int64)
    out = np.zeros(8, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(_PI64)
    rc = lib.cosmo_hip_schur_analyze(int(n), int(m), ptr(Pp), ptr(Pi), ptr(Ap), ptr(Ai), int(row_threshold), ptr(out))
    if rc != 0:
        raise CosmoHipError(rc, "cosmo_hip_schur_analyze failed (bad pattern)")
    return dict(zip(SCHUR_PLAN_KEYS + ["dense_bytes", "accepted", "small_components"], out.tolist()))


def load_library(dtype=np.float64):
    """Loads libcosmo_hip.so (dtype float64) or libcosmo_hip_f32.so (float32), both built by `__graft_entry__.build()` /
    `make -C cosmo.jl_amd/csrc` from the same sources.  Raises if absent."""
    f32 = _is_f32(dtype)
    if f32 in _libs:
        return _libs[f32]
    path = LIB_PATH_F32 if f32 else LIB_PATH
    if not os.path.exists(path):
        raise ImportError("%s not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback." % (os.path.basename(path), path))
    try:
        # torch bundles its own libamdhip64; if it is going to live in this process (tests, bench: torch.distributed,
        # device selection) it must be loaded FIRST so that both share one HIP runtime.  Pure plumbing: no torch
        # symbol is used by the library, and the binding works without torch installed.
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path)
    preal = _PF if f32 else _PD
    fnmap = {PROJECT_FN: PROJECT_FN_F32, CONE_TEST_FN: CONE_TEST_FN_F32} if f32 else {}
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = [preal if a is _PR else fnmap.get(a, a) for a in args]
    got = int(lib.cosmo_hip_version())
    if got != ABI_VERSION:
        raise ImportError("%s reports ABI version %d, these bindings were generated for %d (include/cosmo_hip.h) -- rebuild the library "
                          "(`make -C cosmo.jl_amd/csrc`) or regenerate the bindings (`python tools/gen_abi_structs.py`)"
                          % (os.path.basename(path), got, ABI_VERSION))
    _libs[f32] = lib
    return lib


def _dp(a):
    """pointer to a data array in ITS element type (the arrays handed to a library are made with that library's dtype)"""
    return None if a is None else a.ctypes.data_as(_PF if a.dtype == np.float32 else _PD)


def _f64(a, n=None, name="array", dtype=np.float64):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if n is not None and a.size != n:
        raise ValueError("%s has length %d, expected %d" % (name, a.size, n))
    return a


def csc_julia(M, dtype=np.float64):
    """SciPy sparse -> the arrays of a Julia SparseMatrixCSC{T,Int64} (1-based, sorted rows), T = Float64 | Float32."""
    import scipy.sparse as sp
    # copy: a dtype conversion copies `data` but may SHARE `indices` with the caller's matrix; sorting the indices in place would
    # then permute the caller's index array without its values
    M = sp.csc_matrix(M, dtype=dtype, copy=True)
    M.sum_duplicates()
    M.sort_indices()
    colptr = np.ascontiguousarray(M.indptr, dtype=np.int64) + 1
    rowval = np.ascontiguousarray(M.indices, dtype=np.int64) + 1
    nzval = np.ascontiguousarray(M.data, dtype=dtype)
    return colptr, rowval, nzval


def check_device_tensor(t, shape, dtype, device, name="tensor"):
    """The argument check of the device-memory entry points (Batch.update_qb_device, ...): `t` is a torch tensor of exactly `shape`, of the
    library's element type `dtype` (numpy float64 / float32), contiguous, on `device` (a torch.device).  ValueError otherwise, before any
    pointer reaches the library; None passes (the entry points take NULL)."""
    if t is None:
        return None
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch tensor on %s, got %s" % (name, device, type(t).__name__))
    want = torch.float32 if _is_f32(dtype) else torch.float64
    if t.dtype != want:
        raise ValueError("%s has dtype %s, the batch computes in %s" % (name, t.dtype, want))
    if tuple(t.shape) != tuple(int(v) for v in shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(int(v) for v in shape)))
    if not t.is_contiguous():
        raise ValueError("%s is not contiguous" % name)
    dev = torch.device(device)
    if t.device.type != dev.type or (dev.index is not None and t.device.index != dev.index):
        raise ValueError("%s lives on %s, the batch on %s (device memory only: there is no host path behind this call)" % (name, t.device, dev))
    return t


def default_params(dtype=np.float64):
    p = Params()
    load_library(dtype).cosmo_hip_default_params(C.byref(p))
    return p


class Handle:
    """Thin object wrapper: one method per C entry point, NumPy arrays in and out."""

    def __init__(self, device=0, dtype=np.float64):
        self.dtype = np.dtype(np.float32 if _is_f32(dtype) else np.float64)      # element type of every data array (cosmo_hip_real)
        self.lib = load_library(self.dtype)
        self._h = C.c_void_p()
        rc = self.lib.cosmo_hip_create(C.byref(self._h), int(device))
        if rc != OK:
            raise CosmoHipError(rc, "cosmo_hip_create failed (no MI355X visible? this library has no CPU path)")
        self.n = self.m = 0
        self.nnz_P = self.nnz_A = 0
        self.ncones = 0
        self._callbacks = {}

    def _f(self, a, n=None, name="array"):
        return _f64(a, n, name, self.dtype)

    def close(self):
        if self._h:
            self.lib.cosmo_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            msg = self.lib.cosmo_hip_last_error(self._h)
            raise CosmoHipError(rc, msg.decode() if msg else "")

    # ---- problem ----------------------------------------------------------------------------------------
    def set_problem(self, P, q, A, b):
        m, n = A.shape
        pc, pr, pv = csc_julia(P, self.dtype)
        ac, ar, av = csc_julia(A, self.dtype)
        q = self._f(q, n, "q"); b = self._f(b, m, "b")
        self._chk(self.lib.cosmo_hip_set_problem(self._h, n, m, pc.ctypes.data_as(_PI64), pr.ctypes.data_as(_PI64), _dp(pv),
                                                 ac.ctypes.data_as(_PI64), ar.ctypes.data_as(_PI64), _dp(av), _dp(q), _dp(b)))
        self.n, self.m = n, m
        self.nnz_P, self.nnz_A = int(pv.size), int(av.size)

    def set_cones(self, types, dims, box_l=None, box_u=None, cone_param=None):
        t = np.ascontiguousarray(types, dtype=np.int32)
        d = np.ascontiguousarray(dims, dtype=np.int64)
        bl = self._f(box_l); bu = self._f(box_u)
        if cone_param is None:
            self._chk(self.lib.cosmo_hip_set_cones(self._h, t.size, t.ctypes.data_as(_PI32), d.ctypes.data_as(_PI64), _dp(bl), _dp(bu)))
        else:
            cp = self._f(cone_param, t.size, "cone_param")
            self._chk(self.lib.cosmo_hip_set_cones_ex(self._h, t.size, t.ctypes.data_as(_PI32), d.ctypes.data_as(_PI64), _dp(bl), _dp(bu), _dp(cp)))
        self.ncones = t.size
        self._callbacks = {}

    def set_custom_cone(self, cone, project, in_dual=None, in_pol_recc=None):
        """cosmo_hip_set_custom_cone: `project(x)` projects the NumPy view x (the cone's slice) in place; `in_dual(x, tol)` /
        `in_pol_recc(x, tol)` return truth values (optional).  The ctypes thunks are kept alive on the handle."""
        def _view(ptr, dim):
            return np.ctypeslib.as_array(ptr, shape=(int(dim),)) if dim > 0 else np.zeros(0, dtype=self.dtype)

        def _proj(ptr, dim, _user):
            project(_view(ptr, dim))

        def _mk(fn):
            if fn is None:
                return test_t(0)
            return test_t(lambda ptr, dim, tol, _user: 1 if fn(_view(ptr, dim), float(tol)) else 0)

        f32 = self.dtype == np.float32
        proj_t, test_t = (PROJECT_FN_F32, CONE_TEST_FN_F32) if f32 else (PROJECT_FN, CONE_TEST_FN)
        thunks = (proj_t(_proj), _mk(in_dual), _mk(in_pol_recc))
        self._callbacks[int(cone)] = thunks
        self._chk(self.lib.cosmo_hip_set_custom_cone(self._h, int(cone), thunks[0], thunks[1], thunks[2], None))

    def default_params(self):
        return default_params(self.dtype)

    def set_params(self, params, rho_vec=None):
        rv = self._f(rho_vec, self.m, "rho_vec")
        self._chk(self.lib.cosmo_hip_set_params(self._h, C.byref(params), _dp(rv)))

    def update_rho(self, rho_vec):
        rv = self._f(rho_vec, self.m, "rho_vec")
        self._chk(self.lib.cosmo_hip_update_rho(self._h, _dp(rv)))

    def set_accelerator(self, kind=ACCEL_ANDERSON, mem=15, min_mem=3, safeguard=True, safeguard_tol=2.0, start_iter=2, start_accuracy=None, eta_max=None):
        """`_make_accelerator!` (src/setup.jl:10-16); kind ACCEL_EMPTY removes it."""
        ap = AccelParams()
        self.lib.cosmo_hip_default_accel_params(C.byref(ap))
        ap.kind, ap.mem, ap.min_mem, ap.safeguard = int(kind), int(mem), int(min_mem), 1 if safeguard else 0
        ap.safeguard_tol, ap.start_iter = float(safeguard_tol), int(start_iter)
        if start_accuracy is not None:
            ap.start_accuracy = float(start_accuracy)
        if eta_max is not None:
            ap.eta_max = float(eta_max)
        self._chk(self.lib.cosmo_hip_set_accelerator(self._h, C.byref(ap)))

    # ---- the accelerator one step at a time (the functions the accelerated loop calls, on given vectors; they overwrite the iterates) ----
    ACCEL_PRE_INFO = ("attempted", "success", "l", "j", "restarts", "fail_singular", "fail_eta", "active", "mem")

    def accel_pre(self, it, g, x):
        """acceleration_pre! at loop index `it` on g = w, x = w_prev (length n + m).  Returns (candidate, info): info holds the ACCEL_PRE_INFO
        integers, nrm_f, eta_norm, eta (mem) and R (mem x mem: the triangular factor, or M = L'F of the normal-equations variants)."""
        N = self.n + self.m
        w = np.array(self._f(g, N, "g"), copy=True)
        wp = self._f(x, N, "x")
        out = np.zeros(9, dtype=np.int64)
        scal = np.zeros(2, dtype=self.dtype)
        eta = np.zeros(32, dtype=self.dtype); R = np.zeros(32 * 32, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_accel_pre(self._h, int(it), _dp(w), _dp(wp), out.ctypes.data_as(_PI64), _dp(scal), _dp(eta), _dp(R)))
        info = {k: int(v) for k, v in zip(self.ACCEL_PRE_INFO, out)}
        mem = info["mem"]
        info.update(nrm_f=scal[0], eta_norm=scal[1], eta=eta[:mem].copy(), R=R[:mem * mem].reshape(mem, mem).T.copy())
        return w, info

    def accel_post(self, w, w_prev):
        """acceleration_post! on the vectors after the ADMM step: (w, w_prev, declined, nrm_f_acc); a declined candidate is reset."""
        N = self.n + self.m
        w = np.array(self._f(w, N, "w"), copy=True)
        wp = np.array(self._f(w_prev, N, "w_prev"), copy=True)
        dec = C.c_int32(0)
        na = np.zeros(1, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_accel_post(self._h, _dp(w), _dp(wp), C.byref(dec), _dp(na)))
        return w, wp, int(dec.value), na[0]

    def accel_restart(self):
        """CA.restart! (what a rho adaption calls): empties the history."""
        self._chk(self.lib.cosmo_hip_accel_restart(self._h))

    def accel_restarts(self):
        """(restarts because the memory was full, restarts because rho was adapted) of the last optimize"""
        out = np.zeros(2, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_get_accel_restarts(self._h, out.ctypes.data_as(_PI64)))
        return int(out[0]), int(out[1])

    def set_psd_projection(self, mode):
        """0 = verified matrix-sign iteration above side 16 (default), 1 = eigendecomposition (Jacobi) at every side; after set_cones."""
        self._chk(self.lib.cosmo_hip_set_psd_projection(self._h, int(mode)))

    def accel_stats(self):
        out = np.zeros(6, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_get_accel_stats(self._h, out.ctypes.data_as(_PI64)))
        return dict(accelerated=int(out[0]), accepted=int(out[1]), declined=int(out[2]), restarts=int(out[3]), active=bool(out[4]),
                    safeguarding_iter=int(out[5]))

    def scale_ruiz(self, iterations, min_scaling=1e-4, max_scaling=1e4):
        """Device Ruiz equilibration of the resident (unscaled) problem; returns (D, E, c)."""
        D = np.empty(self.n, dtype=self.dtype); E = np.empty(self.m, dtype=self.dtype); c = C.c_double(1.0)
        self._chk(self.lib.cosmo_hip_scale_ruiz(self._h, int(iterations), float(min_scaling), float(max_scaling), _dp(D), _dp(E), C.byref(c)))
        return D, E, float(c.value)

    def set_scaling(self, Dinv, Einv, cinv):
        self._chk(self.lib.cosmo_hip_set_scaling(self._h, _dp(self._f(Dinv, self.n)), _dp(self._f(Einv, self.m)), float(cinv)))

    def set_scaling_full(self, D, Dinv, E, Einv, c, cinv):
        self._chk(self.lib.cosmo_hip_set_scaling_full(self._h, _dp(self._f(D, self.n)), _dp(self._f(Dinv, self.n)), _dp(self._f(E, self.m)),
                                                      _dp(self._f(Einv, self.m)), float(c), float(cinv)))

    def update_qb(self, q=None, b=None):
        self._chk(self.lib.cosmo_hip_update_qb(self._h, _dp(self._f(q, self.n)), _dp(self._f(b, self.m))))

    def update_matrices(self, P_data=None, A_data=None, apply_scaling=False):
        """cosmo_hip_update_matrices: new values of the stored entries of P / A in the order of the CSC arrays set_problem passed (csc_julia: sorted
        row indices); None = unchanged.  apply_scaling: the handle's D, E, c are applied on the device (the values are the unscaled ones)."""
        self._chk(self.lib.cosmo_hip_update_matrices(self._h, _dp(self._f(P_data, self.nnz_P, "P_data")), _dp(self._f(A_data, self.nnz_A, "A_data")), 1 if apply_scaling else 0))

    def update_matrices_info(self):
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_update_matrices_info(self._h, out.ctypes.data_as(_PI64)))
        return dict(updates=int(out[0]), refreshed_arrays=int(out[1]), host_rebuilds=int(out[2]), bytes_uploaded=int(out[3]), map_bytes=int(out[4]),
                    analyses=int(out[5]))

    def get_rho_classes(self):
        out = np.empty(self.m, dtype=np.int32)
        self._chk(self.lib.cosmo_hip_get_rho_classes(self._h, out.ctypes.data_as(_PI32)))
        return out

    def get_rho_vec(self):
        out = np.empty(self.m, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_get_rho_vec(self._h, _dp(out)))
        return out

    # ---- fine-grained ---------------------------------------------------------------------------------------
    def kkt_solve(self, rhs):
        rhs = self._f(rhs, self.n + self.m, "rhs")
        lhs = np.empty(self.n + self.m, dtype=self.dtype)
        it = C.c_int64(0)
        self._chk(self.lib.cosmo_hip_kkt_solve(self._h, _dp(lhs), _dp(rhs), C.byref(it)))
        return lhs, it.value

    def project(self, s):
        s = np.array(s, dtype=self.dtype).copy()
        ranks = np.empty(max(self.ncones, 1), dtype=np.int64)
        br = np.empty(max(self.ncones, 1), dtype=np.int32)
        self._chk(self.lib.cosmo_hip_project(self._h, _dp(s), ranks.ctypes.data_as(_PI64), br.ctypes.data_as(_PI32)))
        return s, ranks[:self.ncones], br[:self.ncones]

    def spmv(self, which, x):
        nin = {MAT_A: self.n, MAT_AT: self.m, MAT_P: self.n}[which]
        nout = {MAT_A: self.m, MAT_AT: self.n, MAT_P: self.n}[which]
        x = self._f(x, nin, "x")
        y = np.empty(nout, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_spmv(self._h, which, _dp(y), _dp(x)))
        return y

    # ---- loop -------------------------------------------------------------------------------------------------
    def set_iterates(self, x0=None, s0=None, mu0=None):
        self._chk(self.lib.cosmo_hip_set_iterates(self._h, _dp(self._f(x0, self.n)), _dp(self._f(s0, self.m)), _dp(self._f(mu0, self.m))))

    def check_certificates(self, dx, dy):
        """The infeasibility certificates on given differences dx (n), dy (m) of the scaled iterates: PRIMAL_INFEASIBLE, DUAL_INFEASIBLE or
        UNDETERMINED.  Overwrites the iterates (set_iterates again before iterating)."""
        if dx is None or dy is None:
            raise ValueError("check_certificates needs dx and dy")
        st = C.c_int32(0)
        self._chk(self.lib.cosmo_hip_check_certificates(self._h, _dp(self._f(dx, self.n, "dx")), _dp(self._f(dy, self.m, "dy")), C.byref(st)))
        return int(st.value)

    def admm_init(self):
        self._chk(self.lib.cosmo_hip_admm_init(self._h))

    def admm_iterate(self, n_iters):
        self._chk(self.lib.cosmo_hip_admm_iterate(self._h, int(n_iters)))

    def admm_iterate_checked(self, n_iters):
        st = C.c_int32(0)
        self._chk(self.lib.cosmo_hip_admm_iterate_checked(self._h, int(n_iters), C.byref(st)))
        return st.value

    def set_setup_time(self, seconds):
        self._chk(self.lib.cosmo_hip_set_setup_time(self._h, float(seconds)))

    def rho_interval(self):
        """(adaptive_rho_interval in force, iteration at which the automatic rule fixed it or -1)"""
        out = np.zeros(2, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_get_rho_interval(self._h, out.ctypes.data_as(_PI64)))
        return int(out[0]), int(out[1])

    def residuals(self):
        out = np.empty(5)
        self._chk(self.lib.cosmo_hip_residuals(self._h, _dp(out)))
        return out

    def optimize(self):
        r = ResultStruct()
        self._chk(self.lib.cosmo_hip_optimize(self._h, C.byref(r)))
        return r

    def get_iterates(self):
        N = self.n + self.m
        w = np.empty(N, dtype=self.dtype); wp = np.empty(N, dtype=self.dtype); s = np.empty(self.m, dtype=self.dtype); mu = np.empty(self.m, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_get_iterates(self._h, _dp(w), _dp(wp), _dp(s), _dp(mu)))
        return w, wp, s, mu

    def get_kkt_solution(self):
        sol = np.empty(self.n + self.m, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_get_kkt_solution(self._h, _dp(sol)))
        return sol

    def get_stats(self):
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_get_stats(self._h, out.ctypes.data_as(_PI64)))
        keys = ["admm_iters", "kkt_solves", "kkt_iters_total", "kkt_budget_stalls", "spmv_A", "spmv_AT", "spmv_P", "rho_updates"]
        return dict(zip(keys, out.tolist()))

    def cg_persist_stats(self):
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_cg_persist_stats(self._h, out.ctypes.data_as(_PI64)))
        return dict(zip(["enabled", "workgroups", "launches", "fallbacks", "tickets", "arrivals", "abort", "lds_per_quarter"], out.tolist()))

    def set_kkt_perm(self, perm):
        """The ordering of the direct KKT solver (perm[k] = original index at position k, n + m entries); None = the default ordering.
        Takes effect at the next set_params with KKT_DIRECT."""
        if perm is None:
            self._chk(self.lib.cosmo_hip_set_kkt_perm(self._h, 0, None))
            return
        p = np.ascontiguousarray(perm, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_set_kkt_perm(self._h, int(p.size), p.ctypes.data_as(_PI64)))

    def direct_info(self):
        """Figures of the direct KKT solver (cosmo_hip_direct_info)."""
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_direct_info(self._h, out.ctypes.data_as(_PI64)))
        keys = ["nnz_L", "nnz_stored", "supernodes", "height", "max_width", "factorizations", "positive_pivots", "last_factor_ns"]
        return dict(zip(keys, out.tolist()))

    def set_schur_options(self, row_threshold=0, nd_max=0, block_max=0, refine_steps=2):
        """Options of the Schur-complement KKT solver (cosmo_hip_set_schur_options); they take effect at the next set_params with KKT_SCHUR.
        0 keeps a default, except for refine_steps."""
        self._chk(self.lib.cosmo_hip_set_schur_options(self._h, int(row_threshold), int(nd_max), int(block_max), int(refine_steps)))

    def schur_info(self):
        """Figures of the Schur-complement KKT solver (cosmo_hip_schur_info)."""
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_schur_info(self._h, out.ctypes.data_as(_PI64)))
        return dict(zip(SCHUR_PLAN_KEYS + ["factorizations", "refine_steps_taken", "refine_steps_rejected"], out.tolist()))

    def schur_residual(self):
        """(||rhs - M x|| / ||rhs|| of the last solve, the same before refinement) (cosmo_hip_schur_residual)."""
        out = np.zeros(2, dtype=np.float64)
        self._chk(self.lib.cosmo_hip_schur_residual(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return float(out[0]), float(out[1])

    def kkt_recurrence(self):
        """Which Krylov recurrence / kernels the KKT solves of this handle run (cosmo_hip_kkt_recurrence)."""
        return self.lib.cosmo_hip_kkt_recurrence(self._h).decode()

    def fold_stats(self):
        out = np.zeros(6, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_fold_stats(self._h, out.ctypes.data_as(_PI64)))
        return dict(zip(["enabled", "nnz", "terms", "tiles", "factored_rows", "stored_entries"], out.tolist()))

    # ---- measurement -------------------------------------------------------------------------------------------
    def time_spmv(self, which, reps=50):
        t = C.c_double(0); by = C.c_double(0)
        self._chk(self.lib.cosmo_hip_time_spmv(self._h, which, reps, C.byref(t), C.byref(by)))
        return t.value, by.value

    def psd_stats(self):
        out = np.zeros(4, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_psd_stats(self._h, out.ctypes.data_as(_PI64)))
        return dict(zip(["max_sweeps_wg", "sweeps_large", "not_converged", "ncones"], out.tolist()))

    POLAR_STAT_KEYS = ["large_cones", "batch_cones", "tile_side", "k_split", "launches_64_1", "launches_96_1", "launches_96_2", "launches_batch",
                       "products_last_large", "fallback_rounds", "verified", "products_last_batch", "schedule_steps", "unverified", "projections",
                       "err_max_e18"]

    def polar_streamk_stats(self):
        out = np.zeros(4, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_polar_streamk_stats(self._h, out.ctypes.data_as(_PI64)))
        return dict(zip(["enabled", "workgroups", "classes", "timeouts"], out.tolist()))

    def polar_stats(self):
        out = np.zeros(16, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_polar_stats(self._h, out.ctypes.data_as(_PI64)))
        return dict(zip(self.POLAR_STAT_KEYS, out.tolist()))

    def polar_dataflow_stats(self, reset=False):
        """The batch's main schedule as one persistent dependency-driven launch (cosmo_hip_polar_dataflow_stats)."""
        out = np.zeros(8, dtype=np.float64)
        self._chk(self.lib.cosmo_hip_polar_dataflow_stats(self._h, out.ctypes.data_as(_PD)))
        if reset:
            self._chk(self.lib.cosmo_hip_polar_dataflow_reset_timing(self._h))
        return dict(enabled=int(out[0]), launches=int(out[1]), products_per_launch=int(out[2]), timed_launches=int(out[3]), avg_launch_seconds=float(out[4]),
                    flops_per_launch=float(out[5]), workgroups=int(out[6]), tiles_per_product=int(out[7]))

    def time_psd_product(self, which=0, reps=20):
        t = C.c_double(0); fl = C.c_double(0)
        self._chk(self.lib.cosmo_hip_time_psd_product(self._h, int(which), int(reps), C.byref(t), C.byref(fl)))
        return t.value, fl.value

    # ---- clique sharding -----------------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        rc = load_library().cosmo_hip_comm_unique_id(buf)
        if rc != OK:
            raise CosmoHipError(rc, "cosmo_hip_comm_unique_id failed")
        return bytes(buf)

    def comm_init(self, rank, nranks, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._chk(self.lib.cosmo_hip_comm_init(self._h, int(rank), int(nranks), buf))

    def set_cone_shard(self, first_cone):
        fc = np.ascontiguousarray(first_cone, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_set_cone_shard(self._h, fc.ctypes.data_as(_PI64)))

    def set_cone_ownership(self, lo, hi):
        self._chk(self.lib.cosmo_hip_set_cone_ownership(self._h, int(lo), int(hi)))

    def comm_selftest(self):
        self._chk(self.lib.cosmo_hip_comm_selftest(self._h))

    def polar_depth_stats(self):
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_polar_depth_stats(self._h, out.ctypes.data_as(_PI64)))
        d = dict(zip(["adaptive", "depth_min", "depth_max", "depth_mean_x1000", "weighted_products_x1000", "failed_verifications", "downward_probes", "projections"], out.tolist()))
        d["depth_mean"] = d.pop("depth_mean_x1000") / 1000.0
        d["weighted_products_per_projection"] = d.pop("weighted_products_x1000") / 1000.0
        return d

    def time_krylov(self, reps):
        """(seconds per Krylov iteration incl. the kernel boundaries between its launches, algorithmic bytes per iteration, launches per iteration)."""
        t, b, nl = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
        self._chk(self.lib.cosmo_hip_time_krylov(self._h, int(reps), C.byref(t), C.byref(b), C.byref(nl)))
        return t.value, b.value, nl.value

    def comm_allreduce_check(self, count):
        """Known-answer all-reduce of `count` reals through the loop's own exchange path (collective: all ranks call it).  The caller compares
        `hash` across the ranks: the replicated n-side of a row-sharded run needs the SAME bits everywhere."""
        out = np.zeros(6, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_comm_allreduce_check(self._h, int(count), out.ctypes.data_as(_PI64)))
        d = dict(zip(["exact_mismatches", "inexact_outside_bound", "hash", "transport", "nranks", "rccl_version_code"], out.tolist()))
        d["count"] = int(count)
        return d

    def comm_init_hostshm(self, rank, nranks, name: str):
        self._chk(self.lib.cosmo_hip_comm_init_hostshm(self._h, int(rank), int(nranks), name.encode()))

    def comm_stats(self):
        out = np.zeros(4, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_comm_stats(self._h, out.ctypes.data_as(_PI64)))
        return dict(zip(["nranks", "rank", "exchanges", "transport"], out.tolist()))

    def set_row_shard(self, first_cone):
        """Row sharding (csrc/rowshard.hip): this rank keeps the cones first_cone[rank] <= k < first_cone[rank+1] and their rows."""
        fc = np.ascontiguousarray(first_cone, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_set_row_shard(self._h, fc.ctypes.data_as(_PI64)))

    def row_shard_info(self):
        out = np.zeros(6, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_row_shard_info(self._h, out.ctypes.data_as(_PI64)))
        return dict(zip(["row_lo", "row_hi", "m_global", "nnz_A_local", "cones_local", "first_cone"], out.tolist()))

    def comm_stats_ex(self):
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_comm_stats_ex(self._h, out.ctypes.data_as(_PI64)))
        d = dict(zip(["nranks", "rank", "collectives", "transport", "mode", "bytes", "allreduces", "allreduce_elems"], out.tolist()))
        d["mode"] = {0: "none", 1: "cones", 2: "rows"}[d["mode"]]
        return d

    def set_profiling(self, on):
        self._chk(self.lib.cosmo_hip_set_profiling(self._h, int(on)))

    def get_kernel_times(self):
        sec = np.zeros(NUM_KERNEL_CLASSES); cnt = np.zeros(NUM_KERNEL_CLASSES, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_get_kernel_times(self._h, _dp(sec), cnt.ctypes.data_as(_PI64)))
        out = {}
        for k in range(NUM_KERNEL_CLASSES):
            if cnt[k]:
                out[self.lib.cosmo_hip_kernel_class_name(k).decode()] = (float(sec[k]), int(cnt[k]))
        return out


class Batch:
    """Batch of independent problems with identical (n, m, cone structure): one persistent workgroup per problem."""

    def __init__(self, nprob, n, m, device=0, dtype=np.float64):
        self.dtype = np.dtype(np.float32 if _is_f32(dtype) else np.float64)
        self.lib = load_library(self.dtype)
        self._b = C.c_void_p()
        rc = self.lib.cosmo_hip_batch_create(C.byref(self._b), int(device), int(nprob), int(n), int(m))
        if rc != OK:
            raise CosmoHipError(rc, "cosmo_hip_batch_create failed (no MI355X visible? this library has no CPU path)")
        self.nprob, self.n, self.m = int(nprob), int(n), int(m)
        self.device = int(device)

    def _f(self, a, n=None, name="array"):
        return _f64(a, n, name, self.dtype)

    def _t(self, t, shape, name):
        """device pointer of a checked torch tensor (check_device_tensor), NULL for None"""
        import torch
        t = check_device_tensor(t, shape, self.dtype, torch.device("cuda", self.device), name)
        return None if t is None else C.cast(C.c_void_p(t.data_ptr()), _PF if self.dtype == np.float32 else _PD)

    def _stream(self, stream):
        """the caller's hipStream_t: `stream` (a torch stream) or the current stream of the batch's device"""
        import torch
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        return C.c_void_p(s.cuda_stream)

    def update_qb_device(self, q=None, b=None, members=None, stream=None):
        """cosmo_hip_batch_update_qb_device: RAW q (len(members), n) and / or b (len(members), m) from torch tensors on the batch's device, applied at
        once on the device; row j belongs to member members[j] (None: all members in order).  Ordered against `stream` (default: the current one)."""
        mem = None if members is None else np.ascontiguousarray(members, dtype=np.int64).ravel()
        cnt = self.nprob if mem is None else int(mem.size)
        qp = self._t(q, (cnt, self.n), "q"); bp = self._t(b, (cnt, self.m), "b")
        self._chk(self.lib.cosmo_hip_batch_update_qb_device(self._b, cnt, None if mem is None else mem.ctypes.data_as(_PI64), qp, bp, self._stream(stream)))

    def set_iterates_device(self, x0=None, s0=None, y0=None, stream=None):
        """cosmo_hip_batch_set_iterates_device: UNSCALED x0 (nprob, n), s0, y0 (nprob, m) from torch tensors (None: zeros), scaled on the device."""
        xp = self._t(x0, (self.nprob, self.n), "x0"); sp_ = self._t(s0, (self.nprob, self.m), "s0"); yp = self._t(y0, (self.nprob, self.m), "y0")
        self._chk(self.lib.cosmo_hip_batch_set_iterates_device(self._b, xp, sp_, yp, self._stream(stream)))

    def get_solution_device(self, x=None, s=None, y=None, stream=None):
        """cosmo_hip_batch_get_solution_device: the unscaled x (nprob, n), s, y (nprob, m) of all members into the given torch tensors (None: skip)."""
        xp = self._t(x, (self.nprob, self.n), "x"); sp_ = self._t(s, (self.nprob, self.m), "s"); yp = self._t(y, (self.nprob, self.m), "y")
        self._chk(self.lib.cosmo_hip_batch_get_solution_device(self._b, xp, sp_, yp, self._stream(stream)))

    def close(self):
        if self._b:
            self.lib.cosmo_hip_batch_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            msg = self.lib.cosmo_hip_batch_last_error(self._b)
            raise CosmoHipError(rc, msg.decode() if msg else "")

    def set_problem(self, k, P, q, A, b):
        pc, pr, pv = csc_julia(P, self.dtype)
        ac, ar, av = csc_julia(A, self.dtype)
        q = self._f(q, self.n, "q"); b = self._f(b, self.m, "b")
        self._chk(self.lib.cosmo_hip_batch_set_problem(self._b, int(k), pc.ctypes.data_as(_PI64), pr.ctypes.data_as(_PI64), _dp(pv),
                                                       ac.ctypes.data_as(_PI64), ar.ctypes.data_as(_PI64), _dp(av), _dp(q), _dp(b)))
        self.__dict__.setdefault("nnz", {})[int(k)] = (int(pv.size), int(av.size))

    def set_cones(self, types, dims, box_l=None, box_u=None, cone_param=None):
        t = np.ascontiguousarray(types, dtype=np.int32); d = np.ascontiguousarray(dims, dtype=np.int64)
        bl = self._f(box_l); bu = self._f(box_u)
        if cone_param is None:
            self._chk(self.lib.cosmo_hip_batch_set_cones(self._b, t.size, t.ctypes.data_as(_PI32), d.ctypes.data_as(_PI64), _dp(bl), _dp(bu)))
        else:                                                 # alpha of the power cones (as Handle.set_cones)
            cp = self._f(cone_param, t.size)
            self._chk(self.lib.cosmo_hip_batch_set_cones_ex(self._b, t.size, t.ctypes.data_as(_PI32), d.ctypes.data_as(_PI64), _dp(bl), _dp(bu), _dp(cp)))

    def set_scaling(self, k, Dinv, Einv, cinv):
        self._chk(self.lib.cosmo_hip_batch_set_scaling(self._b, int(k), _dp(self._f(Dinv, self.n)), _dp(self._f(Einv, self.m)), float(cinv)))

    def set_scaling_full(self, k, D, Dinv, E, Einv, c, cinv):
        """set_scaling plus D, E, c themselves: the device update pass (apply_updates) scales with exactly these."""
        self._chk(self.lib.cosmo_hip_batch_set_scaling_full(self._b, int(k), _dp(self._f(D, self.n)), _dp(self._f(Dinv, self.n)), _dp(self._f(E, self.m)),
                                                            _dp(self._f(Einv, self.m)), float(c), float(cinv)))

    def set_params(self, params):
        self._chk(self.lib.cosmo_hip_batch_set_params(self._b, C.byref(params)))

    def scale_ruiz(self, iterations, min_scaling=1e-4, max_scaling=1e4):
        """Device Ruiz equilibration of every staged member in one launch (csrc/batch_ruiz.hip); after set_problem / set_cones, before set_params,
        instead of set_scaling*.  Read D, E, c with get_scaling."""
        self._chk(self.lib.cosmo_hip_batch_scale_ruiz(self._b, int(iterations), float(min_scaling), float(max_scaling)))

    def get_scaling(self, k):
        """(D, E, c) of member k as the batch holds them."""
        D = np.empty(self.n, dtype=self.dtype); E = np.empty(self.m, dtype=self.dtype); c = C.c_double(1.0)
        self._chk(self.lib.cosmo_hip_batch_get_scaling(self._b, int(k), _dp(D), _dp(E), C.byref(c)))
        return D, E, float(c.value)

    def get_scaled_problem(self, k, nnzP, nnzA, nbox=0):
        """The staged problem of member k (before set_params): (values of P row by row, values of A in CSC order, q, b, box_l, box_u).  Raises if the
        member's three staged copies of A differ in a bit."""
        Pv = np.empty(int(nnzP), dtype=self.dtype); Av = np.empty(int(nnzA), dtype=self.dtype)
        q = np.empty(self.n, dtype=self.dtype); b = np.empty(self.m, dtype=self.dtype)
        bl = np.empty(int(nbox), dtype=self.dtype); bu = np.empty(int(nbox), dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_batch_get_scaled_problem(self._b, int(k), _dp(Pv), _dp(Av), _dp(q), _dp(b), _dp(bl) if nbox else None, _dp(bu) if nbox else None))
        return Pv, Av, q, b, bl, bu

    def ruiz_info(self):
        """dict(work_vectors = 'lds' | 'global', lds_bytes, members, rounds) of the device equilibration pass."""
        out = np.zeros(4, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_ruiz_info(self._b, out.ctypes.data_as(_PI64)))
        return dict(work_vectors=("lds", "global")[int(out[0])], lds_bytes=int(out[1]), members=int(out[2]), rounds=int(out[3]))

    def stage_qb(self, k, q=None, b=None):
        """Stage the RAW (unscaled) q and / or b of member k for the next apply_updates (host only)."""
        self._chk(self.lib.cosmo_hip_batch_stage_qb(self._b, int(k), _dp(self._f(q, self.n, "q")), _dp(self._f(b, self.m, "b"))))

    def stage_matrices(self, k, P_vals=None, A_vals=None, apply_scaling=False):
        """Stage new VALUES of P and / or A of member k (the order of set_problem's CSC arrays, same pattern) for the next apply_updates (host only).
        apply_scaling: the device applies the batch's D, E, c; else the values are taken as given."""
        nP, nA = getattr(self, "nnz", {}).get(int(k), (None, None))           # (an index the library refuses: its error, not a KeyError)
        self._chk(self.lib.cosmo_hip_batch_stage_matrices(self._b, int(k), _dp(self._f(P_vals, nP, "P values")), _dp(self._f(A_vals, nA, "A values")),
                                                          1 if apply_scaling else 0))

    def update_matrices(self, members, P_vals=None, A_vals=None, apply_scaling=False):
        """stage_matrices of len(members) members (P_vals / A_vals: the members' value arrays one after the other, or None), then apply_updates."""
        mem = np.ascontiguousarray(members, dtype=np.int64)
        nP = sum(self.nnz[int(k)][0] for k in mem); nA = sum(self.nnz[int(k)][1] for k in mem)
        self._chk(self.lib.cosmo_hip_batch_update_matrices(self._b, mem.size, mem.ctypes.data_as(_PI64), _dp(self._f(P_vals, nP, "P values")),
                                                           _dp(self._f(A_vals, nA, "A values")), 1 if apply_scaling else 0))

    def update_matrices_info(self):
        """dict(updates, arrays_per_update, host_rebuilds, last_bytes, map_bytes, factorizations) of the matrix updates of this batch."""
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_update_matrices_info(self._b, out.ctypes.data_as(_PI64)))
        keys = ("updates", "arrays_per_update", "host_rebuilds", "last_bytes", "map_bytes", "factorizations")
        return dict(zip(keys, (int(v) for v in out[:6])))

    def get_matrix_values(self, k, which):
        """The device copy of member k's values: which = 0 / 'A' the CSR of A, 1 / 'AT' the CSR of A' (CSC order of A), 2 / 'PT' the rows of [P | A']."""
        w = {"A": 0, "AT": 1, "PT": 2}.get(which, which)
        nP, nA = self.nnz[int(k)]
        out = np.empty(nP + nA if w == 2 else nA, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_batch_get_matrix_values(self._b, int(k), int(w), _dp(out)))
        return out

    def get_image(self, k):
        """The raw bytes of member k's LDS image followed by its row of the register-resident diagonal of P (empty for a batch that has neither)."""
        nb = C.c_int64(0)
        self._chk(self.lib.cosmo_hip_batch_get_image(self._b, int(k), None, 0, C.byref(nb)))
        out = np.zeros(int(nb.value), dtype=np.uint8)
        if out.size:
            self._chk(self.lib.cosmo_hip_batch_get_image(self._b, int(k), out.ctypes.data_as(C.c_void_p), out.size, C.byref(nb)))
        return out

    def apply_updates(self):
        """Every staged vector in one copy and one launch: scaled on the device, rows of Nonnegatives cones re-classified."""
        self._chk(self.lib.cosmo_hip_batch_apply_updates(self._b))

    def update_qb(self, members, q=None, b=None):
        """stage_qb of len(members) members (q: len * n raw values or None, b: len * m or None), then apply_updates."""
        mem = np.ascontiguousarray(members, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_update_qb(self._b, mem.size, mem.ctypes.data_as(_PI64), _dp(self._f(q, mem.size * self.n, "q")),
                                                     _dp(self._f(b, mem.size * self.m, "b"))))

    def warm_restart(self):
        """The next optimize starts from the batch's own final iterates (re-optimize: accelerator, status and counters restarted, rho kept)."""
        self._chk(self.lib.cosmo_hip_batch_warm_restart(self._b))

    def get_qb(self, k):
        """(q, b) of member k as the device holds them (scaled)."""
        q = np.empty(self.n, dtype=self.dtype); b = np.empty(self.m, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_batch_get_qb(self._b, int(k), _dp(q), _dp(b)))
        return q, b

    def set_accelerator(self, kind=ACCEL_ANDERSON, mem=15, min_mem=3, safeguard=True, safeguard_tol=2.0, start_iter=2, start_accuracy=None):
        """`_make_accelerator!` (src/setup.jl:10-16) for every problem of the batch; before set_params.  mem <= 16 in batch mode."""
        ap = AccelParams()
        self.lib.cosmo_hip_default_accel_params(C.byref(ap))
        ap.kind, ap.mem, ap.min_mem, ap.safeguard = int(kind), int(mem), int(min_mem), 1 if safeguard else 0
        ap.safeguard_tol, ap.start_iter = float(safeguard_tol), int(start_iter)
        if start_accuracy is not None:
            ap.start_accuracy = float(start_accuracy)
        self._chk(self.lib.cosmo_hip_batch_set_accelerator(self._b, C.byref(ap)))

    def set_direct(self, on=True, perm=None):
        """cosmo_hip_batch_set_direct: the next set_params takes kkt_kind DIRECT (one LDL' per problem, one analysis for the batch); before set_params.
        perm: None = the default ordering, else n + m entries (perm[k] = original index at position k)."""
        if perm is None:
            self._chk(self.lib.cosmo_hip_batch_set_direct(self._b, 1 if on else 0, None))
            return
        p = np.ascontiguousarray(perm, dtype=np.int64)
        if p.size != self.n + self.m:
            raise ValueError("perm needs n + m = %d entries" % (self.n + self.m))
        self._chk(self.lib.cosmo_hip_batch_set_direct(self._b, 1 if on else 0, p.ctypes.data_as(_PI64)))

    def set_psd_side_max(self, side):
        """cosmo_hip_batch_set_psd_side_max: the largest PSD cone side set_cones accepts (64 .. 256, default 64); before set_cones."""
        self._chk(self.lib.cosmo_hip_batch_set_psd_side_max(self._b, int(side)))

    def direct_info(self):
        """Figures of the batch's direct KKT solver (cosmo_hip_batch_direct_info)."""
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_direct_info(self._b, out.ctypes.data_as(_PI64)))
        keys = ("nnz_L", "panel_size", "supernodes", "height", "max_width", "analysis_ns", "factorizations", "min_positive_pivots")
        return dict(zip(keys, (int(v) for v in out)))

    def direct_counts(self):
        """Factorisations of every member so far, the set-up one included (int64 array of nprob)."""
        out = np.zeros(self.nprob, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_direct_counts(self._b, out.ctypes.data_as(_PI64)))
        return out

    def polish(self, delta=1e-6, refine_iter=3):
        """cosmo_hip_batch_polish: the active-set polish of every member the last optimize() reported Solved (csrc/batch_polish.hip)."""
        self._chk(self.lib.cosmo_hip_batch_polish(self._b, float(delta), int(refine_iter)))

    def polish_info(self, status_out=None):
        """cosmo_hip_batch_polish_info: dict of arrays over the members -- status (1 accepted, -1 rejected, 0 not attempted), r_prim_before,
        r_dual_before, r_prim, r_dual and cost of the candidate, active_rows.  status_out: an int32 torch tensor of nprob entries on the batch's device
        receives the statuses without a host copy (the dict then has no "status")."""
        out = np.zeros(6 * self.nprob, dtype=np.float64)
        if status_out is not None:
            import torch
            if not (isinstance(status_out, torch.Tensor) and status_out.dtype == torch.int32 and status_out.is_contiguous() and status_out.numel() == self.nprob
                    and status_out.device == torch.device("cuda", self.device)):
                raise ValueError("polish_info: status_out is a contiguous int32 tensor of %d entries on cuda:%d" % (self.nprob, self.device))
            sp_ = C.cast(C.c_void_p(status_out.data_ptr()), _PI32)
            self._chk(self.lib.cosmo_hip_batch_polish_info(self._b, sp_, out.ctypes.data_as(_PD)))
            st = None
        else:
            st = np.zeros(self.nprob, dtype=np.int32)
            self._chk(self.lib.cosmo_hip_batch_polish_info(self._b, st.ctypes.data_as(_PI32), out.ctypes.data_as(_PD)))
        q = out[:4 * self.nprob].reshape(self.nprob, 4)
        d = dict(r_prim_before=q[:, 0].copy(), r_dual_before=q[:, 1].copy(), r_prim=q[:, 2].copy(), r_dual=q[:, 3].copy(),
                 active_rows=out[4 * self.nprob:5 * self.nprob].astype(np.int64), cost=out[5 * self.nprob:].copy())
        if st is not None:
            d["status"] = st
        return d

    def accel_stats(self):
        """Per problem: dict of int64 arrays (accelerated, accepted, declined, restarts, active, safeguarding_iter)."""
        out = np.zeros(6 * self.nprob, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_get_accel_stats(self._b, out.ctypes.data_as(_PI64)))
        keys = ("accelerated", "accepted", "declined", "restarts", "active", "safeguarding_iter")
        return {k: out[i::6].copy() for i, k in enumerate(keys)}

    def get_rho_classes(self, k):
        out = np.empty(self.m, dtype=np.int32)
        self._chk(self.lib.cosmo_hip_batch_get_rho_classes(self._b, int(k), out.ctypes.data_as(_PI32)))
        return out

    def set_iterates(self, x0=None, s0=None, mu0=None):
        self._chk(self.lib.cosmo_hip_batch_set_iterates(self._b, _dp(self._f(x0, self.nprob * self.n)), _dp(self._f(s0, self.nprob * self.m)),
                                                        _dp(self._f(mu0, self.nprob * self.m))))

    def check_certificates(self, dx, dy):
        """Handle.check_certificates for every problem (dx: nprob * n, dy: nprob * m): list of nprob statuses.  Overwrites the iterates."""
        if dx is None or dy is None:
            raise ValueError("check_certificates needs dx and dy")
        st = np.zeros(self.nprob, dtype=np.int32)
        self._chk(self.lib.cosmo_hip_batch_check_certificates(self._b, _dp(self._f(dx, self.nprob * self.n, "dx")), _dp(self._f(dy, self.nprob * self.m, "dy")),
                                                              st.ctypes.data_as(_PI32)))
        return [int(v) for v in st]

    def optimize(self):
        res = (ResultStruct * self.nprob)()
        self._chk(self.lib.cosmo_hip_batch_optimize(self._b, res))
        return list(res)

    def iterate(self, n_iters, with_init=False):
        """n_iters more loop bodies of every undecided problem (residual / adaptive-rho checks on schedule).  A loop body starts with admm_z
        (w_prev = w, then s = Pi(w_s), solver.jl:151-152) and ends with the KKT solve and the update of w, which never writes s: after iterate(1)
        get_iterates returns in w_prev[n:] the exact input of the cone projection and in s its result (tests/test_gpu_batch_projections.py relies
        on this order).  with_init runs one KKT solve and update in front of the first body (solver.jl:137-138).  The infeasibility certificates
        are NOT evaluated here -- only optimize() cuts the persistent launch for them -- so rates measured through iterate() exclude their cost."""
        self._chk(self.lib.cosmo_hip_batch_iterate(self._b, int(n_iters), 1 if with_init else 0))

    def kernel_info(self):
        """Which kernel the batch runs: dict(form = 'streaming' | 'lds_image' | 'register_1_2' | 'register_2_4', sliced, lds_bytes, p_in_registers,
        registers / scratch_bytes per thread and static_lds_bytes of that instantiation (from the loaded code object), sorted_assignment)."""
        out = np.zeros(8, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_kernel_info(self._b, out.ctypes.data_as(_PI64)))
        return dict(form=("streaming", "lds_image", "register_1_2", "register_2_4")[int(out[0])], sliced=bool(out[1]), lds_bytes=int(out[2]), p_in_registers=bool(out[3]),
                    registers=int(out[4]), scratch_bytes=int(out[5]), static_lds_bytes=int(out[6]), sorted_assignment=bool(out[7] & 1), long_rows=bool(out[7] & 2))

    def counters(self):
        """Per problem: ADMM iterations, KKT solves, Krylov iterations in total (three int64 arrays)."""
        out = np.zeros(3 * self.nprob, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_get_counters(self._b, out.ctypes.data_as(_PI64)))
        return out[0::3].copy(), out[1::3].copy(), out[2::3].copy()

    def get_iterates(self, k):
        N = self.n + self.m
        w = np.empty(N, dtype=self.dtype); wp = np.empty(N, dtype=self.dtype); s = np.empty(self.m, dtype=self.dtype); mu = np.empty(self.m, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_batch_get_iterates(self._b, int(k), _dp(w), _dp(wp), _dp(s), _dp(mu)))
        return w, wp, s, mu


class BatchGroup:
    """Batch of independent problems of DIFFERENT structure (csrc/batch_group.hip): every problem brings its own (n, m, cones); the library
    partitions them into classes of identical structure, one `Batch` per class, and solves all classes concurrently.  The reference's batch is a
    loop over arbitrary models (src/solver.jl:78)."""

    def __init__(self, nprob, device=0, dtype=np.float64):
        self.dtype = np.dtype(np.float32 if _is_f32(dtype) else np.float64)
        self.lib = load_library(self.dtype)
        self._g = C.c_void_p()
        rc = self.lib.cosmo_hip_batch_group_create(C.byref(self._g), int(device), int(nprob))
        if rc != OK:
            raise CosmoHipError(rc, "cosmo_hip_batch_group_create failed (no MI355X visible? this library has no CPU path)")
        self.nprob = int(nprob)
        self.dims = [None] * self.nprob

    def _f(self, a, n=None, name="array"):
        return _f64(a, n, name, self.dtype)

    def close(self):
        if self._g:
            self.lib.cosmo_hip_batch_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            msg = self.lib.cosmo_hip_batch_group_last_error(self._g)
            raise CosmoHipError(rc, msg.decode() if msg else "")

    def set_problem(self, k, P, q, A, b):
        m, n = A.shape
        pc, pr, pv = csc_julia(P, self.dtype)
        ac, ar, av = csc_julia(A, self.dtype)
        q = self._f(q, n, "q"); b = self._f(b, m, "b")
        self._chk(self.lib.cosmo_hip_batch_group_set_problem(self._g, int(k), int(n), int(m), pc.ctypes.data_as(_PI64), pr.ctypes.data_as(_PI64), _dp(pv),
                                                             ac.ctypes.data_as(_PI64), ar.ctypes.data_as(_PI64), _dp(av), _dp(q), _dp(b)))
        self.dims[int(k)] = (int(n), int(m))
        self.__dict__.setdefault("nnz", {})[int(k)] = (int(pv.size), int(av.size))

    def set_cones(self, k, types, dims, box_l=None, box_u=None, cone_param=None):
        t = np.ascontiguousarray(types, dtype=np.int32); d = np.ascontiguousarray(dims, dtype=np.int64)
        bl = self._f(box_l); bu = self._f(box_u)
        cp = self._f(cone_param, t.size) if cone_param is not None else None
        self._chk(self.lib.cosmo_hip_batch_group_set_cones(self._g, int(k), t.size, t.ctypes.data_as(_PI32), d.ctypes.data_as(_PI64), _dp(bl), _dp(bu), _dp(cp)))

    def set_scaling(self, k, Dinv, Einv, cinv):
        n, m = self.dims[int(k)]
        self._chk(self.lib.cosmo_hip_batch_group_set_scaling(self._g, int(k), _dp(self._f(Dinv, n)), _dp(self._f(Einv, m)), float(cinv)))

    def set_scaling_full(self, k, D, Dinv, E, Einv, c, cinv):
        n, m = self.dims[int(k)]
        self._chk(self.lib.cosmo_hip_batch_group_set_scaling_full(self._g, int(k), _dp(self._f(D, n)), _dp(self._f(Dinv, n)), _dp(self._f(E, m)), _dp(self._f(Einv, m)),
                                                                  float(c), float(cinv)))

    def set_accelerator(self, kind=ACCEL_ANDERSON, mem=15, min_mem=3, safeguard=True, safeguard_tol=2.0, start_iter=2, start_accuracy=None):
        ap = AccelParams()
        self.lib.cosmo_hip_default_accel_params(C.byref(ap))
        ap.kind, ap.mem, ap.min_mem, ap.safeguard = int(kind), int(mem), int(min_mem), 1 if safeguard else 0
        ap.safeguard_tol, ap.start_iter = float(safeguard_tol), int(start_iter)
        if start_accuracy is not None:
            ap.start_accuracy = float(start_accuracy)
        self._chk(self.lib.cosmo_hip_batch_group_set_accelerator(self._g, C.byref(ap)))

    def set_direct(self, on=True):
        """cosmo_hip_batch_group_set_direct: every class's batch takes kkt_kind DIRECT (default ordering); before set_params."""
        self._chk(self.lib.cosmo_hip_batch_group_set_direct(self._g, 1 if on else 0))

    def set_psd_side_max(self, side):
        """cosmo_hip_batch_group_set_psd_side_max: every class's batch accepts PSD cones up to this side (64 .. 256, default 64); before set_params."""
        self._chk(self.lib.cosmo_hip_batch_group_set_psd_side_max(self._g, int(side)))

    def set_device_scaling(self, iterations, min_scaling=1e-4, max_scaling=1e4):
        """cosmo_hip_batch_group_set_device_scaling: set_params equilibrates every member without a caller's scaling on the device; before set_params."""
        self._chk(self.lib.cosmo_hip_batch_group_set_device_scaling(self._g, int(iterations), float(min_scaling), float(max_scaling)))

    def get_scaling(self, k):
        """(D, E, c) of problem k; after set_params."""
        n, m = self.dims[int(k)]
        D = np.empty(n, dtype=self.dtype); E = np.empty(m, dtype=self.dtype); c = C.c_double(1.0)
        self._chk(self.lib.cosmo_hip_batch_group_get_scaling(self._g, int(k), _dp(D), _dp(E), C.byref(c)))
        return D, E, float(c.value)

    def set_params(self, params):
        self._chk(self.lib.cosmo_hip_batch_group_set_params(self._g, C.byref(params)))

    def stage_qb(self, k, q=None, b=None):
        n, m = self.dims[int(k)]
        self._chk(self.lib.cosmo_hip_batch_group_stage_qb(self._g, int(k), _dp(self._f(q, n, "q")), _dp(self._f(b, m, "b"))))

    def stage_matrices(self, k, P_vals=None, A_vals=None, apply_scaling=False):
        nP, nA = self.nnz[int(k)]
        self._chk(self.lib.cosmo_hip_batch_group_stage_matrices(self._g, int(k), _dp(self._f(P_vals, nP, "P values")), _dp(self._f(A_vals, nA, "A values")),
                                                                1 if apply_scaling else 0))

    def apply_updates(self):
        self._chk(self.lib.cosmo_hip_batch_group_apply_updates(self._g))

    def warm_restart(self):
        self._chk(self.lib.cosmo_hip_batch_group_warm_restart(self._g))

    def set_schur_options(self, row_threshold=0, nd_max=0, block_max=0, refine_steps=2):
        """cosmo_hip_batch_group_set_schur_options: the options of the members that run KKT_SCHUR (on their own handles); before set_params."""
        self._chk(self.lib.cosmo_hip_batch_group_set_schur_options(self._g, int(row_threshold), int(nd_max), int(block_max), int(refine_steps)))

    def get_qb(self, k):
        n, m = self.dims[int(k)]
        q = np.empty(n, dtype=self.dtype); b = np.empty(m, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_batch_group_get_qb(self._g, int(k), _dp(q), _dp(b)))
        return q, b

    def class_info(self, with_modes=False):
        """(number of structure classes, class index of every problem[, mode of every problem: 0 persistent batch kernel, 1 its own handle])"""
        nc = C.c_int64(0)
        cls = np.zeros(self.nprob, dtype=np.int64); mode = np.zeros(self.nprob, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_group_class_info(self._g, C.byref(nc), cls.ctypes.data_as(_PI64), mode.ctypes.data_as(_PI64)))
        return (int(nc.value), cls, mode) if with_modes else (int(nc.value), cls)

    def rho_interval(self, k):
        """(adaptive_rho_interval in force for problem k, iteration at which the automatic rule fixed it or -1)"""
        out = np.zeros(2, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_group_get_rho_interval(self._g, int(k), out.ctypes.data_as(_PI64)))
        return int(out[0]), int(out[1])

    def run_info(self):
        """worker threads and jobs of the last optimize (a bounded pool), classes, problems"""
        out = np.zeros(5, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_group_run_info(self._g, out.ctypes.data_as(_PI64)))
        return dict(zip(["workers", "jobs", "classes", "problems", "merged_classes"], out.tolist()))

    def set_iterates(self, k, x0=None, s0=None, mu0=None):
        n, m = self.dims[int(k)]
        self._chk(self.lib.cosmo_hip_batch_group_set_iterates(self._g, int(k), _dp(self._f(x0, n)), _dp(self._f(s0, m)), _dp(self._f(mu0, m))))

    def optimize(self):
        res = (ResultStruct * self.nprob)()
        self._chk(self.lib.cosmo_hip_batch_group_optimize(self._g, res))
        return list(res)

    def get_iterates(self, k):
        n, m = self.dims[int(k)]
        w = np.empty(n + m, dtype=self.dtype); wp = np.empty(n + m, dtype=self.dtype); s = np.empty(m, dtype=self.dtype); mu = np.empty(m, dtype=self.dtype)
        self._chk(self.lib.cosmo_hip_batch_group_get_iterates(self._g, int(k), _dp(w), _dp(wp), _dp(s), _dp(mu)))
        return w, wp, s, mu

    def counters(self):
        out = np.zeros(3 * self.nprob, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_group_get_counters(self._g, out.ctypes.data_as(_PI64)))
        return out[0::3].copy(), out[1::3].copy(), out[2::3].copy()

    def accel_stats(self):
        out = np.zeros(6 * self.nprob, dtype=np.int64)
        self._chk(self.lib.cosmo_hip_batch_group_get_accel_stats(self._g, out.ctypes.data_as(_PI64)))
        keys = ("accelerated", "accepted", "declined", "restarts", "active", "safeguarding_iter")
        return {k: out[i::6].copy() for i, k in enumerate(keys)}
