"""What test_gpu_residual_checks.py and test_gpu_batch_residual_checks.py share on the device side: how a problem of tests/residual_cases.py is handed to the
library, and the bit-level comparisons.  No test functions, no state."""
import numpy as np

import cosmo_jl_amd as cj
from tests import residual_cases as R
from tests import util

F = cj._ffi
CASE_LIMIT_S = 120
SOLVED, MAX_ITER, UNSOLVED = 1, 2, 3


def cone_args(pb):
    sets = util.projection_sets(pb.cones)
    bl = np.concatenate([K.l for K in sets if K.kind == F.BOX] or [np.zeros(0)])
    bu = np.concatenate([K.u for K in sets if K.kind == F.BOX] or [np.zeros(0)])
    return [K.kind for K in sets], [K.dim for K in sets], bl, bu


def params(dtype, **kw):
    """the defaults with the CG solver, unscaled residuals, a check every iteration, eps = 0, no certificates, the rho rule off but due every iteration"""
    p = F.default_params(dtype)
    p.kkt_kind = F.KKT_CG
    p.unscale_residuals = 1
    p.check_termination = 1
    p.check_infeasibility = 10 ** 9
    p.adaptive_rho = 0
    p.adaptive_rho_interval = 1
    p.eps_abs = p.eps_rel = 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all(bits(a) == bits(b)))


def recovered_mu(run, rho, did):
    """rho .* (w_prev[n+1:end] - s) in the type (solver.jl:307; the library is built without contraction)"""
    t = R.DTYPES[did]
    return np.asarray(rho, dtype=t) * (run.w_prev[len(run.w_prev) - len(run.s):] - run.s)
