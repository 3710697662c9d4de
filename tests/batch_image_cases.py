"""The cases of the batch LDS-image tests (tests/test_batch_image_host.py, tests/test_gpu_batch_image.py), read from tests/golden/batch_image_cases.npz
(written by tests/golden/make_fixtures_batch_image.py, which also describes them).

A FAMILY is the members of one batch as set_problem takes them: CSC patterns and values of P and A, q, b, the cones, the Box bounds and, for the
families of the kernel forms, a start (x0, s0, mu0).  A CASE is a family with a precision, the COSMO_HIP_BATCH_* switches and the accelerator flag.
The fixture also holds what the commit before the host-only planner answered for every case (HASHES[case]): SHA-256 of get_image(k) and of the
iterates after 30 iterations, kernel_info(); and the SHA-256 of the planner's other arrays, taken from the planner's first state (the old function
body moved verbatim)."""
import hashlib
import json
import os

import numpy as np
import scipy.sparse as sp

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_image_cases.npz")
SWITCHES = ("LDS", "BS", "EXT", "REG", "SLICED", "LONG", "LDSCG", "LDSCG_SORTED", "STORE_SORTED", "SORTED", "COLOR")      # COSMO_HIP_BATCH_<name>, BatchImageOpts order
ZERO, NONNEG, BOX, SOC, PSD_SQUARE, PSD_TRIANGLE, EXP, DUAL_EXP, POW, DUAL_POW = range(10)       # include/cosmo_hip.h (asserted against _ffi by the GPU test)
MAX_LDS = 163840                                        # bytes of LDS a workgroup can have on gfx950

_z = np.load(PATH)
CASES = json.loads(bytes(_z["cases_json"]).decode())    # name -> dict(family, dtype, env, aa, iterates)
HASHES = json.loads(bytes(_z["hashes_json"]).decode())  # name -> dict(image=[...], iterates=[...], kernel_info={...}, host={array: sha256})
FORMS = [c for c in CASES if CASES[c]["iterates"]]      # the kernel forms of tests/test_gpu_batch_update_matrices.py


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class Family:
    def __init__(self, name):
        g = lambda key: _z["%s.%s" % (name, key)]
        self.name = name
        self.nprob, self.n, self.m = (int(v) for v in g("dims"))
        self.cone_types, self.cone_dims = g("cone_types"), g("cone_dims")
        self.box_l, self.box_u = g("box_l"), g("box_u")
        self.q, self.b = g("q").reshape(self.nprob, self.n), g("b").reshape(self.nprob, self.m)
        self.P, self.A = [], []
        for mats, key, shape in ((self.P, "P", (self.n, self.n)), (self.A, "A", (self.m, self.n))):
            ptr, idx, val = g(key + "p").reshape(self.nprob, self.n + 1), g(key + "i"), g(key + "x")
            o = 0
            for k in range(self.nprob):
                nz = int(ptr[k, -1])
                mats.append(sp.csc_matrix((val[o:o + nz].copy(), idx[o:o + nz].copy(), ptr[k].copy()), shape=shape))
                o += nz
        self.start = tuple(g(key) for key in ("x0", "s0", "mu0")) if "%s.x0" % name in _z.files else None

    def cone_counts(self):
        """(npsd, nmid, n3) as set_params counts them: PSD cones of dimension > 1, those of side 17 .. 64, three-dimensional cones"""
        npsd = nmid = n3 = 0
        for t, d in zip(self.cone_types, self.cone_dims):
            if t in (PSD_SQUARE, PSD_TRIANGLE) and d > 1:
                npsd += 1
                nmid += int(d > (16 * 16 if t == PSD_SQUARE else 16 * 17 // 2))
            n3 += int(EXP <= t <= DUAL_POW)
        return npsd, nmid, n3


_fams = {}


def family(name):
    if name not in _fams:
        _fams[name] = Family(name)
    return _fams[name]


def dtype_of(case):
    return np.dtype(CASES[case]["dtype"])


def env_of(case):
    return {"COSMO_HIP_BATCH_" + k: str(v) for k, v in CASES[case]["env"].items()}


# ---- the planner on the CPU: csrc/batch_image.cpp through tests/batch_image_probe.cpp ------------------------------------------------------------
_probes = {}
FLAGS = ("fits", "bs", "reg_mode", "long_rows", "force_ext", "want_sliced", "p_all_diag", "rcg_form", "rcg_sorted", "rcg_stored", "stride", "stride2")
BATCH_ARRAYS = dict(permA=(2, np.int32), permT=(3, np.int32), posN=(4, np.int32), posM=(5, np.int32), qposA=(6, np.int32), slA=(7, np.uint32),
                    slT=(8, np.uint32), pdiag=(9, None), pdiag_has=(10, np.uint8))
MEMBER_ARRAYS = dict(img=(0, np.uint8), img2=(1, np.uint8), um_imgA=(11, np.int32), um_imgA2=(12, np.int32), um_imgP=(13, np.int32), um_pd=(14, np.int32),
                     um_A=(15, np.int32), um_PT=(16, np.int32))


def _probe(dtype):
    f32 = np.dtype(dtype) == np.float32
    if f32 not in _probes:
        import atexit, ctypes, shutil, subprocess, tempfile
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        csrc = os.path.join(root, "cosmo.jl_amd", "csrc")
        tmp = tempfile.mkdtemp(prefix="batch_image_probe_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "batch_image_probe.so")
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall"] + (["-DCOSMO_HIP_REAL_FLOAT"] if f32 else []) +
                       ["-I" + csrc, "-o", so, os.path.join(root, "tests", "batch_image_probe.cpp"), os.path.join(csrc, "batch_image.cpp"),
                        os.path.join(csrc, "value_maps.cpp")], check=True)
        lib = ctypes.CDLL(so)
        P = ctypes.c_void_p
        lib.bimg_probe_new.restype = P; lib.bimg_probe_new.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong]
        lib.bimg_probe_free.argtypes = [P]
        lib.bimg_probe_set.argtypes = [P, ctypes.c_int] + [P] * 6
        lib.bimg_probe_corrupt.argtypes = [P, ctypes.c_int, ctypes.c_int]
        lib.bimg_probe_plan.argtypes = [P, P, P, ctypes.c_int, ctypes.c_longlong]
        lib.bimg_probe_error.restype = ctypes.c_char_p; lib.bimg_probe_error.argtypes = [P]
        lib.bimg_probe_flags.argtypes = [P, P]
        lib.bimg_probe_get.restype = ctypes.c_longlong; lib.bimg_probe_get.argtypes = [P, ctypes.c_int, ctypes.c_int, P]
        assert lib.bimg_probe_real_bytes() == (4 if f32 else 8)
        _probes[f32] = lib
    return _probes[f32]


def opts_of(case):
    """the eleven switches as batch.hip parses them: unset = the default, LDS / REG / ... = 0 disables, EXT != 0 enables, BS as given"""
    env = CASES[case]["env"]
    on = lambda k: int(not (k in env and int(env[k]) == 0))
    return [int(env.get("BS", 512)) if k == "BS" else (int(int(env.get("EXT", 0)) != 0) if k == "EXT" else on(k)) for k in SWITCHES]


def plan(case, max_lds=MAX_LDS, corrupt=None):
    """the planner's answer for the case: dict of the flags, error, the whole-batch arrays and lists over the members of the per-member arrays.
    corrupt = (k, t): entry t of member k's staged A' is changed first"""
    from cosmo_jl_amd._ffi import csc_julia
    c, f, dtype = CASES[case], family(CASES[case]["family"]), dtype_of(case)
    lib = _probe(dtype)
    h = lib.bimg_probe_new(f.nprob, f.n, f.m)
    try:
        for k in range(f.nprob):
            arrs = csc_julia(f.P[k], dtype) + csc_julia(f.A[k], dtype)
            assert lib.bimg_probe_set(h, k, *[a.ctypes.data for a in arrs]) == 0
        if corrupt is not None:
            lib.bimg_probe_corrupt(h, *corrupt)
        o = np.array(opts_of(case), dtype=np.int32); cones = np.array(f.cone_counts(), dtype=np.int32)
        rc = lib.bimg_probe_plan(h, o.ctypes.data, cones.ctypes.data, int(c["aa"]), int(max_lds))
        fl = np.zeros(len(FLAGS), dtype=np.int64)
        lib.bimg_probe_flags(h, fl.ctypes.data)
        out = dict(zip(FLAGS, (int(v) for v in fl)))
        out["error"] = lib.bimg_probe_error(h).decode() if rc else ""

        def get(which, k, dt):
            a = np.zeros(lib.bimg_probe_get(h, which, k, None), dtype=np.uint8)
            lib.bimg_probe_get(h, which, k, a.ctypes.data)
            return a.view(dtype if dt is None else dt)
        for name, (which, dt) in BATCH_ARRAYS.items():
            out[name] = get(which, 0, dt)
        for name, (which, dt) in MEMBER_ARRAYS.items():
            out[name] = [get(which, k, dt) for k in range(f.nprob)]
    finally:
        lib.bimg_probe_free(h)
    return out


def image_bytes(pl, k, sliced, n):
    """what get_image(k) returns for the plan: the member's image padded to the batch's stride, then its row of pdiag when P is in registers"""
    img, stride = (pl["img2"][k], pl["stride2"]) if sliced else (pl["img"][k], pl["stride"])
    out = np.zeros(stride, dtype=np.uint8); out[:img.size] = img
    return np.concatenate([out, pl["pdiag"][k * n:(k + 1) * n].view(np.uint8)]) if sliced and pl["pdiag"].size else out


def host_hashes(pl):
    """SHA-256 of the arrays the library cannot export"""
    out = {name: sha(pl[name]) for name in ("permA", "permT", "posN", "posM", "qposA", "slA", "slT", "pdiag_has")}
    for name in ("um_imgA", "um_imgA2", "um_imgP", "um_pd"):
        out[name] = sha(*[np.concatenate([np.array([a.size], dtype=np.int32), a]) for a in pl[name]])
    return out


def finalized_batch(case):
    """the case's batch through the library, set_params done (the caller has set env_of(case)); parameters of tests/test_gpu_batch_update_matrices.py"""
    from cosmo_jl_amd import _ffi
    c, f, dtype = CASES[case], family(CASES[case]["family"]), dtype_of(case)
    B = _ffi.Batch(f.nprob, f.n, f.m, 0, dtype=dtype)
    for k in range(f.nprob):
        B.set_problem(k, f.P[k], f.q[k], f.A[k], f.b[k])
    B.set_cones(f.cone_types, f.cone_dims, f.box_l if f.box_l.size else None, f.box_u if f.box_u.size else None)
    if c["aa"]:
        B.set_accelerator()
    p = _ffi.default_params(dtype)
    p.kkt_kind = _ffi.KKT_CG
    p.tol_constant, p.tol_exponent = (1e-4, 0.0) if dtype == np.float32 else (1e-9, 0.0)
    p.adaptive_rho_interval = 10
    B.set_params(p)
    return B


def answers(case, B):
    """what the fixture records of a finalised batch: SHA-256 of every member's get_image, kernel_info(), and for the kernel forms SHA-256 of every
    member's iterates after set_iterates(start) and iterate(30, with_init=True)"""
    f = family(CASES[case]["family"])
    out = dict(image=[sha(B.get_image(k)) for k in range(f.nprob)], kernel_info=B.kernel_info())
    if CASES[case]["iterates"]:
        B.set_iterates(*f.start)
        B.iterate(30, with_init=True)
        its = [B.get_iterates(k) for k in range(f.nprob)]
        assert all(np.all(np.isfinite(a)) for it in its for a in it)
        out["iterates"] = [sha(*it) for it in its]
    return out
