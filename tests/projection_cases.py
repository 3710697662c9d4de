"""Inputs for the cone projections of the persistent batch kernels (csrc/batch.hip: proj_simple, the second-order-cone routines of batch_admm_body and of
k_batch_admm_reg, batch_project_psd, batch_project_psd_mid, batch_project_cone3) and a plain reference written from the definitions.  No test
functions, no GPU code, nothing from the oracle: imported by test_projection_cases_host.py (CPU) and test_gpu_batch_projections.py (GPU).

A CASE is one cone structure with a handful of MEMBERS (row vectors of that structure): one batch.  Every cone of every member carries a tag that says
what the tests hold it to:

  exact     the expected output is a bit pattern (simple cones; second-order cones whose sum of squares is exact in any summation order and whose
            scale factor is a dyadic rational)
  random    second-order cone, closed form in long double:  ||out - ref|| <= 8 eps d ||x||          (the bound of test_project_soc)
  psd       PSD cone, eigh in float64:                      ||out - ref||_F <= 64 d eps ||X||_F     (check_projection / SURVEY 8c)
  gapped    psd, and min |lambda| >= 0.1 ||X||_2: the rank is unambiguous, eigvalsh(out) >= -64 d eps ||X||_F is asserted too
  zero      psd, the zero matrix: exact zeros
  cone3     exponential / power cone or a dual: the result lies in the cone and result - input in its dual, both to 1e-3 (the membership tolerance
            of test_projection_matches_oracle), checked from the definitions (cone3_violation)
  poison    a second-order cone that holds one NaN: every row of it comes back NaN, nothing else does

Which line of the kernels a case is there for:

  soc_exact_small     d = 1 (the empty sum), the ties nx == t and nx == -t, (0, 3, 4), zeros; d - 1 in {64, 65, 128}: one / two trips of the lane loop
  soc_exact_1025      d - 1 = 1024 entries of +-1, ||x|| = 32: sixteen trips, m > 1024 (the register kernel <512, 2, 4>)
  soc_exact_4097      d - 1 = 4096 entries of +-1, ||x|| = 64: more rows than the register kernel holds
  soc_random          dims 1, 2, 3, 63, 64, 65, 66, 129, 1000, every cone in every branch (one member per rotation)
  soc_64_cones        64 cones = JS * (BS / 64): the register kernel keeps offsets and dims in registers (soc_in_regs)
  soc_70_cones        70 cones: the register kernel's other loop; d = 1 cones and a cone longer than a wave
  psd_small_*         sides 2, 3, 8, 15, 16, triangle and square, ten spectra each: more cones than wave workspaces, every workspace reused
  psd_19_small        19 cones of mixed sides in one member: more than any psd_nws (at most 8)
  psd_side_one        PsdCone(1) / PsdConeTriangle(1) next to larger cones: set_params gives their row the Nonnegatives rule (batch.hip, "the 1-D case is
                      max(x, 0)"), so NaN stays and -0.0 becomes +0.0 -- tagged exact
  psd_mid_*           sides 17, 24, 25, 32, 33, 48, 63, 64 (ld = 32, 48, 64; ncp = 32 .. 64: the padding edges of the psdG slab), ten spectra each
  psd_mid_three       three mid cones of different sides in one member: mid_goff
  cone3_*             300 cones of one kind per member: one thread per cone, two trips of the 256-thread loop of the streaming kernel
  mixed               every kind interleaved with ZeroSet / Nonnegatives / Box rows
  poison              NaN, +-inf, -0.0 in simple rows and one NaN inside one second-order cone of ONE member; `clean` is the same batch without that member
"""
import dataclasses
import math

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)

ZERO, NONNEG, BOX, SOC, PSD_TRI, PSD_SQ, EXP, DUAL_EXP, POW, DUAL_POW = ("zero", "nonneg", "box", "soc", "psd_tri", "psd_sq", "exp", "dual_exp",
                                                                        "pow", "dual_pow")
SIMPLE = (ZERO, NONNEG, BOX)
PSD = (PSD_TRI, PSD_SQ)
CONE3 = (EXP, DUAL_EXP, POW, DUAL_POW)
SOC_RANDOM_DIMS = [1, 2, 3, 63, 64, 65, 66, 129, 1000]
SMALL_SIDES = [2, 3, 8, 15, 16]
MID_SIDES = [17, 24, 25, 32, 33, 48, 63, 64]
SPECTRA = ["psd", "negdef", "zero", "cI", "clusters", "pair", "1e8", "1e-9", "gapped", "rank1"]
GAPPED_SPECTRA = ("cI", "clusters", "pair", "1e8", "1e-9", "gapped")
CONE3_TOL = 1e-3


@dataclasses.dataclass
class Cone:
    kind: str
    dim: int
    l: object = None             # Box
    u: object = None
    alpha: float = 0.0           # power cones

    @property
    def side(self):
        if self.kind == PSD_SQ:
            return int(round(math.sqrt(self.dim)))
        if self.kind == PSD_TRI:
            return int((math.isqrt(1 + 8 * self.dim) - 1) // 2)
        return 0


@dataclasses.dataclass
class Member:
    rows: np.ndarray             # float64, one entry per row of the structure
    tags: list                   # one per cone
    branch: list                 # one per cone: the branch a second-order cone is built to take (0 unchanged, 1 zeros, 2 scaled), else -1
    note: list                   # one per cone: the name of the spectrum / of the special value, for messages


@dataclasses.dataclass
class Case:
    name: str
    cones: list
    members: list
    float32: bool = False        # the Float32 library runs it too (second-order, small PSD, mixed, simple)
    clean: object = None         # poison: the indices of the members that also form the batch without the poisoned one

    @property
    def m(self):
        return sum(c.dim for c in self.cones)

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum([c.dim for c in self.cones])]).astype(np.int64)

    @property
    def mid_sides(self):
        return [c.side for c in self.cones if c.kind in PSD and c.side > 16]


# ---- layouts of the PSD cones ------------------------------------------------------------------------------------------------------------------
def svec(X):
    """column-major upper triangle, off-diagonals times sqrt(2) (src/convexset.jl:462-472)"""
    d = X.shape[0]
    jj, ii = np.tril_indices(d)                                              # j outer, i <= j inner
    return np.where(ii == jj, X[ii, jj], math.sqrt(2.0) * X[ii, jj])


def smat(x, d):
    X = np.zeros((d, d))
    jj, ii = np.tril_indices(d)
    v = np.where(ii == jj, x, np.asarray(x, dtype=np.float64) / math.sqrt(2.0))
    X[ii, jj] = v
    X[jj, ii] = v
    return X


def psd_matrix(x, cone):
    """the symmetric matrix a PSD cone's rows stand for, in float64 (square layout: symmetrised)"""
    d = cone.side
    x = np.asarray(x, dtype=np.float64)
    if cone.kind == PSD_TRI:
        return smat(x, d)
    X = x.reshape(d, d, order="F")
    return (X + X.T) / 2.0


def psd_rows(X, cone):
    return svec(X) if cone.kind == PSD_TRI else X.reshape(-1, order="F")


def psd_bound(X, d, eps):
    return 64.0 * d * eps * float(np.linalg.norm(X))


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------
def ref_simple(x, cone):
    """Nonnegatives: Julia's max(x, 0) (NaN stays, -0.0 -> +0.0); Box: clip (src/algebra.jl:5-7); ZeroSet: zeros.  Comparisons only: exact in any type."""
    x = np.asarray(x)
    zero = x.dtype.type(0.0)
    if cone.kind == ZERO:
        return np.zeros_like(x)
    if cone.kind == NONNEG:
        return np.where(np.isnan(x), x, np.where(x > zero, x, zero))
    lo, hi = np.asarray(cone.l, dtype=x.dtype), np.asarray(cone.u, dtype=x.dtype)
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def ref_soc(x):
    """(projection, branch): the closed form (src/convexset.jl:100-114) in long double, rounded once to the type of x"""
    x = np.asarray(x)
    if x.size == 0:
        return x.copy(), 0
    v = x.astype(LD)
    t = v[0]
    nx = np.sqrt(np.sum(v[1:] * v[1:])) if x.size > 1 else LD(0.0)
    if nx <= t:
        return x.copy(), 0
    if nx <= -t:
        return np.zeros_like(x), 1
    out = np.empty_like(v)
    out[0] = (nx + t) / LD(2.0)
    out[1:] = (nx + t) / (LD(2.0) * nx) * v[1:]
    return out.astype(x.dtype), 2


def ref_psd(x, cone):
    """numpy.linalg.eigh in float64 on the symmetrised input, the spectrum clipped at zero, rebuilt; rounded once to the type of x"""
    x = np.asarray(x)
    if cone.dim == 1:                                                         # max(x, 0): the Nonnegatives rule (src/convexset.jl:303-305, 404-405)
        return ref_simple(x, Cone(NONNEG, 1))
    X = psd_matrix(x, cone)
    w, V = np.linalg.eigh(X)
    Xp = (V * np.maximum(w, 0.0)) @ V.T
    Xp = (Xp + Xp.T) / 2.0
    return psd_rows(Xp, cone).astype(x.dtype)


def project_reference(cones, rows):
    """(out, branches): every cone but the 3-d ones projected by the reference in the type of rows; the rows of exponential / power cones come back NaN
    (they have no closed form: cone3_violation checks a result against the definition instead)"""
    rows = np.asarray(rows)
    out = np.empty_like(rows)
    branches = []
    off = 0
    for c in cones:
        x = rows[off:off + c.dim]
        br = -1
        if c.kind in SIMPLE:
            out[off:off + c.dim] = ref_simple(x, c)
        elif c.kind == SOC:
            out[off:off + c.dim], br = ref_soc(x)
        elif c.kind in PSD:
            out[off:off + c.dim] = ref_psd(x, c)
        else:
            out[off:off + c.dim] = np.nan
        branches.append(br)
        off += c.dim
    return out, branches


# ---- the 3-d cones from their definitions ----------------------------------------------------------------------------------------------------------
def _in_exp(v, tol):
    """K_exp = cl {(x, y, z): y > 0, y exp(x / y) <= z}"""
    x, y, z = (float(t) for t in v)
    if y > 0 and x / y < 700.0 and y * math.exp(x / y) <= z + tol:
        return True
    return x <= tol and abs(y) <= tol and z >= -tol                           # the closure: {x <= 0, y = 0, z >= 0}


def _in_exp_dual(v, tol):
    """K_exp* = cl {(u, v, w): u < 0, -u exp(v / u) <= e w}"""
    u, v_, w = (float(t) for t in v)
    if u < 0 and v_ / u < 700.0 and -u * math.exp(v_ / u) - math.e * w <= tol:
        return True
    return abs(u) <= tol and v_ >= -tol and w >= -tol                         # the closure: {u = 0, v >= 0, w >= 0}


def _in_pow(v, a, tol):
    """K_pow(a) = {(x, y, z): x, y >= 0, x^a y^(1 - a) >= |z|}"""
    x, y, z = (float(t) for t in v)
    return x >= -tol and y >= -tol and max(x, 0.0) ** a * max(y, 0.0) ** (1.0 - a) >= abs(z) - tol


def _in_pow_dual(v, a, tol):
    """K_pow(a)* = {(u, v, w): u, v >= 0, (u / a)^a (v / (1 - a))^(1 - a) >= |w|}"""
    u, v_, w = (float(t) for t in v)
    return u >= -tol and v_ >= -tol and (max(u, 0.0) / a) ** a * (max(v_, 0.0) / (1.0 - a)) ** (1.0 - a) >= abs(w) - tol


def cone3_violation(cone, v, p, tol=CONE3_TOL):
    """p = Proj_K(v) iff p in K, p - v in K* and <p, p - v> = 0.  Returns the list of the conditions p misses (empty: p passes), membership to `tol`
    relative to max(1, ||v||_inf), the complementarity to tol * max(1, ||v||^2)."""
    v = np.asarray(v, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    sc = max(1.0, float(np.max(np.abs(v))))
    a = cone.alpha
    prim = {EXP: lambda y: _in_exp(y, tol), DUAL_EXP: lambda y: _in_exp_dual(y, tol), POW: lambda y: _in_pow(y, a, tol),
            DUAL_POW: lambda y: _in_pow_dual(y, a, tol)}
    dual = {EXP: DUAL_EXP, DUAL_EXP: EXP, POW: DUAL_POW, DUAL_POW: POW}
    bad = []
    if not np.isfinite(p).all():
        return ["finite"]
    if not prim[cone.kind](p / sc):
        bad.append("in_cone")
    if not prim[dual[cone.kind]]((p - v) / sc):
        bad.append("residual_in_dual")
    if abs(float(p @ (p - v))) > tol * max(1.0, float(v @ v)):
        bad.append("complementarity")
    return bad


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------------
class _Builder:
    """collects (cone, rows, tag, branch, note) per member; every member of a case must produce the same structure"""

    def __init__(self):
        self.cones, self.rows, self.tags, self.branch, self.note = [], [], [], [], []

    def add(self, cone, rows, tag, branch=-1, note=""):
        rows = np.asarray(rows, dtype=np.float64).ravel()
        assert rows.size == cone.dim, (cone, rows.size)
        self.cones.append(cone); self.rows.append(rows); self.tags.append(tag); self.branch.append(branch); self.note.append(note)

    def member(self):
        return Member(np.concatenate(self.rows) if self.rows else np.zeros(0), self.tags, self.branch, self.note)


def _case(name, builders, **kw):
    first = builders[0].cones
    for b in builders[1:]:
        assert [(c.kind, c.dim, c.alpha) for c in b.cones] == [(c.kind, c.dim, c.alpha) for c in first], name
    return Case(name, first, [b.member() for b in builders], **kw)


def _box(rng, k):
    l = rng.standard_normal(k) - 1.0
    u = l + rng.uniform(0.0, 2.0, k)
    if k >= 4:
        l[0] = -np.inf; u[1] = np.inf; u[2] = l[2]                            # one-sided, one-sided, an equality row
    return Cone(BOX, k, l, u)


def _simple_rows(rng, k):
    s = rng.standard_normal(k) * 2.0
    s[::5] = 0.0
    s[3::7] = -0.0
    return s


def simple_case():
    bs = []
    boxes = [_box(np.random.default_rng(100), 40), _box(np.random.default_rng(101), 7)]
    for k in range(4):
        rng = np.random.default_rng(110 + k)
        b = _Builder()
        b.add(Cone(NONNEG, 70), _simple_rows(rng, 70), "exact")
        b.add(Cone(ZERO, 13), _simple_rows(rng, 13), "exact")
        b.add(boxes[0], _simple_rows(rng, 40), "exact")
        b.add(Cone(NONNEG, 1), [(-1.0) ** k * 0.5], "exact")
        b.add(Cone(ZERO, 30), _simple_rows(rng, 30), "exact")
        b.add(boxes[1], _simple_rows(rng, 7), "exact")
        bs.append(b)
    return _case("simple", bs, float32=True)


def _exact_tail(rng, count, n3, n4):
    """count entries from {0, +-3, +-4}: n3 threes and n4 fours with random signs, shuffled -- every partial sum of squares is a small integer"""
    v = np.zeros(count)
    v[:n3] = 3.0
    v[n3:n3 + n4] = 4.0
    v *= rng.choice([-1.0, 1.0], count)
    rng.shuffle(v)
    return v


_T_CHOICES = [(1.0, 0), (-1.0, 1), (0.0, 2), (0.5, 2)]      # t / ||x|| and the branch: the two ties, f = 1/2, f = 3/4 (dyadic: one rounding in the kernel too)


def soc_exact_small_case():
    bs = []
    ones = [2.5, -2.5, 0.0, -0.0]
    triples = [((5.0, 3.0, 4.0), 0), ((-5.0, 3.0, 4.0), 1), ((0.0, 3.0, 4.0), 2), ((0.0, 0.0, 0.0), 0)]
    tails = [(64, 16, 16, 20.0), (65, 16, 16, 20.0), (128, 64, 64, 40.0)]     # 9 * 16 + 16 * 16 = 400, 9 * 64 + 16 * 64 = 1600
    for k in range(4):
        rng = np.random.default_rng(200 + k)
        b = _Builder()
        for i in range(4):
            t = ones[(i + k) % 4]
            b.add(Cone(SOC, 1), [t], "exact", 1 if t < 0 else 0, "d=1 t=%r" % t)
        for (t, a, c), br in triples:
            sa, sc = rng.choice([-1.0, 1.0], 2)
            tail = (a * sa, c * sc) if k % 2 == 0 else (c * sc, a * sa)
            b.add(Cone(SOC, 3), (t,) + tail, "exact", br, "triple t=%r" % t)
        for i, (cnt, n3, n4, nx) in enumerate(tails):
            f, br = _T_CHOICES[(i + k) % 4]
            b.add(Cone(SOC, cnt + 1), np.concatenate([[f * nx], _exact_tail(rng, cnt, n3, n4)]), "exact", br, "tail %d t=%r" % (cnt, f * nx))
        bs.append(b)
    return _case("soc_exact_small", bs, float32=True)


def soc_exact_long_case(count, nx):
    bs = []
    for k, (f, br) in enumerate(_T_CHOICES):
        rng = np.random.default_rng(300 + count + k)
        b = _Builder()
        b.add(Cone(SOC, count + 1), np.concatenate([[f * nx], rng.choice([-1.0, 1.0], count)]), "exact", br, "ones %d t=%r" % (count, f * nx))
        bs.append(b)
    return _case("soc_exact_%d" % (count + 1), bs, float32=True)


def _soc_random_rows(rng, d, br):
    """all three branches forced, as test_project_soc does, with room to spare: t = +-(2 ||x|| + 1) for the first two, |t| = ||x|| / 2 for the third"""
    x = rng.standard_normal(d)
    nx = float(np.linalg.norm(x[1:]))
    if br == 0:
        x[0] = 2.0 * nx + 1.0
    elif br == 1:
        x[0] = -(2.0 * nx + 1.0)
    elif d == 1:
        br = 0 if x[0] >= 0 else 1                                            # d = 1: ||x|| = 0, the third branch does not exist
    else:
        x[0] = math.copysign(0.5 * nx, x[0])
    return x, br


def soc_dims_case(name, dims, seed):
    bs = []
    for k in range(3):
        rng = np.random.default_rng(seed + k)
        b = _Builder()
        for i, d in enumerate(dims):
            x, br = _soc_random_rows(rng, d, (i + k) % 3)
            b.add(Cone(SOC, d), x, "random", br, "d=%d" % d)
        bs.append(b)
    return _case(name, bs, float32=True)


def _sym_with_spectrum(rng, lam):
    d = lam.size
    Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    X = (Q * lam) @ Q.T
    return (X + X.T) / 2.0


def _gapped_spectrum(rng, d):
    npos = int(rng.integers(0, d + 1))
    lam = np.concatenate([rng.uniform(0.35, 2.0, npos), -rng.uniform(0.35, 2.0, d - npos)])
    rng.shuffle(lam)
    return lam


def spectrum_matrix(rng, d, name):
    """the eight matrices of test_psd_special_spectra, one gapped random spectrum, one rank-1 matrix"""
    B = rng.standard_normal((d, d))
    if name == "psd":
        return B @ B.T / d + 0.2 * np.eye(d)
    if name == "negdef":
        return -(B @ B.T / d + 0.2 * np.eye(d))
    if name == "zero":
        return np.zeros((d, d))
    if name == "cI":
        return 3.0 * np.eye(d)
    if name == "clusters":
        return _sym_with_spectrum(rng, np.concatenate([np.full(d // 2, 1.5), np.full(d - d // 2, -0.7)]))
    if name == "pair":
        return _sym_with_spectrum(rng, np.concatenate([[3.0, -3.0], _gapped_spectrum(rng, d - 2)]))
    if name == "1e8":
        return 1e8 * _sym_with_spectrum(rng, _gapped_spectrum(rng, d))
    if name == "1e-9":
        return 1e-9 * _sym_with_spectrum(rng, _gapped_spectrum(rng, d))
    if name == "gapped":
        return _sym_with_spectrum(rng, _gapped_spectrum(rng, d))
    v = rng.standard_normal(d)
    return np.outer(v, v)


def _add_psd(b, rng, d, kind, name):
    X = spectrum_matrix(rng, d, name)
    cone = Cone(kind, d * (d + 1) // 2 if kind == PSD_TRI else d * d)
    if kind == PSD_SQ and name not in ("zero", "cI"):                         # the square layout is symmetrised by the kernel: hand it an unsymmetric matrix
        R = rng.standard_normal((d, d))
        X = X + 0.25 * (np.linalg.norm(X, 2) / math.sqrt(d)) * (R - R.T) / 2.0
        rows = X.reshape(-1, order="F")
    else:
        rows = psd_rows(X, cone)
    b.add(cone, rows, "zero" if name == "zero" else ("gapped" if name in GAPPED_SPECTRA else "psd"), note="side %d %s %s" % (d, kind, name))


def psd_spectra_case(name, sides, kind, spectra, members, seed, per_member=None, **kw):
    """members x cones: member k takes, for every side, the spectra[k * per_member : (k + 1) * per_member] (per_member None: all of them, redrawn)"""
    bs = []
    for k in range(members):
        rng = np.random.default_rng(seed + k)
        b = _Builder()
        names = spectra if per_member is None else [spectra[(k * per_member + j) % len(spectra)] for j in range(per_member)]
        for d in sides:
            for nm in names:
                _add_psd(b, rng, d, kind, nm)
        bs.append(b)
    return _case(name, bs, **kw)


def psd_19_small_case():
    sides = [2, 16, 3, 15, 8, 5, 2, 9, 16, 3, 7, 15, 4, 8, 2, 16, 3, 12, 6]
    assert len(sides) == 19
    bs = []
    for k in range(3):
        rng = np.random.default_rng(500 + k)
        b = _Builder()
        for i, d in enumerate(sides):
            _add_psd(b, rng, d, PSD_TRI if i % 2 == 0 else PSD_SQ, SPECTRA[(i + 3 * k) % len(SPECTRA)])
        bs.append(b)
    return _case("psd_19_small", bs, float32=True)


def psd_side_one_case():
    bs = []
    vals = [(1.5, -2.0), (-0.0, np.nan), (-3.0, 0.25), (np.nan, -0.0)]
    for k in range(4):
        rng = np.random.default_rng(520 + k)
        b = _Builder()
        _add_psd(b, rng, 4, PSD_TRI, "gapped")
        b.add(Cone(PSD_SQ, 1), [vals[k][0]], "exact", note="PsdCone(1) %r" % vals[k][0])
        _add_psd(b, rng, 3, PSD_SQ, "gapped")
        b.add(Cone(PSD_TRI, 1), [vals[k][1]], "exact", note="PsdConeTriangle(1) %r" % vals[k][1])
        _add_psd(b, rng, 16, PSD_TRI, "clusters")
        bs.append(b)
    return _case("psd_side_one", bs, float32=True)


def psd_mid_three_case():
    bs = []
    for k in range(3):
        rng = np.random.default_rng(540 + k)
        b = _Builder()
        _add_psd(b, rng, 33, PSD_TRI, SPECTRA[(4 + k) % 10])
        b.add(Cone(NONNEG, 3), rng.standard_normal(3), "exact")
        _add_psd(b, rng, 17, PSD_SQ, SPECTRA[(8 + k) % 10])
        _add_psd(b, rng, 5, PSD_TRI, "gapped")
        _add_psd(b, rng, 48, PSD_TRI, SPECTRA[(5 + k) % 10])
        bs.append(b)
    return _case("psd_mid_three", bs)


def cone3_inputs(rng, nc):
    """the sampling of test_projection_matches_oracle: uniform in [-25, 25]^3, the first rows scaled by 1e-3, rows with z = 0 and with y = 0"""
    X = -25.0 + 50.0 * rng.random((nc, 3))
    X[:50] *= 1e-3
    X[50:60, 2] = 0.0
    X[60:70, 1] = 0.0
    return X


def cone3_case(kind, nc=300):
    alphas = (0.1 + 0.85 * np.random.default_rng(600).random(nc)) if kind in (POW, DUAL_POW) else np.zeros(nc)
    bs = []
    for k in range(3):
        X = cone3_inputs(np.random.default_rng(610 + 10 * CONE3.index(kind) + k), nc)
        b = _Builder()
        for i in range(nc):
            b.add(Cone(kind, 3, alpha=float(alphas[i])), X[i], "cone3")
        bs.append(b)
    return _case("cone3_" + kind, bs)


def _mixed_builder(rng, boxes, poison=False):
    """every kind, with ZeroSet / Nonnegatives / Box rows between the cones (as test_psd_one_by_one_and_mixed_composite interleaves them)"""
    b = _Builder()
    b.add(Cone(NONNEG, 5), _simple_rows(rng, 5), "exact")
    b.add(Cone(PSD_TRI, 1), rng.standard_normal(1), "exact")
    b.add(Cone(PSD_SQ, 1), rng.standard_normal(1), "exact")
    x, br = _soc_random_rows(rng, 4, 2)
    b.add(Cone(SOC, 4), x, "random", br)
    b.add(Cone(ZERO, 2), rng.standard_normal(2), "exact")
    _add_psd(b, rng, 4, PSD_TRI, "gapped")
    b.add(boxes[0], _simple_rows(rng, 6), "exact")
    _add_psd(b, rng, 3, PSD_SQ, "pair")
    b.add(Cone(EXP, 3), -25.0 + 50.0 * rng.random(3), "cone3")
    b.add(Cone(NONNEG, 2), rng.standard_normal(2), "exact")
    b.add(Cone(POW, 3, alpha=0.3), -25.0 + 50.0 * rng.random(3), "cone3")
    b.add(Cone(SOC, 1), rng.standard_normal(1), "random", -1)
    b.add(Cone(DUAL_EXP, 3), -25.0 + 50.0 * rng.random(3), "cone3")
    b.add(Cone(ZERO, 1), rng.standard_normal(1), "exact")
    b.add(Cone(DUAL_POW, 3, alpha=0.7), -25.0 + 50.0 * rng.random(3), "cone3")
    _add_psd(b, rng, 6, PSD_TRI, "clusters")
    b.add(boxes[1], _simple_rows(rng, 4), "exact")
    x, br = _soc_random_rows(rng, 70, 2)
    b.add(Cone(SOC, 70), x, "random", br)
    b.add(Cone(NONNEG, 3), _simple_rows(rng, 3), "exact")
    if poison:
        r = b.rows
        r[0][:] = [np.nan, np.inf, -np.inf, -0.0, 1.0]                         # Nonnegatives
        r[4][:] = [np.nan, -np.inf]                                            # ZeroSet
        r[6][:] = [np.nan, np.inf, -np.inf, -0.0, 0.5, np.inf]                 # Box (rows 0, 1: one-sided bounds; 2: equality)
        r[17][33] = np.nan                                                     # one NaN inside SecondOrderCone(70)
        b.tags[17] = "poison"; b.branch[17] = -1
        r[18][:] = [np.inf, np.nan, -0.0]
    for i, c in enumerate(b.cones):
        if c.kind == SOC and b.branch[i] == -1 and b.tags[i] == "random":
            b.branch[i] = ref_soc(b.rows[i])[1]
    return b


def mixed_case():
    boxes = [_box(np.random.default_rng(700), 6), _box(np.random.default_rng(701), 4)]
    return _case("mixed", [_mixed_builder(np.random.default_rng(710 + k), boxes) for k in range(4)], float32=True)


def poison_case():
    """members 0, 1, 3 are clean; member 2 carries the poison.  `clean` = the batch of members 0, 1, 3 alone."""
    boxes = [_box(np.random.default_rng(700), 6), _box(np.random.default_rng(701), 4)]
    bs = [_mixed_builder(np.random.default_rng(720 + k), boxes, poison=(k == 2)) for k in range(4)]
    return _case("poison", bs, float32=True, clean=[0, 1, 3])


def _soc_many_dims(count, seed, long_one):
    rng = np.random.default_rng(seed)
    dims = [int(d) for d in rng.choice([1, 2, 3, 4, 5, 7, 9, 16, 31], count)]
    dims[0] = 1; dims[count // 2] = 1; dims[-1] = 1
    dims[3] = long_one
    dims[count - 2] = 66
    return dims


CASES = {
    "simple": simple_case,
    "soc_exact_small": soc_exact_small_case,
    "soc_exact_1025": lambda: soc_exact_long_case(1024, 32.0),
    "soc_exact_4097": lambda: soc_exact_long_case(4096, 64.0),
    "soc_random": lambda: soc_dims_case("soc_random", SOC_RANDOM_DIMS, 400),
    "soc_64_cones": lambda: soc_dims_case("soc_64_cones", _soc_many_dims(64, 410, 65), 420),
    "soc_70_cones": lambda: soc_dims_case("soc_70_cones", _soc_many_dims(70, 411, 130), 430),
    "psd_small_2_3_8_tri": lambda: psd_spectra_case("psd_small_2_3_8_tri", [2, 3, 8], PSD_TRI, SPECTRA, 3, 800, float32=True),
    "psd_small_2_3_8_sq": lambda: psd_spectra_case("psd_small_2_3_8_sq", [2, 3, 8], PSD_SQ, SPECTRA, 3, 810, float32=True),
    "psd_small_15_tri": lambda: psd_spectra_case("psd_small_15_tri", [15], PSD_TRI, SPECTRA, 3, 820, float32=True),
    "psd_small_15_sq": lambda: psd_spectra_case("psd_small_15_sq", [15], PSD_SQ, SPECTRA, 4, 830, per_member=5, float32=True),
    "psd_small_16_tri": lambda: psd_spectra_case("psd_small_16_tri", [16], PSD_TRI, SPECTRA, 3, 840, float32=True),
    "psd_small_16_sq": lambda: psd_spectra_case("psd_small_16_sq", [16], PSD_SQ, SPECTRA, 4, 850, per_member=5, float32=True),
    "psd_19_small": psd_19_small_case,
    "psd_side_one": psd_side_one_case,
    "psd_mid_three": psd_mid_three_case,
    "cone3_exp": lambda: cone3_case(EXP),
    "cone3_dual_exp": lambda: cone3_case(DUAL_EXP),
    "cone3_pow": lambda: cone3_case(POW),
    "cone3_dual_pow": lambda: cone3_case(DUAL_POW),
    "mixed": mixed_case,
    "poison": poison_case,
}
for _d in MID_SIDES:
    for _kind in (PSD_TRI, PSD_SQ):
        # five members; two of the ten spectra per member, or -- where two cones of that side do not fit one workgroup's LDS image (side 63 / 64 square:
        # 3969 / 4096 rows each) -- one per member in two cases
        _dim = _d * (_d + 1) // 2 if _kind == PSD_TRI else _d * _d
        _nm = "psd_mid_%d_%s" % (_d, "tri" if _kind == PSD_TRI else "sq")
        if 2 * _dim <= 4700:
            CASES[_nm] = (lambda nm=_nm, d=_d, kind=_kind: psd_spectra_case(nm, [d], kind, SPECTRA, 5, 900 + 7 * d, per_member=2))
        else:
            CASES[_nm + "_a"] = (lambda nm=_nm, d=_d, kind=_kind: psd_spectra_case(nm + "_a", [d], kind, SPECTRA[:5], 5, 900 + 7 * d, per_member=1))
            CASES[_nm + "_b"] = (lambda nm=_nm, d=_d, kind=_kind: psd_spectra_case(nm + "_b", [d], kind, SPECTRA[5:], 5, 950 + 7 * d, per_member=1))

_cases = {}


def case(name):
    """built once, shared, never modified"""
    if name not in _cases:
        c = CASES[name]()
        assert c.name == name, (c.name, name)
        for mb in c.members:
            mb.rows.setflags(write=False)
        _cases[name] = c
    return _cases[name]
