"""Input sequences and a definition-level reference for the Anderson accelerator, one update and one candidate at a time.  Host only: this module
does not import the GPU library.

The accelerator is fed pairs (g, x) = (w, w_prev): f = x - g; the first pair after a (re)start only stores (x, f, g); every later pair adds one
column of differences dX = x - x_last, dF = f - f_last, dG = g - g_last.  With the stored columns (all of them since the last restart for a restarted
memory, the latest `mem` for a rolling one; the memory is `mem = min(mem, N)` columns)

    Type2 (QR and normal equations):  eta = argmin || f - dF eta ||_2         Type1:  (dX' dF) eta = dX' f         candidate = g - dG eta.

A restarted memory that is full is emptied by the next update (the new column is its first again); a rolling memory overwrites its oldest column:
column number d (counted since the last restart) sits in slot j = d % mem.  No candidate while fewer than `min_mem` columns are stored; a step fails
when the factor is singular (an exactly zero or non-finite diagonal entry of R / pivot of the LU of M) or when ||eta||_2 > eta_max.
(oracle/cosmo_oracle.py, the comment above class AndersonAcceleratorNE.)

ReferenceAccelerator keeps the explicit (x, f, g) history, forms the differences in the working dtype -- as any implementation must, the inputs ARE
working-dtype numbers -- and solves in np.longdouble by Householder QR (Type2) or by LU with partial pivoting of M (Type1); it is the definition, not
a port of the kernels.

Error metric of a candidate:   e = ||cand - cand_ref|| / (cond * (||g|| + ||dG||_2 ||eta_ref||))   <=   C * eps(dtype),
cond = cond_2(dF) for the QR kind and cond_2(M) for the normal-equations kinds (M = dF'dF squares the condition number of dF).
"""
import numpy as np

LD = np.longdouble

# kind name -> (value of ACCEL_* in the library, type1, rolling, normal equations)
KINDS = {
    "qr": (1, False, False, False),
    "type1_restarted": (2, True, False, True),
    "type1_rolling": (3, True, True, True),
    "type2ne_restarted": (4, False, False, True),
    "type2ne_rolling": (5, False, True, True),
}
DTYPES = {"f64": np.float64, "f32": np.float32}
SEQUENCES = ("random", "contractive", "repeat", "near_dependent", "scaled_up", "scaled_down", "large_eta")
DEGENERATE = ("repeat", "near_dependent")
SCALE = {("scaled_up", "f64"): 1e100, ("scaled_down", "f64"): 1e-100, ("scaled_up", "f32"): 1e15, ("scaled_down", "f32"): 1e-15}
# (n, m, mem): the smallest shapes that reach each path of csrc/anderson.hip (tests/test_gpu_anderson_steps.py lists what each one reaches)
SHAPES = ((2, 6, 15), (10, 30, 32), (300, 725, 17), (1000, 2000, 9))
MIN_MEM = 3
ETA_MAX = 1e4
DEGENERATE_AT = 5            # index of the repeated / dependent pair: column 4 is the zero / dependent one, with at least min_mem good columns before it
PERTURBATION = 1e-7
# `large_eta`: the pairs of `random` times 2^-6 around one fixed pair (g0, x0).  The difference columns are those of `random` (cond(dF) < 1e2) times 2^-6
# while f stays of the size of x0 - g0, so ||eta|| is large by the size of f and not by ill-conditioning: with eta_max = 3 the test ||eta|| > eta_max
# fails most steps, passes some at N >= 1025, and is decidable in every kind and dtype (cond(M) stays below 1e6; measured ||eta|| 0.9 .. 7.5e4).
LARGE_ETA_STEP = 2.0 ** -6
ETA_MAX_OF = {"large_eta": 3.0}

# ---- the constant of the bound ------------------------------------------------------------------------------------------------------------------
# Worst e / eps64 of the oracle's AndersonAccelerator / AndersonAcceleratorNE (Float64 numpy) against ReferenceAccelerator over every kind, sequence,
# shape and min_mem of this file (tests/test_anderson_cases_host.py::test_the_constant_of_the_bound_is_the_measured_one measures it again and fails
# when it is exceeded).  Measured per kind: see ORACLE_WORST_BY_KIND.  C = max(4, 16 x the worst): the device sums in another order and contracts to
# FMA, and the Float32 library can only be measured through the Float64 oracle; the floor keeps a lucky measurement from making the bound flaky.
# 4.5e4 = 1e-11 / eps64 is the constant tests/test_oracle_anderson_definition.py anchors the oracle with: a measurement that asks for more is wrong.
ORACLE_WORST_BY_KIND = {"qr": 1.21, "type1_restarted": 0.67, "type1_rolling": 0.62, "type2ne_restarted": 0.77, "type2ne_rolling": 0.63}      # C_BOUND = 19.36
ORACLE_WORST_E_OVER_EPS = max(ORACLE_WORST_BY_KIND.values())
C_BOUND = max(4.0, 16.0 * ORACLE_WORST_E_OVER_EPS)
C_LIMIT = 1e-11 / np.finfo(np.float64).eps
assert C_BOUND <= C_LIMIT
# eta itself is less accurate than the candidate it produces (the candidate forgives an error of eta along the directions in which dG eta barely moves): the
# oracle's worst ||eta - eta_ref|| / (the bound of ReferenceAccelerator.eta_bound with C = 1), measured the same way over the same cases, is 20.8 for the
# QR kind (`contractive`, N = 8, step 11, cond 1.2e4: modified Gram-Schmidt and Q'f) and at most 3.2 for the others (`large_eta`, N = 3000); the host test
# named above measures these again too.  The bound on eta, and the margin inside which the decision ||eta|| <= eta_max is left open, use C_ETA.
ORACLE_WORST_ETA_BY_KIND = {"qr": 20.8, "type1_restarted": 2.96, "type1_rolling": 1.38, "type2ne_restarted": 3.17, "type2ne_rolling": 1.81}      # C_ETA = 332.8
ORACLE_WORST_ETA_OVER_EPS = max(ORACLE_WORST_ETA_BY_KIND.values())
C_ETA = max(C_BOUND, 16.0 * ORACLE_WORST_ETA_OVER_EPS)
assert C_ETA <= C_LIMIT


def eta_max_of(seq_name):
    return ETA_MAX_OF.get(seq_name, ETA_MAX)


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def gamma(k, dtype):
    """gamma_k = k u / (1 - k u), u = eps / 2 the unit roundoff: |fl(a'b) - a'b| <= gamma_k sum |a_i b_i| for k terms in ANY order of summation, with or without
    FMA (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  The tests use gamma_k = k eps / (1 - k eps), this bound with eps in place of u,
    i.e. twice as wide."""
    e = eps_of(dtype)
    return k * e / (1.0 - k * e)


# ---- sequences ----------------------------------------------------------------------------------------------------------------------------------
class Sequence:
    """pairs (g, x) in the working dtype.  `next(feedback)` returns pair number `count`; `feedback` is the candidate the implementation under test
    returned for the previous pair (only the contractive sequence uses it: it continues from the implementation's own candidate)."""

    def __init__(self, name, N, seed, dtype):
        assert name in SEQUENCES
        self.name, self.N, self.dtype = name, int(N), np.dtype(dtype)
        self.rng = np.random.default_rng([seed, self.N, SEQUENCES.index(name if not name.startswith("scaled") and name != "large_eta" else "random")])
        self.count = 0
        self.pairs = []
        self.factor = SCALE.get((name, "f32" if self.dtype == np.float32 else "f64"), 1.0)
        if name == "contractive":
            self.d = self.rng.uniform(0.1, 0.9, self.N).astype(self.dtype)
            self.c = self.rng.standard_normal(self.N).astype(self.dtype)
            self.x0 = self.rng.standard_normal(self.N).astype(self.dtype)
        if name == "large_eta":
            base = np.random.default_rng([seed, self.N, len(SEQUENCES)])
            self.g0, self.x0 = base.standard_normal(self.N), base.standard_normal(self.N)

    def _random_pair(self):
        g = self.rng.standard_normal(self.N); x = self.rng.standard_normal(self.N)
        return g, x

    def next(self, feedback=None):
        k = self.count
        if self.name == "contractive":
            x = self.x0 if k == 0 else np.asarray(feedback, dtype=self.dtype)
            g = (self.d * x + self.c).astype(self.dtype)
        else:
            g, x = self._random_pair()                                     # drawn for every k, so the later pairs do not depend on the sequence's kind
            if k == DEGENERATE_AT and self.name == "repeat":
                g, x = self.pairs[-1]
            elif k == DEGENERATE_AT and self.name == "near_dependent":
                (g1, x1), (g0, x0) = self.pairs[-1], self.pairs[-2]
                g = g1.astype(np.float64) + (g1.astype(np.float64) - g0) + PERTURBATION * g
                x = x1.astype(np.float64) + (x1.astype(np.float64) - x0) + PERTURBATION * x
            elif self.name == "large_eta":
                g = self.g0 + LARGE_ETA_STEP * g; x = self.x0 + LARGE_ETA_STEP * x
            elif self.factor != 1.0:
                g = g * self.factor; x = x * self.factor
            g = np.asarray(g, dtype=self.dtype); x = np.asarray(x, dtype=self.dtype)
        self.pairs.append((g, x))
        self.count += 1
        return g.copy(), x.copy()


def steps_of(mem, N):
    return 2 * int(mem) + 5


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
class Step:
    """what ReferenceAccelerator.step returns; arrays are np.longdouble, columns in slot order"""
    __slots__ = ("active", "attempted", "success", "singular", "eta_too_large", "l", "j", "restarts", "fail_singular", "fail_eta", "g", "f", "nrm_f", "sum_f2",
                 "eta", "eta_norm", "cand", "R", "M", "M_abs", "cond", "cond_dF", "cond_M", "norm_dF", "norm_dG", "res_norm", "decided")

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, None)


def householder_r(A):
    """R of A = QR with a positive diagonal, by Householder reflections in the precision of A; an exactly zero column below the diagonal leaves an exactly
    zero diagonal entry.  Returns (R, Q'[:, :ncol] applied to nothing) -- only R: eta comes from lstsq_qr."""
    A = np.array(A, dtype=LD, copy=True)
    m, n = A.shape
    vs = []
    for k in range(min(m, n)):
        x = A[k:, k]
        nx = np.sqrt(x @ x)
        if nx == 0 or not np.isfinite(nx):
            vs.append(None)
            continue
        v = x.copy()
        v[0] += nx if x[0] >= 0 else -nx
        v /= np.sqrt(v @ v)
        A[k:, k:] -= 2.0 * np.outer(v, v @ A[k:, k:])
        vs.append(v)
    return A, vs


def lstsq_qr(dF, f):
    """(eta, R, singular): eta = argmin ||f - dF eta||, R with positive diagonal"""
    m, n = dF.shape
    T, vs = householder_r(dF)
    R = np.triu(T[:n, :n]) if m >= n else None
    y = np.array(f, dtype=LD, copy=True)
    for k, v in enumerate(vs):
        if v is not None:
            y[k:] -= 2.0 * v * (v @ y[k:])
    sgn = np.where(np.diag(R) < 0, LD(-1), LD(1))
    R = sgn[:, None] * R
    rhs = sgn * y[:n]
    d = np.diag(R)
    if not np.all(np.isfinite(R)) or np.any(d == 0):
        return None, R, True
    eta = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        eta[i] = (rhs[i] - R[i, i + 1:] @ eta[i + 1:]) / R[i, i]
    return eta, R, False


def solve_lu(M, rhs):
    """(eta, singular): LU with partial pivoting in np.longdouble; singular = a pivot is exactly zero or not finite"""
    M = np.array(M, dtype=LD, copy=True); b = np.array(rhs, dtype=LD, copy=True)
    n = M.shape[0]
    for c in range(n):
        pv = c + int(np.argmax(np.abs(M[c:, c]))) if np.all(np.isfinite(M[c:, c])) else c
        if not np.isfinite(M[pv, c]) or M[pv, c] == 0:
            return None, True
        if pv != c:
            M[[c, pv], :] = M[[pv, c], :]; b[[c, pv]] = b[[pv, c]]
        for r in range(c + 1, n):
            t = M[r, c] / M[c, c]
            M[r, c:] -= t * M[c, c:]
            b[r] -= t * b[c]
    eta = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        eta[i] = (b[i] - M[i, i + 1:] @ eta[i + 1:]) / M[i, i]
    return eta, False


def _cond(A):
    s = np.linalg.svd(np.asarray(A, dtype=np.float64), compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else float("inf")


def _norm2(A):
    """the 2-norm, of a matrix whose entries may be outside the range where their squares are finite (the scaled sequences)"""
    A = np.asarray(A, dtype=LD)
    big = np.max(np.abs(A)) if A.size else LD(0)
    if big == 0 or not np.isfinite(big):
        return float(big)
    return float(LD(np.linalg.norm(np.asarray(A / big, dtype=np.float64), 2)) * big)


class ReferenceAccelerator:
    def __init__(self, kind, N, mem, min_mem=MIN_MEM, eta_max=ETA_MAX, dtype=np.float64, start_iter=2, C=None):
        _, self.type1, self.rolling, self.ne = KINDS[kind]
        self.kind, self.N, self.dtype = kind, int(N), np.dtype(dtype)
        self.mem = max(1, min(int(mem), self.N))
        self.min_mem, self.eta_max, self.start_iter = int(min_mem), float(eta_max), int(start_iter)
        self.C = C_BOUND if C is None else float(C)
        self.C_eta = C_ETA if C is None else float(C)
        self.active = False
        self.restarts = 0
        self.restart()

    def restart(self):
        """CA.restart!: the history is emptied, the next pair only initialises"""
        self.hist = []              # (x, f, g) in the working dtype: the base triple and one triple per stored column
        self.ncol = 0               # columns added since the last (memory) restart
        self.fail_singular = self.fail_eta = 0      # failed steps since the history was last emptied

    def columns(self):
        """dX, dF, dG (working dtype, N x l) in SLOT order, and the slot of the newest column"""
        l = len(self.hist) - 1
        first = self.ncol - l                                          # number of the oldest stored column
        cols = [None] * l
        for i in range(l):
            a, b = self.hist[i], self.hist[i + 1]
            cols[(first + i) % self.mem] = tuple((b[t] - a[t]).astype(self.dtype) for t in range(3))
        return [np.column_stack([c[t] for c in cols]) if l else np.zeros((self.N, 0), dtype=self.dtype) for t in range(3)]

    def step(self, g, x, it=None):
        g = np.asarray(g, dtype=self.dtype); x = np.asarray(x, dtype=self.dtype)
        S = Step()
        if not self.active and (it is None or it >= self.start_iter):
            self.active = True
        S.active = self.active
        S.attempted = S.success = S.singular = S.eta_too_large = False
        S.decided = True
        S.g = g.astype(LD); S.cand = S.g.copy()
        if not self.active:
            S.l, S.j, S.restarts = min(self.ncol, self.mem), -1, self.restarts
            S.fail_singular, S.fail_eta = self.fail_singular, self.fail_eta
            return S
        f = (x - g).astype(self.dtype)                                  # one rounding, as in every implementation
        S.f = f.astype(LD)
        S.sum_f2 = float(S.f @ S.f); S.nrm_f = float(np.sqrt(S.f @ S.f))
        if not self.hist:
            self.hist = [(x.copy(), f, g.copy())]
            S.j = -1
        else:
            if not self.rolling and self.ncol == self.mem:             # RestartedMemory, full: start over; the new column is the first again
                self.hist = self.hist[-1:]
                self.ncol = 0
                self.restarts += 1
                self.fail_singular = self.fail_eta = 0
            self.hist.append((x.copy(), f, g.copy()))
            if len(self.hist) - 1 > self.mem:                           # RollingMemory: the oldest column leaves
                self.hist.pop(0)
            S.j = self.ncol % self.mem
            self.ncol += 1
        l = S.l = min(self.ncol, self.mem)
        S.restarts = self.restarts
        if l >= self.min_mem:
            S.attempted = True
            dX, dF, dG = (A.astype(LD) for A in self.columns())
            S.norm_dF, S.norm_dG = _norm2(dF), _norm2(dG)
            sc = LD(np.max(np.abs(dF))) if np.max(np.abs(dF)) > 0 else LD(1)
            S.cond_dF = _cond(dF / sc)
            L = dX if self.type1 else dF
            S.M = L.T @ dF
            S.M_abs = np.abs(L).T @ np.abs(dF)
            mx = np.max(np.abs(S.M))
            S.cond_M = _cond(S.M / mx) if mx > 0 and np.all(np.isfinite(S.M)) else float("inf")
            S.cond = S.cond_M if self.ne else S.cond_dF
            eta_ls, S.R, sing_qr = lstsq_qr(dF, S.f)
            if self.type1:
                S.eta, S.singular = solve_lu(S.M, dX.T @ S.f)
            else:
                # Type2, QR or normal equations: the same least-squares problem; a zero pivot of the Gram matrix M = dF'dF is a zero diagonal entry of R
                S.eta, S.singular = eta_ls, sing_qr
            if S.singular:
                self.fail_singular += 1
            else:
                S.eta_norm = float(np.sqrt(S.eta @ S.eta))
                res = S.f - dF @ S.eta
                S.res_norm = float(np.sqrt(res @ res))
                S.eta_too_large = not (S.eta_norm <= self.eta_max)
                # the decision ||eta|| <= eta_max is taken on a computed eta with relative error up to C_ETA eps cond: a reference norm closer to the threshold
                # than that (twice the bound on eta) decides nothing about an implementation's flag
                S.decided = bool(self.C_eta * eps_of(self.dtype) * S.cond < 0.5 and abs(S.eta_norm - self.eta_max) > 2.0 * self.eta_bound(S))
                if S.eta_too_large:
                    self.fail_eta += 1
                else:
                    S.success = True
                    S.cand = S.g - dG @ S.eta
        S.fail_singular, S.fail_eta = self.fail_singular, self.fail_eta
        return S

    def error(self, cand, S):
        """e of the module docstring for an implementation's candidate"""
        g_norm = float(np.sqrt(S.g @ S.g))
        d = np.asarray(cand, dtype=LD) - S.cand
        return float(np.sqrt(d @ d)) / (S.cond * (g_norm + S.norm_dG * S.eta_norm))


    def eta_bound(self, S):
        """bound on ||eta - eta_ref||.  A linear system (Type1) or the normal equations (whose cond is already cond(dF)^2): C eps cond ||eta_ref||.  The
        least-squares problem solved through a QR factor has the sensitivity eps cond (||eta|| + cond ||r|| / ||dF||), r = f - dF eta the residual (Wedin;
        Higham, Accuracy and Stability of Numerical Algorithms, theorem 20.1): without the residual term the Float64 oracle itself misses the bound (by a
        factor 1.3 on `contractive` at N = 8 and 58 on the nearly dependent column at N = 3000, where its candidates are inside theirs)."""
        rel = self.C_eta * eps_of(self.dtype) * S.cond
        if self.kind == "qr":
            return rel * (S.eta_norm + S.cond_dF * S.res_norm / S.norm_dF)
        return rel * S.eta_norm


def make_oracle(O, kind, N, mem, min_mem):
    _, type1, rolling, ne = KINDS[kind]
    return O.AndersonAcceleratorNE(N, mem, min_mem, type1=type1, rolling=rolling) if ne else O.AndersonAccelerator(N, mem, min_mem)


def run_oracle(O, kind, seq_name, n, m, mem, min_mem=MIN_MEM, seed=0):
    """the Float64 oracle and the reference on one sequence: list of (oracle record, reference Step)"""
    N = n + m
    seq = Sequence(seq_name, N, seed, np.float64)
    ref = ReferenceAccelerator(kind, N, mem, min_mem, eta_max=eta_max_of(seq_name), dtype=np.float64)
    aa = make_oracle(O, kind, N, mem, min_mem)
    aa.ETA_MAX = eta_max_of(seq_name)
    out = []
    cand = None
    for k in range(steps_of(mem, N)):
        g, x = seq.next(cand)
        S = ref.step(g, x)
        was_init = aa.init_phase
        j = -1 if was_init else aa.iter % aa.mem
        with np.errstate(all="ignore"):
            aa.update(g, x)
            cand = g.copy()
            fs, fe = aa.fail_singular, aa.fail_eta
            aa.accelerate(cand)
        rec = dict(l=min(aa.iter, aa.mem), j=j, restarts=aa.num_restarts, success=bool(aa.was_successful()), singular=aa.fail_singular > fs, eta_too_large=aa.fail_eta > fe,
                   cand=cand.copy(), g=g, eta=aa.eta.copy())
        out.append((rec, S))
    return out
