"""Device-memory inputs and results of a resident batch (cj.BatchSolver.update_device, optimize(x0=, s0=, y0=, results="device"); csrc/batch_devio.hip:
k_batch_update_qb_dev, k_batch_set_iterates_dev, k_batch_export_solution behind cosmo_hip_batch_update_qb_device / set_iterates_device /
get_solution_device).  The yardstick is the host path of the same batch -- stage_qb / apply_updates, warm_start="models", _write_back -- on a twin
BatchSolver over the same problems: the device path has to leave the same BITS on the device and hand the same bits back.

Shapes: n = 30, m = 36 (the 6-member family of tests/test_gpu_batch_resident.py: less than one 256-thread stride per member, several members per
workgroup), m = 1030 (the "tall" family of tests/batch_update_cases.py: a member spans more than four strides), n = 270 > 256; the member list
[4, 0, 3] is out of order and incomplete, so the position in the list and the member cannot be confused."""
import numpy as np
import pytest
import torch

import cosmo_jl_amd as cj
from cosmo_jl_amd import _ffi as F
from tests import batch_update_cases as BC
from tests import util

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
U32 = 2.0 ** -24                                        # unit roundoff of float32
NONNEG0 = 4                                             # first Nonnegatives row of every family (4 ZeroSet rows in front)
SUBSET = [4, 0, 3]


def _family(name):
    if name == "res6":
        return [util.random_qp(np.random.default_rng(21 + j), 30, 4, 20, 12, p_shift=1.0) for j in range(6)]
    if name == "wide":
        return [util.random_qp(np.random.default_rng(50 + j), 270, 4, 20, 12, p_shift=1.0) for j in range(5)]
    return BC.family(name)


def _models(probs, dtype, **kw):
    kw.setdefault("kkt_solver", cj.CGIndirectKKTSolver)
    kw.setdefault("eps_abs", 1e-4); kw.setdefault("eps_rel", 1e-4)
    st = cj.Settings(device_scaling=False, **kw)        # host Ruiz scaling, as the batch set-up does it
    out = []
    for p in probs:
        md = cj.Model(dtype=dtype)
        md.set(p["P"], p["q"], p["A"], p["b"], p["sets"], st)
        out.append(md)
    return out


def _loosened(p, rng):
    """b with more room in the Nonnegatives rows only: the point the problem was built around stays feasible, so the re-solves end in Solved"""
    b = p["b"].copy()
    nn = next(K.dim for K in p["sets"] if isinstance(K, cj.Nonnegatives))
    b[NONNEG0:NONNEG0 + nn] += rng.uniform(0.0, 0.2, nn)
    return b


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _state(B):
    return [B.get_qb(k) + (B.get_rho_classes(k),) for k in range(B.nprob)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["res6", "tall", "wide"])
def test_update_device_leaves_the_bits_of_the_host_path(name, dtype):
    probs = _family(name)
    nprob, n, m = len(probs), probs[0]["q"].size, probs[0]["b"].size
    rng = np.random.default_rng(5)
    with cj.BatchSolver(_models(probs, dtype)) as host, cj.BatchSolver(_models(probs, dtype)) as dev:
        host.optimize(); dev.optimize()
        H, D = host.batch, dev.batch
        for what, members in (("q", SUBSET), ("b", None), ("qb", SUBSET), ("qb", None), ("q", None), ("b", SUBSET)):
            mem = list(range(nprob)) if members is None else members
            q = rng.standard_normal((len(mem), n)) if "q" in what else None
            b = np.stack([probs[k]["b"] * rng.uniform(0.9, 1.1, m) for k in mem]) if "b" in what else None
            if b is not None:
                b[1, NONNEG0 + 3] = 1e22                                     # an infinite Nonnegatives row of member mem[1]: class 2
            before = _state(D)
            for j, k in enumerate(mem):
                H.stage_qb(k, None if q is None else q[j], None if b is None else b[j])
            H.apply_updates()
            dev.update_device(q=None if q is None else _dev(q, dtype), b=None if b is None else _dev(b, dtype), members=members)
            after_h, after_d = _state(H), _state(D)
            for k in range(nprob):
                for a, c in zip(after_d[k], after_h[k]):
                    assert np.array_equal(a, c), (what, members, k)
                if k not in mem:
                    for a, c in zip(after_d[k], before[k]):
                        assert np.array_equal(a, c), (what, members, k)
            if b is not None:
                assert after_d[mem[1]][2][NONNEG0 + 3] == 2 and np.count_nonzero(after_d[mem[1]][2] == 2) >= 1
            if q is not None:                                                # ... and it is the formula, not two equal mistakes
                k = mem[-1]; sm = dev.models[k].sm
                assert np.array_equal(after_d[k][0], (sm.D.astype(dtype) * q[-1].astype(dtype)) * np.dtype(dtype).type(sm.c))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["res6", "tall", "wide"])
def test_exported_solution_is_the_write_back(name, dtype):
    probs = _family(name)
    models = _models(probs, dtype)
    nprob, n, m = len(probs), models[0].n, models[0].m
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    with cj.BatchSolver(models) as rb:
        rs = rb.optimize()
        B = rb.batch
        x = torch.full((nprob, n), float("nan"), dtype=tdt, device="cuda:0"); s = torch.full((nprob, m), float("nan"), dtype=tdt, device="cuda:0")
        y = torch.full((nprob, m), float("nan"), dtype=tdt, device="cuda:0")
        B.get_solution_device(x=x, s=s, y=y)
        x, s, y = x.cpu().numpy(), s.cpu().numpy(), y.cpu().numpy()
        only_y = torch.full((nprob, m), float("nan"), dtype=tdt, device="cuda:0")
        B.get_solution_device(y=only_y)                                      # any of the three may be left out
        assert np.array_equal(only_y.cpu().numpy(), y)
        for k, (md, r) in enumerate(zip(models, rs)):
            if dtype == np.float64:
                assert np.array_equal(x[k], r.x) and np.array_equal(y[k], r.y) and np.array_equal(s[k], r.s), k
                continue
            _, w_prev, sk, mu = B.get_iterates(k)
            f32 = np.float32
            assert np.array_equal(x[k], md.sm.D.astype(f32) * w_prev[:n]), k
            assert np.array_equal(s[k], md.sm.Einv.astype(f32) * sk), k
            assert np.array_equal(y[k], -((md.sm.E.astype(f32) * mu) * f32(md.sm.cinv))), k
            # _write_back multiplies in float64: rounding E and cinv to float32 costs one unit roundoff each and the two products one each
            for a, c in ((x[k], r.x), (y[k], r.y), (s[k], r.s)):
                assert np.all(np.abs(a - c) <= 4 * U32 * np.abs(c)), (k, float(np.max(np.abs(a - c) / np.maximum(np.abs(c), 1e-300))))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["res6", "tall", "wide"])
def test_warm_start_from_device_tensors_is_the_warm_start_from_models(name, dtype):
    """Float64: w, w_prev, s are the bits of warm_start="models", and so is the truncated solve that follows.  Float32: the host path scales in float64
    and rounds once on the way into the library, the device multiplies in float32, so the two cannot agree in every bit.  There the x and s parts are
    pinned bit for bit to the float32 formula of the kernel, and the iterates to the host path within what the roundings allow: x = Dinv * x0 and
    s = E * s0 differ by at most 3 units (rounding the scale factor and the product on the device, one rounding on the host); for
    w_s = (1 / rho) * mu + s the device's mu carries 4 roundings (Einv, the product, c, the product) against 1 on the host and one more each for
    the product with 1 / rho, which makes 7 units of |mu / rho|, plus the 3 of s and one of the sum on either side: at most 12 units of
    |mu / rho| + |s|."""
    probs = _family(name)
    nprob, n, m = len(probs), probs[0]["q"].size, probs[0]["b"].size
    rng = np.random.default_rng(9)
    x0 = rng.standard_normal((nprob, n)).astype(dtype); s0 = rng.uniform(0.0, 1.0, (nprob, m)).astype(dtype); y0 = rng.standard_normal((nprob, m)).astype(dtype)
    with cj.BatchSolver(_models(probs, dtype, max_iter=20)) as host, cj.BatchSolver(_models(probs, dtype, max_iter=20)) as dev:
        host.optimize(); dev.optimize()
        for k, md in enumerate(host.models):
            md.x[:] = x0[k]; cj.warm_start_slack(md, s0[k]); cj.warm_start_dual(md, y0[k])
        tens = dict(x0=_dev(x0, dtype), s0=_dev(s0, dtype), y0=_dev(y0, dtype))
        host._warm_start("models")                                            # what optimize() does between the updates and the solve
        dev._warm_start("device", **tens)
        for k in range(nprob):
            wh, wph, sh, _ = host.batch.get_iterates(k)
            wd, wpd, sd, _ = dev.batch.get_iterates(k)
            assert np.array_equal(wd, wpd)
            if dtype == np.float64:
                assert np.array_equal(wd, wh) and np.array_equal(wpd, wph) and np.array_equal(sd, sh), k
                continue
            sm = dev.models[k].sm
            assert np.array_equal(wd[:n], sm.Dinv.astype(dtype) * x0[k]) and np.array_equal(sd, sm.E.astype(dtype) * s0[k]), k
            assert np.all(np.abs(wd[:n] - wh[:n]) <= 3 * U32 * np.abs(wh[:n])) and np.all(np.abs(sd - sh) <= 3 * U32 * np.abs(sh)), k
            assert np.all(np.abs(wd[n:] - wh[n:]) <= 12 * U32 * (np.abs(wh[n:] - sh) + np.abs(sh))), k
        rh = host.optimize(warm_start="models")
        rd = dev.optimize(**tens)
        for k, (a, c) in enumerate(zip(rd, rh)):
            if dtype == np.float64:                                           # the same bits went in: the same 20 iterations come out
                assert a.status == c.status and a.iter == c.iter, (k, a.status, c.status, a.iter, c.iter)
                assert np.array_equal(a.x, c.x) and np.array_equal(a.y, c.y) and np.array_equal(a.s, c.s), k
        # a tensor left out counts as zeros, as in cosmo_hip_batch_set_iterates
        dev._warm_start("device", x0=tens["x0"])
        w, _, s, _ = dev.batch.get_iterates(1)
        assert np.array_equal(w[:n], (dev.models[1].sm.Dinv.astype(dtype) * x0[1]).astype(dtype)) and not w[n:].any() and not s.any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["res6", "tall"])
def test_three_resolves_on_the_device_path_equal_the_host_path(name, dtype):
    probs = _family(name)
    nprob, n, m = len(probs), probs[0]["q"].size, probs[0]["b"].size
    rng = np.random.default_rng(31)
    mh, md = _models(probs, dtype, max_iter=400), _models(probs, dtype, max_iter=400)
    with cj.BatchSolver(mh) as host, cj.BatchSolver(md) as dev:
        host.optimize(); dev.optimize()
        kept = [(m_.x.copy(), m_.s.copy(), m_.mu.copy()) for m_ in md]
        calls = []
        dev.batch.get_iterates = lambda k, _f=dev.batch.get_iterates: (calls.append(k), _f(k))[1]
        out = None
        for step in range(3):
            q = np.stack([p["q"] + 0.2 * rng.standard_normal(n) for p in probs]); b = np.stack([_loosened(p, rng) for p in probs])
            for k, m_ in enumerate(mh):
                cj.update(m_, q=q[k], b=b[k])
            rh = host.optimize()
            dev.update_device(q=_dev(q, dtype), b=_dev(b, dtype))
            rd = dev.optimize(results="device", out=out)
            assert isinstance(rd, cj.DeviceBatchResult) and rd.x.shape == (nprob, n) and rd.y.shape == rd.s.shape == (nprob, m)
            assert rd.x.device.type == "cuda" and rd.x.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
            if out is not None:
                assert rd.x is out[0] and rd.y is out[1] and rd.s is out[2]
            out = (rd.x, rd.y, rd.s)                                          # the second and third solve write into the first one's tensors
            x, y, s = rd.x.cpu().numpy(), rd.y.cpu().numpy(), rd.s.cpu().numpy()
            for k, r in enumerate(rh):
                assert rd.status[k] == r.status and rd.iter[k] == r.iter, (step, k, rd.status[k], r.status, rd.iter[k], r.iter)
                assert rd.obj_val[k] == r.obj_val and rd.r_prim[k] == r.info.r_prim and rd.r_dual[k] == r.info.r_dual and rd.kkt_iters_total[k] == r.kkt_iters_total
                if dtype == np.float64:
                    assert np.array_equal(x[k], r.x) and np.array_equal(y[k], r.y) and np.array_equal(s[k], r.s), (step, k)
                else:                                                         # _write_back multiplies in float64 (see the export test)
                    for a, c in ((x[k], r.x), (y[k], r.y), (s[k], r.s)):
                        assert np.all(np.abs(a - c) <= 4 * U32 * np.abs(c)), (step, k)
            # res6 is strictly convex and keeps its feasible point (_loosened); the tall members (an empty column of A, a variable without a
            # diagonal entry of P) may end in any status, which the two paths then share
            assert name != "res6" or all(st == "Solved" for st in rd.status), rd.status
        assert not calls                                                      # no iterate went to the host ...
        for m_, (x_, s_, mu_) in zip(md, kept):                               # ... and the models' x, s, mu are as the first solve left them
            assert np.array_equal(m_.x, x_) and np.array_equal(m_.s, s_) and np.array_equal(m_.mu, mu_)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_callers_stream_orders_producer_and_consumer(dtype):
    probs = _family("res6")
    nprob, n, m = len(probs), 30, 36
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    rng = np.random.default_rng(77)
    q = _dev(rng.standard_normal((nprob, n)), dtype)
    with cj.BatchSolver(_models(probs, dtype)) as rb:
        rb.optimize()
        B = rb.batch
        rb.update_device(q=q)
        torch.cuda.synchronize()
        want = [B.get_qb(k)[0] for k in range(nprob)]
        rb.update_device(q=torch.zeros_like(q))
        assert not any(B.get_qb(k)[0].any() for k in range(nprob))
        # producer: the values reach the tensor on a side stream, behind a large fill; only the event the library records on that stream orders its read
        side = torch.cuda.Stream(device=0)
        staged = torch.zeros_like(q)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            big = torch.empty(1 << 27, dtype=torch.float64, device="cuda:0")
            big.fill_(1.0)
            staged.copy_(q)
            rb.update_device(q=staged)
        got = [B.get_qb(k)[0] for k in range(nprob)]
        assert all(np.array_equal(a, c) for a, c in zip(got, want))
        del big
        # consumer: a clone queued on the side stream right behind the solve reads what the export kernel wrote
        out = tuple(torch.full(shape, float("nan"), dtype=tdt, device="cuda:0") for shape in ((nprob, n), (nprob, m), (nprob, m)))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            res = rb.optimize(results="device", out=out)
            early = (res.x.clone(), res.y.clone(), res.s.clone())
        torch.cuda.synchronize()
        for a, c in zip(early, (res.x, res.y, res.s)):
            assert torch.equal(a, c) and not torch.isnan(c).any()


def _raw_batch(probs, dtype):
    """a finalised batch that has never had iterates (prepare_batch without its set_iterates; no scaling)"""
    models = _models(probs, dtype, scaling=0)
    md = models[0]
    B = F.Batch(len(models), md.n, md.m, 0, dtype=dtype)
    bl, bu = [], []
    for k, m_ in enumerate(models):
        B.set_problem(k, m_.P, m_.q, m_.A, m_.b)
        bl += [K.l for K in m_.sets if K.kind == F.BOX]; bu += [K.u for K in m_.sets if K.kind == F.BOX]
    B.set_cones([K.kind for K in md.sets], [K.dim for K in md.sets], np.concatenate(bl), np.concatenate(bu))
    B.set_params(cj.model._params_from_settings(None, md.settings))
    return B


def test_the_library_refuses_what_it_cannot_order_or_place():
    probs = _family("res6")
    q = _dev(np.ones((2, 30)), np.float64)
    with cj.BatchSolver(_models(probs, np.float64)) as rb:
        rb.optimize()
        B = rb.batch
        before = _state(B)
        with pytest.raises(cj.CosmoHipError, match="member 6 out of range"):
            rb.update_device(q=q, members=[0, 6])
        with pytest.raises(cj.CosmoHipError, match="member -1 out of range"):
            rb.update_device(q=q, members=[-1, 2])
        with pytest.raises(cj.CosmoHipError, match="member 3 is listed twice"):
            rb.update_device(q=q, members=[3, 3])
        B.stage_qb(2, q=np.zeros(30))
        with pytest.raises(cj.CosmoHipError, match="member 2 has a host-staged q / b pending: apply_updates first"):
            rb.update_device(q=q, members=[5, 2])
        rb.update_device(q=q, members=[5, 1])                                 # members with nothing staged pass meanwhile
        B.apply_updates()
        rb.update_device(q=q, members=[5, 2])
        after = _state(B)
        for k in (0, 3, 4):                                                   # no refused call wrote anything
            assert all(np.array_equal(a, c) for a, c in zip(after[k], before[k])), k
        with pytest.raises(ValueError, match="shape"):                        # (3 members, 2 rows: refused in Python)
            rb.update_device(q=q, members=[0, 1, 2])
    B = _raw_batch(probs, np.float64)
    try:
        x = torch.zeros((6, 30), dtype=torch.float64, device="cuda:0")
        with pytest.raises(cj.CosmoHipError, match="batch_get_solution_device: the batch has no iterates yet"):
            B.get_solution_device(x=x)
        B.set_iterates_device(x0=x)                                           # ... and has them after a warm start from the device
        B.get_solution_device(x=x)
        assert not x.cpu().numpy().any()
    finally:
        B.close()
    B = F.Batch(6, 30, 36, 0)
    try:
        with pytest.raises(cj.CosmoHipError, match="set_params first"):
            B.update_qb_device(q=_dev(np.ones((6, 30)), np.float64))
    finally:
        B.close()


def test_a_mixed_list_keeps_to_the_host_path():
    rng = np.random.default_rng(12)
    probs = [util.random_qp(rng, 30, 4, 20, 40), util.random_qp(rng, 24, 3, 10, 5), util.random_qp(rng, 30, 4, 20, 40)]
    models = _models(probs, np.float64)
    with cj.BatchSolver(models) as rb:
        with pytest.raises(NotImplementedError, match="mixed list"):
            rb.optimize(results="device")
        assert rb.batch is None
        r0 = rb.optimize()
        assert rb.mixed and all(r.status == "Solved" for r in r0)
        with pytest.raises(NotImplementedError, match="mixed list"):
            rb.update_device(q=_dev(np.zeros((3, 30)), np.float64))
        with pytest.raises(NotImplementedError, match="mixed list"):
            rb.optimize(results="device")
        with pytest.raises(NotImplementedError, match="mixed list"):
            rb.optimize(x0=_dev(np.zeros((3, 30)), np.float64))
        cj.update(models[1], q=probs[1]["q"] * 1.2)
        r1 = rb.optimize()
        assert all(r.status == "Solved" for r in r1)
