"""The cases and the reference of tests/projection_cases.py on the CPU (no GPU): what test_gpu_batch_projections.py relies on.

  * the reference (written from the definitions) agrees with the oracle's O.project on every cone of every member of every case, within the bounds the
    GPU test uses -- and bit for bit on every cone tagged exact, in Float64 and in Float32;
  * the second-order cones take the branch they were built for, no random one sits within 1e-6 (relative) of a tie;
  * every PSD cone tagged gapped has min |lambda| >= 0.1 ||X||_2;
  * the cases are the ones the GPU test needs: dims, sides, spectra, the 64 / 70 cone members, 19 small cones, three mid cones, side-1 cones, the poison.

The only tolerances in this file are the bounds of projection_cases (8 eps d ||x||, 64 d eps ||X||_F, the 1e-3 membership of the 3-d cones)."""
import numpy as np
import pytest

from oracle import cosmo_oracle as O
from tests import projection_cases as S
from tests import util

NAMES = list(S.CASES)
DTYPES = [np.float64, np.float32]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    """bit equality; two NaNs count as equal whatever their payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _oracle_project(case, rows):
    """O.project_cone cone by cone in the type of rows (the 3-d cones in float64: their oracle is a float64 restatement)"""
    out = rows.copy()
    cones = util.oracle_cones(util.projection_sets(case.cones))
    off = 0
    branches = []
    for c, oc in zip(case.cones, cones):
        info = {}
        if c.kind in S.CONE3:
            v = out[off:off + c.dim].astype(np.float64)
            O.project_cone(v, oc)
            out[off:off + c.dim] = v
        else:
            O.project_cone(out[off:off + c.dim], oc, info)
        branches.append(info.get("soc_branch", [-1])[0])
        off += c.dim
    return out, branches


def _cases_of(dtype):
    return [n for n in NAMES if dtype is np.float64 or S.case(n).float32]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_the_oracle(name, dtype):
    case = S.case(name)
    if dtype is np.float32 and not case.float32:
        return                                                                # the Float32 library does not run this case: nothing to prove
    eps = S.EPS if dtype is np.float64 else S.EPS32
    worst = {}
    for k, mb in enumerate(case.members):
        rows = mb.rows.astype(dtype)
        ref, rbr = S.project_reference(case.cones, rows)
        orc, obr = _oracle_project(case, rows)
        assert ref.dtype == orc.dtype == np.dtype(dtype)
        for i, (c, a, b) in enumerate(zip(case.cones, case.offsets[:-1], case.offsets[1:])):
            x, r, o, tag = rows[a:b], ref[a:b], orc[a:b], mb.tags[i]
            where = (name, k, i, c.kind, c.dim, tag, mb.note[i])
            if c.kind in S.SIMPLE or tag == "exact":
                assert tag == "exact", where
                if c.kind in S.PSD and np.signbit(x[0]) and x[0] == 0:
                    # PsdCone(1) with -0.0: Julia's max(-0.0, 0.0) is +0.0 (the reference, the kernels); the oracle's Python max keeps the sign
                    assert r[0] == 0 and not np.signbit(r[0]) and o[0] == 0, where
                    continue
                assert same_bits(r, o), where + (r, o)
            elif tag == "poison":
                assert np.isnan(r).all() and np.isnan(o).all() and np.isnan(x).sum() == 1, where
            elif c.kind == S.SOC:
                assert tag == "random" and rbr[i] == obr[i], where
                ratio = np.linalg.norm(r.astype(np.float64) - o) / (8 * eps * c.dim * max(np.linalg.norm(x.astype(np.float64)), 1e-300))
                worst["soc"] = max(worst.get("soc", 0.0), ratio)
                assert ratio <= 1.0, where + (ratio,)
            elif c.kind in S.PSD:
                X = S.psd_matrix(x, c)
                d = c.side
                R, Om = S.psd_matrix(r, c), S.psd_matrix(o, c)
                bound = S.psd_bound(X, d, eps)
                if tag == "zero":
                    assert not x.any() and not r.any() and not o.any(), where
                    continue
                ratio = np.linalg.norm(R - Om) / bound
                worst["psd"] = max(worst.get("psd", 0.0), ratio)
                assert ratio <= 1.0, where + (ratio,)
                if c.kind == S.PSD_SQ:
                    assert np.array_equal(r.reshape(d, d), r.reshape(d, d).T), where
                if tag == "gapped":
                    assert np.linalg.eigvalsh(R).min() >= -bound, where
            else:
                assert tag == "cone3" and np.isnan(r).all(), where
                # the oracle's result satisfies the definition ten times tighter than the GPU test asks of the kernels -- except where the reference
                # algorithm itself does not converge: a power cone with y = 0 and z != 0 (phi_y stays at its floor of 1e-10, src/convexset.jl:686-688)
                miss = S.cone3_violation(c, x, o, tol=S.CONE3_TOL / 10)
                if miss:
                    assert c.kind in (S.POW, S.DUAL_POW) and x[1] == 0 and x[2] != 0, where + (x, o, miss)
    print("%s %s: worst error / bound between reference and oracle: %s" % (name, np.dtype(dtype).name, worst))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_exact_second_order_cones_have_the_literal_results(dtype):
    """the expected outputs of the exact cases are bit patterns one can write down"""
    T = np.dtype(dtype).type
    for x, want, br in (([5, 3, 4], [5, 3, 4], 0), ([-5, 3, 4], [0, 0, 0], 1), ([0, 3, 4], [2.5, 1.5, 2], 2), ([0, 0, 0], [0, 0, 0], 0),
                        ([2.5], [2.5], 0), ([-2.5], [0], 1), ([0.0], [0.0], 0), ([-0.0], [-0.0], 0), ([20, 12, -16], [20, 12, -16], 0), ([10, 12, -16], [15, 9, -12], 2),
                        ([10] + [3, -4] * 16, [15] + [2.25, -3] * 16, 2)):
        out, b = S.ref_soc(np.array(x, dtype=dtype))
        assert b == br and same_bits(out, np.array(want, dtype=dtype)), (x, out)
    for name in ("soc_exact_small", "soc_exact_1025", "soc_exact_4097"):
        case = S.case(name)
        for mb in case.members:
            for i, (c, a, b) in enumerate(zip(case.cones, case.offsets[:-1], case.offsets[1:])):
                x = mb.rows[a:b].astype(dtype)
                assert mb.tags[i] == "exact"
                sq = x[1:].astype(np.float64) ** 2
                assert np.array_equal(sq, np.round(sq)) and sq.sum() < 2 ** 20       # integers: every partial sum is exact in Float32 too, in any order
                nx = float(np.sqrt(sq.sum()))
                assert nx == round(nx)
                out, br = S.ref_soc(x)
                assert br == mb.branch[i]
                if br == 2:                                                    # f = (nx + t) / (2 nx) is a dyadic rational: f * x_i rounds nowhere
                    f = (nx + float(x[0])) / (2 * nx)
                    assert f in (0.5, 0.75)
                    assert same_bits(out, np.concatenate([[T((nx + float(x[0])) / 2)], T(f) * x[1:]]).astype(dtype))
                elif br == 1:
                    assert not out.any() and not np.signbit(out).any()
                else:
                    assert same_bits(out, x)
    # every value of t / ||x|| is met by every long cone
    for name in ("soc_exact_1025", "soc_exact_4097"):
        assert sorted(mb.branch[0] for mb in S.case(name).members) == [0, 1, 2, 2]


def test_second_order_cones_take_the_branch_they_were_built_for():
    seen = {}
    for name in NAMES:
        case = S.case(name)
        for mb in case.members:
            _, br = S.project_reference(case.cones, mb.rows)
            for i, c in enumerate(case.cones):
                if c.kind != S.SOC or mb.tags[i] == "poison":
                    continue
                assert br[i] == mb.branch[i] and br[i] in (0, 1, 2), (name, i, br[i], mb.branch[i])
                seen.setdefault((name, c.dim), set()).add(br[i])
    for d in S.SOC_RANDOM_DIMS:                                                # every dim of soc_random in every branch (d = 1 has two)
        assert seen[("soc_random", d)] == ({0, 1} if d == 1 else {0, 1, 2}), d
    for name in ("soc_64_cones", "soc_70_cones"):
        assert set().union(*[v for (nm, _), v in seen.items() if nm == name]) == {0, 1, 2}


def test_no_random_second_order_cone_is_near_a_tie():
    for name in NAMES:
        case = S.case(name)
        for mb in case.members:
            for i, (c, a, b) in enumerate(zip(case.cones, case.offsets[:-1], case.offsets[1:])):
                if c.kind == S.SOC and mb.tags[i] == "random":
                    for dtype in DTYPES:
                        x = mb.rows[a:b].astype(dtype).astype(S.LD)
                        nx, t = np.sqrt(np.sum(x[1:] * x[1:])), abs(x[0])
                        if nx == 0 and t == 0:
                            continue
                        assert abs(nx - t) > 1e-6 * max(nx, t), (name, i)


def test_gapped_psd_cases_have_an_unambiguous_rank():
    count = 0
    for name in NAMES:
        case = S.case(name)
        for mb in case.members:
            for i, (c, a, b) in enumerate(zip(case.cones, case.offsets[:-1], case.offsets[1:])):
                if mb.tags[i] == "gapped":
                    for dtype in DTYPES:
                        w = np.linalg.eigvalsh(S.psd_matrix(mb.rows[a:b].astype(dtype), c))
                        assert np.abs(w).min() >= 0.1 * np.abs(w).max(), (name, i, mb.note[i])
                    count += 1
                elif c.kind in S.PSD and c.dim > 1:
                    assert mb.tags[i] in ("psd", "zero"), (name, i)
    assert count > 300


def test_the_cases_are_the_ones_the_gpu_test_needs():
    soc = S.case("soc_random")
    assert [c.dim for c in soc.cones] == [1, 2, 3, 63, 64, 65, 66, 129, 1000]
    c64, c70 = S.case("soc_64_cones"), S.case("soc_70_cones")
    assert len(c64.cones) == 64 and len(c70.cones) == 70                      # soc_in_regs: nsoc <= 8 * (512 / 64) = 64, and past it
    assert c64.m <= 1024 and c70.m <= 1024                                    # both fit the register kernel <512, 1, 2>
    assert len(set(c.dim for c in c64.cones)) > 4 and len(set(c.dim for c in c70.cones)) > 4
    assert min(c.dim for c in c70.cones) == 1 and max(c.dim for c in c70.cones) > 64 and max(c.dim for c in c64.cones) > 64
    # PSD: every side in both layouts with every spectrum
    seen = {}
    for name in NAMES:
        case = S.case(name)
        for mb in case.members:
            for i, c in enumerate(case.cones):
                if c.kind in S.PSD and c.dim > 1 and (name.startswith("psd_small") or name.startswith("psd_mid_") and name != "psd_mid_three"):
                    seen.setdefault((c.side, c.kind), set()).add(mb.note[i].split()[-1])
    for d in S.SMALL_SIDES + S.MID_SIDES:
        for kind in S.PSD:
            assert seen[(d, kind)] == set(S.SPECTRA), (d, kind, seen.get((d, kind)))
    p19 = S.case("psd_19_small")
    assert len(p19.cones) == 19 and all(2 <= c.side <= 16 for c in p19.cones) and len(set(c.side for c in p19.cones)) > 6
    assert {c.kind for c in p19.cones} == set(S.PSD)
    three = S.case("psd_mid_three")
    assert len(three.mid_sides) == 3 and len(set(three.mid_sides)) == 3
    one = S.case("psd_side_one")
    assert [c.dim for c in one.cones if c.kind in S.PSD].count(1) == 2 and {c.kind for c in one.cones if c.dim == 1} == set(S.PSD)
    vals = np.concatenate([mb.rows[[a for c, a in zip(one.cones, one.offsets) if c.dim == 1]] for mb in one.members])
    assert np.isnan(vals).any() and (np.signbit(vals) & (vals == 0)).any() and (vals > 0).any() and (vals < 0).any()
    for kind in S.CONE3:
        c3 = S.case("cone3_" + kind)
        assert len(c3.cones) == 300 and all(c.kind == kind for c in c3.cones)
        X = c3.members[0].rows.reshape(300, 3)
        assert (X[50:60, 2] == 0).all() and (X[60:70, 1] == 0).all() and np.abs(X[:50]).max() <= 0.025 and np.abs(X[70:]).max() > 20
        a = np.array([c.alpha for c in c3.cones])
        assert (kind in (S.POW, S.DUAL_POW)) == bool((a > 0).all()) and (a < 0.95).all()
    mixed = S.case("mixed")
    kinds = [c.kind for c in mixed.cones]
    assert set(kinds) == {S.ZERO, S.NONNEG, S.BOX, S.SOC, S.PSD_TRI, S.PSD_SQ, S.EXP, S.DUAL_EXP, S.POW, S.DUAL_POW}
    assert all(kinds[i] in S.SIMPLE or kinds[i + 1] in S.SIMPLE or mixed.cones[i].dim == 1 or mixed.cones[i + 1].dim == 1
               or {kinds[i], kinds[i + 1]} & set(S.CONE3) for i in range(len(kinds) - 1))
    poison = S.case("poison")
    assert poison.clean == [0, 1, 3] and [(c.kind, c.dim) for c in poison.cones] == [(c.kind, c.dim) for c in mixed.cones]
    for k, mb in enumerate(poison.members):
        bad = ~np.isfinite(mb.rows)
        if k != 2:
            assert not bad.any() and "poison" not in mb.tags
            continue
        assert mb.tags.count("poison") == 1
        for i, (c, a, b) in enumerate(zip(poison.cones, poison.offsets[:-1], poison.offsets[1:])):
            x = mb.rows[a:b]
            if mb.tags[i] == "poison":
                assert c.kind == S.SOC and np.isnan(x).sum() == 1 and not np.isinf(x).any()
            elif c.kind not in S.SIMPLE:
                assert np.isfinite(x).all(), (i, c.kind)                       # no NaN in PSD, exponential or power cones, nor in the other second-order cones
        for kind in S.SIMPLE:                                                  # NaN and an infinity in rows of every simple kind
            x = np.concatenate([mb.rows[a:b] for c, a, b in zip(poison.cones, poison.offsets[:-1], poison.offsets[1:]) if c.kind == kind])
            assert np.isnan(x).any() and np.isinf(x).any(), kind
        assert any((np.signbit(mb.rows[a:b]) & (mb.rows[a:b] == 0)).any() for c, a, b in zip(poison.cones, poison.offsets[:-1], poison.offsets[1:])
                   if c.kind in S.SIMPLE)
    # 3 .. 6 members everywhere, one structure per case
    for name in NAMES:
        assert 3 <= len(S.case(name).members) <= 6, name
        assert all(mb.rows.size == S.case(name).m for mb in S.case(name).members)
