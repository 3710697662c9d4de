"""What the batch kernels take for granted about their LDS images (csrc/batch.hip: k_batch_admm_lds, k_batch_admm_reg), checked on the host-only planner
csrc/batch_image.cpp through tests/batch_image_probe.cpp (g++, its own shared object per precision, nothing preloaded): one promise per test, on the
cases of tests/batch_image_cases.py -- every kernel form under its switches, every switch on its own, the accelerator, and the smallest shapes at which
a rule changes.  The last tests pin the bytes: the images against what the library answered before the planner left batch.hip, the arrays the library
cannot export against the planner's first state (the old body moved verbatim)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import batch_image_cases as IC

HDR = ("nnzA", "nnzP", "nbA", "nbAT", "nbPT", "oAval", "oPval", "oArp", "oAcol", "oTrp", "oTpr", "oPrp", "oPcol", "oRbA", "oRbAT", "oRbPT", "bytes", "oAord", "oTord")
_plans = {}


def plan(case):
    if case not in _plans:
        _plans[case] = IC.plan(case)
        assert _plans[case]["error"] == ""
    return _plans[case]


IMAGE = [c for c in IC.CASES if IC.CASES[c]["env"].get("LDS", 1) != 0]              # the cases with an image
ASSIGNED = [c for c in IMAGE if plan(c)["permA"].size]
STORED = [c for c in IMAGE if plan(c)["qposA"].size or plan(c)["rcg_stored"]]
COLOURED = [c for c in IMAGE if plan(c)["posN"].size]
SLICED = [c for c in IMAGE if plan(c)["want_sliced"] and plan(c)["slA"].size]
PDIAG = [c for c in SLICED if plan(c)["pdiag"].size]


class Member:
    """member k of a case: the caller's matrices in the case's precision and the decoded row-major image"""

    def __init__(self, case, k):
        f, pl, dt = IC.family(IC.CASES[case]["family"]), plan(case), IC.dtype_of(case)
        self.f, self.pl, self.k, self.dt, self.n, self.m = f, pl, k, dt, f.n, f.m
        self.Acsc, self.Pcsc = f.A[k].astype(dt), f.P[k].astype(dt)
        self.A, self.P = self.Acsc.tocsr(), self.Pcsc.tocsr()
        self.A.sort_indices(); self.P.sort_indices()
        self.caller = np.concatenate([self.Pcsc.data, self.Acsc.data])          # [P_nzval | A_nzval]
        self.img = img = pl["img"][k]
        self.h = h = dict(zip(HDR, (int(v) for v in img[:4 * len(HDR)].view(np.int32))))
        arr = lambda off, t, cnt: img[off:off + cnt * np.dtype(t).itemsize].view(t)
        self.Aval, self.Pval = arr(h["oAval"], dt, h["nnzA"]), arr(h["oPval"], dt, h["nnzP"])
        self.Arp, self.Acol = arr(h["oArp"], np.uint16, self.m + 1).astype(int), arr(h["oAcol"], np.uint16, h["nnzA"]).astype(int)
        self.Trp, self.Tpr = arr(h["oTrp"], np.uint16, self.n + 1).astype(int), arr(h["oTpr"], np.uint32, h["nnzA"]).astype(np.int64)
        self.Prp, self.Pcol = arr(h["oPrp"], np.uint16, self.n + 1).astype(int), arr(h["oPcol"], np.uint16, h["nnzP"]).astype(int)
        self.rb = {key: arr(h["oRb" + key], np.int32, 4 * h["nb" + key]).reshape(-1, 4) for key in ("A", "AT", "PT")}
        # the row / column stored at every position, and what a gather index stands for
        ident_m, ident_n = np.arange(self.m), np.arange(self.n)
        if pl["rcg_stored"]:
            self.rowat, self.colat = arr(h["oAord"], np.uint16, self.m).astype(int), arr(h["oTord"], np.uint16, self.n).astype(int)
        elif pl["qposA"].size:
            self.rowat = np.argsort(pl["qposA"][k * self.m:(k + 1) * self.m]); self.colat = pl["permT"][k * 512:k * 512 + self.n].astype(int)
        else:
            self.rowat, self.colat = ident_m, ident_n
        self.posN = pl["posN"][k * self.n:(k + 1) * self.n] if pl["posN"].size else ident_n
        self.posM = pl["posM"][k * self.m:(k + 1) * self.m] if pl["posM"].size else ident_m
        self.posof_row = np.argsort(self.rowat)

    def serpentine(self):
        """(rows, columns) in sorted-position order from permA / permT: rows through odd slots backwards, columns forwards"""
        JM, JN = (4, 2) if self.pl["rcg_sorted"] else (2, 1)
        pA = self.pl["permA"][self.k * JM * 512:(self.k + 1) * JM * 512]; pT = self.pl["permT"][self.k * JN * 512:(self.k + 1) * JN * 512]
        q = np.arange(self.m)
        return pA[(q // 512) * 512 + np.where((q // 512) % 2 == 1, 511 - q % 512, q % 512)], pT[:self.n], pA, pT


def members(case):
    return [Member(case, k) for k in range(IC.family(IC.CASES[case]["family"]).nprob)]


@pytest.mark.parametrize("case", IMAGE)
def test_the_A_pass_finds_every_entry_of_A_in_exactly_one_slot(case):
    for M in members(case):
        assert M.Arp[0] == 0 and M.Arp[-1] == M.h["nnzA"] == M.A.nnz and np.all(np.diff(M.Arp) >= 0)      # the rows tile the slots 0 .. nnzA - 1
        inv = np.argsort(M.posN)
        for q in range(M.m):
            r, s = M.rowat[q], slice(M.Arp[q], M.Arp[q + 1])
            rs = slice(M.A.indptr[r], M.A.indptr[r + 1])
            assert np.array_equal(inv[M.Acol[s]], M.A.indices[rs]) and np.array_equal(M.Aval[s], M.A.data[rs]), (M.k, q, r)


@pytest.mark.parametrize("case", IMAGE)
def test_every_Tpr_entry_names_the_slot_of_the_same_value_and_its_row(case):
    for M in members(case):
        assert M.Trp[0] == 0 and M.Trp[-1] == M.h["nnzA"] and np.all(np.diff(M.Trp) >= 0)
        invM, invN = np.argsort(M.posM), np.argsort(M.posN)
        for q in range(M.n):
            c, s = M.colat[q], slice(M.Trp[q], M.Trp[q + 1])
            cs = slice(M.Acsc.indptr[c], M.Acsc.indptr[c + 1])
            slot, row = M.Tpr[s] & 0xffff, invM[M.Tpr[s] >> 16]
            assert np.array_equal(row, M.Acsc.indices[cs]) and np.array_equal(M.Aval[slot], M.Acsc.data[cs]), (M.k, q, c)
            pos = M.posof_row[row]
            assert np.all((M.Arp[pos] <= slot) & (slot < M.Arp[pos + 1])) and np.all(invN[M.Acol[slot]] == c)     # the slot lies in that row and holds column c


@pytest.mark.parametrize("case", IMAGE)
def test_the_P_pass_finds_every_entry_of_P_in_exactly_one_slot(case):
    for M in members(case):
        assert M.Prp[0] == 0 and M.Prp[-1] == M.h["nnzP"] == M.P.nnz and np.all(np.diff(M.Prp) >= 0)
        inv = np.argsort(M.posN)
        for q in range(M.n):
            c, s = M.colat[q], slice(M.Prp[q], M.Prp[q + 1])
            ps = slice(M.P.indptr[c], M.P.indptr[c + 1])
            assert np.array_equal(inv[M.Pcol[s]], M.P.indices[ps]) and np.array_equal(M.Pval[s], M.P.data[ps]), (M.k, q, c)


def _no_overlap(h, sizes):
    spans = sorted((h[key], h[key] + size) for key, size in sizes.items() if size)
    assert all(off % 16 == 0 for off, _ in spans) and spans[0][0] >= 4 * len(HDR)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= h["bytes"]


@pytest.mark.parametrize("case", IMAGE)
def test_the_header_lays_the_arrays_out_apart_and_within_the_fit_formula(case):
    pl, it = plan(case), IC.dtype_of(case).itemsize
    assert pl["fits"]
    for M in members(case):
        h, n, m = M.h, M.n, M.m
        _no_overlap(h, dict(oAval=it * h["nnzA"], oPval=it * h["nnzP"], oRbA=16 * h["nbA"], oRbAT=16 * h["nbAT"], oRbPT=16 * h["nbPT"], oArp=2 * (m + 1),
                            oAcol=2 * h["nnzA"], oTrp=2 * (n + 1), oTpr=4 * h["nnzA"], oPrp=2 * (n + 1), oPcol=2 * h["nnzP"],
                            oAord=2 * m if pl["rcg_stored"] else 0, oTord=2 * n if pl["rcg_stored"] else 0))
        assert (h["oAord"] != 0) == (h["oTord"] != 0) == bool(pl["rcg_stored"])
        assert h["bytes"] == M.img.size <= pl["stride"]
        assert h["bytes"] + it * (n + m) + it * 2 * (pl["bs"] // 64) <= IC.MAX_LDS                 # image + gathered vectors + two block-sum slots per wave
        # the tile lists chain over all rows and all entries: of the STORED order in the LDS-image kernel, which reads them; the register kernels do not,
        # and their lists are cut on the index-order pointers whatever the storage order
        stored = (M.Arp, M.Trp, M.Trp + M.Prp) if pl["reg_mode"] == 0 else (M.A.indptr, M.Acsc.indptr, M.Acsc.indptr + M.P.indptr)
        for key, nrows, rp in zip(("A", "AT", "PT"), (m, n, n), stored):
            rb = M.rb[key]
            assert rb[0, 0] == 0 and rb[-1, 1] == nrows and np.array_equal(rb[1:, 0], rb[:-1, 1]) and np.array_equal(rb[:, 2], rp[rb[:, 0]]) and np.array_equal(rb[:, 3], rp[rb[:, 1]])
        if pl["want_sliced"] and pl["slA"].size:
            h2 = dict(zip(HDR, (int(v) for v in pl["img2"][M.k][:4 * len(HDR)].view(np.int32))))
            nT = (h2["oAcol"] - h2["oTpr"]) // 4
            _no_overlap(h2, dict(oAval=it * h2["nnzA"], oTpr=4 * nT, oAcol=2 * h2["nnzA"], oPval=it * h2["nnzP"], oPrp=2 * (n + 1) if h2["nnzP"] else 0, oPcol=2 * h2["nnzP"]))
            assert h2["bytes"] == pl["img2"][M.k].size <= pl["stride2"] and h2["nnzA"] <= 65535
            assert 8 * (512 + 2 * 512 + 2 * 8) + h2["bytes"] <= IC.MAX_LDS                         # SL_WS0 (double precision) + the sliced image


@pytest.mark.parametrize("case", ASSIGNED)
def test_the_assignment_holds_every_row_once_longest_first_odd_slots_backwards(case):
    for M in members(case):
        rows, cols, pA, pT = M.serpentine()
        assert np.array_equal(np.sort(rows), np.arange(M.m)) and np.count_nonzero(pA == -1) == pA.size - M.m
        assert np.array_equal(np.sort(cols), np.arange(M.n)) and np.count_nonzero(pT == -1) == pT.size - M.n
        assert np.all(np.diff(np.diff(M.A.indptr)[rows]) <= 0)
        assert np.all(np.diff((np.diff(M.P.indptr) + np.diff(M.Acsc.indptr))[cols]) <= 0)
        if M.m > 512:
            assert pA[512 + 511] == rows[512] and (M.m == 513 or pA[512 + 510] == rows[513])        # the second slot starts at thread 511 and runs down


@pytest.mark.parametrize("case", STORED)
def test_sorted_storage_is_indexed_by_position_and_qposA_is_its_inverse(case):
    pl = plan(case)
    for M in members(case):
        rows, cols, _, _ = M.serpentine()
        assert np.array_equal(M.rowat, rows) and np.array_equal(M.colat, cols)                       # the stored order is the assignment's
        if pl["qposA"].size:
            assert np.array_equal(pl["qposA"][M.k * M.m:(M.k + 1) * M.m][rows], np.arange(M.m))
        assert np.array_equal(np.diff(M.Arp), np.diff(M.A.indptr)[rows])
        assert np.array_equal(np.diff(M.Trp), np.diff(M.Acsc.indptr)[cols]) and np.array_equal(np.diff(M.Prp), np.diff(M.P.indptr)[cols])


@pytest.mark.parametrize("case", COLOURED)
def test_positions_are_permutations_that_fill_every_bank_pair_to_its_capacity(case):
    for M in members(case):
        for pos, cnt in ((M.posN, M.n), (M.posM, M.m)):
            assert np.array_equal(np.sort(pos), np.arange(cnt))
            assert np.array_equal(np.bincount(pos % 32, minlength=32), np.bincount(np.arange(cnt) % 32, minlength=32))


@pytest.mark.parametrize("case", SLICED)
def test_the_sliced_image_strides_by_32_and_every_read_ahead_stays_inside(case):
    """Lane l of a 32-row slice finds trip tt at off + 32 tt.  A lane runs to its WAVE's longest row and reads two trips ahead: every such index lies
    inside nS / nT; what it meets there is another slice's entries or zeros -- every slot that holds no entry is zero, the tail behind the last slice
    included."""
    pl, it = plan(case), 8
    for M in members(case):
        k, n, m = M.k, M.n, M.m
        img2 = pl["img2"][k]
        h2 = dict(zip(HDR, (int(v) for v in img2[:4 * len(HDR)].view(np.int32))))
        nS, nT = h2["nnzA"], (h2["oAcol"] - h2["oTpr"]) // 4
        Aval2 = img2[h2["oAval"]:h2["oAval"] + 8 * nS].view(np.float64); Acol2 = img2[h2["oAcol"]:h2["oAcol"] + 2 * nS].view(np.uint16)
        Tpr2 = img2[h2["oTpr"]:h2["oTpr"] + 4 * nT].view(np.uint32).astype(np.int64)
        slA = pl["slA"][k * 1024:(k + 1) * 1024].reshape(2, 512); slT = pl["slT"][k * 512:(k + 1) * 512]
        usedA, usedT = np.zeros(nS, dtype=bool), np.zeros(nT, dtype=bool)
        ws0 = it * (512 + 2 * 512 + 2 * 8)                                                       # SL_WS0
        for j in range(2):
            lens = (slA[j] >> 16).astype(int)
            for t in range(512):
                q = 512 * j + (511 - t if j else t)
                off, ln = int(slA[j, t] & 0xffff), int(lens[t])
                assert off % 32 == t % 32 and ln == (M.Arp[q + 1] - M.Arp[q] if q < m else 0)
                e = off + 32 * np.arange(ln); s = slice(M.Arp[q], M.Arp[q] + ln) if q < m else slice(0, 0)
                assert np.array_equal(Aval2[e], M.Aval[s]) and np.array_equal(Acol2[e], M.Acol[s] * it) and not usedA[e].any()
                usedA[e] = True
                assert off + 32 * (lens[64 * (t // 64):64 * (t // 64) + 64].max() + 1) < nS       # two trips past the wave's longest row
        lens = (slT >> 16).astype(int)
        for t in range(512):
            off, ln = int(slT[t] & 0xffff), int(lens[t])
            assert off % 32 == t % 32 and ln == (M.Trp[t + 1] - M.Trp[t] if t < n else 0)
            e = off + 32 * np.arange(ln); s = slice(M.Trp[t], M.Trp[t] + ln) if t < n else slice(0, 0)
            addr, rowpos = Tpr2[e] & ((1 << 21) - 1), Tpr2[e] >> 21
            assert np.all(addr < (1 << 18)) and np.array_equal(rowpos, M.Tpr[s] >> 16) and not usedT[e].any()
            assert np.array_equal(Aval2[(addr - ws0 - h2["oAval"]) // it], M.Aval[M.Tpr[s] & 0xffff]) and np.all((addr - ws0 - h2["oAval"]) % it == 0)
            usedT[e] = True
            assert off + 32 * (lens[64 * (t // 64):64 * (t // 64) + 64].max() + 1) < nT
        assert not Aval2[~usedA].any() and not Acol2[~usedA].any() and not Tpr2[~usedT].any()
        if h2["nnzP"]:
            for key, cnt, t in (("oPval", h2["nnzP"], np.float64), ("oPrp", n + 1, np.uint16), ("oPcol", h2["nnzP"], np.uint16)):
                size = cnt * np.dtype(t).itemsize
                assert np.array_equal(img2[h2[key]:h2[key] + size], M.img[M.h[key]:M.h[key] + size])
        else:
            assert pl["p_all_diag"]


@pytest.mark.parametrize("case", PDIAG)
def test_a_diagonal_P_sits_in_registers_with_its_missing_entries(case):
    pl = plan(case)
    missing = 0
    for M in members(case):
        s = slice(M.k * M.n, (M.k + 1) * M.n)
        d, has = M.Pcsc.diagonal(), np.diff(M.Pcsc.indptr) > 0
        assert (M.Pcsc - sp.diags(d)).nnz == 0
        assert np.array_equal(pl["pdiag_has"][s].astype(bool), has) and np.array_equal(pl["pdiag"][s], np.where(has, d, 0.0))
        src = pl["um_pd"][M.k]
        assert np.array_equal(src >= 0, has) and np.array_equal(M.caller[src[has]], d[has]) and np.all(src[~has] == -1)
        missing += int(np.count_nonzero(~has))
    assert missing > 0                                           # the family has a member that lacks a diagonal entry


@pytest.mark.parametrize("case", IMAGE)
def test_every_value_slot_knows_its_source_in_the_callers_arrays(case):
    pl = plan(case)
    for M in members(case):
        nP, nA = M.Pcsc.nnz, M.Acsc.nnz
        sA, sP = pl["um_imgA"][M.k], pl["um_imgP"][M.k]
        assert np.array_equal(np.sort(sA), nP + np.arange(nA)) and np.array_equal(M.Aval, M.caller[sA])
        assert np.array_equal(np.sort(sP), np.arange(nP)) and np.array_equal(M.Pval, M.caller[sP])
        if pl["want_sliced"] and pl["slA"].size:
            img2, s2 = pl["img2"][M.k], pl["um_imgA2"][M.k]
            h2 = dict(zip(HDR, (int(v) for v in img2[:4 * len(HDR)].view(np.int32))))
            Aval2 = img2[h2["oAval"]:h2["oAval"] + 8 * h2["nnzA"]].view(np.float64)
            assert s2.size == h2["nnzA"] and np.array_equal(np.sort(s2[s2 >= 0]), nP + np.arange(nA)) and np.all(s2[s2 < 0] == -1)
            assert np.array_equal(Aval2[s2 >= 0], M.caller[s2[s2 >= 0]]) and not Aval2[s2 < 0].any()
        else:
            assert pl["um_imgA2"][M.k].size == 0 or not pl["want_sliced"]


def test_the_rules_change_where_they_say():
    f = lambda case, key: plan(case)[key]
    assert (f("n512", "reg_mode"), f("n513", "reg_mode"), f("m1024", "reg_mode"), f("m1025", "reg_mode")) == (1, 2, 1, 2)
    assert (f("row63", "long_rows"), f("row64", "long_rows"), f("row64_f32", "long_rows"), f("register_long_off", "long_rows")) == (0, 1, 1, 0)
    assert f("row63", "want_sliced") and not f("row64", "want_sliced") and not f("register_unsliced_f32", "want_sliced")
    assert f("m512", "permA").size == f("m513", "permA").size == 2 * 2 * 512                       # the second slot exists from the start, used from m = 513
    assert np.all(f("m512", "permA").reshape(2, 2, 512)[:, 1] == -1) and np.count_nonzero(f("m513", "permA").reshape(2, 2, 512)[:, 1] >= 0) == 2
    # the accelerator: the register kernel without extended cones, the register-CG form of the LDS-image kernel with them
    assert (f("register_accelerated", "reg_mode"), f("register_accelerated", "rcg_form")) == (1, 0)
    assert (f("lds_accelerated_psd", "reg_mode"), f("lds_accelerated_psd", "rcg_form"), f("lds_accelerated_psd", "bs")) == (0, 1, 512)
    assert (f("lds_forced_ext", "force_ext"), f("lds_forced_ext", "rcg_stored"), f("lds_bs256", "bs"), f("lds_bs1024", "bs")) == (1, 1, 256, 1024)
    assert (f("lds_ldscg_off", "rcg_form"), f("lds_ldscg_unsorted", "rcg_sorted"), f("lds_ldscg_index_storage", "rcg_stored")) == (0, 0, 0)
    assert not f("register_unsorted", "permA").size and not f("register_index_storage", "qposA").size and not f("register_uncoloured", "posN").size
    assert not f("streaming", "fits") and f("register_sliced_P_in_registers", "p_all_diag") and not f("register_sliced_P_in_image", "p_all_diag")


def test_a_batch_that_does_not_fit_is_left_to_the_streaming_kernel():
    case = "register_sliced_P_in_image"            # row-major 4656 bytes + 66 doubles + 16 slots; sliced 12416 + 11376 bytes
    small = IC.plan(case, max_lds=4096)
    assert not small["fits"] and small["error"] == ""
    mid = IC.plan(case, max_lds=20000)             # the row-major image fits, the sliced one does not
    assert mid["fits"] and not mid["want_sliced"] and mid["error"] == ""
    assert all(np.array_equal(a, b) for a, b in zip(mid["img"], plan(case)["img"]))


def test_a_member_whose_A_and_A_transpose_disagree_is_reported():
    bad = IC.plan("register_sliced_P_in_image", corrupt=(1, 5))
    assert "A / A' mismatch" in bad["error"] and not bad["fits"]


@pytest.mark.parametrize("case", list(IC.CASES))
def test_the_images_are_the_bytes_the_library_built_before_the_planner_moved(case):
    f, pl, rec = IC.family(IC.CASES[case]["family"]), plan(case), IC.HASHES[case]
    info = rec["kernel_info"]
    if info["form"] == "streaming":
        assert not pl["fits"] and rec["image"] == [IC.sha(np.zeros(0, dtype=np.uint8))] * f.nprob
        return
    assert (info["form"], info["long_rows"]) == (("lds_image", "register_1_2", "register_2_4")[pl["reg_mode"]], bool(pl["long_rows"]))
    assert info["p_in_registers"] == bool(info["sliced"] and pl["pdiag"].size) and (not info["sliced"] or (pl["want_sliced"] and pl["slA"].size))
    assert [IC.sha(IC.image_bytes(pl, k, info["sliced"], f.n)) for k in range(f.nprob)] == rec["image"]


@pytest.mark.parametrize("case", list(IC.CASES))
def test_the_other_arrays_are_the_bytes_of_the_planners_first_state(case):
    assert IC.host_hashes(plan(case)) == IC.HASHES[case]["host"]
