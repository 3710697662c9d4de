"""What the sign iteration's kernels take for granted about their tile lists (csrc/psd_polar.hip), checked on the host-only planner
csrc/polar_tiles.cpp through tests/polar_tiles_probe.cpp (g++, its own shared object, nothing preloaded): every upper 16 x 16 block of a cone in exactly
one ragged tile, 64-wide panel loads inside the leading dimension, a cone's tiles and queue items in ONE XCD's list, at most three distinct panels
per queue item, per-cone item counts that match the queue, the launch order, the quadrant lists, the large cones' geometry and the lifting-depth rule.

Sides: the smallest at which the rules change, in parts P = ceil(ceil(d / 16) / 4) of a cone's side."""
import atexit
import collections
import ctypes
import itertools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARTS = {17: 1, 64: 1, 65: 2, 80: 2, 128: 2, 129: 3, 192: 3, 193: 4, 200: 4, 256: 4}
SIDES = sorted(PARTS) + [96, 130]                       # 96, 130: for the 96-tile class
BATCHES = {"one_%d" % d: [d] for d in SIDES}            # a single cone: seven XCD lists stay empty
BATCHES["eight"] = [17, 64, 65, 80, 128, 129, 192, 193]
BATCHES["nine"] = [200, 17, 256, 64, 65, 129, 80, 193, 96]
BATCHES["twenty"] = [65, 256, 17, 129, 200, 64, 193, 80, 128, 192, 96, 130, 256, 17, 200, 65, 193, 129, 64, 96]

BCONE = np.dtype([("woff", "<i8"), ("off", "<i4"), ("d", "<i4"), ("kind", "<i4"), ("ld", "<i4"), ("idx", "<i4"), ("ts", "<i4")])
QTILE = np.dtype([("cone", "<i4"), ("ti", "<i4"), ("tj", "<i4"), ("pad", "<i4")])
RTILE = np.dtype([("cone", "<i4"), ("i0", "<i4"), ("j0", "<i4"), ("ext", "<i4"), ("ld", "<i4"), ("d", "<i4"), ("woff", "<i8")])
RPAIR = np.dtype([("cone", "<i4"), ("i0", "<i4"), ("j0", "<i4"), ("i1", "<i4"), ("j1", "<i4"), ("ext0", "<i4"), ("ext1", "<i4"), ("ld", "<i4"),
                  ("d", "<i4"), ("pad", "<i4"), ("woff", "<i8")])

_lib = None


def _probe():
    global _lib
    if _lib is None:
        csrc = os.path.join(_ROOT, "cosmo.jl_amd", "csrc")
        tmp = tempfile.mkdtemp(prefix="polar_tiles_probe_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "polar_tiles_probe.so")
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + csrc, "-o", so,
                        os.path.join(_ROOT, "tests", "polar_tiles_probe.cpp"), os.path.join(csrc, "polar_tiles.cpp")], check=True)
        lib = ctypes.CDLL(so)
        lib.polar_probe_batch.restype = ctypes.c_void_p
        lib.polar_probe_batch.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)] + [ctypes.c_int] * 5
        lib.polar_probe_free.argtypes = [ctypes.c_void_p]
        lib.polar_probe_sizes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
        lib.polar_probe_copy.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        lib.polar_probe_large.argtypes = [ctypes.c_int] * 4 + [ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)]
        lib.polar_probe_cost.restype = ctypes.c_longlong
        lib.polar_probe_cost.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.polar_probe_lift.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)] * 2
        assert lib.polar_probe_xcds() == 8
        _lib = lib
    return _lib


def plan(ds, ts96=0, flat=0, ragged=1, pair=3, sort=1):
    """the batch plan of cones of sides ds as numpy views of the device descriptors"""
    lib = _probe()
    arr = (ctypes.c_int * len(ds))(*ds)
    h = lib.polar_probe_batch(len(ds), arr, ts96, flat, ragged, pair, sort)
    assert h, "the planner refused the batch"
    try:
        sz = (ctypes.c_longlong * 9)()
        lib.polar_probe_sizes(h, sz)
        keys = ["cones", "qtiles", "nbtiles", "nbtiles96", "rtiles", "items", "pairs", "df_ntiles", "work"]
        out = dict(zip(keys, [int(v) for v in sz]))

        def get(which, dtype, n):
            a = np.zeros(n, dtype=dtype)
            lib.polar_probe_copy(h, which, a.ctypes.data_as(ctypes.c_void_p))
            return a
        out["cones"] = get(0, BCONE, out["cones"])
        out["qtiles"] = get(1, QTILE, out["qtiles"])
        out["rtiles"] = get(2, RTILE, out["rtiles"])
        out["items"] = get(3, RTILE, out["items"])
        out["pairs"] = get(4, RPAIR, out["pairs"])
        out["xoff"] = get(5, np.int32, 9)
        out["cone_nt"] = get(6, np.int32, len(ds) if ragged else 0)
        out["flops_performed"], out["flops_useful"] = get(7, np.float64, 2)
    finally:
        lib.polar_probe_free(h)
    return out


def nb16(d):
    return (d + 15) // 16


def ext_of(e):
    return e & 255, (e >> 8) & 255, (e >> 16) & 1


def tile_key(t):
    return tuple(int(t[k]) for k in ("cone", "i0", "j0", "ext", "ld", "d", "woff"))


def halves(it):
    """the one or two ragged tiles of an RPair, as tile_key tuples"""
    common = (int(it["ld"]), int(it["d"]), int(it["woff"]))
    out = [(int(it["cone"]), int(it["i0"]), int(it["j0"]), int(it["ext0"])) + common]
    if it["ext1"]:
        out.append((int(it["cone"]), int(it["i1"]), int(it["j1"]), int(it["ext1"])) + common)
    return out


def cost(d, ext):
    return int(_probe().polar_probe_cost(int(d), int(ext)))


@pytest.mark.parametrize("sort", [1, 0])
@pytest.mark.parametrize("pair", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_ragged_tiles_and_queue_items(name, pair, sort):
    ds = BATCHES[name]
    p = plan(ds, pair=pair, sort=sort)
    cones, rt = p["cones"], p["rtiles"]
    assert len(cones) == len(ds)
    # ---- cone table: pass-through members, leading dimensions, work offsets
    for i, (c, d) in enumerate(zip(cones, ds)):
        assert (c["d"], c["off"], c["kind"], c["idx"], c["ts"]) == (d, 7 * i, i % 3, 100 + i, 64)
        assert c["ld"] % c["ts"] == 0 and c["ld"] >= d
    by_off = sorted(cones, key=lambda c: c["woff"])
    end = 0
    for c in by_off:                                                         # the ranges [woff, woff + 4 ld^2) tile [0, work)
        assert c["woff"] == end
        end += 4 * int(c["ld"]) ** 2
    assert end == p["work"]
    # ---- interleaved list: entry 8 s + x belongs to XCD x, padding is null, a cone has one XCD
    assert len(rt) % 8 == 0 and len(rt) > 0
    real = [t for t in rt if t["cone"] >= 0]
    assert all(t["cone"] == -1 for t in rt if t["cone"] < 0)
    xcd = {}
    for pos, t in enumerate(rt):
        if t["cone"] >= 0:
            assert xcd.setdefault(int(t["cone"]), pos % 8) == pos % 8
    for x in range(8):                                                       # padding only at the end of an XCD's list
        col = [int(t["cone"]) for t in rt[x::8]]
        n_real = sum(c >= 0 for c in col)
        assert all(c >= 0 for c in col[:n_real])
    assert set(xcd) == set(range(len(ds)))
    if len(ds) == 1:
        assert len({pos % 8 for pos, t in enumerate(rt) if t["cone"] >= 0}) == 1
    elif len(ds) >= 8:
        assert len(set(xcd.values())) == 8                                   # the dealing uses every XCD before it wraps around
    # ---- bounds of every tile, coverage of every upper block
    seen = {c: np.zeros((nb16(d), nb16(d)), dtype=int) for c, d in enumerate(ds)}
    for t in real:
        c = int(t["cone"]); d = ds[c]
        ei, ej, dg = ext_of(int(t["ext"]))
        i0, j0 = int(t["i0"]), int(t["j0"])
        assert (t["ld"], t["d"], t["woff"]) == (cones[c]["ld"], d, cones[c]["woff"])
        assert i0 % 16 == 0 and j0 % 16 == 0 and 0 <= i0 <= j0
        assert i0 + 64 <= t["ld"] and j0 + 64 <= t["ld"]
        assert 1 <= ei <= 4 and 1 <= ej <= 4
        assert i0 + 16 * ei <= 16 * nb16(d) and j0 + 16 * ej <= 16 * nb16(d)
        assert dg == (1 if i0 == j0 else 0)
        if dg:
            assert ei == ej
        else:
            assert i0 + 16 * ei <= j0                                        # an off-diagonal tile lies strictly above the diagonal blocks
        for bi in range(i0 // 16, i0 // 16 + ei):
            for bj in range(j0 // 16, j0 // 16 + ej):
                if not dg or bi <= bj:
                    seen[c][bi, bj] += 1
    for c, d in enumerate(ds):
        assert np.array_equal(seen[c], np.triu(np.ones((nb16(d), nb16(d)), dtype=int))), (c, d)
    # ---- queue items: list x = [xoff[x], xoff[x + 1]), the same tiles, the same XCD, counts
    xoff = [int(v) for v in p["xoff"]]
    items = p["pairs"] if pair else p["items"]
    assert len(p["items" if pair else "pairs"]) == 0
    assert xoff[0] == 0 and all(a <= b for a, b in zip(xoff, xoff[1:])) and xoff[8] == len(items)
    assert p["df_ntiles"] == len(real)
    per_cone = collections.Counter()
    tiles_of_items = []
    for x in range(8):
        for it in items[xoff[x]:xoff[x + 1]]:
            assert it["cone"] >= 0 and xcd[int(it["cone"])] == x
            per_cone[int(it["cone"])] += 1
            tiles_of_items += halves(it) if pair else [tile_key(it)]
    assert collections.Counter(tiles_of_items) == collections.Counter(tile_key(t) for t in real)
    assert [per_cone[c] for c in range(len(ds))] == [int(v) for v in p["cone_nt"]]
    # ---- pairs
    if pair:
        for it in items:
            assert it["pad"] == 0
            assert len({int(it["i0"]), int(it["j0"]), int(it["i1"]), int(it["j1"])}) <= 3          # distinct panels an item stages
            if not it["ext1"]:
                assert (it["i1"], it["j1"]) == (it["i0"], it["j0"])
            elif pair == 1:
                assert it["i0"] == it["i1"]
            elif pair == 3:
                assert it["i0"] == it["i1"] or it["j0"] == it["j1"]
            assert pair != 2 or it["ext1"] == 0
    # items per cone from the pairing rule: block row I of P parts has P - I tiles, taken two at a time; mode 3 pairs the left-over ones as well
    want = {1: {1: 1, 2: 2, 3: 4, 4: 6}, 3: {1: 1, 2: 2, 3: 3, 4: 5}}
    for c, d in enumerate(ds):
        if d in PARTS:
            P = PARTS[d]
            assert per_cone[c] == (want[pair][P] if pair in want else P * (P + 1) // 2), (d, pair)
    # ---- order inside an XCD's list
    for x in range(8):
        tl = [t for t in rt[x::8] if t["cone"] >= 0]
        il = items[xoff[x]:xoff[x + 1]]
        if sort:
            tc = [cost(t["d"], t["ext"]) for t in tl]
            ic = [max(cost(it["d"], it["ext0"]), cost(it["d"], it["ext1"]) if it["ext1"] else 0) for it in il] if pair else [cost(it["d"], it["ext"]) for it in il]
            assert all(a >= b for a, b in zip(tc, tc[1:])) and all(a >= b for a, b in zip(ic, ic[1:]))
        else:
            for lst in (tl, il):                                             # cones by decreasing ld, ties in input order, a cone's entries together
                order = [k for k, _ in itertools.groupby(int(t["cone"]) for t in lst)]
                assert len(order) == len(set(order))
                keys = [(-int(cones[c]["ld"]), c) for c in order]
                assert keys == sorted(keys)


def test_tile_cost_model():
    """10 * slots + 2 per 16-row step, plus 125; slots = blocks of the fullest wave (blocks dealt to four waves, upper blocks only on the diagonal)"""
    assert cost(64, 4 | 4 << 8 | 1 << 16) == 4 * (10 * 3 + 2) + 125           # 10 blocks: 3 slots
    assert cost(64, 4 | 4 << 8) == 4 * (10 * 4 + 2) + 125                     # 16 blocks: 4 slots
    assert cost(200, 3 | 3 << 8 | 1 << 16) == 13 * (10 * 2 + 2) + 125         # 6 blocks: 2 slots
    assert cost(17, 2 | 2 << 8 | 1 << 16) == 2 * (10 * 1 + 2) + 125           # 3 blocks: 1 slot


@pytest.mark.parametrize("ts96", [0, 1])
@pytest.mark.parametrize("flat", [0, 1])
@pytest.mark.parametrize("name", ["one_96", "one_130", "one_256", "eight", "nine", "twenty"])
def test_quadrant_lists(name, flat, ts96):
    ds = BATCHES[name]
    p = plan(ds, ts96=ts96, flat=flat, ragged=0)
    cones, qt = p["cones"], p["qtiles"]
    assert len(p["rtiles"]) == len(p["items"]) == len(p["pairs"]) == 0
    assert len(qt) == p["nbtiles"] + p["nbtiles96"]
    for c, d in zip(cones, ds):
        assert c["ts"] == (96 if ts96 and (64 < d <= 96 or 128 < d <= 192) else 64)
        assert c["ld"] % c["ts"] == 0 and c["ld"] >= d
    if not ts96:
        assert p["nbtiles96"] == 0
    want = collections.Counter()
    for c, cn in enumerate(cones):
        nt = int(cn["ld"]) // int(cn["ts"])
        for tj in range(nt):
            for ti in range(tj + 1):
                want[(int(cn["ts"]), c, ti, tj)] += 1
    got = collections.Counter()
    for cls, part in ((64, qt[:p["nbtiles"]]), (96, qt[p["nbtiles"]:])):
        assert flat or len(part) % 8 == 0
        xcd = {}
        for pos, t in enumerate(part):
            assert t["pad"] == 0
            if t["cone"] < 0:
                assert not flat and t["cone"] == -1
                continue
            assert cones[int(t["cone"])]["ts"] == cls
            got[(cls, int(t["cone"]), int(t["ti"]), int(t["tj"]))] += 1
            if not flat:
                assert xcd.setdefault(int(t["cone"]), pos % 8) == pos % 8
    assert got == want
    quad = sum(2.0 * (nt * (nt + 1) // 2) * ts * ts * ((d + 31) // 32 * 32) for d, ts, nt in ((d, int(c["ts"]), int(c["ld"]) // int(c["ts"])) for c, d in zip(cones, ds)))
    assert p["flops_performed"] == quad
    assert p["flops_useful"] == sum(float(d) * d * (d + 1) for d in ds)


@pytest.mark.parametrize("name", ["one_17", "one_200", "nine", "twenty"])
def test_flops_of_the_ragged_lists(name):
    ds = BATCHES[name]
    p = plan(ds)
    blocks = collections.Counter()
    for t in p["rtiles"]:
        if t["cone"] >= 0:
            ei, ej, dg = ext_of(int(t["ext"]))
            blocks[int(t["cone"])] += ei * (ei + 1) // 2 if dg else ei * ej
    assert p["flops_performed"] == sum(2.0 * 256 * 16 * nb16(d) * blocks[c] for c, d in enumerate(ds))
    assert p["flops_useful"] == sum(float(d) * d * (d + 1) for d in ds)


def large(d, streamk=0, ts=0, sk=0, skg=0):
    out = (ctypes.c_int * 5)()
    _probe().polar_probe_large(d, streamk, ts, sk, skg, out)
    return dict(zip(["ts", "sk", "ld", "skg", "skc"], [int(v) for v in out]))


@pytest.mark.parametrize("d", [257, 1000, 2000])
def test_large_cone_geometry(d):
    def upper(ts):
        nt = -(-d // ts)
        return nt * (nt + 1) // 2
    rounds_x_work = {ts: -(-upper(ts) // 256) * ts * ts for ts in (64, 96)}    # rounds of upper tiles over the 256 CUs x tile work
    g = large(d)
    assert rounds_x_work[g["ts"]] == min(rounds_x_work.values()) and (g["ts"] == 64 or rounds_x_work[96] < rounds_x_work[64])
    assert g["ld"] % g["ts"] == 0 and 0 <= g["ld"] - d < g["ts"]
    assert g["sk"] == (2 if g["ts"] == 96 and upper(96) <= 256 else 1) and g["skg"] == 0
    for ts in (64, 96):                                                      # a forced tile side; the k-split only where it exists
        f = large(d, ts=ts)
        assert f["ts"] == ts and f["ld"] % ts == 0 and f["ld"] >= d
        assert f["sk"] == (2 if ts == 96 and upper(96) <= 256 else 1)
        assert large(d, ts=ts, sk=1)["sk"] == 1 and large(d, ts=ts, sk=2)["sk"] == (2 if ts == 96 else f["sk"])
    s = large(d, streamk=1)
    assert s["ts"] == 96 and s["sk"] == 3 and s["ld"] % 96 == 0 and s["ld"] >= d
    assert s["skc"] in (1, 8) and s["skg"] > 0 and s["skg"] % s["skc"] == 0 and s["skg"] <= 512
    r = large(d, streamk=1, skg=64)
    assert r["skg"] > 0 and r["skg"] % r["skc"] == 0 and r["skg"] <= 64


def lift(k, patience, cap, floor, failed):
    n = len(failed)
    out = (ctypes.c_int * (3 * n))()
    _probe().polar_probe_lift(k, patience, cap, floor, n, (ctypes.c_int * n)(*failed), out)
    return [tuple(out[3 * t:3 * t + 3]) for t in range(n)]


def test_lift_depth_rule():
    """(k, streak, patience) after every verification result, by hand"""
    # failures: one step deeper up to the cap of 18, patience doubled up to 96
    assert lift(16, 3, 18, 0, [1] * 7) == [(17, 0, 6), (18, 0, 12), (18, 0, 24), (18, 0, 48), (18, 0, 96), (18, 0, 96), (18, 0, 96)]
    # passes: one step shallower after `patience` in a row; a failure resets the streak
    assert lift(3, 3, 18, 0, [0, 0, 1, 0, 0, 0, 0, 0, 0]) == [(3, 1, 3), (3, 2, 3), (4, 0, 6), (4, 1, 6), (4, 2, 6), (4, 3, 6), (4, 4, 6), (4, 5, 6), (3, 0, 6)]
    # floor 0 (batch): down to no lifting step at all
    assert lift(1, 1, 18, 0, [0, 0, 0]) == [(0, 0, 1), (0, 1, 1), (0, 2, 1)]
    # floor 2 (large cones)
    assert lift(3, 3, 18, 2, [0] * 7) == [(3, 1, 3), (3, 2, 3), (2, 0, 3), (2, 1, 3), (2, 2, 3), (2, 3, 3), (2, 4, 3)]
    # patience 96 really waits for 96 passes
    seq = lift(10, 96, 18, 2, [0] * 96)
    assert seq[94] == (10, 95, 96) and seq[95] == (9, 0, 96)
