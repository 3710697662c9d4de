"""Generates tests/golden/batch_image_cases.npz: the inputs of the batch LDS-image tests and what the library answered for them BEFORE the image
planner moved into csrc/batch_image.cpp.  tests/batch_image_cases.py reads it.

Inputs (the arrays themselves, so that no test depends on NumPy's generator stream):
  * the five families of tests/batch_update_cases.py with the UNSCALED P and A of every member (the `tall` family thinned to members 0 and 3, which have
    different patterns: five members of m = 1030 would be half of the file), each with the start of test_gpu_batch_update_matrices.same_iterates;
  * the smallest shapes at which a rule of the planner changes, two members of different patterns each, values in eighths: m = 512 | 513 (the second,
    backwards slot of the rows starts), n = 512 | 513 and m = 1024 | 1025 (register kernel <512, 1, 2> | <512, 2, 4>), a row of 63 | 64 entries (LONG_ROW).
Cases: the eleven kernel forms of tests/test_gpu_batch_update_matrices.FORMS under their switches, every other switch on its own, the accelerator,
the shapes.

Recorded answers (tests/batch_image_cases.answers for `parent`; the probe's arrays for `host`) come from JSON files written on a machine with the
GPU and are merged with --parent FILE / --host FILE; without them the ones in the existing fixture are kept.
Deterministic: seeded draws, a zip written with fixed time stamps.
Usage:  python tests/golden/make_fixtures_batch_image.py [--parent parent.json] [--host host.json]"""
import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "batch_image_cases.npz")

F64, F32 = "float64", "float32"
CASES = {
    # name: (family, dtype, switches COSMO_HIP_BATCH_<name>, accelerator, iterates recorded)
    # -- tests/test_gpu_batch_update_matrices.FORMS
    "streaming": ("base", F64, {"LDS": 0}, False, True),
    "streaming_f32": ("base", F32, {"LDS": 0}, False, True),
    "lds_index_order": ("base", F64, {"REG": 0}, False, True),
    "lds_index_order_f32": ("base", F32, {"REG": 0}, False, True),
    "lds_sorted_storage": ("psd", F64, {"REG": 0}, False, True),
    "lds_sorted_storage_f32": ("psd", F32, {"REG": 0}, False, True),
    "register_sliced_P_in_image": ("base", F64, {}, False, True),
    "register_sliced_P_in_registers": ("pdiag", F64, {}, False, True),
    "register_unsliced_f32": ("base", F32, {}, False, True),
    "register_long_rows": ("long", F64, {}, False, True),
    "register_2_4": ("tall", F64, {}, False, True),
    # -- the other switches, the accelerator, PSD cones in the register kernel
    "register_psd": ("psd", F64, {}, False, False),
    "register_accelerated": ("base", F64, {}, True, False),
    "lds_accelerated_psd": ("psd", F64, {}, True, False),
    "lds_forced_ext": ("base", F64, {"REG": 0, "EXT": 1}, False, False),
    "lds_forced_ext_n513": ("n513", F64, {"REG": 0, "EXT": 1}, False, False),     # the register-CG form's columns over two slots
    "lds_ldscg_off": ("psd", F64, {"REG": 0, "LDSCG": 0}, False, False),
    "lds_ldscg_unsorted": ("psd", F64, {"REG": 0, "LDSCG_SORTED": 0}, False, False),
    "lds_ldscg_index_storage": ("psd", F64, {"REG": 0, "STORE_SORTED": 0}, False, False),
    "lds_bs256": ("base", F64, {"REG": 0, "BS": 256}, False, False),
    "lds_bs1024": ("base", F64, {"REG": 0, "BS": 1024}, False, False),
    "register_index_storage": ("base", F64, {"STORE_SORTED": 0}, False, False),
    "register_unsorted": ("base", F64, {"SORTED": 0}, False, False),
    "register_uncoloured": ("base", F64, {"COLOR": 0}, False, False),
    "register_sliced_off": ("base", F64, {"SLICED": 0}, False, False),
    "register_long_off": ("long", F64, {"LONG": 0}, False, False),
    # -- shapes
    "m512": ("m512", F64, {}, False, False), "m513": ("m513", F64, {}, False, False),
    "m1024": ("m1024", F64, {}, False, False), "m1025": ("m1025", F64, {}, False, False),
    "n512": ("n512", F64, {}, False, False), "n513": ("n513", F64, {}, False, False),
    "row63": ("row63", F64, {}, False, False), "row64": ("row64", F64, {}, False, False),
    "row64_f32": ("row64", F32, {}, False, False),
}
SHAPES = {"m512": (30, 512, None), "m513": (30, 513, None), "m1024": (30, 1024, None), "m1025": (30, 1025, None), "n512": (512, 520, None),
          "n513": (513, 520, None), "row63": (70, 40, 63), "row64": (70, 40, 64)}       # n, m, entries of row 5
TALL_MEMBERS = (0, 3)


def _csc(M):
    M = sp.csc_matrix(M); M.sort_indices()
    return M


def _eighths(rng, count):
    return rng.integers(1, 17, count) * rng.choice([-1.0, 1.0], count) / 8.0


def shape_member(rng, n, m, dense):
    """1 .. 4 entries in every row of A (one row empty, one of `dense` entries), a tridiagonal P that lacks a diagonal entry"""
    rows, cols = [], []
    for i in range(m):
        cnt = 0 if i == 3 else (dense if dense and i == 5 else int(rng.integers(1, 5)))
        rows += [i] * cnt; cols += list(rng.choice(n, cnt, replace=False))
    A = _csc(sp.coo_matrix((_eighths(rng, len(rows)), (rows, cols)), shape=(m, n)))
    d = rng.integers(8, 17, n) / 8.0; d[7] = 0.0
    o = rng.integers(0, 2, n - 1) / 8.0; o[6] = o[7] = 0.0
    P = sp.diags([o, d, o], [-1, 0, 1]).tocsc(); P.eliminate_zeros()
    return dict(P=_csc(P), A=A, q=_eighths(rng, n), b=_eighths(rng, m))


def families():
    from tests import batch_update_cases as BC
    ZERO, NONNEG, BOX = 0, 1, 2
    out = {}
    for name in BC.SHAPES:
        fam = BC.family(name)
        if name == "tall":
            fam = [fam[k] for k in TALL_MEMBERS]
        sets = fam[0]["sets"]
        m, n = fam[0]["A"].shape
        rng = np.random.default_rng(23)                          # the start of same_iterates
        start = (rng.standard_normal(len(fam) * n), rng.standard_normal(len(fam) * m), rng.standard_normal(len(fam) * m))
        out[name] = dict(members=[dict(P=_csc(c["P"]), A=_csc(c["A"]), q=c["q"], b=c["b"]) for c in fam],
                         cone_types=[K.kind for K in sets], cone_dims=[K.dim for K in sets], start=start,
                         box_l=[K.l for c in fam for K in c["sets"] if K.kind == BOX], box_u=[K.u for c in fam for K in c["sets"] if K.kind == BOX])
    for j, (name, (n, m, dense)) in enumerate(SHAPES.items()):
        rng = np.random.default_rng(500 + j)
        out[name] = dict(members=[shape_member(rng, n, m, dense) for _ in range(2)], cone_types=[ZERO, NONNEG], cone_dims=[4, m - 4], start=None,
                         box_l=[], box_u=[])
        assert out[name]["members"][0]["A"].indices.tobytes() != out[name]["members"][1]["A"].indices.tobytes()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--host")
    args = ap.parse_args()
    hashes = {}
    if os.path.exists(OUT):
        hashes = json.loads(bytes(np.load(OUT)["hashes_json"]).decode())
    if args.parent:
        for case, ans in json.load(open(args.parent)).items():
            hashes.setdefault(case, {}).update(ans)
    if args.host:
        for case, ans in json.load(open(args.host)).items():
            hashes.setdefault(case, {})["host"] = ans
    arrays = {}
    for name, f in families().items():
        mem = f["members"]
        m, n = mem[0]["A"].shape
        cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt).ravel() for x in xs]) if len(xs) else np.zeros(0, dtype=dt)
        put = lambda key, v: arrays.__setitem__("%s.%s" % (name, key), v)
        put("dims", np.array([len(mem), n, m], dtype=np.int64))
        put("cone_types", np.array(f["cone_types"], dtype=np.int32)); put("cone_dims", np.array(f["cone_dims"], dtype=np.int64))
        put("box_l", cat(f["box_l"], np.float64)); put("box_u", cat(f["box_u"], np.float64))
        put("q", cat([c["q"] for c in mem], np.float64)); put("b", cat([c["b"] for c in mem], np.float64))
        for key in ("P", "A"):
            put(key + "p", cat([c[key].indptr for c in mem], np.int32)); put(key + "i", cat([c[key].indices for c in mem], np.int32))
            put(key + "x", cat([c[key].data for c in mem], np.float64))
        if f["start"] is not None:
            for key, v in zip(("x0", "s0", "mu0"), f["start"]):
                put(key, v)
    cases = {k: dict(family=v[0], dtype=v[1], env=v[2], aa=v[3], iterates=v[4]) for k, v in CASES.items()}
    arrays["cases_json"] = np.frombuffer(json.dumps(cases, sort_keys=True).encode(), dtype=np.uint8)
    arrays["hashes_json"] = np.frombuffer(json.dumps(hashes, sort_keys=True).encode(), dtype=np.uint8)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO(); np.save(buf, arrays[key])
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(2020, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print("%s: %d bytes, %d cases, %d with recorded answers" % (OUT, os.path.getsize(OUT), len(cases), len(hashes)))


if __name__ == "__main__":
    main()
