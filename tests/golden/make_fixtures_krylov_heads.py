"""Writes tests/golden/krylov_heads_parent.json: per case of tests/test_gpu_krylov_heads.py (route x size) the SHA-256 of x and the Krylov iteration count.
Run it on the GPU from a checkout of the PARENT of the commit that changed the heads of the Krylov kernels, with this file and the test module copied in
(they use the public Python API only):    python tests/golden/make_fixtures_krylov_heads.py [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_gpu_krylov_heads as T  # noqa: E402


def setenv(k, v):
    os.environ[k] = v


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    cases = {}
    for n in T.NS:
        prob = T.heads_qp(n)
        for route in sorted(T.ROUTES):
            x, kkt, fs = T.run_case(route, n, prob, setenv)
            cases["%s-%d" % (route, n)] = {"x_sha256": T.x_hash(x), "kkt_iters": kkt, "fold_enabled": int(fs["enabled"]), "factored_rows": int(fs["factored_rows"])}
            print(route, n, cases["%s-%d" % (route, n)], flush=True)
    with open(out, "w") as f:
        json.dump({"written_by": "tests/golden/make_fixtures_krylov_heads.py on the parent build", "iters": T.ITERS, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
