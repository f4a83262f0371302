"""The eigensolver runs whose outputs are pinned bit for bit (not a test module): tests/golden/make_lobpcg_digests.py
recorded them with the library as it was before the eigensolver applied its V-cycles and products to blocks of columns,
tests/test_gpu_lobpcg_block.py holds the block path to them.  The block kernels keep every row's order of additions, so
no bit of any output may move."""
import hashlib

import numpy as np

import lobpcg_cases as lc

# (case of lobpcg_cases.PROBLEMS, mass, nev, nb)
CASES = [("skew3", "q1", 4, 4), ("cube8", None, 4, 4), ("elast", None, 3, 6)]
FIELDS = ("evals", "evecs", "res", "hist", "iters", "converged")


def case_id(c):
    return "%s-%s-%d-%d" % (c[0], c[1] or "I", c[2], c[3])


def run(capi, case):
    """one solve on a hierarchy of its own -> {field: sha256 of its bytes}"""
    name, kind, nev, nb = case
    h = capi.Hierarchy.from_problem(lc.problem(name), lc.params(name))
    try:
        lam, X, res, iters, converged, hist = h.lobpcg(nev, nb, M=lc.mass(name, kind), x0=lc.start_block(name, nb),
                                                       tol=lc.TOL, max_iter=lc.MAX_ITER)
    finally:
        h.close()
    out = {"evals": lam, "evecs": np.asfortranarray(X).T, "res": res, "hist": hist,
           "iters": np.int64(iters), "converged": np.int64(converged)}
    return {k: hashlib.sha256(np.ascontiguousarray(np.asarray(v)).tobytes()).hexdigest() for k, v in out.items()}
