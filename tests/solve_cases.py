"""Problems, references and stopping thresholds for the tests of the solve phase at every smoother degree and every PCG
stopping rule (not a test module): tests/test_gpu_solve_params.py holds the device to them, tests/test_solve_cases.py
checks them on the host.

The tests vary what the C ABI exposes and every other test leaves at its default: `nu_relax` per level (the SAS polynomial of
level l has 3 nu_l + 1 roots, so nu = 1, 2, 3, 4 gives the degrees 4, 7, 10, 13 -- both parities, and with them both
arms of the two ping-pong loops in csrc/cycle.hip), and `squared_tol`, `abs_tol`, `max_iter`, `zero_guess` of the
outer PCG.

    tiles   2 730 rows   constant coefficient: ten staged 256-row tiles and the folded partial one, pair-coded slices,
                         D^-1 byte codes
    skew2   2 197 rows   'skew' coefficient: offset-coded slices, no two values alike
    skew3   2 601 / 611 / 55 rows   three levels with simple eigenvalues (no freedom in the coarse basis)
"""
import functools
import math

import numpy as np
import scipy.sparse as sp

from saamge_amd import problems as pr

PROBLEMS = {
    "tiles": (lambda: pr.poisson3d_problem((20, 12, 9), blk=(4, 4, 3)), 1),
    "skew2": (lambda: pr.poisson3d_problem((12, 12, 12), blk=(4, 4, 4), coef="skew"), 1),
    "skew3": (lambda: pr.poisson3d_problem((16, 16, 8), blk=(4, 4, 2), coarse_blk=[(2, 2, 2)], coef="skew"), 2),
}
ROWS = {"tiles": 2730, "skew2": 2197, "skew3": 2601}
NUS = (1, 2, 3, 4)
THETA = 0.003

SMOOTHER_TOL = 1e-13       # || x - x_ld || <= SMOOTHER_TOL || x_ld ||: test_smoother_matches_oracle's bound for this operation
HEADROOM_TOL = 1e-14       # the float64 oracle against poly_ld: a factor 10 left for the device's summation order and FMAs
SEPARATION = 10.0          # every stopping threshold lies this factor away from every entry of the oracle's history
PCG_NUS = (1, 2)           # part C: 5 iterations at rel_tol = 1e-8
PCG_REL_TOL = 1e-8


def _oracle():
    from oracle import saamge_oracle as o
    return o


@functools.lru_cache(maxsize=None)
def problem(name):
    return PROBLEMS[name][0]()


def coarsenings(name):
    return PROBLEMS[name][1]


@functools.lru_cache(maxsize=None)
def oracle_hierarchy(name):
    """The oracle's hierarchy of a problem, built ONCE: the degree enters nothing in its setup (build_level only stores
    `roots`), so oracle_with_degrees serves every degree tuple from this one build."""
    o, prob = _oracle(), problem(name)
    return o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:coarsenings(name)], theta=THETA)


def oracle_with_degrees(H, nus):
    """H with the SAS roots of degree 3 nus[l] + 1 on level l (in place; returns H)."""
    o = _oracle()
    assert len(nus) == len(H.levels)
    for lv, nu in zip(H.levels, nus):
        lv.roots = o.sas_poly_roots(int(nu))
    return H


def params_with_degrees(nus, **kw):
    """capi.default_params(...) with nu_relax[l] = nus[l]; the slots beyond the last level keep the last value."""
    from saamge_amd import capi
    kw.setdefault("num_coarsenings", len(nus))
    kw.setdefault("theta", THETA)
    p = capi.default_params(nu_relax=int(nus[-1]), **kw)
    for lev, nu in enumerate(nus):
        p.nu_relax[lev] = int(nu)
    return p


def smoother_data(n, seed=3):
    """(b, x0) of the smoother tests: a non-zero start, so every step of the polynomial goes through the residual kernel"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(n)


def _row_sums(terms, indptr):
    out = np.zeros(len(indptr) - 1, dtype=terms.dtype)
    nz = np.nonzero(np.diff(indptr) > 0)[0]
    if nz.size:
        out[nz] = np.add.reduceat(terms, indptr[nz])
    return out


def poly_ld(A, b, x0, roots, dinv_neg):
    """oracle.saamge_oracle.compute_poly in np.longdouble: x += (1 / tau) dinv_neg (A x - b) for every root tau, the row
    sums of A x accumulated in longdouble, 1 / tau as well.  The inputs are the fp64 numbers the device gets; the result
    stays longdouble.  x0 may be a scalar (0: the start of the pre-smoother)."""
    ld = np.longdouble
    assert np.finfo(ld).eps < 1e-18, "np.longdouble is no wider than float64 here: no reference for the smoother"
    A = sp.csr_matrix(A)
    n = A.shape[0]
    val, ind, indptr = A.data.astype(ld), A.indices, A.indptr
    b, d = np.asarray(b, dtype=ld), np.asarray(dinv_neg, dtype=ld)
    x = np.zeros(n, dtype=ld) + np.asarray(x0, dtype=ld)
    for tau in roots:
        tmp = (_row_sums(val * x[ind], indptr) - b) * d
        x = x + (ld(1.0) / ld(tau)) * tmp
    return x


def rel_dev(x, ref):
    """|| x - ref || / || ref || in the precision of ref (longdouble references stay longdouble)"""
    ref = np.asarray(ref)
    e = np.asarray(x, dtype=ref.dtype) - ref
    return float(np.sqrt(e @ e) / np.sqrt(ref @ ref))


def smoother_twice(apply, A, b, x0, roots, dinv_neg):
    """The check of part A for one (operator, degree): apply(b, x) -> new x (fp64) is run twice in a row, the second time
    from its own first result, and each application is held to poly_ld from the SAME start.  Returns the two deviations."""
    x1 = np.array(apply(b, x0.copy()), dtype=np.float64)
    d1 = rel_dev(x1, poly_ld(A, b, x0, roots, dinv_neg))
    x2 = np.array(apply(b, x1.copy()), dtype=np.float64)
    d2 = rel_dev(x2, poly_ld(A, b, x1, roots, dinv_neg))
    return d1, d2


# ---------------------------------------------------------------------------------------------------------------------
# part C: thresholds of the outer PCG's stopping rules, derived from the oracle's history
# ---------------------------------------------------------------------------------------------------------------------
def gmean(a, b):
    return math.sqrt(a * b)


def stopping_cases(histr):
    """name -> {kw: arguments of pcg, iters: where the oracle's history says it stops, threshold: what (B r_k, r_k) is compared
    with}.  `histr`: the oracle's history at PCG_NUS, rel_tol = PCG_REL_TOL (squared), at least 4 entries."""
    h = [float(v) for v in histr]
    rel = gmean(h[2] / h[0], h[3] / h[0])
    mid = gmean(h[1], h[2])
    return {
        "squared_rel": {"kw": dict(rel_tol=PCG_REL_TOL), "iters": len(h) - 1, "threshold": PCG_REL_TOL ** 2 * h[0]},
        "unsquared_rel": {"kw": dict(rel_tol=rel, squared_tol=False), "iters": 3, "threshold": rel * h[0]},
        "abs_squared": {"kw": dict(rel_tol=1e-30, abs_tol=math.sqrt(mid)), "iters": 2, "threshold": mid},
        "abs_unsquared": {"kw": dict(rel_tol=1e-30, abs_tol=mid, squared_tol=False), "iters": 2, "threshold": mid},
    }


def separation(threshold, hist):
    """the smallest factor between the threshold and an entry of the history (>= 1); zero entries are infinitely far"""
    f = [max(threshold / v, v / threshold) for v in hist if v > 0.0]
    return min(f) if f else math.inf


@functools.lru_cache(maxsize=None)
def pcg_oracle_history():
    """(x, iterations, converged, history) of the oracle's PCG on skew3 at PCG_NUS, rel_tol = PCG_REL_TOL"""
    o = _oracle()
    H = oracle_with_degrees(oracle_hierarchy("skew3"), PCG_NUS)
    return o.solve(H, problem("skew3").b, rel_tol=PCG_REL_TOL)
