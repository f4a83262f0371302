"""Hierarchies, columns and PCG settings of the block solve tests (not a test module): tests/test_gpu_cycle_block.py holds
the device's block calls to its single-vector calls bit for bit, tests/test_cycle_block_cases.py checks on the CPU, with the
oracle's PCG, that the columns leave the loop at different steps."""
import functools

import numpy as np

import lobpcg_cases as lc
import solve_cases as sc

HIERARCHIES = ("tiles", "skew3", "elast")
NUS = (1, 3)                    # degrees 4 and 10: both parities of the smoother's ping-pong
COARSE = (1, 2, 3)              # dense inverse, inner PCG, block-tridiagonal
KS = (1, 2, 5, 8, 11)
KMAX = max(KS)
LD_PAD = 5
# The outer PCG of the tests.  With a relative tolerance alone every column but the zero one takes the same number of steps
# (the V-cycle's convergence factor hardly depends on the right-hand side), so the threshold is an ABSOLUTE one, squared like
# rel_tol: (B r, r) < abs_tol^2, placed between steps 2 and 3 of the random column's history in the oracle's PCG (the
# geometric middle, per hierarchy and degree).  Columns of other scales cross it sooner or later: the exits below.
# MAX_ITER = 3: the random column converges on the last step allowed, the column of scale 1e3 stops on max_iter.
PCG_KW = dict(rel_tol=1e-8, squared_tol=True, zero_guess=True)
ABS_TOL = {("tiles", 1): 1.3e-2, ("tiles", 3): 1.1e-4, ("skew3", 1): 7.9e-3, ("skew3", 3): 3.7e-5,
           ("elast", 1): 2.0e-1, ("elast", 3): 2.3e-2, ("q2", 3): 0.0}
MAX_ITER = 3


@functools.lru_cache(maxsize=None)
def problem(name):
    if name == "q2":
        from saamge_amd import problems as pr
        return pr.elasticity3d_q2_problem((10, 10, 10), blk=(2, 2, 2))
    return lc.problem(name) if name in lc.PROBLEMS else sc.problem(name)


def coarsenings(name):
    return 1 if name == "q2" else lc.coarsenings(name)


def params(name, nu, coarse_solver):
    from saamge_amd import capi
    return capi.default_params(num_coarsenings=coarsenings(name), theta=sc.THETA, nu_relax=nu, coarse_solver=coarse_solver)


@functools.lru_cache(maxsize=None)
def columns(name):
    """KMAX columns, one per row of the result, chosen to leave the PCG loop at different steps:
    0 zero (0 iterations)   1 the problem's b   2 b + 1e3 random (stops on max_iter)   3 random (converges on the last
    step)   4 A times a smooth vector   5 .. A times the constant, a random column of scale 1e-7 (0 iterations: below the
    absolute threshold from the start), and further ones whose scales differ by orders of magnitude"""
    p = problem(name)
    A = p.A.tocsr()
    n = A.shape[0]
    rng = np.random.default_rng(29)
    t = np.linspace(0.0, 1.0, n)
    smooth = np.sin(np.pi * t) + 0.25 * np.cos(3.0 * np.pi * t)
    rnd = rng.standard_normal(n)
    b = np.asarray(p.b, dtype=np.float64).copy()
    cols = [np.zeros(n), b, b + 1e3 * rnd, rnd, A @ smooth, A @ np.ones(n)]
    cols.append(1e-7 * rng.standard_normal(n))
    cols.append(A @ (smooth ** 2))
    while len(cols) < KMAX:
        cols.append(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4))
    return np.ascontiguousarray(np.stack(cols[:KMAX]))


def block(cols, k, n, pad):
    """the first k columns as a (k, n + pad) block, padding rows NaN"""
    B = np.full((k, n + pad), np.nan)
    B[:, :n] = cols[:k]
    return B
