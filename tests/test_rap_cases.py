"""The host emulation that test_gpu_rap.py holds the Galerkin product to (rap_cases.py), checked without a GPU: the
vectorised exactly rounded fma against the definition with rationals, and the vectorised walk against the scalar one."""
import numpy as np
import scipy.sparse as sp

import rap_cases as rc


def test_vectorised_fma_is_exactly_rounded():
    rng = np.random.default_rng(0)
    n = 4000
    a = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    b = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    c = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    # cancellation (c close to -a b, to the last bits and to half of them), ties (few mantissa bits), zeros, equal exponents
    c[:800] = -(a[:800] * b[:800]) * (1.0 + rng.integers(-3, 4, 800) * 2.0 ** -52)
    c[800:1200] = -(a[800:1200] * b[800:1200]) * (1.0 + rng.standard_normal(400) * 2.0 ** -26)
    a[1200:1600] = rng.integers(-2 ** 27, 2 ** 27, 400) * 2.0 ** rng.integers(-30, 30, 400)
    b[1200:1600] = rng.integers(-2 ** 27, 2 ** 27, 400) + 0.5
    c[1200:1600] = rng.integers(-4, 5, 400) * 2.0 ** rng.integers(-60, 60, 400)
    a[1600:1700] = 0.0
    c[1700:1800] = 0.0
    c[1800:2400] = rng.standard_normal(600) * np.abs(a[1800:2400] * b[1800:2400])
    got = rc.fma(a, b, c)
    ref = np.array([rc.fma_exact(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:8]
    assert np.count_nonzero(got != a * b + c) > 100      # (the cases do tell an fma from a product and a sum)


def _synthetic(seed):
    rng = np.random.default_rng(seed)
    n, nm = 60, 14
    mises = rng.integers(0, nm, n).astype(np.int32)
    mises[:nm] = np.arange(nm)                       # every MIS has a dof
    order = np.argsort(mises, kind="stable")
    m2d_I = np.concatenate(([0], np.cumsum(np.bincount(mises, minlength=nm)))).astype(np.int32)
    m2d_J = order.astype(np.int32)
    k = rng.integers(0, 4, nm).astype(np.int32)
    k[3] = 0
    A = sp.random(n, n, density=0.15, random_state=seed, format="csr") + sp.eye(n, format="csr")
    A = sp.csr_matrix(A)
    A.data[::7] = 0.0                                # stored zeros count as adjacency
    coloff = rc.coloff_of(k)
    indptr = np.concatenate(([0], np.cumsum(k[mises]))).astype(np.int32)
    indices = np.concatenate([np.arange(coloff[m], coloff[m] + k[m]) for m in mises]).astype(np.int32)
    P = sp.csr_matrix((rng.standard_normal(len(indices)), indices, indptr), shape=(n, int(coloff[-1])))
    return A, P, mises, k, m2d_I, m2d_J


def test_vectorised_walk_is_the_scalar_definition():
    A, P, mises, k, m2d_I, m2d_J = _synthetic(1)
    for m1 in range(len(k)):
        if k[m1] == 0:
            continue
        c1, v1 = rc.emulate_mis_rows(A, P, mises, k, m2d_I, m2d_J, m1, scalar=True)
        c2, v2 = rc.emulate_mis_rows(A, P, mises, k, m2d_I, m2d_J, m1)
        assert np.array_equal(c1, c2) and np.array_equal(v1, v2)
        ref = (P.T @ A @ P).toarray()[rc.coloff_of(k)[m1]:rc.coloff_of(k)[m1 + 1]][:, c1]
        assert np.allclose(v2, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))
