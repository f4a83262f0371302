"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same
inputs.  Bit-exact for integer topology; fp64 quantities within the tolerances written in
each test.  Run with `pytest -m gpu` on an MI355X."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from saamge_amd import problems as pr

pytestmark = pytest.mark.gpu

EIG_TOL = 1e-11      # eigenvalues, absolute (spectrum of D^-1 A lies in [0, 1])
PROJ_TOL = 1e-9      # D-orthogonal projectors onto the wanted eigenspaces
VCYCLE_TOL = 1e-10   # relative, V-cycle output / PCG residual history (north_star)


def _capi():
    from saamge_amd import capi
    return capi


def _oracle():
    from oracle import saamge_oracle as o
    return o


def test_spmv_matches_scipy():
    capi = _capi()
    rng = np.random.default_rng(0)
    for (n, m, dens) in [(1, 1, 1.0), (37, 53, 0.2), (1000, 1000, 0.03), (5000, 300, 0.01)]:
        A = sp.random(n, m, density=dens, random_state=rng, format="csr")
        A.data[:] = rng.standard_normal(A.nnz)
        x = rng.standard_normal(m)
        y = capi.spmv(A, x)
        ref = A @ x
        assert np.allclose(y, ref, rtol=1e-13, atol=1e-13 * (np.abs(A) @ np.abs(x)).max() + 1e-300)
    # empty rows
    A = sp.csr_matrix((5, 4))
    assert np.array_equal(capi.spmv(A, np.ones(4)), np.zeros(5))


def _proj(X, D):
    """D-orthogonal projector onto span(X) applied to a fixed probe."""
    n = X.shape[0]
    probe = np.cos(np.arange(n) * 0.7 + 0.3)
    G = X.T @ (D[:, None] * X)
    return X @ np.linalg.solve(G, X.T @ (D * probe))


@pytest.mark.parametrize("seed", [0, 1])
def test_batched_lower_eigens_vs_lapack(seed):
    """xpacks_calc_lower_eigens_dense: same counts, eigenvalues and eigenspaces as dsygvx."""
    capi, o = _capi(), _oracle()
    rng = np.random.default_rng(seed)
    mats, diags, thetas = [], [], []
    for n in [1, 2, 3, 5, 8, 17, 33, 64, 65, 100, 130, 257]:
        # sparse-ish SPSD "stiffness" matrix with a known null vector, like an AE matrix
        G = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=rng).toarray()
        W = np.abs(G + G.T)
        L = np.diag(W.sum(axis=1)) - W
        L += 1e-3 * np.diag(rng.random(n)) * (seed == 1)
        if n == 1:
            L = np.array([[2.0]])
        L = L + np.diag(np.where(np.diag(L) <= 0, 1.0, 0.0))
        D = o.snd_D_from_dense(L)
        mats.append(L)
        diags.append(D)
    theta = 0.05
    res = capi.lower_eigens_batched(mats, diags, -1.0, theta)
    for L, D, (w, X) in zip(mats, diags, res):
        wr, Xr = o.lower_eigens_dense(L, D, theta)
        assert len(w) == len(wr), (L.shape, w, wr)
        assert np.allclose(w, wr, rtol=0, atol=EIG_TOL)
        # D-orthonormality and residuals
        G = X.T @ (D[:, None] * X)
        assert np.allclose(G, np.eye(len(w)), atol=1e-10)
        R = L @ X - (D[:, None] * X) * w[None, :]
        assert np.abs(R).max() <= 1e-10 * max(1.0, np.abs(L).max())
        assert np.allclose(_proj(X, D), _proj(Xr, D), atol=PROJ_TOL)


def test_batched_lower_eigens_large_agglomerates():
    """Agglomerate sizes of the headline configs (405 = 8x8x4 Q1, 729 = 8^3 Q1) and beyond the
    LDS-resident band of the dense path (n > 588: band and bulge in global memory, csrc/eig_dense_plan.h;
    2187 = the 4^3 Q2 elasticity agglomerate of BASELINE config 5).  Under the default eig_min_n these matrices
    take the few-eigenpairs path: test_dense_path_reaches_every_kernel_plan below holds the dense path to them."""
    capi, o = _capi(), _oracle()
    rng = np.random.default_rng(5)
    mats, diags = [], []
    for n in [405, 729, 1300, 2187]:
        G = sp.random(n, n, density=8.0 / n, random_state=rng).toarray()
        W = np.abs(G + G.T)
        L = np.diag(W.sum(axis=1)) - W + 1e-4 * np.diag(rng.random(n))
        mats.append(L)
        diags.append(o.snd_D_from_dense(L))
    theta = 0.01
    res = capi.lower_eigens_batched(mats, diags, -1.0, theta)
    for L, D, (w, X) in zip(mats, diags, res):
        wr, Xr = o.lower_eigens_dense(L, D, theta)
        assert len(w) == len(wr) and len(w) >= 1
        assert np.allclose(w, wr, rtol=0, atol=EIG_TOL)
        assert np.allclose(X.T @ (D[:, None] * X), np.eye(len(w)), atol=1e-10)
        R = L @ X - (D[:, None] * X) * w[None, :]
        assert np.abs(R).max() <= 1e-10 * max(1.0, np.abs(L).max())
        assert np.allclose(_proj(X, D), _proj(Xr, D), atol=PROJ_TOL)


_LARGE_AGGLOMERATES = {}


def _large_agglomerates():
    """The four matrices of the test above (same generator, seed 5), their diagonals and the oracle's pairs at theta = 0.01:
    built once, shared and left unchanged by the cases below."""
    if not _LARGE_AGGLOMERATES:
        o = _oracle()
        rng = np.random.default_rng(5)
        for n in [405, 729, 1300, 2187]:
            G = sp.random(n, n, density=8.0 / n, random_state=rng).toarray()
            W = np.abs(G + G.T)
            L = np.diag(W.sum(axis=1)) - W + 1e-4 * np.diag(rng.random(n))
            D = o.snd_D_from_dense(L)
            _LARGE_AGGLOMERATES[n] = (L, D, o.lower_eigens_dense(L, D, 0.01))
    return _LARGE_AGGLOMERATES


# Batches that reach the plan values of the dense path (csrc/eig_dense_plan.h) under eig_dense_only:
#   [405]         register QR only (npmax <= 389), band in LDS (405 <= 588), 256-thread back-transformation
#   [729]         register and LDS QR (npmax = 713 at k0 = 0), band in HBM
#   [1300, 2187]  all three QR kernels as k0 grows (npmax = 2171: the 1 024-thread one), band in HBM, 1 024-thread
#                 back-transformation, both variants of the fused update
#   [405] with eig_dense_one_stage: the one-stage kernel
# (The global-workspace eigenvector kernel, from 2 749 rows on, is reached by no GPU test: tests/cxx/eig_dense_plan_test.cpp
# holds its threshold.)
@pytest.mark.parametrize("sizes,one_stage", [((405,), 0), ((729,), 0), ((1300, 2187), 0), ((405,), 1)])
def test_dense_path_reaches_every_kernel_plan(sizes, one_stage):
    """The assertions of test_batched_lower_eigens_large_agglomerates, on its matrices, with the dense path forced."""
    capi = _capi()
    cases = [_large_agglomerates()[n] for n in sizes]
    theta = 0.01
    old = capi.set_options(eig_dense_only=1, eig_dense_one_stage=one_stage)
    try:
        res = capi.lower_eigens_batched([L for L, _, _ in cases], [D for _, D, _ in cases], -1.0, theta)
    finally:
        capi.set_options(eig_dense_only=old.eig_dense_only, eig_dense_one_stage=old.eig_dense_one_stage)
    for (L, D, (wr, Xr)), (w, X) in zip(cases, res):
        assert len(w) == len(wr) and len(w) >= 1
        assert np.allclose(w, wr, rtol=0, atol=EIG_TOL)
        assert np.allclose(X.T @ (D[:, None] * X), np.eye(len(w)), atol=1e-10)
        R = L @ X - (D[:, None] * X) * w[None, :]
        assert np.abs(R).max() <= 1e-10 * max(1.0, np.abs(L).max())
        assert np.allclose(_proj(X, D), _proj(Xr, D), atol=PROJ_TOL)


def test_batched_eigens_degenerate_and_split():
    """Degenerate clusters (block-diagonal copies) and splitting tridiagonals."""
    capi, o = _capi(), _oracle()
    B = np.array([[2.0, -1, 0, -1], [-1, 2, -1, 0], [0, -1, 2, -1], [-1, 0, -1, 2]])
    L = np.kron(np.eye(3), B) + 1e-9 * np.eye(12)  # three identical blocks: 3-fold eigenvalues
    D = o.snd_D_from_dense(L)
    for theta in [1e-6, 0.6, 1.5]:
        (w, X), = capi.lower_eigens_batched([L], [D], -1.0, theta)
        wr, Xr = o.lower_eigens_dense(L, D, theta)
        assert len(w) == len(wr)
        assert np.allclose(w, wr, atol=EIG_TOL)
        assert np.allclose(_proj(X, D), _proj(Xr, D), atol=PROJ_TOL)
        assert np.allclose(X.T @ (D[:, None] * X), np.eye(len(w)), atol=1e-10)
    # nothing below theta -> the single smallest pair (atleast_one)
    L2 = np.diag([3.0, 2.0, 5.0]) + 0.1
    D2 = np.ones(3) * 0.5
    (w, X), = capi.lower_eigens_batched([L2], [D2], -1.0, 1e-3)
    wr, Xr = o.lower_eigens_dense(L2, D2, 1e-3)
    assert len(w) == 1 and np.allclose(w, wr, atol=1e-12)


def test_batched_eigens_many_identical_blocks():
    """An agglomerate made of 32 identical disconnected pieces (randomly permuted): 32-fold
    eigenvalues.  The tridiagonal decouples into blocks sharing their spectra; eigenvectors are
    computed block by block like dstebz + dstein do (one undivided inverse iteration loses
    directions of such a cluster)."""
    capi, o = _capi(), _oracle()
    rng = np.random.default_rng(11)
    Bk = np.array([[2.0, -1, 0, -1], [-1, 2, -1, 0], [0, -1, 2, -1], [-1, 0, -1, 2.0]]) + np.diag([0.0, 0.01, 0.02, 0.05])
    L = np.kron(np.eye(32), Bk)
    perm = rng.permutation(128)
    L = L[np.ix_(perm, perm)]
    D = o.snd_D_from_dense(L)
    for theta in (0.02, 0.6):
        (w, X), = capi.lower_eigens_batched([L], [D], -1.0, theta)
        wr, Xr = o.lower_eigens_dense(L, D, theta)
        assert len(w) == len(wr) and len(w) % 32 == 0
        assert np.allclose(w, wr, atol=EIG_TOL) and np.all(np.diff(w) >= -1e-14)
        assert np.allclose(X.T @ (D[:, None] * X), np.eye(len(w)), atol=1e-10)
        R = L @ X - (D[:, None] * X) * w[None, :]
        assert np.abs(R).max() <= 1e-10
        assert np.allclose(_proj(X, D), _proj(Xr, D), atol=PROJ_TOL)


def test_batched_eigens_banded_matrices_take_the_few_eigenpairs_path():
    """Banded agglomerate matrices (graph Laplacians of band graphs, half bandwidths 1 .. n - 1) through the
    banded Cholesky + shift-invert path: the band fits the LDS window (first batch: windows 68 / 80 / 128
    are picked by the widest band of a batch) or goes through HBM (second batch).  STRICT turns the silent
    dense fallback into an error, so this passes only on the path it names."""
    capi, o = _capi(), _oracle()
    rng = np.random.default_rng(23)

    def band_laplacian(n, bw):
        W = np.zeros((n, n))
        for d in range(1, bw + 1):
            w = rng.uniform(0.5, 1.5, size=n - d)
            W += np.diag(-w, d) + np.diag(-w, -d)
        L = W + np.diag(-W.sum(axis=1))
        return L + np.diag(1e-4 * rng.uniform(0.5, 1.0, size=n))     # SPD, one eigenvalue near zero

    old = capi.set_options(eig_strict=1)
    try:
        for shapes in ([(70, 1), (96, 5), (130, 17), (64, 40)], [(200, 52)], [(150, 60), (90, 3)], [(300, 100), (77, 2)],
                       [(300, 120), (257, 256), (80, 4)]):
            _check_banded_batch(capi, o, [band_laplacian(n, bw) for n, bw in shapes])
    finally:
        capi.set_options(eig_strict=old.eig_strict)


def _check_banded_batch(capi, o, mats):
    Ds = [o.snd_D_from_dense(L) for L in mats]
    theta = 2e-3
    res = capi.lower_eigens_batched(mats, Ds, -1.0, theta)
    for L, D, (w, X) in zip(mats, Ds, res):
        wr, Xr = o.lower_eigens_dense(L, D, theta)
        assert len(w) == len(wr) and 1 <= len(w) <= 6
        assert np.allclose(w, wr, atol=EIG_TOL)
        R = L @ X - (D[:, None] * X) * w[None, :]
        assert np.abs(R).max() <= 1e-10
        assert np.allclose(_proj(X, D), _proj(Xr, D), atol=PROJ_TOL)


def _band_laplacian_fast(rng, n, bw):
    """band_laplacian of the test above without its loop over the diagonals (a stream of its own: the cases above keep theirs)"""
    U = np.triu(rng.uniform(0.5, 1.5, size=(n, n)), 1)
    U -= np.triu(U, bw + 1)                      # distances 1 .. bw
    W = -(U + U.T)
    L = W + np.diag(-W.sum(axis=1))
    return L + np.diag(1e-4 * rng.uniform(0.5, 1.0, size=n))     # SPD, one eigenvalue near zero


# Batches that reach the plan values (csrc/eig_ss_plan.h) the batches above do not:
#   wide1024  two-panel walk (eig_outer_panels = 2) with 1 024-thread panels, min(800, 750 + 32) > 768; LDS solves with 512 threads
#   g4_512    blocked walk with G = 4 and 512-thread panels, min(500, 330 + 64) > 448
#   two_halves 64 matrices: with eig_outer_panels = 2 the two halves of the batch on two streams; band 120 > 112, so the in-place
#             inertia pass with save / restore runs on all 64
#   stream1024 the streaming solves with 1 024 threads: the window of 2 431 rows x 8 vectors (155 584 B) is over 150 KB
_PLAN_BATCHES = {
    "wide1024": [(800, 750)],
    "g4_512": [(500, 330), (90, 3)],
    "two_halves": [(130 + k % 5, 120) for k in range(64)],
    "stream1024": [(2400, 2399)],
}


@pytest.mark.parametrize("name,panels", [("wide1024", 2), ("wide1024", 4), ("wide1024", 8), ("g4_512", 4), ("two_halves", 2),
                                         ("two_halves", 8), ("stream1024", 8)])
def test_batched_eigens_banded_matrices_reach_every_kernel_plan(name, panels):
    """The strict test above (same body, oracle and tolerances) on the batches of _PLAN_BATCHES, under the factor walk that
    eig_outer_panels names."""
    capi, o = _capi(), _oracle()
    rng = np.random.default_rng(23)
    mats = [_band_laplacian_fast(rng, n, bw) for n, bw in _PLAN_BATCHES[name]]
    old = capi.set_options(eig_strict=1, eig_outer_panels=panels)
    try:
        _check_banded_batch(capi, o, mats)
    finally:
        capi.set_options(eig_strict=old.eig_strict, eig_outer_panels=old.eig_outer_panels)


@pytest.mark.gpu
def test_wide_band_matrices_without_a_wanted_eigenvalue_keep_the_inertia_factor():
    """Wide-band matrices (the HBM path of the few-eigenpairs solver) whose spectrum lies entirely above theta:
    the certified count is 0, the inertia pass's L S L^T is the Cholesky factorisation of C - theta I and is
    kept (no second factorisation), the one pair the reference's "at least one" rule asks for is the smallest
    (amg/src/spectral.cpp:124-237).  Mixed with matrices that do have a wanted pair, so that the second
    factorisation runs on a part of the batch only.  Strict mode: no dense fallback."""
    capi, o = _capi(), _oracle()
    rng = np.random.default_rng(5)

    def band_matrix(n, bw, lift):
        W = np.zeros((n, n))
        for d in range(1, bw + 1):
            w = rng.uniform(0.5, 1.5, size=n - d)
            W += np.diag(-w, d) + np.diag(-w, -d)
        L = W + np.diag(-W.sum(axis=1))
        return L + np.diag((lift * L.diagonal() if lift else 1e-4) * rng.uniform(0.5, 1.0, size=n))

    old = capi.set_options(eig_strict=1)
    try:
        for shapes in ([(300, 130, 0.05), (257, 256, 0.05), (80, 4, 0.05)],
                       [(300, 120, 0.05), (280, 140, 0.0), (90, 7, 0.05), (200, 150, 0.0)]):
            mats = [band_matrix(n, bw, lift) for n, bw, lift in shapes]
            Ds = [o.snd_D_from_dense(L) for L in mats]
            theta = 2e-3
            res = capi.lower_eigens_batched(mats, Ds, -1.0, theta)
            for (n, bw, lift), L, D, (w, X) in zip(shapes, mats, Ds, res):
                wr, Xr = o.lower_eigens_dense(L, D, theta)
                assert len(w) == len(wr) == 1
                assert (w[0] > theta) == bool(lift)
                assert np.allclose(w, wr, rtol=1e-10, atol=EIG_TOL)
                R = L @ X - (D[:, None] * X) * w[None, :]
                assert np.abs(R).max() <= 1e-10
                assert np.allclose(_proj(X, D), _proj(Xr, D), atol=PROJ_TOL)
    finally:
        capi.set_options(eig_strict=old.eig_strict)


def _range_projection(P, probe):
    """Orthogonal projection of `probe` onto range(P) (basis independent)."""
    G = (P.T @ P).toarray()
    return P @ np.linalg.solve(G, P.T @ probe)


def _compare_level(h, H, lev, theta, strict=True, degenerate=False):
    """Compare one level of the HIP hierarchy `h` with the oracle hierarchy `H`.

    On level 0 everything is compared.  On coarser levels the coarse *basis* is only
    defined up to the sign of each column (and a rotation inside degenerate eigenspaces,
    `strict=False`), so vectors are compared through basis-independent quantities."""
    olv = H.levels[lev]
    rel = olv.rel
    info = h.level_info(lev)
    assert info["n"] == olv.A.shape[0]
    assert info["nparts"] == rel.nparts
    # --- integer topology: bit exact ---
    for name, T in [("AE_to_dof", rel.AE_to_dof), ("dof_to_AE", rel.dof_to_AE),
                    ("mis_to_dof", rel.mis_to_dof), ("mis_to_AE", rel.mis_to_AE),
                    ("AE_to_mis", rel.AE_to_mis), ("elem_to_dof", rel.elem_to_dof)]:
        I, J = h.get_table(lev, name)
        assert np.array_equal(I, T.I), name
        if lev > 0 and name in ("AE_to_dof", "elem_to_dof"):
            # On coarse levels the *order* inside these rows follows the numerically non-zero
            # pattern of P_tent (amg/src/contrib.cpp:186-187), i.e. LAPACK round-off on rows
            # that are zero in exact arithmetic; membership is what is pinned.
            for i in range(len(I) - 1):
                assert np.array_equal(np.sort(J[I[i]:I[i + 1]]), np.sort(T.J[T.I[i]:T.I[i + 1]])), name
        else:
            assert np.array_equal(J, T.J), name
    mises, k, ncols, flags = h.get_mis(lev)
    assert np.array_equal(mises, rel.mises)
    assert np.array_equal(flags.astype(np.int64) & 3, rel.agg_flags & 3)
    # --- coarse-space dimensions: bit exact ---
    assert np.array_equal(k, olv.mis_numcoarsedof)
    assert info["ncoarse"] == olv.P.shape[1]
    # --- local spectral problems ---
    m, ev, X, Ds = h.get_ae_eigens(lev)
    for i in range(rel.nparts):
        assert m[i] == olv.evects[i].shape[1]
        if lev == 0 or strict:
            assert np.allclose(Ds[i], olv.Ds[i], rtol=1e-12)
            assert np.allclose(ev[i], olv.evals[i][:len(ev[i])], atol=EIG_TOL)
        if lev == 0:
            assert np.allclose(_proj(X[i], Ds[i]), _proj(olv.evects[i], olv.Ds[i]), atol=PROJ_TOL)
    # --- per-MIS singular values and column spaces ---
    off, sig, U = h.get_mis_svd(lev)
    uo = 0
    for mis in range(rel.num_mises):
        r = rel.mis_to_dof.row_size(mis)
        kk = int(k[mis])
        Um = U[uo:uo + r * kk].reshape(kk, r).T
        uo += r * kk
        Uo = olv.mis_tent_interps[mis]
        assert Uo.shape == (r, kk)
        if kk:
            assert np.allclose(Um.T @ Um, np.eye(kk), atol=1e-11)
            if lev == 0:
                assert np.allclose(Um @ (Um.T @ np.ones(r)), Uo @ (Uo.T @ np.ones(r)), atol=1e-9)
        s_or = olv.mis_svals[mis]
        if s_or is not None and r > 1 and (lev == 0 or strict) and not degenerate:
            s_gpu = sig[off[mis]:off[mis] + len(s_or)]
            assert np.allclose(s_gpu, s_or, atol=1e-10)
    # --- prolongator / coarse operator ---
    P = h.get_csr(lev, "P")
    R = h.get_csr(lev, "R")
    Ac = h.get_csr(lev, "Ac")
    assert abs(P - R.T).max() == 0.0
    A = h.get_csr(lev, "A")
    Ac_ref = (P.T @ A @ P).toarray()
    assert np.allclose(Ac.toarray(), Ac_ref, rtol=0, atol=1e-12 * np.abs(Ac_ref).max())
    # range of the composite prolongator down to this level, in fine-level coordinates
    Pc_gpu, Pc_or = P, olv.P
    for l2 in range(lev - 1, -1, -1):
        Pc_gpu = h.get_csr(l2, "P") @ Pc_gpu
        Pc_or = H.levels[l2].P @ Pc_or
    probe = np.sin(np.arange(Pc_gpu.shape[0]) * 0.37)
    tol = 1e-8 if (lev == 0 or strict) else 1e-6
    assert np.allclose(_range_projection(sp.csr_matrix(Pc_gpu), probe),
                       _range_projection(sp.csr_matrix(Pc_or), probe), atol=tol)


def _build_pair(prob, ncoars, theta=0.003, testmesh=False, nu_relax=3):
    capi, o = _capi(), _oracle()
    params = capi.default_params(num_coarsenings=ncoars, theta=theta, nu_relax=nu_relax,
                                 testmesh=testmesh, keep_debug=True, coarse_rtol=1e-28)
    h = capi.Hierarchy.from_problem(prob, params)
    H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr,
                          prob.partitions[:ncoars], theta=theta, nu_relax=nu_relax, testmesh=testmesh)
    return h, H


@pytest.mark.parametrize("order,levels", [(1, 2), (1, 3), (2, 2)])
def test_mltest_fixture_matches_oracle(order, levels):
    """The reference's own ctest fixture (mltest / threelevel / mltest2)."""
    o = _oracle()
    prob = pr.mltest_problem(order=order, levels=levels)
    h, H = _build_pair(prob, levels - 1, testmesh=True)
    for lev in range(levels - 1):
        _compare_level(h, H, lev, 0.003)
    # V-cycle on a fixed right-hand side
    b = np.cos(np.arange(prob.ND) * 0.3) * (~prob.ess)
    x_gpu = h.vcycle(b)
    x_ref = o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= VCYCLE_TOL * np.linalg.norm(x_ref)
    # PCG with the reference driver's tolerance
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-6)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-6)
    assert conv and it == itr
    assert np.allclose(hist[:2], histr[:2], rtol=1e-9)
    assert np.linalg.norm(x - xr) <= 1e-9 * np.linalg.norm(xr)
    h.close()


def test_mltest_elasticity_fixture_matches_oracle():
    """The reference's ctest `elasticity` (amg/CMakeLists.txt:226-233): mltest.mesh, two
    displacement components, zero right-hand side, random start (3 iterations)."""
    o = _oracle()
    prob = pr.mltest_elasticity_problem()
    h, H = _build_pair(prob, 1, testmesh=True)
    _compare_level(h, H, 0, 0.003, strict=False, degenerate=True)
    x0 = np.random.default_rng(0).uniform(-1.0, 1.0, prob.ND)
    x, it, conv, hist = h.pcg(prob.b, x=x0.copy(), rel_tol=1e-6, zero_guess=False)
    xr, itr, convr, histr = o.solve(H, prob.b, x0=x0, rel_tol=1e-6)
    assert conv and convr and it == itr == 3
    assert np.allclose(hist, histr, rtol=1e-6)
    assert np.allclose(x, xr, atol=1e-9 * np.abs(x0).max())
    h.close()


@pytest.mark.parametrize("n,blk,cblk,K", [
    ((8, 8, 8), (4, 4, 2), None, (1, 1, 1)),
    ((8, 8, 8), (4, 4, 4), [(2, 2, 1)], (1, 1, 1)),
    ((12, 8, 4), (4, 4, 2), None, (1, 1, 1000.0)),
    # 64 eigenvectors on the interior AEs: wide MIS blocks (row-wise Jacobi SVD) and multi-pass RAP blocks
    ((16, 16, 16), (8, 8, 4), None, (1, 1.3, 1000.0001)),
])
def test_poisson3d_matches_oracle(n, blk, cblk, K):
    o = _oracle()
    prob = pr.poisson3d_problem(n, blk=blk, coarse_blk=cblk, K=K)
    ncoars = 1 + (len(cblk) if cblk else 0)
    theta = 0.003 if K[2] in (1, 1000.0001) else 0.02
    h, H = _build_pair(prob, ncoars, theta=theta)
    for lev in range(ncoars):
        _compare_level(h, H, lev, theta, strict=False)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu = h.vcycle(b)
    x_ref = o.vcycle(H, b)
    # degenerate eigenspaces (symmetric AEs) make the coarse *basis* non-unique; with two
    # levels the V-cycle is invariant to it, with three the level-1 smoother is not -- where there IS such a freedom.
    # The three-level row here, (8, 8, 8) / (4, 4, 4) / [(2, 2, 1)], has none: one vector per agglomerate on both levels, the
    # oracle with rotated eigenvectors and flipped MIS signs agrees with itself to 1e-16 (tests/test_conditional_cases.py), and
    # the library's V-cycle deviates by 5.4e-16 with 3 / 3 iterations (measured 2026-10-20).  So it carries VCYCLE_TOL and equal
    # iteration counts, not the 5e-2 / +-1 it had; the cases where the freedom is real are held level by level in
    # tests/test_gpu_conditional_parity.py.
    # The 64-vector case keeps singular directions down to 1e-10 sigma_0 on rank-deficient MIS
    # blocks; those directions are round-off (LAPACK's differs from ours), so the coarse spaces
    # agree only to ~1e-8 there.
    many = K[2] == 1000.0001
    tol = 1e-6 if many else VCYCLE_TOL
    dev = np.linalg.norm(x_gpu - x_ref) / np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    print("poisson %s / %s / %s: V-cycle deviation %.2e, iterations %d / %d" % (n, blk, cblk, dev, it, itr))
    assert dev <= tol
    assert conv and convr
    assert it == itr
    if ncoars == 1:
        assert np.allclose(hist, histr, rtol=1e-4 if many else 1e-7, atol=1e-10 * histr[0])
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


@pytest.mark.parametrize("n,blk,cblk", [
    ((16, 16, 8), (4, 4, 2), [(2, 2, 2)]),
    ((12, 12, 12), (4, 4, 4), [(3, 3, 3)]),
])
def test_poisson3d_three_level_without_symmetry_matches_oracle_tightly(n, blk, cblk):
    """The three-level cases above carry 5e-2 / +-1 iteration because a constant-coefficient box has symmetric
    agglomerates: repeated eigenvalues, a coarse BASIS that is not unique, and a level-1 smoother that is not invariant
    to it.  The same sizes with the 'skew' coefficient (no two elements alike, problems.py) have simple eigenvalues and
    leave no such freedom: every level's counts exactly, the V-cycle to VCYCLE_TOL, PCG with the same iteration count
    and history."""
    o = _oracle()
    prob = pr.poisson3d_problem(n, blk=blk, coarse_blk=cblk, coef="skew")
    h, H = _build_pair(prob, 2)
    for lev in range(2):
        _compare_level(h, H, lev, 0.003, strict=False)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu = h.vcycle(b)
    x_ref = o.vcycle(H, b)
    dev = np.linalg.norm(x_gpu - x_ref) / np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    rel = np.abs(np.asarray(hist[:len(histr)]) - histr) / histr if len(hist) == len(histr) else np.array([np.inf])
    print("three-level skew %s: V-cycle deviation %.2e, iterations %d / %d, history deviation %.2e" % (n, dev, it, itr, rel.max()))
    assert dev <= VCYCLE_TOL                 # (measured: 1e-14 .. 8e-14)
    assert conv and convr and it == itr
    assert rel.max() <= 1e-9                 # (measured: 3e-12)
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


@pytest.mark.parametrize("nwant", [13, 14])
def test_thirteen_and_fourteen_wanted_pairs_take_the_block_of_sixteen(nwant):
    """More wanted pairs than a block of eight reaches with one lock (twelve): the batch takes the block of SIXTEEN vectors
    (round 4: ss_rr_kernel<16> with its 16 x 16 Rayleigh-Ritz step, the triangular solves that stream the factor) instead of
    the dense path.  STRICT: any fallback is an error.  Matrices with exactly 13 / 14 small eigenvalues and a gap above them
    (weakly coupled band Laplacians, each with its own near-null vector), next to one with two and one with six wanted
    pairs; eigenvalues, residuals and D-orthogonal projectors against LAPACK (the oracle's lower_eigens_dense)."""
    capi, o = _capi(), _oracle()
    rng = np.random.default_rng(100 + nwant)

    def chain(ncomp, size, bw, lift, couple):
        n = ncomp * size
        L = np.zeros((n, n))
        for c in range(ncomp):
            W = np.zeros((size, size))
            for d in range(1, bw + 1):
                w = rng.uniform(0.5, 1.5, size=size - d)
                W += np.diag(-w, d) + np.diag(-w, -d)
            B = W + np.diag(-W.sum(axis=1))
            L[c * size:(c + 1) * size, c * size:(c + 1) * size] = B
        for c in range(ncomp - 1):          # a weak edge between neighbouring components (inside the band)
            i, j = (c + 1) * size - 1, (c + 1) * size
            L[i, i] += couple; L[j, j] += couple; L[i, j] -= couple; L[j, i] -= couple
        return L + np.diag(lift * rng.uniform(0.5, 1.0, size=n))
    mats = [chain(nwant, 40, 5, 1e-5, 1e-4), chain(2, 150, 7, 1e-5, 1e-4), chain(6, 60, 4, 1e-5, 1e-4)]
    Ds = [o.snd_D_from_dense(L) for L in mats]
    import scipy.linalg as sla
    w_all = sla.eigh(mats[0], np.diag(Ds[0]), eigvals_only=True)
    theta = float(np.sqrt(w_all[nwant - 1] * w_all[nwant]))          # inside the gap of the first matrix ...
    for L, D, k in zip(mats[1:], Ds[1:], (2, 6)):                    # ... and of the others
        w = sla.eigh(L, np.diag(D), eigvals_only=True)
        assert w[k - 1] < theta < w[k], (w[:k + 1], theta)
    old = capi.set_options(eig_strict=1, eig_min_n=0)
    try:
        res = capi.lower_eigens_batched(mats, Ds, -1.0, theta)
    finally:
        capi.set_options(eig_strict=old.eig_strict, eig_min_n=old.eig_min_n)
    for L, D, (w, X), k in zip(mats, Ds, res, (nwant, 2, 6)):
        wr, Xr = o.lower_eigens_dense(L, D, theta)
        assert len(w) == len(wr) == k
        assert np.allclose(w, wr, atol=EIG_TOL)
        R = L @ X - (D[:, None] * X) * w[None, :]
        assert np.abs(R).max() <= 1e-10
        assert np.allclose(_proj(X, D), _proj(Xr, D), atol=PROJ_TOL)


@pytest.mark.parametrize("theta,m_interior", [(0.06, 7), (0.08, 8)])
def test_more_wanted_pairs_than_the_block_holds_are_locked(theta, m_interior):
    """Agglomerates with seven to twelve wanted pairs (the reference's dsygvx has no such limit, src/xpacks.cpp:222-314):
    the few-eigenpairs path locks the first six when they have converged and goes on for the others on the same factor
    (csrc/eig2.hip: ss_lock_kernel, ss_deflate_kernel) instead of sending the agglomerate -- or, beyond a tenth of them,
    the whole chunk -- to the dense path.  STRICT: any fallback is an error.  The eight interior agglomerates of a
    32 x 32 x 16 mesh carry 7 (theta = 0.06) / 8 (0.08) pairs; counts, coarse dimension, iterations and history against
    the oracle.  (With theta = 0.12 they carry 13, but the window's end then sits in a dense part of the spectrum -- the 13th pair
    converges like 0.9^k even with sixteen vectors -- and the agglomerates rightly go to the dense path:
    test_thirteen_and_fourteen_wanted_pairs_take_the_block_of_sixteen uses matrices with a gap there.)"""
    capi, o = _capi(), _oracle()
    prob = pr.poisson3d_problem((32, 32, 16), blk=(8, 8, 4))
    old = capi.set_options(eig_strict=1)
    try:
        h, H = _build_pair(prob, 1, theta=theta)
    finally:
        capi.set_options(eig_strict=old.eig_strict)
    m, ev, X, Ds = h.get_ae_eigens(0)
    assert sorted(m.tolist())[-8:] == [m_interior] * 8 and max(m.tolist()) == m_interior
    # (a box of equal elements: repeated eigenvalues, so the eigenspaces are compared -- projectors -- and not the
    # singular values of the MIS blocks, which depend on the basis inside them)
    _compare_level(h, H, 0, theta, strict=False, degenerate=True)
    assert h.level_info(0)["ncoarse"] == H.levels[0].P.shape[1]
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and it == itr
    assert np.allclose(hist, histr, rtol=1e-9, atol=1e-12 * histr[0])
    h.close()


@pytest.mark.parametrize("levels", [2, 3])
def test_elasticity3d_matches_oracle(levels):
    """Vector dofs (3 per vertex, byVDIM, 24 x 24 element matrices): the six rigid-body modes
    are an exactly degenerate zero eigenvalue on every AE away from the clamped face, so the
    eigenvector *basis* (and with it the column normalisation before the SVD) is not unique;
    counts, spans and the preconditioned iteration are.  With three levels this test pins only what does not depend on
    that basis (ncoarse on level 1, the V-cycle to 5e-2, iterations +-1); level 1 itself -- D, eigenvalues, singular values,
    Ac, the cycle, at the level-0 tolerances -- is held in tests/test_gpu_conditional_parity.py (case q1_elasticity), where
    the oracle is given the library's own basis."""
    o = _oracle()
    cblk = [(2, 2, 1)] if levels == 3 else None
    prob = pr.elasticity3d_problem((8, 6, 4), blk=(4, 3, 2), coarse_blk=cblk)
    h, H = _build_pair(prob, levels - 1)
    _compare_level(h, H, 0, 0.003, strict=False, degenerate=True)
    m, ev, X, Ds = h.get_ae_eigens(0)
    assert sorted(m.tolist()) == [1, 1, 1, 1, 6, 6, 6, 6]
    if levels == 3:
        assert h.level_info(1)["ncoarse"] == H.levels[1].P.shape[1]
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu = h.vcycle(b)
    x_ref = o.vcycle(H, b)
    tol = 1e-8 if levels == 2 else 5e-2
    assert np.linalg.norm(x_gpu - x_ref) <= tol * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and abs(it - itr) <= (0 if levels == 2 else 1)
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


@pytest.mark.parametrize("n,blk", [((4, 2, 3), (2, 2, 3)), ((8, 4, 5), (4, 4, 5))])
def test_q2_elasticity3d_matches_oracle(n, blk):
    """BASELINE config 5's element type in small: 27-node hexes with 3 displacement components
    (81 x 81 element matrices), six rigid-body modes per free agglomerate.  First case: 525-dof
    agglomerates (band in LDS); second: config 5's agglomerate size class (4 x 4 x 5 elements, 2 673 dofs, half
    bandwidth in the hundreds: the factorisations, the inertia pass and the solves through HBM panels) against
    LAPACK's dsygvx on the same matrices.
    (2 x 3 / 4 x 5 elements across, so that the bending modes of the clamped agglomerate are not a
    degenerate pair of which "at least one" would pick an arbitrary member.)"""
    o = _oracle()
    prob = pr.elasticity3d_q2_problem(n, blk=blk)
    h, H = _build_pair(prob, 1)
    _compare_level(h, H, 0, 0.003, strict=False, degenerate=True)
    m, ev, X, Ds = h.get_ae_eigens(0)
    assert m.tolist() == [H.levels[0].evects[i].shape[1] for i in range(2)] and m[1] >= 6
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= 1e-8 * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and it == itr
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


def test_q2_elasticity3d_three_level_matches_oracle():
    """Config 5's agglomerate shape (4 x 4 x 4 Q2 elements, 2 187 dofs, six rigid-body modes) through TWO coarsenings:
    the wide-band eigen path on level 0, coarse element matrices P_loc^T A_e P_loc of 81-dof elements, a second
    spectral level.  Pinned against the oracle (LAPACK dsygvx / dgesvd on the same matrices): every level dimension,
    eigenvector count and coarse dof count per MIS exactly, the level-1 operator through its spectrum (1e-10).
    NOT pinned: anything that depends on the basis dgesvd returns inside a MIS with several coarse dofs.  The
    weighted-l1 diagonal D_ii = sum_j |a_ij| sqrt(a_ii / a_jj) of a coarse agglomerate matrix (src/mbox.cpp:913-949)
    is not invariant under a rotation of that basis, the six rigid-body modes give every MIS repeated singular
    values, so the level-1 eigenvalues of two correct implementations differ in the second digit (measured: 5.22e-4
    vs 5.27e-4) and with them the coarsest space; the iteration counts then agree to within a few.
    Where level 1 IS held: tests/test_gpu_conditional_parity.py (case q2_elasticity, the size of
    tests/test_oracle_mis_rotation.py) gives the oracle the library's own basis on every level and asks the level-0
    tolerances of the level-1 Ds, eigenvalues, singular values, Ac entries, V-cycle and PCG history."""
    o = _oracle()
    prob = pr.elasticity3d_q2_problem((8, 8, 4), blk=(4, 4, 4))
    nae = int(prob.partitions[0].max()) + 1
    assert nae == 4
    prob.partitions = [prob.partitions[0], np.array([0, 0, 1, 1], dtype=np.int32)]      # halves y < 1/2, y > 1/2
    h, H = _build_pair(prob, 2)
    for lev in range(2):
        info = h.level_info(lev)
        olv = H.levels[lev]
        assert info["n"] == olv.A.shape[0] and info["ncoarse"] == olv.P.shape[1], (lev, info["ncoarse"], olv.P.shape)
        mises, k, ncols, flags = h.get_mis(lev)
        assert np.array_equal(mises, olv.rel.mises) and np.array_equal(k, olv.mis_numcoarsedof), lev
        m, ev, X, Ds = h.get_ae_eigens(lev)
        assert m.tolist() == [olv.evects[i].shape[1] for i in range(olv.rel.nparts)], lev
    _compare_level(h, H, 0, 0.003, strict=False, degenerate=True)
    w_gpu = np.linalg.eigvalsh(h.get_csr(1, "A").toarray())
    w_ref = np.linalg.eigvalsh(H.levels[1].A.toarray())
    assert np.allclose(w_gpu, w_ref, rtol=0, atol=1e-10 * w_ref.max())
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and abs(it - itr) <= 3, (it, itr)
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


@pytest.mark.parametrize("nu_pro,levels", [(1, 2), (2, 2), (1, 3)])
def test_smoothed_prolongator_matches_oracle(nu_pro, levels):
    """P = prod_k (I - tau_k^-1 D^-1 A) P_tent (interp_smooth), R = P^T and
    Ac = R A P through the general sparse products (csrc/spgemm.hip)."""
    capi, o = _capi(), _oracle()
    cblk = [(2, 2, 2)] if levels == 3 else None
    prob = pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2), coarse_blk=cblk, coef="checkerboard")
    nco = levels - 1
    params = capi.default_params(num_coarsenings=nco, keep_debug=True, coarse_rtol=1e-28, nu_pro=nu_pro)
    h = capi.Hierarchy.from_problem(prob, params)
    H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:nco],
                          theta=0.003, nu_relax=3, nu_pro=nu_pro)
    for lev in range(nco):
        P, R, Ac, A = (h.get_csr(lev, w) for w in ("P", "R", "Ac", "A"))
        olv = H.levels[lev]
        assert P.shape == olv.P.shape and Ac.shape == olv.Ac.shape
        assert abs(P - R.T).max() == 0.0
        ref = (P.T @ A @ P).toarray()
        assert np.allclose(Ac.toarray(), ref, rtol=0, atol=1e-12 * np.abs(ref).max())
        assert P.nnz > h.level_info(lev)["n"]            # really smoothed: wider than the tentative one
    # level 0: same prolongator range as the oracle (columns are sign-ambiguous)
    probe = np.sin(np.arange(prob.ND) * 0.37)
    P0 = h.get_csr(0, "P")
    assert np.allclose(_range_projection(sp.csr_matrix(P0), probe),
                       _range_projection(sp.csr_matrix(H.levels[0].P), probe), atol=1e-8)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= (1e-9 if levels == 2 else 5e-2) * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and abs(it - itr) <= (0 if levels == 2 else 1)
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


def test_smooth_drop_tol_matches_oracle():
    """MultilevelParameters::smooth_drop_tol (AltThreshold, amg/src/interp.cpp:89-229): entries of the
    smoothed prolongator with |v| <= tol are dropped before R and Ac are formed."""
    capi, o = _capi(), _oracle()
    prob = pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2), coef="checkerboard")
    tol = 0.02
    params = capi.default_params(num_coarsenings=1, keep_debug=True, coarse_rtol=1e-28, nu_pro=1,
                                 smooth_drop_tol=tol)
    h = capi.Hierarchy.from_problem(prob, params)
    H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:1],
                          theta=0.003, nu_relax=3, nu_pro=1, smooth_drop_tol=tol)
    H0 = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:1],
                           theta=0.003, nu_relax=3, nu_pro=1)
    P, R, Ac, A = (h.get_csr(0, w) for w in ("P", "R", "Ac", "A"))
    Po = H.levels[0].P.copy()
    Po.sort_indices()
    assert Po.nnz < H0.levels[0].P.nnz                   # the tolerance really drops entries
    assert np.abs(P.data).min() > tol
    assert P.nnz == Po.nnz and np.array_equal(P.indptr, Po.indptr) and np.array_equal(P.indices, Po.indices)
    assert np.allclose(np.abs(P.data), np.abs(Po.data), atol=1e-10)      # columns are sign-ambiguous
    assert abs(P - R.T).max() == 0.0
    ref = (P.T @ A @ P).toarray()
    assert np.allclose(Ac.toarray(), ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= 1e-9 * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and it == itr
    h.close()


@pytest.mark.parametrize("levels,coef", [(2, None), (3, "checkerboard")])
def test_aggregates_with_arbitration_match_oracle(levels, coef):
    """`do_aggregates` -- on the last coarsening one aggregate per AE instead of
    the MISes, interface dofs distributed by Arbitrator::suggest (amg/src/aggregates.cpp:324-487,
    amg/src/arbitrator.cpp:93-204).  Integer tables bit-exact."""
    capi, o = _capi(), _oracle()
    cblk = [(2, 2, 2)] if levels == 3 else None
    prob = pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2), coarse_blk=cblk, coef=coef)
    nco = levels - 1
    params = capi.default_params(num_coarsenings=nco, keep_debug=True, coarse_rtol=1e-28, do_aggregates=True)
    h = capi.Hierarchy.from_problem(prob, params)
    H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:nco],
                          theta=0.003, nu_relax=3, do_aggregates=True)
    rel = H.levels[-1].rel
    assert rel.num_mises == rel.nparts and np.array_equal(rel.mis_to_AE.J, np.arange(rel.nparts))
    mises, k, ncols, flags = h.get_mis(nco - 1)
    if levels == 2:
        assert np.array_equal(mises, rel.mises)             # the arbitration itself
        _compare_level(h, H, 0, 0.003, strict=False)
    else:
        # On a coarse level the strengths |a_ij| / sqrt(a_ii a_jj) come from a Galerkin matrix whose
        # basis is sign/rotation-ambiguous and whose exactly tied connections are decided by
        # round-off: the greedy choice is only pinned up to those ties.  Every dof must sit in one
        # of its own AEs and the single-AE dofs in theirs.
        _compare_level(h, H, 0, 0.003, strict=False)
        I, J = h.get_table(nco - 1, "dof_to_AE")
        for d in range(len(mises)):
            assert mises[d] in J[I[d]:I[d + 1]]
        single = np.diff(I) == 1
        assert np.array_equal(mises[single], rel.mises[single])
        assert np.mean(mises == rel.mises) > 0.8
        assert h.level_info(nco - 1)["num_mises"] == rel.nparts
    H_mis = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:nco],
                              theta=0.003, nu_relax=3)
    assert H.levels[-1].Ac.shape[0] < H_mis.levels[-1].Ac.shape[0]     # fewer coarse dofs than with MISes
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= (1e-9 if levels == 2 else 0.2) * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and abs(it - itr) <= (0 if levels == 2 else 2)
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


@pytest.mark.parametrize("levels", [2, 3])
def test_corrected_nullspace_level_matches_oracle(levels):
    """CorrectNullspace (src/solve.cpp:52-164) = one more two-grid level on
    scaling_P under the coarsest spectral operator (the reference drivers' default)."""
    capi, o = _capi(), _oracle()
    cblk = [(2, 2, 2)] if levels == 3 else None
    prob = pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2), coarse_blk=cblk, coef="checkerboard")
    nco = levels - 1
    params = capi.default_params(num_coarsenings=nco, keep_debug=True, coarse_rtol=1e-28, correct_nullspace=True)
    h = capi.Hierarchy.from_problem(prob, params)
    H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:nco],
                          theta=0.003, nu_relax=3, correct_nullspace=True)
    assert h.num_levels == len(H.levels) + 1 == nco + 2
    lv = nco                                          # the extra level
    P, R, Ac, A = (h.get_csr(lv, w) for w in ("P", "R", "Ac", "A"))
    oP = H.levels[lv].P
    assert P.shape == oP.shape and abs(P - R.T).max() == 0.0
    # Two levels: the image of scaling_P on the fine level is the normalised projection of the
    # constants onto each MIS's span -- unique up to the sign of each column.  Deeper: the reference
    # projects the all-ones COEFFICIENT vector of the coarse level (src/contrib.cpp:657-659), which
    # depends on the arbitrary signs of that level's basis, so only structure is comparable.
    if levels == 2:
        Cg, Co = h.get_csr(0, "P") @ P, H.levels[0].P @ oP
        assert np.allclose(np.abs(Cg.toarray()), np.abs(Co.toarray()), atol=1e-8)
    assert np.array_equal(P.indices, oP.indices) and np.array_equal(P.indptr, oP.indptr)
    assert np.allclose(np.linalg.norm(P.toarray(), axis=0), 1.0, atol=1e-12)
    ref = (P.T @ A @ P).toarray()
    assert np.allclose(Ac.toarray(), ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= (1e-9 if levels == 2 else 2e-1) * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and abs(it - itr) <= (0 if levels == 2 else 2)
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


def _node_coords(n):
    nx, ny, nz = n
    iz, iy, ix = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    return np.stack([ix.ravel() / nx, iy.ravel() / ny, iz.ravel() / nz], axis=1)


@pytest.mark.parametrize("case", ["constants", "linears", "rigid_body_modes"])
def test_extra_coarse_space_modes_match_oracle(case):
    """ContribTent::ExtendWithPolynomials / ExtendWithRBMs (src/contrib.cpp:302-436): extra per-dof
    modes appended to every MIS block before the SVD."""
    capi, o = _capi(), _oracle()
    if case == "rigid_body_modes":
        n = (8, 6, 4)
        prob = pr.elasticity3d_problem(n, blk=(4, 3, 2))
        X = _node_coords(n)
        nn = X.shape[0]
        E = np.zeros((3 * nn, 6))
        for d in range(3):
            E[d::3, d] = 1.0                                   # translations
        E[0::3, 3], E[1::3, 3] = X[:, 1], -X[:, 0]              # rotations (Hughes p. 88, as the reference)
        E[1::3, 4], E[2::3, 4] = X[:, 2], -X[:, 1]
        E[0::3, 5], E[2::3, 5] = -X[:, 2], X[:, 0]
        theta = 1e-9                                           # spectral part: only the exact kernel
    else:
        n = (8, 8, 8)
        prob = pr.poisson3d_problem(n, blk=(4, 4, 2), coef="checkerboard")
        E = np.ones((prob.ND, 1)) if case == "constants" else np.concatenate([np.ones((prob.ND, 1)), _node_coords(n)], axis=1)
        theta = 0.003
    params = capi.default_params(num_coarsenings=1, theta=theta, keep_debug=True, coarse_rtol=1e-28, extra_modes=E)
    h = capi.Hierarchy.from_problem(prob, params)
    H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:1],
                          theta=theta, nu_relax=3, extra_modes=E)
    olv = H.levels[0]
    mises, k, ncols, flags = h.get_mis(0)
    assert np.array_equal(k, olv.mis_numcoarsedof)            # coarse-space dimensions: exact
    H0 = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:1],
                           theta=theta, nu_relax=3)
    assert olv.P.shape[1] > H0.levels[0].P.shape[1]           # the modes really enlarged the space
    probe = np.sin(np.arange(prob.ND) * 0.37)
    P = h.get_csr(0, "P")
    assert np.allclose(_range_projection(sp.csr_matrix(P), probe),
                       _range_projection(sp.csr_matrix(olv.P), probe), atol=1e-8)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= 1e-8 * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and it == itr
    h.close()


def _anisotropic_fixture():
    """amg/data/anisotropic.mat.00000 -- the matrix of the reference's `algebraic` ctest
    (amg/test/CMakeLists.txt:72-78) -- with dof 0 eliminated like test/algebraic/algebraic.cpp:229-246."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anisotropic_mat.npz"))
    A = sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=tuple(g["shape"]))
    return A[1:, 1:].tocsr()


@pytest.mark.parametrize("case", ["anisotropic_fixture", "poisson", "laplace2d_window"])
def test_algebraic_mode_matches_oracle(case):
    """element-free mode (ExtractSubMatrices, src/tg.cpp:579-672): elements =
    dofs, non-overlapping AEs, rowsum-free principal submatrices as local matrices; `_window`:
    the WindowSubMatrices variant (src/tg.cpp:741-858), A_TT + A_TX E."""
    capi, o = _capi(), _oracle()
    mode = "window" if case.endswith("_window") else True
    if case == "laplace2d_window":
        T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(24, 24))
        A = (sp.kron(sp.identity(24), T) + sp.kron(T, sp.identity(24))).tocsr()
        part = (np.arange(A.shape[0]) // 48).astype(np.int32)
        theta = 0.02
    elif case == "poisson":
        A = pr.poisson3d_problem((8, 8, 8), blk=(4, 4, 2)).A.tocsr()
        part = (np.arange(A.shape[0]) // 60).astype(np.int32)
        theta = 0.01
    else:
        A = _anisotropic_fixture()
        part = (np.arange(A.shape[0]) // 128).astype(np.int32)     # --elems-per-agg 128, contiguous instead of METIS
        theta = 0.01
    n = A.shape[0]
    b = np.ones(n)
    params = capi.default_params(num_coarsenings=1, theta=theta, keep_debug=True, coarse_rtol=1e-28, algebraic=mode)
    h = capi.Hierarchy.from_matrix(A, part, params)
    H = o.ml_produce_data(A, None, None, None, [part], theta=theta, nu_relax=3, algebraic=mode)
    olv = H.levels[0]
    m, ev, X, Ds = h.get_ae_eigens(0)
    assert [int(v) for v in m] == [e.shape[1] for e in olv.evects]
    for i in range(len(m)):
        assert np.allclose(Ds[i], olv.Ds[i], rtol=1e-12)
        assert np.allclose(ev[i], olv.evals[i][:len(ev[i])], atol=EIG_TOL)
    mises, k, ncols, flags = h.get_mis(0)
    assert np.array_equal(mises, olv.rel.mises) and np.array_equal(k, olv.mis_numcoarsedof)
    # per-AE coarse spaces (MIS == AE here).  On the fixture the first AEs are purely diagonal
    # (boundary rows): all eigenvalues equal 1, none below theta, and "the smallest" eigenvector is
    # an arbitrary member of a fully degenerate eigenspace -- LAPACK's pick and ours differ
    # legitimately, so only AEs whose selection is separated from the rest are compared.
    P, Po = h.get_csr(0, "P").toarray(), olv.P.toarray()
    off, compared = 0, 0
    for i in range(len(m)):
        kk = int(m[i])
        dofs = olv.rel.AE_to_dof.row(i)
        full = np.linalg.eigvalsh(olv.AEs_stiffm[i] / np.sqrt(np.outer(olv.Ds[i], olv.Ds[i])))
        separated = kk == len(full) or full[kk] - full[kk - 1] > 1e-6
        if separated:
            Qa = np.linalg.qr(P[np.ix_(dofs, range(off, off + kk))])[0]
            Qb = np.linalg.qr(Po[np.ix_(dofs, range(off, off + kk))])[0]
            assert np.linalg.norm(Qa - Qb @ (Qb.T @ Qa), 2) <= 1e-7, i
            compared += 1
        off += kk
    assert compared >= len(m) - 4
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    x, it, conv, hist = h.pcg(b, rel_tol=1e-6)
    xr, itr, convr, histr = o.solve(H, b, rel_tol=1e-6)
    assert conv and convr
    if compared == len(m):
        assert np.linalg.norm(x_gpu - x_ref) <= 1e-8 * np.linalg.norm(x_ref) and it == itr
    else:
        assert abs(it - itr) <= 3
    assert np.linalg.norm(A @ x - b) <= 1e-4 * np.linalg.norm(b)
    h.close()


def test_smoother_matches_oracle():
    o = _oracle()
    prob = pr.poisson3d_problem((6, 6, 6), blk=(3, 3, 3))
    h, H = _build_pair(prob, 1)
    rng = np.random.default_rng(3)
    b = rng.standard_normal(prob.ND)
    x0 = rng.standard_normal(prob.ND)
    x = h.smoother(0, b, x0.copy())
    lv = H.levels[0]
    xr = o.compute_poly(lv.A, b, x0.copy(), lv.roots, lv.Dinv_neg)
    assert np.linalg.norm(x - xr) <= 1e-13 * np.linalg.norm(xr)
    h.close()
