"""The block solve phase against the single-vector one, bit for bit per column: saamge_amd_smoother_block at every level,
saamge_amd_vcycle_block in both iterative modes and saamge_amd_pcg_block (iterations, flags and histories per column), over
both parities of the smoother's ping-pong, the three coarsest solvers, the plugs, k below, at and above the width of one
launch, and both leading dimensions.  No tolerance anywhere: np.array_equal / tobytes().  Cases: tests/cycle_block_cases.py."""
import numpy as np
import pytest

import cycle_block_cases as cb

pytestmark = pytest.mark.gpu


def _capi():
    from saamge_amd import capi
    return capi


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


class Singles(object):
    """what the single-vector calls return for each of the KMAX columns, computed once per hierarchy"""

    def __init__(self, h, name, pcg_kw):
        self.cols = cb.columns(name)
        self.n = self.cols.shape[1]
        self.levels = h.num_levels - 1
        rng = np.random.default_rng(41)
        self.start = rng.standard_normal((cb.KMAX, self.n))
        self.sm_in, self.sm = [], []
        for lev in range(self.levels):
            nl = int(h.level_info(lev)["n"])
            b, x0 = rng.standard_normal((cb.KMAX, nl)), rng.standard_normal((cb.KMAX, nl))
            self.sm_in.append((b, x0))
            self.sm.append(np.stack([h.smoother(lev, b[j].copy(), x0[j].copy()) for j in range(cb.KMAX)]))
        self.vc = np.stack([h.vcycle(self.cols[j].copy()) for j in range(cb.KMAX)])
        self.vi = np.stack([h.vcycle_iterative(self.cols[j].copy(), self.start[j].copy()) for j in range(cb.KMAX)])
        self.pcg = [h.pcg(self.cols[j].copy(), **pcg_kw) for j in range(cb.KMAX)]       # (x, iters, converged, hist[:iters + 1])


def _check_blocks(h, S, pcg_kw, ks=cb.KS, pads=(0, cb.LD_PAD)):
    n, max_iter = S.n, pcg_kw["max_iter"]
    for k in ks:
        for pad in pads:
            where = (k, pad)
            for lev in range(S.levels):
                b, x0 = S.sm_in[lev]
                nl = b.shape[1]
                B, X = cb.block(b, k, nl, pad), cb.block(x0, k, nl, pad)
                h.smoother_block(lev, B, X)
                assert _same(X[:, :nl], S.sm[lev][:k]), ("smoother", lev) + where
                assert np.all(np.isnan(X[:, nl:])) and _same(B[:, :nl], b[:k])
            B, X = cb.block(S.cols, k, n, pad), np.full((k, n + pad), np.nan)
            h.vcycle_block(B, X)
            assert _same(X[:, :n], S.vc[:k]), ("vcycle",) + where
            assert np.all(np.isnan(X[:, n:])) and _same(B[:, :n], S.cols[:k])
            X = cb.block(S.start, k, n, pad)
            h.vcycle_block(B, X, iterative_mode=True)
            assert _same(X[:, :n], S.vi[:k]), ("vcycle iterative",) + where
            assert np.all(np.isnan(X[:, n:]))
            X = np.full((k, n + pad), np.nan)
            X, iters, conv, hist = h.pcg_block(B, X, **pcg_kw)
            assert hist.shape == (k, max_iter + 1)
            for j in range(k):
                xs, its, cs, hs = S.pcg[j]
                assert _same(X[j, :n], xs), ("pcg x", j) + where
                assert int(iters[j]) == its and bool(conv[j]) == cs, ("pcg iters", j, int(iters[j]), its) + where
                assert _same(hist[j, :its + 1], hs), ("pcg hist", j) + where
                assert np.all(np.isnan(hist[j, its + 1:])), ("pcg hist past the column's last step", j) + where
            assert np.all(np.isnan(X[:, n:]))
            if k >= 2:
                assert len(set(int(i) for i in iters)) > 1, "every column left the loop at the same step"
            if k >= 5 and pcg_kw.get("abs_tol", 0.0) > 0.0:
                exits = [(int(i), bool(c)) for i, c in zip(iters, conv)]
                assert (max_iter, False) in exits and any(c and 0 < i < max_iter for i, c in exits), exits


@pytest.mark.parametrize("coarse", cb.COARSE)
@pytest.mark.parametrize("nu", cb.NUS)
@pytest.mark.parametrize("name", cb.HIERARCHIES)
def test_block_calls_equal_single_calls_per_column(name, nu, coarse):
    capi = _capi()
    h = capi.Hierarchy.from_problem(cb.problem(name), cb.params(name, nu, coarse))
    try:
        assert h.num_levels == cb.coarsenings(name) + 1
        kind = h.coarse_solver_info()["kind"]
        assert kind == coarse or (coarse == 3 and kind in (2, 3)), kind
        kw = dict(cb.PCG_KW, abs_tol=cb.ABS_TOL[name, nu], max_iter=cb.MAX_ITER)
        _check_blocks(h, Singles(h, name, kw), kw)
    finally:
        h.close()


def test_block_calls_equal_single_calls_on_the_dictionary_operator():
    """the two-level Q2-elasticity 10^3 hierarchy of tests/test_gpu_sell.py: the fine operator's SELL copy is the operator-level
    dictionary, which the block functions apply column by column"""
    capi = _capi()
    h = capi.Hierarchy.from_problem(cb.problem("q2"), cb.params("q2", 3, None))
    try:
        kw = dict(cb.PCG_KW, abs_tol=0.0, max_iter=cb.MAX_ITER)
        _check_blocks(h, Singles(h, "q2", kw), kw, ks=(1, 5, 11), pads=(cb.LD_PAD,))
    finally:
        h.close()


def test_plugs_are_called_once_per_column():
    """a caller's coarsest solver and smoother (host callbacks): block equals per column, and each callback ran k times"""
    capi = _capi()
    name = "tiles"
    prob = cb.problem(name)
    A = prob.A.tocsr()
    dinv = 0.6 / A.diagonal()
    h = capi.Hierarchy.from_problem(prob, cb.params(name, 1, 2))
    try:
        Ac = h.get_csr(0, "Ac").toarray()
        calls = {"coarse": 0, "pre": 0, "post": 0}

        def coarse(rc):
            calls["coarse"] += 1
            return np.linalg.solve(Ac, rc)

        def pre(level, b, x):
            calls["pre"] += 1
            assert not x.any()
            return x + dinv * (b - A @ x)

        def post(level, b, x):
            calls["post"] += 1
            return x + dinv * (b - A @ x)
        h.set_coarse_solver(coarse)
        h.set_smoother(0, pre, post)
        cols, n = cb.columns(name), A.shape[0]
        single = np.stack([h.vcycle(cols[j].copy()) for j in range(cb.KMAX)])
        for k in (2, 5, 11):
            before = dict(calls)
            X = np.full((k, n + cb.LD_PAD), np.nan)
            h.vcycle_block(cb.block(cols, k, n, cb.LD_PAD), X)
            assert _same(X[:, :n], single[:k]), k
            assert {c: calls[c] - before[c] for c in calls} == {"coarse": k, "pre": k, "post": k}
        h.set_smoother(0, None, None)
        h.set_coarse_solver(None)
    finally:
        h.close()


def test_refusals_name_the_argument_and_write_nothing():
    capi = _capi()
    name = "tiles"
    h = capi.Hierarchy.from_problem(cb.problem(name), cb.params(name, 1, 2))
    try:
        cols, n = cb.columns(name), cb.columns(name).shape[1]
        B = cb.block(cols, 3, n, 0)
        X = np.full((3, n), np.nan)
        iters, conv = np.full(3, -7, dtype=np.int32), np.full(3, -7, dtype=np.int32)
        hist = np.full((3, 4), np.nan)

        def calls(k, Bq, ldb, Xq, ldx):
            return [lambda: h.smoother_block(0, Bq, Xq, k=k, ldb=ldb, ldx=ldx),
                    lambda: h.vcycle_block(Bq, Xq, k=k, ldb=ldb, ldx=ldx),
                    lambda: h.vcycle_block(Bq, Xq, True, k=k, ldb=ldb, ldx=ldx),
                    lambda: h.pcg_block(Bq, Xq, max_iter=3, k=k, ldb=ldb, ldx=ldx, hist=hist, iters=iters, converged=conv),
                    lambda: capi.spmv_block(cb.problem(name).A, Bq, Xq, k=k, ldx=ldb, ldy=ldx)]
        big = np.full((4, 2 * n), np.nan)       # X inside the same array as B: overlapping ranges
        big[:3, :n] = cols[:3]
        overlap_x = big.ravel()[n:]              # starts inside B's first column stride
        cases = [("k must lie", 0, B, n, X, n), ("k must lie", 65, B, n, X, n), ("leading dimension", 3, B, n - 1, X, n),
                 ("leading dimension", 3, B, n, X, n - 1), ("null block", 3, None, n, X, n), ("null block", 3, B, n, None, n),
                 ("overlaps", 3, big, 2 * n, overlap_x, 2 * n)]
        for word, k, Bq, ldb, Xq, ldx in cases:
            for call in calls(k, Bq, ldb, Xq, ldx):
                with pytest.raises(RuntimeError) as e:
                    call()
                assert word in str(e.value), (word, str(e.value))
        assert np.all(np.isnan(X)) and np.all(np.isnan(hist)) and np.all(iters == -7) and np.all(conv == -7)
        assert _same(B, cb.block(cols, 3, n, 0)) and _same(big[:3, :n], cols[:3]) and np.all(np.isnan(big[:, n:]))
    finally:
        h.close()


def test_block_workspace_is_taken_on_the_first_block_call_and_returned_with_the_hierarchy():
    capi = _capi()
    name = "tiles"
    prob, cols = cb.problem(name), cb.columns(name)
    n = cols.shape[1]
    base = capi.memory_stats()[0]
    h = capi.Hierarchy.from_problem(prob, cb.params(name, 1, 2))
    h.vcycle(cols[1].copy())
    h.pcg(cols[1].copy(), max_iter=2)
    built = capi.memory_stats()[0]                          # the hierarchy and whatever its single-vector calls keep
    h.vcycle_block(cb.block(cols, 2, n, 0), np.zeros((2, n)))
    two = capi.memory_stats()[0]
    assert two > built
    h.vcycle_block(cb.block(cols, 2, n, 0), np.zeros((2, n)))
    h.vcycle_block(cb.block(cols, 1, n, 0), np.zeros((1, n)))
    assert capi.memory_stats()[0] == two                    # not grown by a call of the same or a smaller width
    h.vcycle_block(cb.block(cols, 11, n, 0), np.zeros((11, n)))
    eight = capi.memory_stats()[0]
    assert eight > two                                      # grown to the width of one launch ...
    h.vcycle_block(cb.block(cols, 9, n, 0), np.zeros((9, n)))
    assert capi.memory_stats()[0] == eight                  # ... and no further
    h.close()
    assert capi.memory_stats()[0] == base
    h2 = capi.Hierarchy.from_problem(prob, cb.params(name, 1, 2))
    h2.vcycle(cols[1].copy())
    h2.pcg(cols[1].copy(), max_iter=2)
    assert capi.memory_stats()[0] == built                 # a hierarchy that makes no block call holds what it held before
    h2.close()
    assert capi.memory_stats()[0] == base
