"""The solve phase at every smoother degree and every stopping rule of the outer PCG (cases and references:
tests/solve_cases.py, checked on the host by tests/test_solve_cases.py).

Every other test of the suite runs nu_relax = 3 on all levels, i.e. an SAS polynomial of the even degree 10, and stops PCG
by the squared relative rule.  Here:

  A  the smoother entry at nu = 1, 2, 3, 4 (degrees 4, 7, 10, 13) on level 0 of `tiles`, `skew2` and on both levels of
     `skew3`, against the polynomial in longdouble.  An odd degree ends smooth_inplace in its scratch vector (the vec_copy
     arm) and starts smooth_from_zero in x (the `cur = x` arm); the cycle's pre-smoother alone, through do-nothing plugs.
  B  one degree per level: V-cycle, stationary iteration and PCG against the oracle at the same degrees, the inner
     coarsest PCG under an odd-degree polynomial, update_operators, and the refusal of nu_relax = 0.
  C  the stopping rules of pcg_loop, each threshold derived from the oracle's history and a factor >= 10 from every entry.
  D  `hist` holds max_iter + 1 doubles and not one more.
  E  pcg, the stationary iteration, the smoother and update_operators on ONE hierarchy: the second pcg repeats the first
     bit for bit.

Hierarchies are built once per (problem, degrees) and closed when the module is done."""
import ctypes as C
import math

import numpy as np
import pytest

import solve_cases as sc

pytestmark = pytest.mark.gpu

VCYCLE_TOL = 1e-10      # tests/test_gpu_parity.py
HIST_RTOL = 1e-9        # test_poisson3d_three_level_without_symmetry_matches_oracle_tightly

_CACHE = {}


def _capi():
    from saamge_amd import capi
    return capi


def _oracle():
    from oracle import saamge_oracle as o
    return o


def _build(name, nus, **kw):
    capi = _capi()
    params = sc.params_with_degrees(nus, keep_debug=True, coarse_rtol=1e-28, **kw)
    h = capi.Hierarchy.from_problem(sc.problem(name), params)
    assert h.num_levels == len(nus) + 1
    return h


def _hier(name, nus, **kw):
    key = (name, tuple(nus), tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = _build(name, nus, **kw)
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _close_hierarchies():
    yield
    for h in _CACHE.values():
        h.close()
    _CACHE.clear()


def _level_operator(h, name, lev):
    """the device's own operator of the level (level 0: the caller's matrix, the same numbers) and the oracle's D^-1 of it"""
    o = _oracle()
    A = sc.problem(name).A.tocsr() if lev == 0 else h.get_csr(lev, "A").tocsr()
    return A, o.build_Dinv_neg(A)


def _check_smoother(h, name, lev, nu):
    o = _oracle()
    A, dinv = _level_operator(h, name, lev)
    assert A.shape[0] == h.level_info(lev)["n"]
    b, x0 = sc.smoother_data(A.shape[0])
    d = sc.smoother_twice(lambda bb, xx: h.smoother(lev, bb, xx), A, b, x0, o.sas_poly_roots(nu), dinv)
    print("smoother %s level %d degree %d: deviation from longdouble %.2e, %.2e" % (name, lev, 3 * nu + 1, d[0], d[1]))
    assert max(d) <= sc.SMOOTHER_TOL, (name, lev, nu, d)


# ---------------------------------------------------------------------------------------------------------------------
# A. the smoother at every degree parity, on every level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", sc.NUS)
@pytest.mark.parametrize("name", ["tiles", "skew2"])
def test_smoother_matches_longdouble_at_every_degree(name, nu):
    """smoother(0, b, x0) from a non-zero start, twice in a row, each application against poly_ld from the same start:
    || x - x_ld || <= 1e-13 || x_ld ||.  nu = 2 and 4 (degrees 7 and 13) take the vec_copy arm of smooth_inplace.
    (measured, degrees 4 / 7 / 10 / 13, the larger of the two applications: tiles 4.0e-16, 5.8e-16, 1.2e-15, 3.5e-15;
    skew2 3.7e-16, 7.9e-16, 2.3e-15, 6.8e-15 -- the float64 oracle's own distance from longdouble, tests/test_solve_cases.py)"""
    h = _hier(name, (nu,))
    fmt = h.level_format(0)
    if name == "tiles":      # ten staged tiles and the folded partial one, pair-coded slices
        assert fmt["slices"]["pair_coded"] > 0 and fmt["slices"]["offset_coded"] == 0 and fmt["staged_tiles"] == 10, fmt
    else:                    # offset-coded slices, nothing staged
        assert fmt["slices"]["offset_coded"] > 0 and fmt["slices"]["pair_coded"] == 0 and fmt["staged_tiles"] == 0, fmt
    _check_smoother(h, name, 0, nu)


@pytest.mark.parametrize("nu", sc.NUS)
@pytest.mark.parametrize("lev", [0, 1])
def test_smoother_matches_longdouble_on_both_levels_of_three(lev, nu):
    """the same on levels 0 (2 601 rows) and 1 (611 rows, the device's own Galerkin operator) of skew3 at nus = (nu, nu).
    (measured, degrees 4 / 7 / 10 / 13: level 0 3.9e-16, 8.8e-16, 2.4e-15, 7.1e-15; level 1 1.8e-16, 2.0e-16, 2.4e-16, 3.5e-16)"""
    h = _hier("skew3", (nu, nu))
    assert [h.level_info(l)["n"] for l in (0, 1)] == [2601, 611] and h.level_info(1)["ncoarse"] == 55
    _check_smoother(h, "skew3", lev, nu)


@pytest.mark.parametrize("nu", [2, 3])
def test_pre_smoother_from_zero_matches_longdouble(nu):
    """With a do-nothing post-smoother and a zero coarse solve plugged in, vcycle(b) is the pre-smoother from x = 0 alone:
    smooth_from_zero, which starts in x for the odd degree 7 (nu = 2) and in its scratch vector for the even degree 10.
    Against poly_ld(A, b, 0, ...) to 1e-13; the built-ins restored, the V-cycle is back to its bits (<= 1e-14).
    (measured: 4.1e-16 at nu = 2, 9.7e-16 at nu = 3; restored cycle 0.0)"""
    o = _oracle()
    h = _hier("tiles", (nu,))
    A, dinv = _level_operator(h, "tiles", 0)
    b, _ = sc.smoother_data(A.shape[0])
    x_builtin = h.vcycle(b)
    calls = []

    def identity(lev, bb, xx):
        calls.append("post")
        return xx

    def zero(rc):
        calls.append("coarse")
        return 0.0 * rc

    h.set_smoother(0, None, identity)
    h.set_coarse_solver(zero)
    try:
        x = h.vcycle(b)
    finally:
        h.set_smoother(0, None, None)
        h.set_coarse_solver(None)
    assert calls == ["coarse", "post"]
    dev = sc.rel_dev(x, sc.poly_ld(A, b, 0, o.sas_poly_roots(nu), dinv))
    back = np.linalg.norm(h.vcycle(b) - x_builtin) / np.linalg.norm(x_builtin)
    print("pre-smoother from zero, degree %d: deviation from longdouble %.2e; restored cycle %.1e" % (3 * nu + 1, dev, back))
    assert dev <= sc.SMOOTHER_TOL
    assert back <= 1e-14
    assert np.linalg.norm(x - x_builtin) > 1e-3 * np.linalg.norm(x_builtin)      # (the plugs were not ignored)


def test_the_degree_is_not_ignored():
    """nu = 2 and nu = 3 give smoother results more than 1e-3 apart (measured: 1.2e-1): none of the tests above would pass
    with the degree ignored"""
    b, x0 = sc.smoother_data(sc.ROWS["tiles"])
    x2 = _hier("tiles", (2,)).smoother(0, b, x0.copy())
    x3 = _hier("tiles", (3,)).smoother(0, b, x0.copy())
    dev = sc.rel_dev(x2, x3)
    print("smoother at nu = 2 against nu = 3: %.2e" % dev)
    assert dev > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# B. one degree per level
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_at(nus):
    return sc.oracle_with_degrees(sc.oracle_hierarchy("skew3"), nus)


def _hist_dev(hist, histr):
    if len(hist) != len(histr):
        return math.inf
    return float(np.max(np.abs(np.asarray(hist) - np.asarray(histr)) / np.asarray(histr)))


@pytest.mark.parametrize("nus,iters", [((3, 3), 4), ((2, 1), 4), ((1, 2), 5), ((4, 2), 3)])
def test_cycle_and_pcg_use_each_levels_own_degree(nus, iters):
    """V-cycle to VCYCLE_TOL = 1e-10 and PCG (rel_tol = 1e-8) with the oracle's iteration count and its history to 1e-9,
    the oracle smoothing level l at degree 3 nus[l] + 1.
    (measured at (3, 3), (2, 1), (1, 2), (4, 2): V-cycle 7.7e-14, 5.5e-14, 6.0e-13, 3.0e-14; history 3.3e-12, 5.6e-12, 2.1e-10,
    5.3e-12)"""
    o = _oracle()
    prob, h = sc.problem("skew3"), _hier("skew3", nus)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_ref = o.vcycle(_oracle_at(nus), b)
    dev = sc.rel_dev(h.vcycle(b), x_ref)
    xr, itr, convr, histr = o.solve(_oracle_at(nus), prob.b, rel_tol=1e-8)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    hd = _hist_dev(hist, histr)
    print("degrees %s: V-cycle deviation %.2e, iterations %d / %d, history deviation %.2e" % (nus, dev, it, itr, hd))
    assert dev <= VCYCLE_TOL
    assert conv and convr and it == itr == iters
    assert hd <= HIST_RTOL
    assert np.linalg.norm(x - xr) <= 1e-9 * np.linalg.norm(xr)
    # (swapped degrees are another cycle: the oracle at (1, 2) is not the oracle at (2, 1))
    if nus == (2, 1):
        assert sc.rel_dev(o.vcycle(_oracle_at((1, 2)), b), x_ref) > 1e-3


def test_stationary_iteration_with_a_degree_per_level():
    """vcycle_iterative(b, x0) at nus = (2, 1) against the oracle's, to 1e-10 (measured: 1.2e-11): level 0 smooths IN PLACE
    with the odd degree 7 on both sides of the coarse correction"""
    o = _oracle()
    prob, h = sc.problem("skew3"), _hier("skew3", (2, 1))
    x0 = np.random.default_rng(1).standard_normal(prob.ND)
    x0[prob.ess] = 0.0
    ref = o.vcycle_iterative(_oracle_at((2, 1)), prob.b, x0)
    dev = sc.rel_dev(h.vcycle_iterative(prob.b, x0.copy()), ref)
    print("stationary iteration at (2, 1): deviation %.2e" % dev)
    assert dev <= 1e-10


def test_inner_coarsest_pcg_under_an_odd_degree_polynomial():
    """nus = (3, 2): the inner PCG of the coarsest level (55 rows) is preconditioned by the LAST level's polynomial, degree
    7 -- smooth_from_zero's odd arm inside pcg_loop.  Its V-cycle agrees with the dense inverse's to 1e-10 (measured:
    1.7e-16, 12 inner iterations) and with the oracle's exact coarse solve to VCYCLE_TOL (measured: 7.7e-14)."""
    o = _oracle()
    prob = sc.problem("skew3")
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    out = {}
    for kind in (2, 1):
        h = _hier("skew3", (3, 2), coarse_solver=kind)
        assert h.coarse_solver_info()["kind"] == kind and h.coarse_solver_info()["n"] == 55
        out[kind] = (h.vcycle(b), h.level_info(0)["coarse_iters"])
    assert out[2][1] > 0 and out[1][1] == 0
    dev = sc.rel_dev(out[2][0], out[1][0])
    ref = sc.rel_dev(out[2][0], o.vcycle(_oracle_at((3, 2)), b))
    print("inner PCG (%d iterations) against the dense inverse: %.2e; against the oracle: %.2e" % (out[2][1], dev, ref))
    assert dev <= 1e-10
    assert ref <= VCYCLE_TOL


def test_update_operators_keeps_each_levels_degree():
    """update_operators(1.5 A) at nus = (2, 1): both levels still smooth with their own degree (7 and 4) on the updated
    operators, whose D^-1 is the old one divided by 1.5.  (measured: level 0 7.4e-16, level 1 2.0e-16)"""
    o = _oracle()
    prob = sc.problem("skew3")
    h = _build("skew3", (2, 1))
    try:
        A1_old = h.get_csr(1, "A").tocsr()
        h.update_operators(1.5 * prob.A.tocsr().data)
        A0 = prob.A.tocsr().copy()
        A0.data = 1.5 * A0.data
        A1 = h.get_csr(1, "A").tocsr()
        assert np.array_equal(A1.indices, A1_old.indices)
        assert np.allclose(A1.data, 1.5 * A1_old.data, rtol=1e-12, atol=1e-14 * np.abs(A1_old.data).max())
        assert np.allclose(o.build_Dinv_neg(A1), o.build_Dinv_neg(A1_old) / 1.5, rtol=1e-12)
        for lev, A, nu in ((0, A0, 2), (1, A1, 1)):
            dinv = o.build_Dinv_neg(A)
            b, x0 = sc.smoother_data(A.shape[0])
            d = sc.smoother_twice(lambda bb, xx: h.smoother(lev, bb, xx), A, b, x0, o.sas_poly_roots(nu), dinv)
            print("after update_operators, level %d degree %d: %.2e, %.2e" % (lev, 3 * nu + 1, d[0], d[1]))
            assert max(d) <= sc.SMOOTHER_TOL, (lev, d)
            # ... and not with the other level's degree
            other = sc.poly_ld(A, b, x0, o.sas_poly_roots(3 - nu), dinv)
            assert sc.rel_dev(h.smoother(lev, b, x0.copy()), other) > 1e-3
    finally:
        h.close()


def test_a_zero_degree_is_refused_and_the_next_build_works():
    capi = _capi()
    prob = sc.problem("skew3")
    with pytest.raises(RuntimeError, match="nu_relax must be positive"):
        capi.Hierarchy.from_problem(prob, sc.params_with_degrees((2, 0)))
    assert b"nu_relax must be positive" in capi.load().saamge_amd_last_error()
    h = _build("skew3", (2, 1))
    try:
        x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
        assert conv and it == 4
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. the stopping rules of the outer PCG
# ---------------------------------------------------------------------------------------------------------------------
def _pcg_pair(**kw):
    """(device result, oracle result) of the same PCG call on skew3 at PCG_NUS"""
    o = _oracle()
    prob, h = sc.problem("skew3"), _hier("skew3", sc.PCG_NUS)
    okw = dict(kw)
    b = okw.pop("b", prob.b)
    x0 = okw.pop("x0", None)
    ref = o.solve(_oracle_at(sc.PCG_NUS), b, x0=x0, **okw)
    got = h.pcg(b, x=None if x0 is None else x0.copy(), zero_guess=x0 is None, **okw)
    return got, ref


@pytest.mark.parametrize("rule", ["unsquared_rel", "abs_squared", "abs_unsquared"])
def test_pcg_stops_by_the_unsquared_rule_and_by_abs_tol(rule):
    """kalchev_pcg's rule (squared_tol = 0) with rel_tol between hist[2] / hist[0] and hist[3] / hist[0]: 3 iterations; an
    abs_tol between hist[1] and hist[2] that decides under either rule (rel_tol = 1e-30): 2 iterations.  Every threshold a
    factor >= 10 from every entry of the oracle's history (asserted; measured 51 and 77); count and `converged` as the
    oracle's, histories to 1e-9.  (measured: history deviation 8.8e-12, 3.1e-12, 3.1e-12)"""
    histr = sc.pcg_oracle_history()[3]
    case = sc.stopping_cases(histr)[rule]
    assert sc.separation(case["threshold"], histr) >= sc.SEPARATION
    (x, it, conv, hist), (xr, itr, convr, hr) = _pcg_pair(**case["kw"])
    hd = _hist_dev(hist, hr)
    print("%s: iterations %d / %d, history deviation %.2e" % (rule, it, itr, hd))
    assert it == itr == case["iters"] and conv and convr
    assert hd <= HIST_RTOL
    assert hist[-1] < case["threshold"] <= hist[-2]
    assert np.linalg.norm(x - xr) <= 1e-9 * np.linalg.norm(xr)


def test_pcg_leaves_by_max_iter():
    """max_iter = 2 at rel_tol = 1e-8 (the oracle needs 5): 2 iterations, not converged, three history entries as the
    oracle's first three to 1e-9, x the oracle's after two steps to 1e-9.  (measured: history 3.1e-12, x 4.9e-15)"""
    histr = sc.pcg_oracle_history()[3]
    assert sc.separation(sc.PCG_REL_TOL ** 2 * histr[0], histr[:3]) >= sc.SEPARATION
    (x, it, conv, hist), (xr, itr, convr, hr) = _pcg_pair(rel_tol=sc.PCG_REL_TOL, max_iter=2)
    assert itr == 2 and not convr and len(hr) == 3 and np.array_equal(hr, histr[:3])
    hd, xd = _hist_dev(hist, hr), sc.rel_dev(x, xr)
    print("max_iter = 2: iterations %d, converged %s, history deviation %.2e, x deviation %.2e" % (it, conv, hd, xd))
    assert it == 2 and conv is False
    assert len(hist) == 3 and hd <= HIST_RTOL
    assert xd <= 1e-9


def test_pcg_on_a_zero_right_hand_side():
    """zero guess: (B r0, r0) = 0 <= r0 = 0 -- the `nom0 <= r0` exit: no iteration, converged, hist[0] = 0, x exactly zero
    whatever the caller's x held.  Random start (zero_guess = 0, rel_tol = 1e-6 as the elasticity fixture): the oracle's
    count, history to 1e-6.  (measured: 4 iterations, history deviation 6.3e-12)"""
    prob, h = sc.problem("skew3"), _hier("skew3", sc.PCG_NUS)
    zero = np.zeros(prob.ND)
    x, it, conv, hist = h.pcg(zero, x=np.ones(prob.ND), rel_tol=sc.PCG_REL_TOL)
    assert it == 0 and conv and len(hist) == 1 and hist[0] == 0.0
    assert not np.any(x)
    x0 = np.random.default_rng(0).uniform(-1.0, 1.0, prob.ND)
    (x, it, conv, hist), (xr, itr, convr, hr) = _pcg_pair(b=zero, x0=x0, rel_tol=1e-6)
    assert sc.separation(1e-12 * hr[0], hr) >= sc.SEPARATION
    hd = _hist_dev(hist, hr)
    print("zero right-hand side, random start: iterations %d / %d, history deviation %.2e" % (it, itr, hd))
    assert conv and convr and it == itr
    assert hd <= 1e-6
    assert np.linalg.norm(x - xr) <= 1e-9 * np.abs(x0).max() * math.sqrt(prob.ND)


def test_pcg_ignores_the_callers_x_at_zero_guess_and_repeats_its_bits():
    """zero_guess = 1 with an x full of NaN: finite, and bit for bit the run from x = 0.  The same call twice gives the same
    bits in x and hist: the dot product is deterministic."""
    prob, h = sc.problem("skew3"), _hier("skew3", sc.PCG_NUS)
    runs = [h.pcg(prob.b, x=x, rel_tol=sc.PCG_REL_TOL)
            for x in (np.zeros(prob.ND), np.full(prob.ND, np.nan), np.zeros(prob.ND))]
    x, it, conv, hist = runs[0]
    assert conv and it == 5 and np.all(np.isfinite(x)) and np.any(x)
    for xn, itn, convn, histn in runs[1:]:
        assert np.all(np.isfinite(xn))
        assert itn == it and convn == conv and xn.tobytes() == x.tobytes() and histn.tobytes() == hist.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# D. hist holds max_iter + 1 doubles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [0, 1, 2])
def test_hist_gets_max_iter_plus_one_doubles_and_no_more(max_iter):
    """saamge_amd_pcg itself (the Hierarchy.pcg wrapper allocates one double more than the header asks for): hist of
    max_iter + 1 doubles and four guards behind them.  With max_iter = 0 the loop still takes its one step (MFEM's
    CGSolver::Mult, the oracle) but must not store hist[1]: the guards stay, iterations and `converged` are the oracle's,
    hist[:max_iter + 1] the oracle's to 1e-9."""
    o, capi = _oracle(), _capi()
    prob, h = sc.problem("tiles"), _hier("tiles", (3,))
    xr, itr, convr, histr = o.solve(sc.oracle_with_degrees(sc.oracle_hierarchy("tiles"), (3,)), prob.b, rel_tol=sc.PCG_REL_TOL, max_iter=max_iter)
    guard = -7.0
    hist = np.full(max_iter + 1 + 4, guard)
    b = np.ascontiguousarray(prob.b, dtype=np.float64)
    x = np.zeros(prob.ND)
    it, conv = C.c_int(-1), C.c_int(-1)
    capi._check(capi.load().saamge_amd_pcg(h.h, capi._ptr(b), capi._ptr(x), C.c_double(sc.PCG_REL_TOL), C.c_double(0.0),
                                           C.c_int(max_iter), C.c_int(1), C.c_int(1), C.byref(it), C.byref(conv), capi._ptr(hist)))
    print("max_iter = %d: iterations %d, converged %d, hist %s" % (max_iter, it.value, conv.value, hist))
    assert np.array_equal(hist[max_iter + 1:], [guard] * 4), hist
    assert it.value == itr == max_iter and bool(conv.value) == convr and not convr
    assert np.allclose(hist[:max_iter + 1], histr[:max_iter + 1], rtol=HIST_RTOL, atol=0.0)
    assert sc.rel_dev(x, xr) <= 1e-9      # (the one step at max_iter = 0 is taken, as in the oracle)


# ---------------------------------------------------------------------------------------------------------------------
# E. the calls of one hierarchy share its workspaces
# ---------------------------------------------------------------------------------------------------------------------
def test_calls_share_a_hierarchys_workspaces_without_disturbing_each_other():
    """skew2 with coarse_solver = 2, so that the inner PCG runs inside every V-cycle (its vectors, and its scalars beside the
    outer solve's): pcg -> x1; the stationary iteration (the outer PCG's r and z), the smoother on level 0 (its scratch
    vector), update_operators with the values unchanged (operator data and coarsest solver rebuilt); pcg again -> x2.
    x1 and x2, the two histories and the iteration counts are equal bit for bit."""
    prob = sc.problem("skew2")
    h = _build("skew2", (3,), coarse_solver=2)
    try:
        assert h.coarse_solver_info()["kind"] == 2
        x1, it1, conv1, hist1 = h.pcg(prob.b, rel_tol=sc.PCG_REL_TOL)
        assert conv1 and it1 > 0 and h.level_info(0)["coarse_iters"] > 0
        b, x0 = sc.smoother_data(prob.ND)
        assert np.all(np.isfinite(h.vcycle_iterative(prob.b, x0.copy())))
        assert np.all(np.isfinite(h.smoother(0, b, x0.copy())))
        h.update_operators(prob.A.tocsr().data.copy())
        x2, it2, conv2, hist2 = h.pcg(prob.b, rel_tol=sc.PCG_REL_TOL)
        print("pcg before / after: %d / %d iterations, %d history entries" % (it1, it2, len(hist1)))
        assert it2 == it1 and conv2 == conv1
        assert x2.tobytes() == x1.tobytes()
        assert hist2.tobytes() == hist1.tobytes()
    finally:
        h.close()
