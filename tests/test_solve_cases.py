"""CPU checks of tests/solve_cases.py, the cases and references that tests/test_gpu_solve_params.py holds the solve phase
to: the longdouble restatement of the polynomial smoother against the float64 oracle (and the room it leaves under the
device's tolerance), the degree helpers, and the distance of every PCG stopping threshold from the oracle's history."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import solve_cases as sc


def _oracle():
    from oracle import saamge_oracle as o
    return o


def _smoother_inputs():
    """(tag, A, Dinv_neg) of every operator part A smooths with: level 0 of the three problems, level 1 of skew3 (here the
    oracle's Galerkin operator; on the GPU the device's own, which _compare_level holds to it)"""
    out = []
    for name in ("tiles", "skew2", "skew3"):
        H = sc.oracle_hierarchy(name)
        out.append((name + "/0", H.levels[0].A, H.levels[0].Dinv_neg))
    lv = sc.oracle_hierarchy("skew3").levels[1]
    out.append(("skew3/1", lv.A, lv.Dinv_neg))
    return out


def test_the_problems_have_the_stated_sizes():
    o = _oracle()
    for name, n in sc.ROWS.items():
        prob, H = sc.problem(name), sc.oracle_hierarchy(name)
        assert prob.A.shape == (n, n) and len(H.levels) == sc.coarsenings(name)
        assert np.array_equal(H.levels[0].Dinv_neg, o.build_Dinv_neg(prob.A))
    H = sc.oracle_hierarchy("skew3")
    assert [lv.A.shape[0] for lv in H.levels] + [H.coarse_dense.shape[0]] == [2601, 611, 55]
    # ten whole tiles of 256 rows and a partial eleventh
    assert sc.ROWS["tiles"] // 256 == 10 and sc.ROWS["tiles"] % 256 != 0
    # (the slice formats these shapes are chosen for exist only on the device: the GPU tests assert them from level_format)


def test_the_degrees_cover_both_parities():
    o = _oracle()
    assert [len(o.sas_poly_roots(nu)) for nu in sc.NUS] == [4, 7, 10, 13]
    assert {len(o.sas_poly_roots(nu)) % 2 for nu in sc.NUS} == {0, 1}


def test_poly_ld_is_the_oracles_polynomial_and_leaves_room_under_the_tolerance():
    """compute_poly in float64 lies within HEADROOM_TOL = 1e-14 of poly_ld on every operator and degree of part A, for both
    of the two applications in a row: a factor 10 under the 1e-13 the device is held to is left for its summation order
    and FMAs.  No degree had to be dropped.
    (measured, largest of the two applications, degrees 4 / 7 / 10 / 13:
       tiles level 0    3.1e-16  5.2e-16  1.1e-15  3.5e-15
       skew2 level 0    2.9e-16  6.8e-16  2.4e-15  7.2e-15
       skew3 level 0    3.1e-16  7.3e-16  2.3e-15  6.9e-15
       skew3 level 1    2.5e-16  2.2e-16  2.9e-16  4.8e-16)"""
    o = _oracle()
    for tag, A, dinv in _smoother_inputs():
        b, x0 = sc.smoother_data(A.shape[0])
        row = []
        for nu in sc.NUS:
            roots = o.sas_poly_roots(nu)
            d = sc.smoother_twice(lambda bb, xx: o.compute_poly(A, bb, xx, roots, dinv), A, b, x0, roots, dinv)
            row.append(max(d))
            assert max(d) <= sc.HEADROOM_TOL, (tag, nu, d)
            assert min(d) > 0.0, (tag, nu)      # (longdouble does see what float64 rounds away)
        print("headroom %-8s degrees 4/7/10/13: %s" % (tag, "  ".join("%.1e" % v for v in row)))


def test_poly_ld_on_exact_data_and_from_a_zero_start():
    """integers and roots that are powers of two: every product and sum is exact in float64, so the two precisions agree
    to the last bit; a scalar 0 start is the zero vector"""
    o = _oracle()
    rng = np.random.default_rng(1)
    n = 40
    A = sp.diags([rng.integers(1, 5, n - 1), rng.integers(4, 9, n), rng.integers(1, 5, n - 1)], [-1, 0, 1], format="csr").astype(np.float64)
    b = rng.integers(-8, 9, n).astype(np.float64)
    x0 = rng.integers(-8, 9, n).astype(np.float64)
    dinv = -(2.0 ** -rng.integers(2, 5, n))
    roots = np.array([0.5, 0.25, 1.0])
    ref = o.compute_poly(A, b, x0.copy(), roots, dinv)
    got = sc.poly_ld(A, b, x0, roots, dinv)
    assert got.dtype == np.longdouble and np.array_equal(got, ref.astype(np.longdouble))
    assert np.array_equal(sc.poly_ld(A, b, 0, roots, dinv), sc.poly_ld(A, b, np.zeros(n), roots, dinv))
    # one step from zero is b / (tau d) with d = -1 / dinv
    assert np.array_equal(sc.poly_ld(A, b, 0, roots[:1], dinv), (-b * dinv / 0.5).astype(np.longdouble))
    # an empty row takes no sum
    E = sp.csr_matrix(([2.0], ([0], [0])), shape=(2, 2))
    assert np.array_equal(sc.poly_ld(E, np.array([1.0, 3.0]), 0, [1.0], np.array([-0.5, -0.5])), [0.5, 1.5])


def test_different_degrees_give_different_results():
    """what the GPU suite asserts of the device, here of the reference: the degree is not ignored"""
    o = _oracle()
    for tag, A, dinv in _smoother_inputs():
        b, x0 = sc.smoother_data(A.shape[0])
        x2, x3 = (sc.poly_ld(A, b, x0, o.sas_poly_roots(nu), dinv) for nu in (2, 3))
        assert sc.rel_dev(x2, x3) > 1e-3, tag


def test_oracle_with_degrees_sets_each_levels_roots_on_one_build():
    o = _oracle()
    H = sc.oracle_hierarchy("skew3")
    P0 = H.levels[0].P.copy()
    for nus in ((3, 3), (2, 1), (1, 2), (4, 2)):
        assert sc.oracle_with_degrees(H, nus) is H
        assert [len(lv.roots) for lv in H.levels] == [3 * nu + 1 for nu in nus]
        assert all(np.array_equal(lv.roots, o.sas_poly_roots(nu)) for lv, nu in zip(H.levels, nus))
    assert abs(H.levels[0].P - P0).max() == 0.0
    # the degree enters nothing in the oracle's setup: a build AT another degree gives the same operators
    prob = sc.problem("skew3")
    H2 = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:2], theta=sc.THETA, nu_relax=1)
    assert all(abs(a.P - c.P).max() == 0.0 and abs(a.Ac - c.Ac).max() == 0.0 for a, c in zip(H.levels, H2.levels))
    assert [len(lv.roots) for lv in H2.levels] == [4, 4]


def test_params_with_degrees_writes_one_value_per_level():
    from saamge_amd import capi
    p = sc.params_with_degrees((4, 2), keep_debug=True, coarse_rtol=1e-28, coarse_solver=2)
    assert p.num_coarsenings == 2 and p.keep_debug == 1 and p.coarse_rtol == 1e-28 and p.coarse_solver == 2
    assert list(p.nu_relax) == [4] + [2] * (capi.MAX_LEVELS - 1)
    assert list(sc.params_with_degrees((2,)).nu_relax) == [2] * capi.MAX_LEVELS
    assert list(sc.params_with_degrees((1, 0)).nu_relax)[:3] == [1, 0, 0]


def test_iteration_counts_of_the_degree_tuples():
    """part B's counts at rel_tol = 1e-8 (squared), from the oracle"""
    o = _oracle()
    H, prob = sc.oracle_hierarchy("skew3"), sc.problem("skew3")
    counts = []
    for nus in ((3, 3), (2, 1), (1, 2), (4, 2)):
        x, it, conv, hist = o.solve(sc.oracle_with_degrees(H, nus), prob.b, rel_tol=1e-8)
        assert conv
        counts.append(it)
    assert counts == [4, 4, 5, 3]


def test_stopping_thresholds_keep_their_distance_from_the_history():
    """Every threshold DERIVED from the oracle's history (unsquared rule, abs_tol in both rules) lies a factor >= 10 from
    every entry of it, so no count can flip on round-off; the oracle stops where the case says.
    (measured: unsquared 51, abs_tol 77 in both rules; consecutive entries are 2.5 to 4 orders apart.)
    The run all of them start from, rel_tol = 1e-8 squared, is set by the issue and not derived: its threshold 1e-16 hist[0]
    lies a factor 1.6 above the last entry and 530 below the one before (measured) -- less than 10, but the device's
    history is held to 1e-9 of the oracle's, which cannot move an entry across a gap of 1.6.  The max_iter = 2 run sees
    hist[:3] only, 2.7e9 away from that threshold."""
    o = _oracle()
    H, prob = sc.oracle_hierarchy("skew3"), sc.problem("skew3")
    xr, itr, convr, histr = sc.pcg_oracle_history()
    assert itr == 5 and convr and len(histr) == 6
    ratios = [histr[k] / histr[k + 1] for k in range(5)]
    assert min(ratios) > 100.0
    cases = sc.stopping_cases(histr)
    for name, c in cases.items():
        sep = sc.separation(c["threshold"], histr)
        print("%-14s threshold %.3e, stops at %d, factor to the nearest entry %.1f" % (name, c["threshold"], c["iters"], sep))
        x, it, conv, hist = o.solve(sc.oracle_with_degrees(H, sc.PCG_NUS), prob.b, **c["kw"])
        assert conv and it == c["iters"] and np.array_equal(hist, histr[:it + 1]), name
        assert hist[-1] < c["threshold"] <= hist[-2], name
        if name == "squared_rel":
            assert sep > 1.5
        else:
            assert sep >= sc.SEPARATION, (name, sep)
    assert sc.separation(cases["squared_rel"]["threshold"], histr[:3]) >= sc.SEPARATION
    # max_iter exit: two steps, not converged, three meaningful entries
    x, it, conv, hist = o.solve(sc.oracle_with_degrees(H, sc.PCG_NUS), prob.b, rel_tol=sc.PCG_REL_TOL, max_iter=2)
    assert it == 2 and not conv and np.array_equal(hist, histr[:3])


def test_zero_right_hand_side_in_the_oracle():
    """zero guess: (B r0, r0) = 0 <= 0, no step.  Random start at rel_tol = 1e-6 (the elasticity fixture's): the threshold
    1e-12 hist[0] lies a factor >= 10 from every entry (measured: 36)."""
    o = _oracle()
    H, prob = sc.oracle_with_degrees(sc.oracle_hierarchy("skew3"), sc.PCG_NUS), sc.problem("skew3")
    zero = np.zeros(prob.ND)
    x, it, conv, hist = o.solve(H, zero, rel_tol=sc.PCG_REL_TOL)
    assert it == 0 and conv and hist == [0.0] and not np.any(x)
    x0 = np.random.default_rng(0).uniform(-1.0, 1.0, prob.ND)
    x, it, conv, hist = o.solve(H, zero, x0=x0, rel_tol=1e-6)
    sep = sc.separation(1e-12 * hist[0], hist)
    print("zero rhs, random start: %d iterations, factor to the nearest entry %.1f" % (it, sep))
    assert conv and it == 4 and sep >= sc.SEPARATION
    assert np.linalg.norm(x) <= 1e-5 * np.linalg.norm(x0)


def test_hist_contract_cases_in_the_oracle():
    """part D on tiles: max_iter = 0 still takes one step (MFEM's control flow) and reports 0 iterations, not converged"""
    o = _oracle()
    H, prob = sc.oracle_with_degrees(sc.oracle_hierarchy("tiles"), (3,)), sc.problem("tiles")
    full = o.solve(H, prob.b, rel_tol=sc.PCG_REL_TOL)
    for max_iter in (0, 1, 2):
        x, it, conv, hist = o.solve(H, prob.b, rel_tol=sc.PCG_REL_TOL, max_iter=max_iter)
        assert it == max_iter and not conv
        assert len(hist) == max(max_iter, 1) + 1 and np.array_equal(hist, full[3][:len(hist)])
        assert np.any(x)
    assert full[1] > 2 and full[2]


def test_gmean_and_separation():
    assert sc.gmean(1e-4, 1e-8) == pytest.approx(1e-6)
    assert sc.separation(1e-6, [1.0, 1e-4, 1e-8, 0.0]) == pytest.approx(100.0)
    assert sc.separation(2.0, [1.0]) == 2.0 and sc.separation(1.0, [0.0]) == math.inf
