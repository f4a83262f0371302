"""CPU checks of tests/conditional_cases.py, the cases and the comparison that tests/test_gpu_conditional_parity.py holds the
library to: the comparison run oracle against oracle (a stand-in implementation that rotates the eigenvectors inside equal
eigenvalues and flips the signs of the MIS basis columns), the preconditions under which the cases leave no freedom once the
basis is shared (the eigenvalue selection and the SVD cut), the regime that the cases at larger theta are there for,
mutations of the stand-in's derived data that the comparison must name, and the same mutations passing the loose criteria
that were all the suite had below level 0."""
import numpy as np
import pytest
import scipy.linalg as sla

import conditional_cases as cc
from saamge_amd import problems as pr

NOISE = 2e-15                 # the stand-in for round-off: relative, N(0, 1), on every injected entry
HARNESS_MARGIN = 1e-12        # what the comparison measures oracle against oracle stays below this ...
HARNESS_MARGIN_PCG = 1e-9     # ... and the PCG history below this (measured 6.8e-12 on mltest, whose last iterate sits near 1e-12 r0)
MIS_SENSITIVITY = 1e-11       # column space of a MIS under NOISE on the eigenvectors: two orders under PROJ_TOL
MUTATION_CASE = "q1_elasticity_interior"       # level 1: 8 agglomerates, six vectors on the free ones, MISes with several coarse dofs


def _numbers(levels, solves):
    """every measured deviation that is a floating-point number (not a count or a table flag): (level, name, value)"""
    skip = ("mises", "m", "k", "ones_column", "min_kept_sigma_ratio", "P")
    out = [(lev, n, v[0]) for lev, d in enumerate(levels) for n, v in d.items() if not n.startswith("table:") and n not in skip]
    return out + [(None, "vcycle", solves["vcycle"][0]), (None, "pcg_history", solves["pcg_history"][0])]


@pytest.mark.parametrize("name", list(cc.CASES))
def test_round_trip_oracle_against_oracle(name):
    """Run A is the stand-in (rotated, sign-flipped, with NOISE; everything downstream computed from those bases); run B the
    conditional oracle on A's view.  The whole comparison passes, bit-exact row orders and bit-identical P included, and what
    it measures stays below HARNESS_MARGIN: the harness does not itself eat the margin.  The stand-in is really another
    member of the family: against the UNCONDITIONED oracle its level-1 eigenvalues differ (elasticity cases)."""
    prob = cc.problem(name)
    H_A, view = cc.standin(name)
    H_B, recorded = cc.conditional_oracle(prob, cc.NCOARS, view, theta=cc.theta_of(name), testmesh=cc.uses_testmesh(name))
    levels, solves = cc.compare_conditional(prob, view, H_B, recorded)
    print(cc.format_measured(name, levels, solves))
    for lev, n, v in _numbers(levels, solves):
        assert v <= (HARNESS_MARGIN_PCG if n == "pcg_history" else HARNESS_MARGIN), (lev, n, v)
    assert all(d["P"][0] == 0.0 for d in levels)
    if name in cc.ELASTICITY:
        H0 = cc.plain_oracle(name)
        moved = max(np.abs(a[:1] - b[:1]).max() for a, b in zip(H_A.levels[1].evals, H0.levels[1].evals))
        print("%s: level-1 eigenvalues of the stand-in against the unconditioned oracle: %.1e" % (name, moved))
        assert moved > 1e-6


@pytest.mark.parametrize("name", list(cc.CASES))
def test_round_off_on_the_injected_bases_stays_orders_below_the_tolerances(name):
    """The conditional oracle fed the stand-in's bases times (1 + NOISE N(0, 1)): what a second implementation's round-off
    does to everything downstream.  Every deviation below HARNESS_MARGIN (the tolerances are 1e-12 ... 1e-9), the PCG history
    below HARNESS_MARGIN_PCG, and the column space of every MIS -- the oracle's own SVD of the noisy eigenvectors against the
    stand-in's basis, amplified by sigma_0 / sigma_k of the last kept direction (2e-5 on the mltest fixture: 1.4e-12) -- below
    MIS_SENSITIVITY on every level.
    (P is the noisy one here, so it is not compared.)"""
    prob = cc.problem(name)
    H_A, view = cc.standin(name)
    H_B, recorded = cc.conditional_oracle(prob, cc.NCOARS, view, theta=cc.theta_of(name), testmesh=cc.uses_testmesh(name),
                                          evect_noise=NOISE, basis_noise=NOISE, seed=2)
    levels, solves = cc.measure_conditional(prob, view, H_B, recorded)
    print(cc.format_measured(name + " (noise %g)" % NOISE, levels, solves))
    for lev, n, v in _numbers(levels, solves):
        if n != "colspace":          # (the amplified one: its own bound below)
            assert v <= (HARNESS_MARGIN_PCG if n == "pcg_history" else HARNESS_MARGIN), (lev, n, v)
    assert solves["pcg_iterations"][0] == 0
    for lev, d in enumerate(levels):
        assert d["colspace"][0] <= MIS_SENSITIVITY, (lev, d["colspace"], d["min_kept_sigma_ratio"])
        assert all(d["table:" + t][0] == 0 for t in cc.TABLES) and d["k"][0] == 0 and d["m"][0] == 0


def _selection_gaps(H, theta=cc.THETA):
    """per level: the smallest (lambda_first dropped - lambda_last kept) / max(theta, lambda_last kept) over the agglomerates,
    and whether a cluster of equal eigenvalues (1e-9) straddles the cut, from the FULL spectrum of every agglomerate"""
    out = []
    for lv in H.levels[:cc.NCOARS]:
        gap, cut = np.inf, []
        for i, (A, D) in enumerate(zip(lv.AEs_stiffm, lv.Ds)):
            lam = sla.eigh(A, np.diag(D), eigvals_only=True)
            m = max(1, int(np.sum(lam <= theta)))              # theta, or "at least one"
            spectral = lv.evects[i].shape[1] - (1 if lv.evects[i].shape[1] > len(lv.evals[i]) else 0)
            assert m == spectral, (i, m, spectral)
            if m < len(lam):
                gap = min(gap, (lam[m] - lam[m - 1]) / max(theta, lam[m - 1]))
                if abs(lam[m] - lam[m - 1]) < 1e-9:
                    cut.append(i)
        out.append((gap, cut))
    return out


@pytest.mark.parametrize("name", list(cc.CASES))
def test_preconditions_of_the_cases_on_the_oracle_alone(name):
    """What makes "given the basis, everything agrees" true: on every level and agglomerate the kept eigenvalues are separated
    from the first dropped one by >= 1e-6 max(theta, lambda_kept), and no cluster of equal eigenvalues is cut by theta or by "at
    least one" -- otherwise the COUNT or the span, not only the basis, would be an implementation's choice.  On the plain
    oracle and on the stand-in (whose level-1 matrices differ).  A case that fails is replaced, not excused."""
    for H in (cc.plain_oracle(name), cc.standin(name)[0]):
        for lev, (gap, cut) in enumerate(_selection_gaps(H, cc.theta_of(name))):
            assert not cut, (name, lev, cut)
            assert gap >= 1e-6, (name, lev, gap)


def test_the_preconditions_reject_cubic_agglomerates_on_the_clamped_face():
    """The precondition test is not vacuous: Q1 elasticity (8, 8, 8) / (2, 2, 2) -- the obvious third case -- has a degenerate pair
    of bending modes as the smallest eigenvalue of the clamped agglomerates, of which "at least one" keeps an arbitrary member
    (two correct implementations keep different vectors: measured on the device, projector deviation 0.41 with eigenvalues,
    residuals and counts all at 1e-15)."""
    o = cc._oracle()
    prob = pr.elasticity3d_problem((8, 8, 8), blk=(2, 2, 2))
    H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:1], theta=cc.THETA, nu_relax=3)
    gap, cut = _selection_gaps(H)[0]
    assert cut and gap < 1e-9


def _gathers(lv):
    """per MIS of a level that has an SVD (more than one dof, not all essential, a non-zero gather):
    (mis, rows, candidate columns, kept, singular values)"""
    rel, m = lv.rel, [z.shape[1] for z in lv.evects]
    rows = np.diff(rel.mis_to_dof.I)
    return [(i, int(rows[i]), sum(m[int(a)] for a in rel.mis_to_AE.row(i)), int(lv.mis_numcoarsedof[i]), lv.mis_svals[i])
            for i in range(rel.num_mises) if rows[i] > 1 and lv.mis_svals[i] is not None]


def _cut_margins(H):
    """over the MISes of all levels: the smallest kept sigma / sigma_0 and the largest dropped one (0 if no cut drops any)"""
    kept, dropped = np.inf, 0.0
    for lv in H.levels[:cc.NCOARS]:
        for mis, rows, cols, k, s in _gathers(lv):
            kept = min(kept, s[k - 1] / s[0])
            if k < len(s):
                dropped = max(dropped, s[k] / s[0])
    return kept, dropped


@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_svd_cut_leaves_no_choice(name):
    """The second place where a COUNT could be an implementation's choice: a MIS keeps the directions with
    sigma > 1e-10 sigma_0.  On every MIS of every level the last kept singular value is >= 1e-6 sigma_0 and the first dropped
    one <= 1e-12 sigma_0 (measured: >= 1.1e-5 and <= 1.5e-15, on pskew_t012 and el_t005), so round-off of either
    implementation, amplified or not, cannot move k.  On the plain oracle and on the stand-in."""
    for H in (cc.plain_oracle(name), cc.standin(name)[0]):
        kept, dropped = _cut_margins(H)
        print("%s: smallest kept sigma / sigma_0 %.1e, largest dropped %.1e" % (name, kept, dropped))
        assert kept >= 1e-6 and dropped <= 1e-12, (name, kept, dropped)


# What the cases at larger theta are FOR, per case: the eigenvectors per agglomerate (smallest, largest) on level 0 and on the
# plain oracle's level 1; the class every member's level 1 stays in (the stand-in's level 1 is another member of the family,
# whose counts differ by one or two on elasticity): its bounds are the eigensolver's own, csrc/eig_ss_plan.h -- up to six pairs
# for the block of eight, up to twelve with its lock, from fifteen on past every block -- and for the two largest cases from a
# quarter of the rows on; and whether level 1 holds a block of the Galerkin product over its LDS budget and a wide MIS of more
# than 64 rows.
REGIME = {
    "pskew_t012": ((4, 6), (6, 6), (1, 6), False),
    "el_t005": ((8, 8), (12, 12), (7, 12), False),              # every agglomerate within the lock path's twelve
    "el_t0057": ((10, 13), (22, 22), (15, 265), False),         # level 0: a batch whose largest want is 13, the block of sixteen
    "el_t006": ((10, 17), (29, 30), (15, 265), False),          # level 0: the lock path beside matrices no block holds
    "pskew_t025": ((40, 44), (175, 180), (120, 482), True),     # level 1: 175-180 pairs of 481-483 rows
    "el_t012": ((25, 39), (127, 129), (95, 379), True),         # level 1: 127-129 pairs of 380 rows
}
assert set(REGIME) == set(cc.LARGE_THETA)


@pytest.mark.parametrize("name", list(cc.LARGE_THETA))
def test_the_cases_at_larger_theta_are_in_the_regime_they_are_named_for(name):
    """Conditions on the inputs, so that a change of a problem generator cannot empty these cases silently: the range of
    eigenvectors per agglomerate on level 0 and (the plain oracle's) on level 1, the class of level 1 on any member, on level 0
    a wide MIS gather (more candidate columns than dofs: the row-wise Jacobi of mis_svd_kernel) and a MIS whose cut drops a
    direction, no block of the Galerkin product that rap_mis would refuse (rap_cases.lds_need), and for pskew_t025 and el_t012 a
    level-1 block that needs more LDS in one pass than rap_mis may take (the multi-pass path) and a wide level-1 MIS of more
    than 64 rows (more than one lane pass over V).  On the plain oracle and on the stand-in."""
    import rap_cases as rc
    range0, range1, class1, heavy = REGIME[name]
    for H in (cc.plain_oracle(name), cc.standin(name)[0]):
        m0, m1 = ([z.shape[1] for z in H.levels[lev].evects] for lev in range(2))
        assert (min(m0), max(m0)) == range0, (name, m0)
        assert class1[0] <= min(m1) and max(m1) <= class1[1], (name, m1)
        if H is cc.plain_oracle(name):
            assert (min(m1), max(m1)) == range1, (name, m1)
        g0, g1 = _gathers(H.levels[0]), _gathers(H.levels[1])
        assert any(cols > rows for mis, rows, cols, k, s in g0), name
        assert any(k < len(s) for mis, rows, cols, k, s in g0), name
        over = 0
        for lv in H.levels[:cc.NCOARS]:
            k = np.asarray(lv.mis_numcoarsedof)
            adj = rc.mis_adjacency(lv.A, lv.rel.mises, k)
            adj.eliminate_zeros()
            need, floor = rc.lds_need(adj, k)
            assert floor.max() <= rc.LDS_BUDGET, (name, floor.max())      # the library must not refuse
            over += int((need > rc.LDS_BUDGET).sum()) if lv is H.levels[1] else 0
        if heavy:
            assert over >= 1, name
            assert any(cols > rows > 64 for mis, rows, cols, k, s in g1), (name, [(rows, cols) for mis, rows, cols, k, s in g1])


@pytest.mark.parametrize("theta,vectors", [(0.15, (7, 8)), (0.19, (14, 14))])
def test_the_sensitivity_bound_rejects_the_skew_problem_between_its_two_cases(theta, vectors):
    """The obvious cases between pskew_t012 and pskew_t025: theta = 0.15 (7-8 vectors per fine agglomerate, the lock path) and
    0.19 (fourteen on every one: the block of sixteen).  Both pass every precondition -- selection gaps, the SVD cut -- but a
    level-0 MIS keeps a direction at 3e-6 sigma_0, and 2e-15 of noise on the injected eigenvectors moves that MIS's column
    space by 4.8e-11 / 3.0e-11: above MIS_SENSITIVITY.  Those regimes come from the elasticity problem instead (el_t005,
    el_t0057); the margin is not widened."""
    prob = cc._pskew()
    H_A = cc.standin_hierarchy(prob, theta=theta)
    m0 = [z.shape[1] for z in H_A.levels[0].evects]
    assert (min(m0), max(m0)) == vectors, m0
    for lev, (gap, cut) in enumerate(_selection_gaps(H_A, theta)):
        assert not cut and gap >= 1e-6, (lev, gap, cut)
    kept, dropped = _cut_margins(H_A)
    assert 1e-6 <= kept <= 1e-5 and dropped <= 1e-12, (kept, dropped)
    view = cc.oracle_view(H_A)
    H_B, recorded = cc.conditional_oracle(prob, cc.NCOARS, view, theta=theta, evect_noise=NOISE, basis_noise=NOISE, seed=2)
    moved = recorded[0]["colspace"][0]
    print("pskew theta %g: smallest kept sigma / sigma_0 %.1e, level-0 column space under the noise %.1e" % (theta, kept, moved))
    assert moved > MIS_SENSITIVITY


# ---------------------------------------------------------------------------------------------------------------------
# the comparison is not vacuous: mutations of the stand-in's DERIVED data (not its basis), each caught by name
# ---------------------------------------------------------------------------------------------------------------------
def _mutate_Ds(L):
    L.Ds[0][3] *= 1.0 + 1e-9


def _mutate_eigenvalue(L):
    L.evals[0][0] += 1e-9


def _mutate_Ac(L):
    L.Ac = L.Ac.copy()
    L.Ac.data[np.argmax(np.abs(L.Ac.data))] *= 1.0 + 1e-9


def _mutate_U(L):
    """one column of a MIS basis replaced by a unit vector 1e-6 outside the span (still orthogonal to the other columns)"""
    mis = next(i for i, U in enumerate(L.U) if 0 < U.shape[1] < U.shape[0])
    U = L.U[mis]
    w = np.cos(np.arange(U.shape[0]) * 1.3 + 0.2)
    w -= U @ (U.T @ w)
    w /= np.linalg.norm(w)
    u = U[:, 0] + 1e-6 * w
    U[:, 0] = u / np.linalg.norm(u)


def _mutate_elem_to_dof(L):
    I, J = L.tables["elem_to_dof"]
    row = next(i for i in range(len(I) - 1) if I[i + 1] - I[i] >= 2)
    J = J.copy()
    J[I[row]], J[I[row] + 1] = J[I[row] + 1], J[I[row]]
    L.tables["elem_to_dof"] = (I, J)


MUTATIONS = {"Ds": _mutate_Ds, "evals": _mutate_eigenvalue, "Ac": _mutate_Ac, "colspace": _mutate_U,
             "table:elem_to_dof": _mutate_elem_to_dof}


def _old_criteria_hold(prob, view, H_plain):
    """What tests/test_gpu_parity.py::test_elasticity3d_matches_oracle[3] asks of levels below 0: the level dimensions, the
    V-cycle to 5e-2, PCG iterations within one (against the UNCONDITIONED oracle)."""
    o = cc._oracle()
    dims = all(L.A.shape[0] == lv.A.shape[0] and L.P.shape[1] == lv.P.shape[1] for L, lv in zip(view.levels, H_plain.levels))
    b = cc.vcycle_rhs(prob)
    xv, xo = view.vcycle(b), o.vcycle(H_plain, b)
    x, it, conv, hist = view.pcg(prob.b, cc.PCG_REL_TOL)
    xr, itr, convr, histr = o.solve(H_plain, prob.b, rel_tol=cc.PCG_REL_TOL)
    return bool(dims and np.linalg.norm(xv - xo) <= 5e-2 * np.linalg.norm(xo) and conv and convr and abs(it - itr) <= 1)


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_a_mutation_of_level_1_is_caught_by_name(what):
    """1e-9 on one level-1 D entry, eigenvalue or Ac entry, 1e-6 out of the span on one level-1 MIS column, two swapped entries
    in one level-1 elem_to_dof row: compare_conditional fails and the FIRST quantity it names (the most upstream one) is the
    mutated one, on level 1.  The loose criteria pass every one of them."""
    prob = cc.problem(MUTATION_CASE)
    view = cc.standin(MUTATION_CASE)[1].mutated()
    MUTATIONS[what](view.levels[1])
    H_B, recorded = cc.conditional_oracle(prob, cc.NCOARS, view)
    with pytest.raises(cc.ConditionalMismatch) as err:
        cc.compare_conditional(prob, view, H_B, recorded)
    print(err.value)
    assert err.value.failures[0][:2] == (1, what), err.value.failures
    assert what in str(err.value)
    assert _old_criteria_hold(prob, view, cc.plain_oracle(MUTATION_CASE))


def test_a_wrong_level_1_agglomerate_matrix_passes_the_old_criteria_and_fails_the_new():
    """The gap, stated as a test.  A WRONG implementation: one diagonal entry of one level-1 agglomerate matrix off by 1e-3 --
    a wrong coarse element matrix entry -- with everything downstream (D, the level-1 eigenpairs, the coarsest space, the
    cycle) computed from it.  The criteria in force below level 0 before this module (dimensions, V-cycle 5e-2, iterations
    +-1) do not notice; the conditional comparison names Ds first, and the eigenvalues and the residual against the
    oracle's agglomerate matrix with it."""
    prob = cc.problem(MUTATION_CASE)

    def spoil(level, rel, stiff):
        if level == 1:
            stiff[0][2, 2] *= 1.0 + 1e-3

    H_W = cc.standin_hierarchy(prob, wrong_level_hook=spoil)
    view = cc.oracle_view(H_W)
    assert _old_criteria_hold(prob, view, cc.plain_oracle(MUTATION_CASE))
    H_B, recorded = cc.conditional_oracle(prob, cc.NCOARS, view)
    with pytest.raises(cc.ConditionalMismatch) as err:
        cc.compare_conditional(prob, view, H_B, recorded)
    print(err.value)
    named = [(lev, n) for lev, n, *_ in err.value.failures]
    assert named[0] == (1, "Ds") and (1, "evals") in named and (1, "resid") in named
    assert not any(lev == 0 for lev, n in named)
