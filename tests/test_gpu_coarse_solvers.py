"""The coarsest-level direct solvers (explicit dense inverse, dense.hip; block-tridiagonal elimination, blocktri.hip) in
isolation, against a high-precision host solve.

Isolation through the ordinary ABI: a two-level hierarchy in the element-free mode with the tentative prolongator and
do-nothing smoothers plugged on level 0 makes saamge_amd_vcycle_mult compute x = P solve(R b) and nothing else.  P has
orthonormal columns (asserted), so solve(rc) = P^T x for rc = R b.  saamge_amd_coarse_solver_info tells which solver ran
and with which block structure; the structure must EQUAL that of the host model tests/coarse_cases.py::level_blocks.

What is judged, per case, solver kind (1 dense inverse, 3 block-tridiagonal) and right-hand side (a random vector, Ac times a
smooth vector, a unit vector in the last block):

    err = || xc - x_ref ||_inf / || x_ref ||_inf           bwd = || rc - Ac xc ||_inf / (|| Ac ||_inf || xc ||_inf + || rc ||_inf)

(residuals in extended precision; x_ref by coarse_cases.reference_solve, whose own residual is asserted to be 100 times
below what it judges) against the same two figures err_lu, bwd_lu of a plain fp64 sparse LU solve with ONE fp64 refinement
step -- the algorithmic shape of the code under test:

    err <= M max(err_lu, eps)          bwd <= M max(bwd_lu, eps)          eps = 2^-52

M allows for what the device does differently from pivoted LU: explicit inverses of up to nblk chained Schur complements,
FMA and matrix-core summation order, and the 2 - 3 eps of recovering xc = P^T x from x = P xc.

The only (case, kind) pair left out is (too_wide, 1): its operator has more rows than one dense inverse may have.
too_wide and semidefinite END in the inner PCG (asserted through the getter where it must happen); there the criterion
is the one of test_dense_and_iterative_coarsest_solvers_agree: 1e-9 with coarse_rtol = 1e-28.

MEASURED (MI355X), worst right-hand side of each row; kind = the kind asked for, nblk = 0 where no block structure is in use;
cond = || Ac ||_1 || Ac^-1 ||_1 (estimate); ratios against max(err_lu, eps) and max(bwd_lu, eps):

    case                     kind    n_c nblk     cond  err/err_lu  bwd/bwd_lu
    one_row                  1      1   0  1.0e+00     1.00     0.31
    one_row                  3      1   1  1.0e+00     1.00     0.31
    two_rows                 1      2   0  8.3e+00     1.67     0.24
    two_rows                 3      2   1  8.3e+00     1.67     0.24
    small_grid_255           1    255   0  1.9e+01     1.05     0.47
    small_grid_255           3    255   1  1.9e+01     1.05     0.47
    small_grid_256           1    256   0  2.2e+01     2.38     0.36
    small_grid_256           3    256   1  2.2e+01     2.38     0.36
    small_grid_257           1    257   0  2.2e+01     1.18     0.47
    small_grid_257           3    257   1  2.2e+01     1.18     0.47
    small_grid_640           1    640   0  2.0e+01     1.50     0.67
    small_grid_640           3    640   2  2.0e+01     1.50     0.64
    dense_edges_63           1     63   0  2.4e+01     1.50     0.36
    dense_edges_63           3     63   1  2.4e+01     1.50     0.36
    dense_edges_64           1     64   0  2.6e+01     1.50     0.30
    dense_edges_64           3     64   1  2.6e+01     1.50     0.30
    dense_edges_65           1     65   0  2.6e+01     1.00     0.34
    dense_edges_65           3     65   1  2.6e+01     1.00     0.34
    dense_edges_127          1    127   0  1.5e+01     1.60     0.43
    dense_edges_127          3    127   1  1.5e+01     1.60     0.43
    dense_edges_129          1    129   0  1.9e+01     1.13     0.44
    dense_edges_129          3    129   1  1.9e+01     1.13     0.44
    dense_edges_197          1    197   0  1.5e+01     1.60     0.41
    dense_edges_197          3    197   1  1.5e+01     1.60     0.41
    dense_edges_1000         1   1000   0  2.6e+01     1.71     0.61
    dense_edges_1000         3   1000   3  2.6e+01     1.44     0.50
    dense_edges_4097         1   4097   0  1.8e+01     1.19     0.59
    dense_edges_4097         3   4097  15  1.8e+01     1.19     0.60
    path                     1   3000   0  1.6e+01     1.45     0.52
    path                     3   3000  11  1.6e+01     1.45     0.51
    rod                      1   9600   0  2.7e+01     1.00     0.52
    rod                      3   9600  37  2.7e+01     1.00     0.50
    rod_stiff                1   9600   0  2.1e+06     1.04     0.71
    rod_stiff                3   9600  37  2.1e+06     0.68     0.72
    slab                     1  14400   0  4.4e+01     1.33     1.02
    slab                     3  14400  40  4.4e+01     1.59     0.91
    cube                     1  14976   0  4.0e+01     1.22     1.05
    cube                     3  14976  26  4.0e+01     1.22     0.88
    cube_stiff               1  14976   0  2.5e+06     1.71     1.07
    cube_stiff               3  14976  26  2.5e+06     2.10     1.12
    two_components           1   2200   0  3.3e+01     0.99     0.53
    two_components           3   2200   8  3.3e+01     0.82     0.57
    three_components_uneven  1   2205   0  3.5e+01     1.28     0.46
    three_components_uneven  3   2205   8  3.5e+01     1.28     0.40
    star                     1   1500   0  8.7e+03     5.91     1.06
    star                     3   1500   1  8.7e+03     5.91     1.06
    permuted_cube            1  14976   0  4.7e+01     1.11     0.79
    permuted_cube            3  14976  26  4.7e+01     1.33     0.87
    too_wide                 3  19608   0  5.2e+01    10.52    12.27
    updated                  3  14976  26  4.2e+01     1.24     0.79

M = 16: the next power of two above 4 x 2.38 (small_grid_256), the largest ratio among the well-conditioned variants
(shift 0.1, cond <= 100).  `star` has the well-conditioned shift but, through its hub row, cond 8.7e3; its 5.91 is within M
too, and so are the stiff variants rod_stiff and cube_stiff (cond 2e6, at most 2.10): no case needs a margin of its own.
too_wide is answered by the inner PCG (the refusal is asserted) and judged by the 1e-9 criterion, its ratios are listed for
completeness.  semidefinite: both direct requests end in the inner PCG (kind 2 reported), relative residual 6.3e-15.

Sensitivity, tried once with scratch builds: bt_schur_kernel's update scaled by 1 + 1e-6 fails 25 tests here (every kind-3
case with more than one block, well-conditioned ones included: small_grid_640, dense_edges_1000, dense_edges_4097, path, rod,
slab, cube, two_components, three_components_uneven, permuted_cube, updated); bt_couple_kernel ignoring the last row of a
block fails 22 (dense_edges_1000, dense_edges_4097, rod, slab, cube, the component cases, permuted_cube, updated, and the
comparison with the inner PCG).  With the first choice of the well-conditioned shift (1.0, cond ~ 5) the first defect
stayed below M on all of them but `updated`: the refinement step squares a factor's relative error times the strength of
the couplings, which is why the shift is 0.1.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import coarse_cases as cc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
THETA = 1e-6            # far below the second eigenvalue (>= 1/2) of every agglomerate's chain: one vector per agglomerate
M = 16.0                # next power of two above 4 x 2.38, the largest ratio of a well-conditioned case in the table
STIFF_MARGIN = {}       # case -> its own stated margin (none needed, see the docstring)
ITERATIVE_TOL = 1e-9    # where the inner PCG (coarse_rtol = 1e-28) must answer

CASES = cc.catalogue()
PAIRS = [(name, kind) for name in CASES for kind in (1, 3) if name not in ("semidefinite", "updated")]


def _capi():
    from saamge_amd import capi
    return capi


class Isolated(object):
    """A two-level hierarchy whose V-cycle is x = P solve(R b)"""

    def __init__(self, A, part, kind, plug=True):
        capi = _capi()
        params = capi.default_params(num_coarsenings=1, theta=THETA, nu_pro=0, coarse_solver=kind, coarse_rtol=1e-28,
                                     algebraic=True)
        self.h = capi.Hierarchy.from_matrix(A, part, params)
        self.calls = {"pre": 0, "post": 0}
        if plug:
            self.plug()
        self.fetch()

    def plug(self):
        def pre(level, b, x):
            self.calls["pre"] += 1
            assert not x.any()                       # a cycle from a zero start vector hands over x = 0
            return x

        def post(level, b, x):
            self.calls["post"] += 1
            return x
        self.h.set_smoother(0, pre, post)

    def fetch(self):
        h = self.h
        self.P, self.R, self.Ac = h.get_csr(0, "P").tocsr(), h.get_csr(0, "R").tocsr(), h.get_csr(0, "Ac").tocsr()
        self.Ac.sort_indices()
        self.info = h.coarse_solver_info()

    def solve(self, rc_target):
        """(rc, xc, x): b = P rc_target; rc = R b as the cycle sees it, evaluated in extended precision; xc = P^T x"""
        b = np.ascontiguousarray(self.P @ rc_target)
        before = dict(self.calls)
        x = self.h.vcycle(b)
        assert self.calls["pre"] == before["pre"] + 1 and self.calls["post"] == before["post"] + 1, \
            "the smoother plugs were not called: the cycle is not isolated"
        rc = cc.matvec_ext(self.R, b)
        # xc = (P^T P)^-1 P^T x; the columns of P have disjoint supports, so P^T P is diagonal (and I to round-off: _assert_shape)
        xc = cc.matvec_ext(self.R, x) / cc.matvec_ext(self.R, self.P @ np.ones(self.P.shape[1]))
        # x = P xc to round-off: nothing but the coarse correction is in x
        assert np.abs(x - self.P @ xc).max() <= 8 * EPS * max(np.abs(x).max(), np.finfo(float).tiny)
        return rc, xc, x

    def close(self):
        self.h.close()


def _assert_shape(name, case, iso, lb):
    """the preconditions of a case on the operator the library returned"""
    nc = case["graph"][0]
    Ac, P = iso.Ac, iso.P
    assert Ac.shape[0] == nc == iso.info["n"], "%s: %d coarse dofs for %d agglomerates -- not the intended case" % (name, Ac.shape[0], nc)
    assert abs(Ac - Ac.T).max() <= 4 * EPS * abs(Ac).max()
    G = (P.T @ P).tocsr()
    assert abs(G - sp.identity(nc)).max() <= 1e-11, "%s: P^T P differs from I by %.2e" % (name, abs(G - sp.identity(nc)).max())
    assert np.all(np.diff(P.indptr) == 1) and G.nnz == nc, "%s: the columns of P overlap" % name
    assert abs(iso.R - P.T).max() == 0.0
    assert cc.num_components(Ac) == case["components"], "%s: not the intended number of components" % name
    E = cc.expected_coarse_operator(case["graph"], case["shift"])
    if case["seed"] is None:
        assert np.array_equal(Ac.indptr, E.indptr) and np.array_equal(Ac.indices, E.indices), "%s: not the intended graph" % name
    cc.check_block_tridiagonal(Ac, lb)
    ex = case["expect"]
    for key in ("nblk", "max_block", "refused", "far_wins"):
        if key in ex:
            assert lb[key] == ex[key], "%s: the model gives %s = %s, the case is meant to have %s" % (name, key, lb[key], ex[key])
    if "min_levels" in ex:
        assert lb["nlev"] >= ex["min_levels"]


def _assert_info(name, kind, iso, lb):
    info, n = iso.info, iso.Ac.shape[0]
    if kind == 1:
        assert info["kind"] == 1, "%s: the dense inverse was asked for, kind %d is in use" % (name, info["kind"])
        assert (info["nblk"], info["max_block"], info["inverse_doubles"]) == (0, 0, n * n)
    elif lb["refused"]:
        assert info["kind"] == 2, "%s: the block limit must refuse this structure" % name
        assert (info["nblk"], info["max_block"], info["inverse_doubles"]) == (0, 0, 0)
    else:
        assert info["kind"] == 3, "%s: block-tridiagonal elimination was asked for, kind %d is in use" % (name, info["kind"])
        assert info["nblk"] == lb["nblk"] and info["max_block"] == lb["max_block"], (name, info, lb["nblk"], lb["max_block"])
        assert info["inverse_doubles"] == int(np.sum(np.diff(lb["off"]).astype(np.int64) ** 2))


_REF = {}
_REC = {}
ROWS = []


def _reference(name, Ac, lb):
    """per case: LU, condition estimate, right-hand sides; per right-hand side x_ref and the figures of the LU-shaped solve"""
    got = _REF.get(name)
    if got is not None and np.array_equal(got["Ac"].data, Ac.data) and np.array_equal(got["Ac"].indices, Ac.indices):
        return got
    lu = cc.factor(Ac)
    ref = {"Ac": Ac, "lu": lu, "cond": cc.cond_estimate(Ac, lu), "targets": cc.right_hand_sides(Ac, lb), "rhs": {}}
    _REF[name] = ref
    return ref


def _judge_reference(ref, rc):
    key = rc.tobytes()
    if key not in ref["rhs"]:
        Ac, lu = ref["Ac"], ref["lu"]
        head, tail, res = cc.reference_solve(Ac, rc, lu=lu)
        xl = cc.lu_shaped_solve(Ac, rc, lu=lu)
        ref["rhs"][key] = {"x_ref": head, "res": res, "err_lu": float(np.abs((xl - head) - tail).max() / np.abs(head).max()),
                           "bwd_lu": cc.backward_error(Ac, xl, rc)}
    return ref["rhs"][key]


def _run(name, kind):
    """build, assert the case's shape and the solver in use, solve the three right-hand sides; memoised"""
    if (name, kind) in _REC:
        return _REC[(name, kind)]
    case = CASES[name]
    A, part = cc.build(case)
    iso = Isolated(A, part, kind)
    try:
        lb = cc.level_blocks(iso.Ac)
        _assert_shape(name, case, iso, lb)
        _assert_info(name, kind, iso, lb)
        ref = _reference(name, iso.Ac, lb)
        rec = {"info": iso.info, "lb": lb, "ref": ref, "sol": {}, "Ac": iso.Ac}
        for rname, target in ref["targets"].items():
            rc, xc, _ = iso.solve(target)
            rec["sol"][rname] = (rc, xc)
            if iso.info["kind"] in (1, 3):
                assert iso.h.level_info(0)["coarse_iters"] == 0
            else:
                assert iso.h.level_info(0)["coarse_iters"] > 0
        # one more solve for linearity
        t = ref["targets"]
        rec["lin"] = iso.solve(0.7 * t["random"] - 1.3 * t["smooth"])[:2]
    finally:
        iso.close()
        _capi().release_cached_memory()
    _REC[(name, kind)] = rec
    return rec


def _margin(name):
    return STIFF_MARGIN.get(name, M)


def _check_solutions(name, kind, rec, margin):
    """item 2: forward and backward error of every right-hand side; returns the worst ratios"""
    ref, Ac = rec["ref"], rec["Ac"]
    worst = [0.0, 0.0]
    failures = []
    for rname, (rc, xc) in rec["sol"].items():
        j = _judge_reference(ref, rc)
        err = float(np.abs(xc - j["x_ref"]).max() / np.abs(j["x_ref"]).max())
        bwd = cc.backward_error(Ac, xc, rc)
        re, rb = err / max(j["err_lu"], EPS), bwd / max(j["bwd_lu"], EPS)
        worst = [max(worst[0], re), max(worst[1], rb)]
        print("RATIO %-24s kind %d %-9s n_c %6d nblk %3d cond %.1e  err %.2e err_lu %.2e ratio %8.2f   bwd %.2e bwd_lu %.2e ratio %8.2f"
              % (name, rec["info"]["kind"], rname, Ac.shape[0], rec["info"]["nblk"], ref["cond"], err, j["err_lu"], re, bwd, j["bwd_lu"], rb))
        if rec["info"]["kind"] == 2:
            if not (err <= ITERATIVE_TOL and np.abs(cc.residual_ext(Ac, xc, rc)).max() <= ITERATIVE_TOL * np.abs(rc).max()):
                failures.append((rname, "inner PCG", err))
            continue
        tol_f, tol_b = margin * max(j["err_lu"], EPS), margin * max(j["bwd_lu"], EPS)
        # the reference is two orders better than what it judges
        assert 100.0 * ref["cond"] * j["res"] <= tol_f and 100.0 * j["res"] <= tol_b, (name, rname, ref["cond"], j["res"])
        if not err <= tol_f:
            failures.append((rname, "forward error %.3e > %.3e" % (err, tol_f)))
        if not bwd <= tol_b:
            failures.append((rname, "backward error %.3e > %.3e" % (bwd, tol_b)))
    ROWS.append((name, kind, Ac.shape[0], rec["info"]["nblk"], ref["cond"], worst[0], worst[1]))
    return failures


@pytest.mark.parametrize("name,kind", PAIRS)
def test_coarsest_solve_against_the_reference(name, kind):
    """Items 1 - 3: the solver in use and its block structure as the model says, forward and backward error of three
    right-hand sides within M of an LU solve of the same shape, symmetry and linearity of the solve as an operator."""
    if kind == 1 and CASES[name]["graph"][0] > cc.DENSE_MAX:
        pytest.skip("%d rows: beyond one dense inverse (the only pair left out)" % CASES[name]["graph"][0])
    rec = _run(name, kind)
    margin = _margin(name)
    failures = _check_solutions(name, kind, rec, margin)
    assert not failures, (name, kind, failures)
    if rec["info"]["kind"] == 2 or CASES[name]["shift"] != cc.WELL:
        return
    # symmetry and linearity, well-conditioned variants: implied by the forward-error bounds of the solves involved (the
    # exact solve is symmetric and linear), so a violation means an error the three right-hand sides did not show
    ref = rec["ref"]
    (u, xu), (v, xv) = rec["sol"]["random"], rec["sol"]["smooth"]
    ju, jv = _judge_reference(ref, u), _judge_reference(ref, v)
    tu, tv = margin * max(ju["err_lu"], EPS), margin * max(jv["err_lu"], EPS)
    nu, nv = np.abs(ju["x_ref"]).max(), np.abs(jv["x_ref"]).max()
    sym = abs(float(np.dot(u.astype(np.longdouble), xv) - np.dot(v.astype(np.longdouble), xu)))
    assert sym <= np.abs(u).sum() * tv * nv + np.abs(v).sum() * tu * nu, (name, kind, sym)
    w, xw = rec["lin"]
    # (w = R P (0.7 u' - 1.3 v') differs from 0.7 u - 1.3 v by round-off of R and P: a few eps, times the norm of the inverse)
    lin = np.abs(xw - (0.7 * xu - 1.3 * xv)).max()
    assert lin <= 2.0 * (0.7 * tu * nu + 1.3 * tv * nv) + 16 * EPS * ref["cond"] * (0.7 * nu + 1.3 * nv), (name, kind, lin)


@pytest.mark.parametrize("name", [n for n in CASES if n not in ("semidefinite", "updated", "too_wide")])
def test_block_tridiagonal_and_dense_inverse_agree(name):
    """Item 4: the two direct solvers on the same inputs differ by no more than the forward-error bound allows each of them"""
    r1, r3 = _run(name, 1), _run(name, 3)
    assert r1["info"]["kind"] == 1 and r3["info"]["kind"] == 3
    assert np.array_equal(r1["Ac"].data, r3["Ac"].data)
    margin = _margin(name)
    for rname in r1["sol"]:
        (rc, x1), (rc3, x3) = r1["sol"][rname], r3["sol"][rname]
        assert np.array_equal(rc, rc3)
        j = _judge_reference(r1["ref"], rc)
        diff = float(np.abs(x1 - x3).max() / np.abs(j["x_ref"]).max())
        assert diff <= margin * max(j["err_lu"], EPS), (name, rname, diff, j["err_lu"])


def test_the_plugs_isolate_the_coarsest_solve():
    """Once, on the smallest case with more than one row: with the plugs in place x = P xc and both callbacks ran; without
    them the same call gives something else (so a plug that did nothing would be noticed)."""
    A, part = cc.build(CASES["two_rows"])
    iso = Isolated(A, part, 1)
    try:
        target = np.array([1.0, -2.0])
        rc, xc, x = iso.solve(target)
        assert iso.calls == {"pre": 1, "post": 1}
        exact = np.linalg.solve(iso.Ac.toarray(), rc)
        assert np.abs(xc - exact).max() <= 16 * EPS * np.abs(exact).max()
        b = np.ascontiguousarray(iso.P @ target)
        iso.h.set_smoother(0, None, None)
        x_full = iso.h.vcycle(b)
        assert iso.calls == {"pre": 1, "post": 1}
        assert np.abs(x_full - x).max() > 1e-3 * np.abs(x).max()
    finally:
        iso.close()


@pytest.mark.parametrize("kind", [1, 3])
def test_semidefinite_operator_is_refused_or_solved(kind):
    """A singular coarse operator (graph Laplacian, constants in the kernel of A and P^T 1 in that of Ac) and consistent
    right-hand sides.  Either the direct request ends in the inner PCG (a non-positive pivot), or the direct solver that
    stays in use meets the backward-error bound; a confident wrong answer is the defect."""
    name = "semidefinite"
    case = CASES[name]
    A, part = cc.build(case)
    iso = Isolated(A, part, kind)
    try:
        lb = cc.level_blocks(iso.Ac)
        _assert_shape(name, case, iso, lb)
        null = cc.matvec_ext(iso.P.T.tocsr(), np.ones(A.shape[0]))
        assert np.abs(iso.Ac @ null).max() <= 64 * EPS * cc.norm_inf_op(iso.Ac) * np.abs(null).max(), "Ac is not singular"
        used = iso.info["kind"]
        assert used in (2, kind)
        rng = np.random.default_rng(4)
        for y in (rng.standard_normal(iso.Ac.shape[0]), np.cos(np.arange(iso.Ac.shape[0]) * 0.01)):
            rc, xc, _ = iso.solve(iso.Ac @ y)
            r = np.abs(cc.residual_ext(iso.Ac, xc, rc)).max()
            bwd = cc.backward_error(iso.Ac, xc, rc)
            print("RATIO semidefinite requested %d in use %d: relative residual %.2e, backward error %.2e (%.1f eps)"
                  % (kind, used, r / np.abs(rc).max(), bwd, bwd / EPS))
            assert np.all(np.isfinite(xc))
            if used == 2:
                assert r <= ITERATIVE_TOL * np.abs(rc).max()
            else:
                assert bwd <= M * EPS, (kind, bwd)
    finally:
        iso.close()


def test_update_operators_sets_the_direct_solver_up_again():
    """`updated`: new matrix values through saamge_amd_update_operators2 with coarse_solver = 3 -- P is kept, Ac and the
    factorisation follow the new values."""
    name = "updated"
    case = CASES[name]
    A, part = cc.build(case)
    iso = Isolated(A, part, 1)
    try:
        assert iso.info["kind"] == 1
        P0 = iso.P.copy()
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        A2 = A.copy()            # same pattern, symmetric, three times as large, still strictly diagonally dominant
        A2.data = 3.0 * A.data * (1.0 + 0.04 * np.cos(rows + A.indices))        # (d = 1.1 off: 0.96 * 1.1 > 1.04)
        iso.h.update_operators(A2.data, coarse_solver=3)
        iso.fetch()
        assert abs(iso.P - P0).max() == 0.0
        want = (P0.T @ A2 @ P0).tocsr()
        assert abs(iso.Ac - want).max() <= 16 * EPS * abs(want).max()
        lb = cc.level_blocks(iso.Ac)
        _assert_shape(name, case, iso, lb)
        _assert_info(name, 3, iso, lb)
        ref = _reference(name, iso.Ac, lb)
        rec = {"info": iso.info, "lb": lb, "ref": ref, "sol": {}, "Ac": iso.Ac}
        for rname, target in ref["targets"].items():
            rc, xc, _ = iso.solve(target)
            rec["sol"][rname] = (rc, xc)
            assert iso.h.level_info(0)["coarse_iters"] == 0
        failures = _check_solutions(name, 3, rec, M)
        assert not failures, failures
    finally:
        iso.close()
        _capi().release_cached_memory()


def test_block_tridiagonal_and_inner_pcg_give_the_same_cycle():
    """Item 5, once on `cube` with the built-in smoothers back in place: kind 3 and kind 2 (coarse_rtol = 1e-28) give the
    same PCG iteration count and the same solution to 1e-9 -- the criterion of test_dense_and_iterative_coarsest_solvers_agree."""
    A, part = cc.build(CASES["cube"])
    b = np.cos(np.arange(A.shape[0]) * 0.21)
    out = {}
    for kind in (3, 2):
        iso = Isolated(A, part, kind)
        try:
            assert iso.info["kind"] == kind
            iso.h.set_smoother(0, None, None)
            x, it, conv, hist = iso.h.pcg(b, rel_tol=1e-8)
            assert conv and iso.calls == {"pre": 0, "post": 0}
            out[kind] = (iso.h.vcycle(b), x, it, iso.h.level_info(0)["coarse_iters"])
        finally:
            iso.close()
    assert out[3][3] == 0 and out[2][3] > 0
    assert out[3][2] == out[2][2]
    for i in (0, 1):
        assert np.linalg.norm(out[3][i] - out[2][i]) <= 1e-9 * np.linalg.norm(out[2][i])


def test_zz_print_the_ratio_table():
    """(not a check: the table of the module docstring, from this run)"""
    print("\nRATIO TABLE  case, kind, n_c, nblk, cond estimate, worst err / err_lu, worst bwd / bwd_lu")
    for row in ROWS:
        print("TABLE %-24s %d %6d %3d %8.1e %8.2f %8.2f" % row)
