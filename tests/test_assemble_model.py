"""The definition of the device assembly (saamge_amd/assemble_model.py) against the host generators of problems.py: same
pattern as prob.A, values within the first-order bound of two summation orders of the same terms (scipy's duplicate
summation does not keep element order), the right-hand-side elimination against the dense formula, and the refusals."""
import numpy as np
import pytest
import scipy.sparse as sp

from saamge_amd import assemble_model as am
from saamge_amd import problems as pr

CASES = {
    "hex_5x4x3": lambda: pr.poisson3d_problem((5, 4, 3), blk=(2, 2, 2)),
    "mixed_4": lambda: pr.poisson3d_mixed_problem(4, (2, 2, 2), wedges="half"),
    "q2_elasticity_2": lambda: pr.elasticity3d_q2_problem(2, blk=(2, 2, 2)),
    "mltest": lambda: pr.mltest_problem(),
}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def mesh_of(prob):
    return getattr(prob, "elem_ptr", None), prob.elem_to_dof


def coo_of_terms(prob, values):
    """sum of `values` (packed like elmat) per (row, column), as CSR with sorted indices"""
    ep, e2d = mesh_of(prob)
    n = prob.ND
    if ep is None:
        nde = e2d.shape[1]
        rows = np.repeat(e2d, nde, axis=1).ravel()
        cols = np.tile(e2d, (1, nde)).ravel()
    else:
        rows = np.concatenate([np.repeat(e2d[ep[e]:ep[e + 1]], ep[e + 1] - ep[e]) for e in range(len(ep) - 1)])
        cols = np.concatenate([np.tile(e2d[ep[e]:ep[e + 1]], ep[e + 1] - ep[e]) for e in range(len(ep) - 1)])
    M = sp.coo_matrix((np.asarray(values, float).ravel(), (rows, cols)), shape=(n, n)).tocsr()
    M.sort_indices()
    return M


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_matches_the_host_generator(name):
    prob = case(name)
    ep, e2d = mesh_of(prob)
    rowptr, col, val = am.assemble(prob.ND, ep, e2d, prob.elmat, prob.bdr)
    A = prob.A.tocsr().copy()
    A.sort_indices()
    assert np.array_equal(rowptr, A.indptr) and np.array_equal(col, A.indices)
    if name == "q2_elasticity_2":
        assert np.diff(rowptr).max() == 375
    m = coo_of_terms(prob, np.ones(np.asarray(prob.elmat).size))
    s = coo_of_terms(prob, np.abs(prob.elmat))
    assert np.array_equal(m.indices, col) and np.array_equal(s.indices, col)
    bound = 2.0 * (m.data - 1.0) * 2.0 ** -53 * s.data
    diff = np.abs(val - A.data)
    print("%s: largest difference %.3e" % (name, diff.max()))
    assert (diff <= bound).all(), (diff - bound).max()


def test_eliminate_rhs_is_the_dense_formula():
    prob = case("hex_5x4x3")
    rng = np.random.default_rng(7)
    n = prob.ND
    elmat = prob.elmat * rng.uniform(0.5, 2.0, prob.NE)[:, None, None]
    x = rng.standard_normal(n)
    b = rng.standard_normal(n)
    rowptr, col, val = am.assemble(n, None, prob.elem_to_dof, elmat, eliminate=False)
    A0 = sp.csr_matrix((val, col, rowptr), shape=(n, n)).toarray()
    ess = am.essential(n, prob.bdr)
    assert ess.any() and not ess.all()
    want = b.copy()
    free = ~ess
    for j in np.flatnonzero(ess):       # ascending; a column outside a row's pattern subtracts a zero: no change
        want[free] = want[free] - A0[free, j] * x[j]
    want[ess] = np.diag(A0)[ess] * x[ess]
    got = am.eliminate_rhs(n, None, prob.elem_to_dof, elmat, prob.bdr, x, b)
    assert np.array_equal(got, want)
    # the eliminated operator and the new right-hand side are the reference's system: A x = b has x = x_ess on the boundary
    _, _, ve = am.assemble(n, None, prob.elem_to_dof, elmat, prob.bdr)
    Ae = sp.csr_matrix((ve, col, rowptr), shape=(n, n)).toarray()
    sol = np.linalg.solve(Ae, got)
    assert np.allclose(sol[ess], x[ess], rtol=0, atol=1e-12)


def test_bdr_none_means_no_essential_dof():
    prob = case("hex_5x4x3")
    a = am.assemble(prob.ND, None, prob.elem_to_dof, prob.elmat, None)
    b = am.assemble(prob.ND, None, prob.elem_to_dof, prob.elmat, prob.bdr, eliminate=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_sum_starts_from_the_first_term_in_ascending_element_order():
    # three elements share the pair (0, 1); in floating point (1e16 + 1) - 1e16 = 0 but (1e16 - 1e16) + 1 = 1
    e2d = np.array([[0, 1], [0, 1], [0, 1]], np.int32)
    t = [1e16, 1.0, -1e16]
    elmat = np.array([[[1.0, v], [v, 1.0]] for v in t])
    _, col, val = am.assemble(2, None, e2d, elmat)
    assert np.array_equal(col, [0, 1, 0, 1]) and val[1] == (1e16 + 1.0) - 1e16 and val[0] == 3.0
    _, _, val = am.assemble(2, None, e2d[[0, 2, 1]], elmat[[0, 2, 1]])
    assert val[1] == 1.0


@pytest.mark.parametrize("what,match", [
    ("start", "start at 0"), ("empty", "needs a dof"), ("decreasing", "needs a dof"), ("range_hi", "out of range"),
    ("range_lo", "out of range"), ("twice", "twice"), ("orphan", "dof 3 lies in no element")])
def test_refusals(what, match):
    ep = np.array([0, 3, 6], np.int64)
    e2d = np.array([0, 1, 2, 2, 1, 4], np.int64)          # dof 3 of n = 5 is in no element
    n = 5
    if what == "start":
        ep = np.array([1, 3, 6])
    elif what == "empty":
        ep = np.array([0, 3, 3])
    elif what == "decreasing":
        ep = np.array([0, 4, 3])
    elif what == "range_hi":
        e2d[5] = 5
    elif what == "range_lo":
        e2d[0] = -1
    elif what == "twice":
        e2d[4] = 2
    nd = np.diff(ep)
    elmat = np.ones(int((nd * nd).sum()) if (nd > 0).all() else 18)
    with pytest.raises(ValueError, match=match):
        am.assemble(n, ep, e2d, elmat)
    if what == "orphan":
        e2d[5] = 3
        e2d2 = np.concatenate([e2d, [4]])
        am.assemble(n, np.array([0, 3, 7]), e2d2, np.ones(9 + 16))
