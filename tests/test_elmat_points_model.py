"""The model of the data at quadrature points (saamge_amd/elmat_model.py element_points, element_eval, element_loads_points,
element_errors) held to facts known without it: the measure, the partition of unity, bit-for-bit consistency with the existing
load vectors, exactness on the element's own polynomials, the degree of the rules, a source that is no finite-element function,
the convergence of the nodal interpolant under refinement, and the layout and refusals.

Tolerances.  u = 2^-53.  A sum of n floating-point terms t_k computed in any order differs from the exact sum by at most
n u sum |t_k| (to first order), and each term that is itself a product of p rounded factors carries p u more; the references
are math.fsum sums, which add no error of their own.  Where the terms have one sign this is the relative bound n u.  The
order-2 shape functions change sign, so there sum |t_k| is L (or L^2) times the sum, L = max_q sum_a |N_a(q)| from the model's
tables (elmat_points_cases.rule_constants; L = 1 for order 1).  Each bound below names its n and its p."""
import math

import numpy as np
import pytest

from saamge_amd import elmat_model as em

import elmat_points_cases as cs

U = cs.U
KINDS = sorted(cs.TYPES)
MOVED = [False, True]


def _sizes(kind):
    X, e2v, _ = cs.mesh(kind)
    dim, nd = X.shape[1], e2v.shape[1]
    return dim, nd, em.MASS_NPOINTS[(dim, nd)]


def _fsum_rows(a):
    return np.array([math.fsum(r) for r in a])


@pytest.mark.parametrize("moved", MOVED, ids=["affine", "moved"])
@pytest.mark.parametrize("kind", KINDS)
def test_measure_equals_the_sum_of_the_unit_mass_matrix(kind, moved):
    """sum_ab M_ab = sum_q wdet_q (sum_a N_a)^2 = sum_q wdet_q.  An entry of M is a sum of NQ terms of 2 products each: n = NQ,
    p = 2; the table entries N_a are products of at most 3 factors of at most 3 operations each (p = 9 per factor N_a, 18 for
    the pair), and sum_a N_a = 1 holds to nd u L.  With sum |terms| = L^2 sum_q wdet_q: tolerance (NQ + 20 + 2 nd) u L^2 sum wdet."""
    X, e2v, ep = cs.mesh(kind, moved)
    dim, nd, nq = _sizes(kind)
    L, _ = cs.rule_constants(dim, nd)
    qp, xq, wdet = em.element_points(X, e2v, ep)
    assert (wdet > 0.0).all()
    M = em.element_mass(X, e2v, np.ones(len(e2v)))
    vol = _fsum_rows(wdet.reshape(len(e2v), nq))
    tol = (nq + 20 + 2 * nd) * U * L * L * vol
    assert (np.abs(_fsum_rows(M.reshape(len(e2v), -1)) - vol) <= tol).all()


@pytest.mark.parametrize("kind", KINDS)
def test_points_lie_in_their_elements_and_eval_of_the_coordinates_is_xq(kind):
    for moved in MOVED:
        X, e2v, ep = cs.mesh(kind, moved)
        dim, nd, nq = _sizes(kind)
        qp, xq, wdet = em.element_points(X, e2v, ep)
        assert qp.dtype == np.int64 and np.array_equal(qp, nq * np.arange(len(e2v) + 1))
        assert xq.shape == (qp[-1], dim) and wdet.shape == (qp[-1],)
        uq, gq = em.element_eval(X, e2v, X, vdim=dim, elem_ptr=ep)
        assert np.array_equal(uq, xq)                               # the same sum in the same order: bit for bit
        if not moved:                                               # the undeformed grid: inside the element's box
            lo, hi = X[e2v].min(axis=1), X[e2v].max(axis=1)
            x = xq.reshape(len(e2v), nq, dim)
            assert (x > lo[:, None, :]).all() and (x < hi[:, None, :]).all()


@pytest.mark.parametrize("moved", MOVED, ids=["affine", "moved"])
@pytest.mark.parametrize("kind", KINDS)
def test_loads_of_the_evaluated_source_are_the_nodal_loads_bit_for_bit(kind, moved):
    X, e2v, ep = cs.mesh(kind, moved)
    dim = X.shape[1]
    coef = np.random.default_rng(1).uniform(0.5, 2.0, len(e2v))
    for vdim in (1, dim):
        src = cs.nodal(X, vdim)
        fq = em.element_eval(X, e2v, src, vdim=vdim, elem_ptr=ep, grad=False)[0]
        for c in (None, coef):
            got = em.element_loads_points(X, e2v, fq, vdim=vdim, coef=c, elem_ptr=ep)
            want = em.element_loads(X, e2v, src, vdim=vdim, coef=c, elem_ptr=ep)
            assert got.shape == want.shape and np.array_equal(got, want)


def _polynomial(kind, dim):
    """(p, grad p) of the element's own degree: linear for order 1; for order 2 a full quadratic, with the products x y (x z,
    y z, x y z) of distinct coordinates that the tensor-product types hold on an axis-parallel grid"""
    rng = np.random.default_rng(4)
    a0, a1 = rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0, dim)
    sq = rng.uniform(-1.0, 1.0, dim) if cs.ORDER[kind] == 2 else np.zeros(dim)
    pairs = [(i, j) for i in range(dim) for j in range(i + 1, dim)] if cs.ORDER[kind] == 2 else []
    cp = rng.uniform(-1.0, 1.0, len(pairs))
    c3 = rng.uniform(-1.0, 1.0) if kind == "hex27" else 0.0

    def p(x):
        v = a0 + x @ a1 + (x * x) @ sq
        for c, (i, j) in zip(cp, pairs):
            v = v + c * x[:, i] * x[:, j]
        return v + (c3 * x[:, 0] * x[:, 1] * x[:, 2] if dim == 3 else 0.0)

    def g(x):
        out = a1[None, :] + 2.0 * sq[None, :] * x
        for c, (i, j) in zip(cp, pairs):
            out[:, i] += c * x[:, j]
            out[:, j] += c * x[:, i]
        if dim == 3:
            for k in range(3):
                i, j = [m for m in range(3) if m != k]
                out[:, k] += c3 * x[:, i] * x[:, j]
        return out
    return p, g


@pytest.mark.parametrize("kind", KINDS)
def test_exact_on_the_elements_own_polynomials(kind):
    """Affine elements (the undeformed grid): the interpolant of p IS p, so the errors are rounding.  Per point, uq is a sum of nd
    terms N_a p(x_a): n = nd, the table entry 9 roundings, p at a node at most 20 (its value is bounded by S = 12: at most 11
    coefficients of size <= 1 on the unit cube), the product 1 -- and exq = p(xq) moves with the rounding of xq, another such
    sum, times the Lipschitz constant of p (a gradient component is at most 1 + 2 + 2 + 1 = 6, its norm at most 6 sqrt 3 <= S).
    |uq - exq| <= 2 (nd + 30) u L S =: d.  The gradient divides differences of size h by h: r[k] = sum_a p(x_a) dN_a[k] has the bound (nd + 30) u G S, the product with the cofactors and the division add
    dim + 2 roundings, and 1 / h = |J^-1|: |g - exact| <= 2 (nd + 30 + dim + 2) u G S / h =: dg.  The squared errors are then at
    most vol_e d^2 and vol_e dim dg^2."""
    X, e2v, ep = cs.mesh(kind)
    dim, nd, nq = _sizes(kind)
    L, G = cs.rule_constants(dim, nd)
    p, g = _polynomial(kind, dim)
    qp, xq, wdet = em.element_points(X, e2v, ep)
    u = p(X)
    E = em.element_errors(X, e2v, u, p(xq), g(xq)[:, None, :], elem_ptr=ep)
    vol = wdet.reshape(len(e2v), nq).sum(axis=1)
    h = (X[e2v].max(axis=1) - X[e2v].min(axis=1)).min()
    S = 12.0
    d = 2.0 * (nd + 30) * U * L * S
    dg = 2.0 * (nd + 30 + dim + 2) * U * G * S / h
    assert E.shape == (len(e2v), 2) and (E >= 0.0).all()
    assert (E[:, 0] <= vol * d * d).all() and (E[:, 1] <= vol * dim * dg * dg).all()
    # a gradient component of a linear field is the constant
    a = np.array([0.75, -1.5, 2.25])[:dim]
    gq = em.element_eval(X, e2v, 0.5 + X @ a, elem_ptr=ep)[1]
    assert gq.shape == (qp[-1], 1, dim) and (np.abs(gq[:, 0, :] - a[None, :]) <= dg).all()
    # a column without exact data is 0.0
    only = em.element_errors(X, e2v, u, p(xq), None, elem_ptr=ep)
    assert np.array_equal(only[:, 0], E[:, 0]) and not only[:, 1].any()
    assert np.array_equal(em.element_errors(X, e2v, u, None, g(xq)[:, None, :], elem_ptr=ep)[:, 1], E[:, 1])


@pytest.mark.parametrize("moved", MOVED, ids=["affine", "moved"])
@pytest.mark.parametrize("kind", KINDS)
def test_loads_of_the_constant_one_are_the_row_sums_of_the_mass_matrix(kind, moved):
    """Entry a: sum_q wdet_q N_a against sum_b sum_q wdet_q N_a N_b.  The row sum has nd NQ terms of 2 products, the load NQ terms
    of 2 products, sum_b N_b = 1 to nd u L, the table entries 18 roundings a pair: (NQ + nd + 2 + 18 + nd) u times the sum of the
    absolute terms, L sum_q wdet_q |N_a|."""
    X, e2v, ep = cs.mesh(kind, moved)
    dim, nd, nq = _sizes(kind)
    L, _ = cs.rule_constants(dim, nd)
    qp, xq, wdet = em.element_points(X, e2v, ep)
    got = em.element_loads_points(X, e2v, np.ones(qp[-1]), elem_ptr=ep)
    M = em.element_mass(X, e2v, np.ones(len(e2v)))
    N = np.abs(np.array([em.shape_values(dim, nd, q) for q in range(nq)]))      # (nq, nd)
    mag = L * (wdet.reshape(len(e2v), nq) @ N)
    rows = np.array([[math.fsum(r) for r in m] for m in M])
    assert (np.abs(got - rows) <= (nq + 2 * nd + 20) * U * mag).all()


def _exact_monomials(kind, dim):
    """the exponents the type's mass rule integrates exactly on an axis-parallel grid: 2 Gauss points are exact to degree 3 per
    axis, 3 to degree 5; the simplex rules in total degree (triangle 2, tetrahedron 2, 6-node triangle 4, 10-node tetrahedron 5);
    the wedge is the degree-2 triangle rule in (x, y) times 2 Gauss points in z"""
    per_axis = {"quad4": 3, "hex8": 3, "quad9": 5, "hex27": 5}
    total = {"tri3": 2, "tet4": 2, "tri6": 4, "tet10": 5}
    top = per_axis.get(kind, total.get(kind, 3))
    out = []
    for alpha in np.ndindex(*([top + 1] * dim)):
        if kind in per_axis or (kind in total and sum(alpha) <= top) or (kind == "wedge6" and alpha[0] + alpha[1] <= 2):
            out.append(alpha)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_rule_degree_on_the_unit_grid(kind):
    """sum_q wdet_q xq^alpha = prod 1 / (alpha_i + 1) on the unit square / cube.  All terms are positive.  wdet: the entries of J
    are sums of nd terms x_a dN_a of size <= G that cancel to h, relative error (nd + 1) u G / h each, dim of them in a product
    and the off-diagonal ones at rounding level: 2 dim (nd + 1) u G / h.  xq^alpha: xq is exact to (nd + 10) u L and the
    derivative of x^alpha on [0, 1] is at most |alpha|, plus |alpha| products.  The sum itself is an fsum."""
    X, e2v, ep = cs.mesh(kind)
    dim, nd, nq = _sizes(kind)
    assert np.array_equal(X.min(axis=0), np.zeros(dim)) and np.array_equal(X.max(axis=0), np.ones(dim))
    L, G = cs.rule_constants(dim, nd)
    h = (X[e2v].max(axis=1) - X[e2v].min(axis=1)).min()
    qp, xq, wdet = em.element_points(X, e2v, ep)
    for alpha in _exact_monomials(kind, dim):
        n = sum(alpha)
        got = math.fsum(wdet * np.prod(xq ** np.array(alpha, np.float64)[None, :], axis=1))
        want = 1.0 / np.prod([a + 1.0 for a in alpha])
        tol = U * (2 * dim * (nd + 1) * G / h + n * ((nd + 10) * L + 1) + 2)
        assert abs(got - want) <= tol, (alpha, got - want, tol)


@pytest.mark.parametrize("kind", ["quad4", "hex8", "tri3", "tet10", "hex27"])
def test_a_discontinuous_source_is_integrated_at_the_points(kind):
    """f = 1 for x < 0.3, else 0, on the grid with 4 cells along x (faces at 0.25 and 0.5).  sum_a b_a = sum_q wdet_q f_q
    (sum_a N_a = 1): the tolerance of the row sums above.  The nodal path integrates the interpolant of f, which differs."""
    X, v = cs.convergence_grids(kind)[0]
    dim, nd = X.shape[1], v.shape[1]
    nq = em.MASS_NPOINTS[(dim, nd)]
    L, _ = cs.rule_constants(dim, nd)
    qp, xq, wdet = em.element_points(X, v)
    fq = (xq[:, 0] < 0.3).astype(np.float64)
    b = em.element_loads_points(X, v, fq)
    want = math.fsum(wdet * fq)
    assert abs(math.fsum(b.ravel()) - want) <= (nq + 2 * nd + 20) * U * L * L * want
    nodal = math.fsum(em.element_loads(X, v, (X[:, 0] < 0.3).astype(np.float64)).ravel())
    assert abs(nodal - want) > 1e-3                                 # not a rewording of the nodal path


# the ratios of the L2 and H1 errors of the nodal interpolant of sin(pi x) sin(pi y) (sin(pi z)) from h = 1/4 to 1/8 and from 1/8
# to 1/16, as the model gives them: they approach 4 and 2 (order 1), 8 and 4 (order 2).
RATIOS = {
    "tri3": (3.854, 3.963, 1.957, 1.989), "quad4": (3.865, 3.966, 2.022, 2.006), "tet4": (3.774, 3.946, 1.846, 1.958),
    "hex8": (3.788, 3.946, 2.108, 2.033), "wedge6": (3.769, 3.941, 1.976, 1.994),
    "quad9": (8.024, 8.007, 3.993, 3.998), "hex27": (8.102, 8.028, 4.008, 4.002), "tri6": (7.833, 7.958, 3.930, 3.982),
    "tet10": (7.701, 7.925, 3.722, 3.929),
}
RATIO_MARGIN = 2e-3      # the figures above are rounded to 3 decimals (5e-4); the model is deterministic, sin and cos of another
                         # libm move a ratio by rounding errors only (1e-12): nothing else is spread


def interpolant_errors(kind):
    """(L2, H1) errors of the nodal interpolant on the three grids"""
    out = []
    for X, v in cs.convergence_grids(kind):
        dim = X.shape[1]
        qp, xq, wdet = em.element_points(X, v)
        s, c = np.sin(np.pi * xq), np.cos(np.pi * xq)
        eg = np.stack([np.pi * c[:, j] * np.prod(np.delete(s, j, axis=1), axis=1) for j in range(dim)], axis=1)
        E = em.element_errors(X, v, np.prod(np.sin(np.pi * X), axis=1), np.prod(s, axis=1), eg[:, None, :])
        out.append(np.sqrt([math.fsum(E[:, 0]), math.fsum(E[:, 1])]))
    return np.array(out)


@pytest.mark.parametrize("kind", KINDS)
def test_interpolant_converges_at_the_order_of_the_type(kind):
    e = interpolant_errors(kind)
    got = (e[0, 0] / e[1, 0], e[1, 0] / e[2, 0], e[0, 1] / e[1, 1], e[1, 1] / e[2, 1])
    print(kind, "L2 %.3f %.3f  H1 %.3f %.3f" % got)
    assert np.abs(np.array(got) - np.array(RATIOS[kind])).max() <= RATIO_MARGIN
    order = cs.ORDER[kind]
    for first, second, limit in ((got[0], got[1], 2.0 ** (order + 1)), (got[2], got[3], 2.0 ** order)):
        assert abs(second - limit) < abs(first - limit)             # approaching the limit; the limit itself is not asserted


# ---- layout and refusals ----
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_mixed_lists(name):
    X, e2v, ep = cs.mixed(name)
    dim = X.shape[1]
    nd = np.diff(ep)
    qp, xq, wdet = em.element_points(X, e2v, ep)
    assert np.array_equal(np.diff(qp), [em.MASS_NPOINTS[(dim, int(c))] for c in nd])
    assert len({int(c) for c in nd}) == 3
    # element by element, the mixed list gives what the element gives alone
    src = cs.nodal(X, dim)
    uq, gq = em.element_eval(X, e2v, src, vdim=dim, elem_ptr=ep)
    ex, eg = cs.nodal(uq, dim, 5), cs.nodal(uq, dim * dim, 6).reshape(-1, dim, dim)
    E = em.element_errors(X, e2v, src, ex, eg, vdim=dim, elem_ptr=ep)
    b = em.element_loads_points(X, e2v, ex, vdim=dim, elem_ptr=ep)
    for e in (0, len(nd) // 2, len(nd) - 1):
        one = e2v[ep[e]:ep[e + 1]][None, :]
        sl = slice(qp[e], qp[e + 1])
        q1, x1, w1 = em.element_points(X, one)
        assert np.array_equal(q1, [0, qp[e + 1] - qp[e]]) and np.array_equal(x1, xq[sl]) and np.array_equal(w1, wdet[sl])
        u1, g1 = em.element_eval(X, one, src, vdim=dim)
        assert np.array_equal(u1, uq[sl]) and np.array_equal(g1, gq[sl])
        assert np.array_equal(em.element_errors(X, one, src, ex[sl], eg[sl], vdim=dim)[0], E[e])
        assert np.array_equal(em.element_loads_points(X, one, ex[sl], vdim=dim).ravel(), b[dim * ep[e]:dim * ep[e + 1]])
    assert np.array_equal(em.element_loads_points(X, e2v, uq, vdim=dim, elem_ptr=ep), em.element_loads(X, e2v, src, vdim=dim, elem_ptr=ep))


def test_no_element_and_one_element():
    X, e2v, _ = cs.mesh("hex8", True)
    none = np.zeros((0, 8), np.int32)
    qp, xq, wdet = em.element_points(X, none)
    assert np.array_equal(qp, [0]) and xq.shape == (0, 3) and wdet.shape == (0,)
    uq, gq = em.element_eval(X, none, X, vdim=3)
    assert uq.shape == (0, 3) and gq.shape == (0, 3, 3)
    assert em.element_loads_points(X, none, np.zeros(0)).shape == (0, 0)
    assert em.element_errors(X, none, X[:, 0], np.zeros(0), None).shape == (0, 2)
    qp, xq, wdet = em.element_points(X, e2v[5:6])
    assert np.array_equal(qp, [0, 8]) and np.array_equal(xq, em.element_points(X, e2v)[1][40:48])


def test_refusals_in_order():
    X, e2v, _ = cs.mesh("tet4", True)
    NE, NV = len(e2v), len(X)
    flipped = e2v.copy()
    flipped[[3, 50], 0], flipped[[3, 50], 1] = e2v[[3, 50], 1], e2v[[3, 50], 0]
    out_of_range = np.where(e2v == 7, NV, e2v)
    u = np.ones(NV)
    calls = {
        "points": lambda lists, vdim, data: em.element_points(X, lists),
        "eval": lambda lists, vdim, data: em.element_eval(X, lists, data and u, vdim=vdim),
        "loads_points": lambda lists, vdim, data: em.element_loads_points(X, lists, data and np.ones(4 * NE), vdim=vdim),
        "errors": lambda lists, vdim, data: em.element_errors(X, lists, data and u, vdim=vdim),
    }
    for name, call in calls.items():
        if name != "points":
            with pytest.raises(ValueError, match="vdim"):           # vdim before the mesh and the data
                call(out_of_range, 2, None)
            with pytest.raises(ValueError, match="out of range"):   # the mesh before the data
                call(out_of_range, 1, None)
            with pytest.raises(ValueError, match="is needed"):      # the data before the determinants
                call(flipped, 1, None)
        else:
            with pytest.raises(ValueError, match="out of range"):
                call(out_of_range, 1, None)
        with pytest.raises(em.ElementError, match="element 3") as err:
            call(flipped, 1, True)
        assert err.value.element == 3
    with pytest.raises(ValueError, match="fq"):                     # point data of the wrong size
        em.element_loads_points(X, e2v, np.ones(NV))
    with pytest.raises(ValueError, match="exq"):
        em.element_errors(X, e2v, u, np.ones(NV))
