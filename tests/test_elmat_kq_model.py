"""The model of the element matrices with coefficients at the points (saamge_amd/elmat_model.py element_matrices_points,
element_mass_points) held to facts known without it: equal coefficients at the points of an element give the per-element forms
(bit for bit where the rules coincide, to rounding on affine simplices), an independent reference formed from element_eval's
gradients of the shape functions, the energy of a linear field under a coefficient that differs at every point, symmetry, row
sums, definiteness, the additivity over the points, the layout and the refusals, and the convergence the feature is for.

Tolerances.  u = 2^-53.  A sum of n floating-point terms t_k computed in any order differs from the exact sum by at most
n u sum |t_k| (to first order), and a term that is a product or nested sum of p rounded operations carries p u more; the
references are math.fsum sums, which add no error of their own.  The stiffness terms change sign, so every bound is relative to
the sum of the ABSOLUTE terms, and that sum comes from data the functions under test did not make: the physical gradients g_a of
the shape functions at the points (element_eval of the nodal indicator of local node a on a copy of the mesh whose elements share
no vertex -- the same J, cofactors and det bits as the model's own point, one division more) and wdet of element_points:
    diffusion   A_ab  = sum_q wdet_q sum_ij |g_a[i]| |K_q[i][j]| |g_b[j]|
    elasticity  A_aibj = sum_q wdet_q (lambda_q |g_a[i] g_b[j]| + mu_q |g_a[j] g_b[i]| + [i == j] mu_q sum_k |g_a[k] g_b[k]|)
Each bound below names its n and its p."""
import math

import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import elmat_model as em

import elmat_cases as ec
import elmat_kq_cases as kq
import elmat_points_cases as cs

U = cs.U
KINDS = sorted(cs.TYPES)
MOVED = [False, True]
SAME_RULE = ["quad4", "hex8", "wedge6", "quad9", "hex27", "tet4"]      # the mass rule is the stiffness rule (tet4: four equal terms)
MORE_POINTS = ["tri3", "tri6", "tet10"]


def _sizes(kind):
    X, e2v, _ = cs.mesh(kind)
    dim, nd = X.shape[1], e2v.shape[1]
    return dim, nd, em.MASS_NPOINTS[(dim, nd)]


def _tensor(c, dim):
    """(n, dim, dim) from rows of 1, dim or dim (dim + 1) / 2 coefficients: xx, yy, zz, xy, yz, xz / xx, yy, xy"""
    c = np.asarray(c, np.float64).reshape(len(c), -1)
    K = np.zeros((len(c), dim, dim))
    for i in range(dim):
        K[:, i, i] = c[:, 0] if c.shape[1] == 1 else c[:, i]
    if c.shape[1] > dim:
        for k, (i, j) in enumerate([(0, 1)] if dim == 2 else [(0, 1), (1, 2), (0, 2)]):
            K[:, i, j] = K[:, j, i] = c[:, dim + k]
    return K


_grads = {}


def _shape_gradients(kind, moved):
    """(g (NE, nq, nd, dim), wdet (NE, nq)): the physical gradient of every shape function at every point, from element_eval on
    the mesh with its elements pulled apart, and weight * det from element_points -- nothing of the functions under test."""
    key = (kind, moved)
    if key not in _grads:
        X, e2v, _ = cs.mesh(kind, moved)
        dim, nd, nq = _sizes(kind)
        NE = len(e2v)
        Xs = np.ascontiguousarray(X[e2v].reshape(-1, dim))
        lists = np.arange(NE * nd, dtype=np.int32).reshape(NE, nd)
        g = np.zeros((NE, nq, nd, dim))
        for a in range(nd):
            ind = (np.arange(NE * nd) % nd == a).astype(np.float64)
            g[:, :, a, :] = em.element_eval(Xs, lists, ind)[1].reshape(NE, nq, dim)
        wdet = em.element_points(X, e2v)[2].reshape(NE, nq)
        _grads[key] = (g, wdet)
    return _grads[key]


_refs = {}


def _reference(kind, moved, form, c):
    """_reference_of, kept for the read-only coefficient arrays of elmat_kq_cases.model (they live as long as the module)"""
    if c.flags.writeable:
        return _reference_of(kind, moved, form, c)
    key = (kind, moved, form, id(c))
    if key not in _refs:
        _refs[key] = _reference_of(kind, moved, form, c)
    return _refs[key]


def _reference_of(kind, moved, form, c):
    """(R, A) per element: the matrix from g, wdet and the coefficients -- an fsum over the points of products of float64 factors --
    and the sum of the absolute terms.  Diffusion: (NE, nd, nd); elasticity: (NE, nd * dim, nd * dim), dof dim * a + i."""
    g, wdet = _shape_gradients(kind, moved)
    NE, nq, nd, dim = g.shape
    c = np.asarray(c, np.float64).reshape(NE, nq, -1)
    if form == 0:
        K = _tensor(c.reshape(NE * nq, -1), dim).reshape(NE, nq, dim, dim)
        T = np.einsum("eq,eqai,eqij,eqbj->eqabij", wdet, g, K, g)      # (each entry one product of four factors; no sum is formed)
        T = T.reshape(NE, nq, nd, nd, dim * dim)
        terms = np.moveaxis(T, 1, -1).reshape(NE, nd, nd, -1)
    else:
        lam, mu = c[:, :, 0], c[:, :, 1]
        P = np.einsum("eqai,eqbj->eqaibj", g, g)                       # g_a[i] g_b[j]
        parts = [wdet[:, :, None, None, None, None] * lam[:, :, None, None, None, None] * P,
                 wdet[:, :, None, None, None, None] * mu[:, :, None, None, None, None] * np.swapaxes(P, 3, 5)]
        eye = np.eye(dim)[None, None, None, :, None, :]
        for k in range(dim):
            parts.append(wdet[:, :, None, None, None, None] * mu[:, :, None, None, None, None] * eye * P[:, :, :, k, :, k][:, :, :, None, :, None])
        T = np.stack(parts, axis=-1)                                   # (NE, nq, a, i, b, j, parts)
        terms = np.moveaxis(T, 1, -2).reshape(NE, nd * dim, nd * dim, -1)
    R = np.array([[[math.fsum(t) for t in row] for row in m] for m in terms])
    A = np.abs(terms).sum(axis=-1)
    return R, A


def _roundings(dim, nq, form):
    """n + p of one entry against the reference.  The model: s = w / det (1), F_a (dim products, dim - 1 sums: dim, relative to
    the absolute sum), the dot product with G_b (dim), the product with s (1), nq - 1 additions: nq + 2 dim + 1; elasticity has
    two products and a sum per part in the place of F_a and three parts: nq + dim + 9.  The reference: wdet (1), the division
    in g_a and in g_b (2), the three products of a term (3).  Two more for the literals of the rule."""
    return nq + (2 * dim + 1 if form == 0 else dim + 9) + 6 + 2


# ---- equal coefficients at the points of an element ----
@pytest.mark.parametrize("moved", MOVED, ids=["affine", "moved"])
@pytest.mark.parametrize("kind", SAME_RULE)
def test_equal_coefficients_give_element_matrices_bit_for_bit(kind, moved):
    X, e2v, ep = cs.mesh(kind, moved)
    dim, nd, nq = _sizes(kind)
    for form, ncoef in kq.forms(dim):
        coef = ec.coefficients(len(e2v), dim, form, ncoef)
        want = em.element_matrices(X, e2v, form, coef, elem_ptr=ep)
        got = em.element_matrices_points(X, e2v, form, np.repeat(coef, nq, axis=0), elem_ptr=ep)
        assert got.shape == want.shape and np.array_equal(got, want), (form, ncoef)


@pytest.mark.parametrize("moved", MOVED, ids=["affine", "moved"])
@pytest.mark.parametrize("kind", KINDS)
def test_equal_coefficients_give_element_mass_bit_for_bit(kind, moved):
    X, e2v, ep = cs.mesh(kind, moved)
    dim, nd, nq = _sizes(kind)
    c = ec.coefficients(len(e2v), dim, 0, 1)[:, 0]
    base = em.element_matrices(X, e2v, 1, ec.coefficients(len(e2v), dim, 1, 2), elem_ptr=ep)
    for vdim, add in ((1, None), (dim, None), (dim, base)):
        want = em.element_mass(X, e2v, c, vdim=vdim, elem_ptr=ep, add_to=add)
        got = em.element_mass_points(X, e2v, np.repeat(c, nq), vdim=vdim, elem_ptr=ep, add_to=add)
        assert got.shape == want.shape and np.array_equal(got, want), vdim


def _norm_bound(kind, form, c):
    """B per entry: sum_q wdet_q |g_a|_1 kmax_q |g_b|_1, kmax_q the largest |K_q[i][j]| (lambda_q + 2 mu_q for elasticity, every
    (i, j) of the node pair alike): what an entry can move by when the gradients TURN, which A (componentwise) does not cover."""
    g, wdet = _shape_gradients(kind, False)
    NE, nq, nd, dim = g.shape
    c = np.abs(np.asarray(c, np.float64).reshape(NE, nq, -1))
    kmax = c.max(axis=2) if form == 0 else c[:, :, 0] + 2.0 * c[:, :, 1]
    n1 = np.abs(g).sum(axis=3)                                       # (NE, nq, nd)
    B = np.einsum("eq,eqa,eqb->eab", wdet * kmax, n1, n1)
    return B if form == 0 else np.repeat(np.repeat(B, dim, axis=1), dim, axis=2)


@pytest.mark.parametrize("kind", MORE_POINTS)
def test_more_points_agree_to_rounding_on_affine_elements(kind):
    """The triangle (3 points against 1) and the order-2 simplices (6 against 3, 14 against 4) on the undeformed grid: both rules
    are exact for the integrand (a constant; a polynomial of degree 2 against rules of degree 2 / 4 / 5), so the two differ by
    rounding.  Two sources.  The arithmetic of an entry: each side within its own n + p (_roundings) of exact; the stiffness
    rule has fewer points, so twice the mass rule's count covers both.  The geometry: the two rules form J at different points;
    an entry of J is a sum of nd terms x_a dN_a of size <= Gr (coordinates in [0, 1]) that cancels to the mesh width h, so J
    moves by eps = (nd + 1) u Gr / h relative to itself, and with it det (dim factors) and the two inverse Jacobians of a term,
    whose direction changes too: (dim + 2) dim eps per side, relative to B of _norm_bound.  Gr: the larger of the two rules'
    sum_a max_k |dN_a[k]|.  Not bit for bit, and it must not be: 1/6 + 1/6 + 1/6 is not 0.5."""
    X, e2v, ep = cs.mesh(kind)
    dim, nd, nq = _sizes(kind)
    h = (X[e2v].max(axis=1) - X[e2v].min(axis=1)).min()
    Gr = max(cs.rule_constants(dim, nd)[1],
             max(sum(max(abs(v) for v in d) for d in em.reference_gradients(dim, nd, q)) for q in range(em.NPOINTS[(dim, nd)])))
    geo = 2 * (dim + 2) * dim * (nd + 1) * Gr / h
    differ = False
    for form, ncoef in kq.forms(dim):
        coef = ec.coefficients(len(e2v), dim, form, ncoef)
        rep = np.repeat(coef, nq, axis=0)
        want = em.element_matrices(X, e2v, form, coef)
        got = em.element_matrices_points(X, e2v, form, rep)
        _, A = _reference(kind, False, form, rep)
        tol = 2 * _roundings(dim, nq, form) * U * A + geo * U * _norm_bound(kind, form, rep)
        assert (np.abs(got - want) <= tol).all(), (form, ncoef, (np.abs(got - want) / tol).max())
        print(kind, form, ncoef, "largest difference / tolerance %.3g" % (np.abs(got - want) / tol).max())
        differ |= not np.array_equal(got, want)
    assert differ


@pytest.mark.parametrize("kind", ["tri6", "tet10"])
def test_curved_order2_simplices_differ_by_the_quadrature(kind):
    """on curved elements the two rules integrate a rational function: the difference is the quadrature's, far above rounding"""
    X, e2v, ep = cs.mesh(kind, True)
    dim, nd, nq = _sizes(kind)
    coef = ec.coefficients(len(e2v), dim, 0, 1)
    d = em.element_matrices_points(X, e2v, 0, np.repeat(coef, nq, axis=0)) - em.element_matrices(X, e2v, 0, coef)
    assert np.abs(d).max() > 1e-6 * np.abs(em.element_matrices(X, e2v, 0, coef)).max()


# ---- a coefficient that differs at every point ----
@pytest.mark.parametrize("moved", MOVED, ids=["affine", "moved"])
@pytest.mark.parametrize("kind", KINDS)
def test_entries_equal_the_reference_from_the_shape_gradients(kind, moved):
    """Every entry against sum_q wdet_q g_a^T K_q g_b (or the three parts of elasticity) with K_q of ITS point: n + p of
    _roundings, relative to A.  A coefficient read at the wrong point misses this by the spread of the coefficients."""
    X, e2v, ep = cs.mesh(kind, moved)
    dim, nd, nq = _sizes(kind)
    w = kq.model(kind, moved)
    for form, ncoef in kq.forms(dim):
        c, got = w[(form, ncoef)]
        R, A = _reference(kind, moved, form, c)
        tol = _roundings(dim, nq, form) * U * A
        assert (np.abs(got - R) <= tol).all(), (form, ncoef, (np.abs(got - R) / A).max() / U)
        if kind not in ("tri3", "tet4"):      # ... and the test can tell: the coefficients rotated by one point (where the gradients
                                              # are constant and the weights equal, the order of the coefficients does not matter)
            wrong = em.element_matrices_points(X, e2v, form, np.roll(np.asarray(c).reshape(len(e2v), nq, -1), 1, axis=1).reshape(np.shape(c)))
            assert not (np.abs(wrong - R) <= tol).all()


@pytest.mark.parametrize("moved", MOVED, ids=["affine", "moved"])
@pytest.mark.parametrize("kind", KINDS)
def test_energy_of_a_linear_field(kind, moved):
    """u = a . x (diffusion) or u = A x (elasticity) is in the space of every type, also of a curved isoparametric element, so
    grad u_h = a at every point whatever the rule: u_e^T K_e u_e = sum_q wdet_q a^T K_q a, or sum_q wdet_q (lambda_q tr(A)^2 +
    2 mu_q eps:eps).  No rule is exact for the coefficient, which differs at every point: the identity holds term by term.
    Left side: an fsum over (a, b) of u_a K_ab u_b (2 roundings a product) of entries within _roundings of exact, and the nodal
    values u_a themselves are rounded sums of dim products (dim + 1 each, twice): (n + p + 2 + 2 dim + 2) u sum |u_a| A_ab |u_b|.
    Right side: an fsum of products of at most 2 dim + 3 rounded factors of one sign per part: (2 dim + 4) u times its absolute sum."""
    X, e2v, ep = cs.mesh(kind, moved)
    dim, nd, nq = _sizes(kind)
    NE = len(e2v)
    w = kq.model(kind, moved)
    wdet = em.element_points(X, e2v)[2].reshape(NE, nq)
    a = np.array([0.75, -1.5, 2.25])[:dim]
    Am = np.array([[0.5, -1.25, 0.75], [2.0, 1.5, -0.5], [-1.0, 0.25, 1.75]])[:dim, :dim]
    for form, ncoef in kq.forms(dim):
        c, K = w[(form, ncoef)]
        _, A = _reference(kind, moved, form, c)
        c = np.asarray(c).reshape(NE, nq, -1)
        if form == 0:
            ue = (X @ a)[e2v]                                       # (NE, nd)
            Kq = _tensor(c.reshape(NE * nq, -1), dim).reshape(NE, nq, dim, dim)
            parts = np.einsum("eq,i,eqij,j->eqij", wdet, a, Kq, a).reshape(NE, -1)
        else:
            ue = (X @ Am.T)[e2v].reshape(NE, nd * dim)              # dof dim * a + i
            eps = 0.5 * (Am + Am.T)
            parts = np.stack([wdet * c[:, :, 0] * np.trace(Am) ** 2] +
                             [2.0 * wdet * c[:, :, 1] * eps[i, j] ** 2 for i in range(dim) for j in range(dim)], axis=-1).reshape(NE, -1)
        want = np.array([math.fsum(p) for p in parts])
        triple = ue[:, :, None] * K * ue[:, None, :]
        got = np.array([math.fsum(t.ravel()) for t in triple])
        tol = (_roundings(dim, nq, form) + 2 * dim + 4) * U * np.einsum("ea,eab,eb->e", np.abs(ue), A, np.abs(ue)) + \
            (2 * dim + 4) * U * np.abs(parts).sum(axis=1)
        assert (want > 0.0).all() and (np.abs(got - want) <= tol).all(), (form, ncoef, (np.abs(got - want) / tol).max())


@pytest.mark.parametrize("moved", MOVED, ids=["affine", "moved"])
@pytest.mark.parametrize("kind", KINDS)
def test_symmetry_row_sums_and_definiteness(kind, moved):
    """Symmetric bit for bit: (b, a) is the same double.  Diffusion: the shape functions sum to 1, so their gradients sum to 0 and a
    row sums to 0 -- to the rounding of an fsum over nd entries each within _roundings of exact, and of sum_b g_b = 0 itself, which
    holds to (nd + 2 dim) u sum_b |g_b| (nd terms, the table entry and the division): (n + p + nd + 2 dim) u sum_b A_ab.
    Definite: the exact K_e is positive semidefinite for positive definite K_q (lambda_q, mu_q > 0); the computed one is within
    E, |E_ab| <= _roundings u A_ab, so its smallest eigenvalue is at least -|E|_F, minus the eigensolver's own size u |K|_F."""
    X, e2v, ep = cs.mesh(kind, moved)
    dim, nd, nq = _sizes(kind)
    w = kq.model(kind, moved)
    for form, ncoef in kq.forms(dim):
        c, K = w[(form, ncoef)]
        assert np.array_equal(K, np.swapaxes(K, 1, 2))
        _, A = _reference(kind, moved, form, c)
        n = _roundings(dim, nq, form)
        if form == 0:
            rows = np.array([[math.fsum(r) for r in m] for m in K])
            assert (np.abs(rows) <= (n + nd + 2 * dim) * U * A.sum(axis=2)).all()
        size = K.shape[1]
        low = np.linalg.eigvalsh(K)[:, 0]
        slack = n * U * np.sqrt((A * A).sum(axis=(1, 2))) + 4 * size * U * np.sqrt((K * K).sum(axis=(1, 2)))
        assert (low >= -slack).all()
        assert (np.linalg.eigvalsh(K)[:, -1] > 0.0).all()
    M = w[("mass", 1)]
    assert np.array_equal(M, np.swapaxes(M, 1, 2))


@pytest.mark.parametrize("kind", KINDS)
def test_an_indicator_coefficient_is_the_sum_of_its_points(kind):
    """Coefficient 1 on some points and 0 on the rest.  A point with the coefficient 0 contributes s * (+-0) = +-0, which changes
    no sum; a point with 1 contributes F_a = G_a exactly.  So the matrices of the single points, added in ascending order from
    0.0, ARE the matrix of the set: no tolerance.  The mass likewise."""
    X, e2v, ep = cs.mesh(kind, True)
    dim, nd, nq = _sizes(kind)
    NE = len(e2v)
    chosen = [q for q in range(nq) if q % 3 != 1] or [0]

    def indicator(points, ncoef):
        c = np.zeros((NE, nq, ncoef))
        c[:, points, :] = 1.0
        return c.reshape(NE * nq, ncoef)
    for form, ncoef in ((0, 1), (1, 2)):
        whole = em.element_matrices_points(X, e2v, form, indicator(chosen, ncoef))
        acc = np.zeros_like(whole)
        for q in chosen:
            acc = acc + em.element_matrices_points(X, e2v, form, indicator([q], ncoef))
        assert np.array_equal(acc, whole), form
        assert np.abs(whole).max() > 0.0
    whole = em.element_mass_points(X, e2v, indicator(chosen, 1)[:, 0])
    acc = np.zeros_like(whole)
    for q in chosen:
        acc = acc + em.element_mass_points(X, e2v, indicator([q], 1)[:, 0])
    assert np.array_equal(acc, whole)


# ---- layout and refusals ----
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_mixed_lists(name):
    """element by element, the mixed list gives what the element gives alone with the rows of its points; packed layout, dof lists"""
    X, e2v, ep = cs.mixed(name)
    dim = X.shape[1]
    nd = np.diff(ep)
    w = kq.model("mixed:" + name, True)
    qp = em.element_points(X, e2v, ep)[0]
    assert w["NQ"] == qp[-1] and len({int(c) for c in nd}) == 3
    for form, ncoef in kq.forms(dim):
        c, K = w[(form, ncoef)]
        comp = dim if form else 1
        assert K.shape == (int(((nd * comp) ** 2).sum()),)
        per = ec.per_element(K, e2v, ep, comp)
        for e in (0, len(nd) // 2, len(nd) - 1):
            one = e2v[ep[e]:ep[e + 1]][None, :]
            assert np.array_equal(em.element_matrices_points(X, one, form, c[qp[e]:qp[e + 1]])[0], per[e])
    for vdim, add in ((1, (0, dim * (dim + 1) // 2)), (dim, (1, 2))):
        M = w[("mass", vdim)]
        per = ec.per_element(M, e2v, ep, vdim)
        e = len(nd) - 1
        one = e2v[ep[e]:ep[e + 1]][None, :]
        assert np.array_equal(em.element_mass_points(X, one, w["sigma"][qp[e]:qp[e + 1]], vdim=vdim)[0], per[e])
        assert np.array_equal(w[("sum", add[0])], w[add][1] + M)    # add_to: one addition per entry
    # equal coefficients on the mixed lists: the hexahedra, wedges and tetrahedra keep their bits; the 2-D list holds triangles
    coef = ec.coefficients(len(nd), dim, 0, 1)
    rep = np.repeat(coef, np.diff(qp), axis=0)
    same = np.array_equal(em.element_matrices_points(X, e2v, 0, rep, elem_ptr=ep), em.element_matrices(X, e2v, 0, coef, elem_ptr=ep))
    assert same == (name == "3d")
    assert np.array_equal(em.element_mass_points(X, e2v, rep[:, 0], elem_ptr=ep), em.element_mass(X, e2v, coef[:, 0], elem_ptr=ep))


def test_no_element_and_one_element():
    X, e2v, _ = cs.mesh("hex8", True)
    none = np.zeros((0, 8), np.int32)
    assert em.element_matrices_points(X, none, 0, np.zeros(0)).shape == (0, 0, 0)
    assert em.element_matrices_points(X, none, 1, np.zeros((0, 2))).shape == (0, 0, 0)
    assert em.element_mass_points(X, none, np.zeros(0), vdim=3).shape == (0, 0, 0)
    c, K = kq.model("hex8", True)[(0, 6)]
    one = em.element_matrices_points(X, e2v[5:6], 0, c[40:48])
    assert one.shape == (1, 8, 8) and np.array_equal(one[0], K[5])
    s = kq.model("hex8", True)["sigma"]
    assert np.array_equal(em.element_mass_points(X, e2v[5:6], s[40:48])[0], kq.model("hex8", True)[("mass", 1)][5])


def test_refusals_in_order():
    X, e2v, _ = cs.mesh("tet4", True)
    NE, NV, NQ = len(e2v), len(X), 4 * len(e2v)
    flipped = e2v.copy()
    flipped[[3, 50], 0], flipped[[3, 50], 1] = e2v[[3, 50], 1], e2v[[3, 50], 0]
    out_of_range = np.where(e2v == 7, NV, e2v)
    one = np.ones(NQ)
    with pytest.raises(ValueError, match="kind"):                   # kind before the mesh
        em.element_matrices_points(X, out_of_range, 2, one)
    with pytest.raises(ValueError, match="out of range"):           # the mesh before the coefficients
        em.element_matrices_points(X, out_of_range, 0, None)
    with pytest.raises(ValueError, match="5 nodes are no supported element type"):
        em.element_matrices_points(X, np.arange(13), 0, one, elem_ptr=[0, 4, 9, 13])
    with pytest.raises(ValueError, match="coefq"):                  # the coefficients before the determinants
        em.element_matrices_points(X, flipped, 0, None)
    with pytest.raises(ValueError, match="coefq"):                  # one row per POINT, not per element
        em.element_matrices_points(X, flipped, 0, np.ones(NE + 1))
    with pytest.raises(ValueError, match="ncoef = 2 is not allowed for kind 0"):
        em.element_matrices_points(X, flipped, 0, np.ones((NQ, 2)))
    with pytest.raises(ValueError, match="ncoef = 3 is not allowed for kind 1"):
        em.element_matrices_points(X, flipped, 1, np.ones((NQ, 3)))
    for form, c in ((0, one), (0, np.ones((NQ, 6))), (1, np.ones((NQ, 2)))):
        with pytest.raises(em.ElementError, match="element 3") as err:
            em.element_matrices_points(X, flipped, form, c)
        assert err.value.element == 3
    with pytest.raises(ValueError, match="vdim"):                   # the mass: vdim, the mesh, the coefficients, the determinants
        em.element_mass_points(X, out_of_range, None, vdim=2)
    with pytest.raises(ValueError, match="out of range"):
        em.element_mass_points(X, out_of_range, None)
    with pytest.raises(ValueError, match="coefq"):
        em.element_mass_points(X, flipped, np.ones(NE))
    with pytest.raises(em.ElementError, match="element 3"):
        em.element_mass_points(X, flipped, one)
    with pytest.raises(ValueError, match="add_to"):
        em.element_mass_points(X, e2v, one, add_to=np.zeros(3))
    # a curved order-2 simplex can be refused at a point of the mass rule that the stiffness rule does not have
    Xc, t2v, _ = cs.mesh("tri6", False)
    Xb = Xc.copy()
    v0, v1, m = Xc[t2v[0, 0]], Xc[t2v[0, 1]], t2v[0, 3]             # the midside node of edge (0, 1), pulled towards vertex 0
    found = False
    for t in np.linspace(0.5, 0.02, 49):
        Xb[m] = v0 + t * (v1 - v0)
        try:
            em.element_matrices(Xb, t2v[:1], 0, np.ones(1))
        except em.ElementError:
            break
        try:
            em.element_matrices_points(Xb, t2v[:1], 0, np.ones(6))
        except em.ElementError as err:
            assert err.element == 0
            found = True
            break
    assert found


# ---- what the feature is for ----
# -div(k grad u) = f on the unit square, k = 1 + x y, u = sin(pi x) sin(pi y), u = 0 on the boundary, 9-node quadrilaterals with
# h = 1/4, 1/8, 1/16.  The ratios of the L2 errors from one grid to the next, as the model gives them (it is deterministic): with k
# at the points they go to 8, the order of the element; with k averaged over each element the error of the coefficient, of
# first order in h inside an element, holds them back.
KQ_RATIOS = (7.862, 7.967)
AVG_RATIOS = (4.028, 4.010)
RATIO_MARGIN = 2e-3      # the figures are rounded to 3 decimals; sin and cos of another libm move a ratio by rounding errors only


def _solve(X, v, K, b):
    NV = len(X)
    ep = np.arange(len(v) + 1, dtype=np.int64) * v.shape[1]
    ess = ((X == 0.0) | (X == 1.0)).any(axis=1)
    rowptr, col, val = am.assemble(NV, ep, v.ravel(), K.ravel(), eliminate=False)
    A = np.zeros((NV, NV))
    A[np.repeat(np.arange(NV), np.diff(rowptr)), col] = val
    free = np.flatnonzero(~ess)
    rhs = am.assemble_rhs(NV, ep, v.ravel(), b.ravel())
    u = np.zeros(NV)
    u[free] = np.linalg.solve(A[np.ix_(free, free)], rhs[free])
    return u


def convergence_errors():
    """(L2 errors with k at the points, with k averaged per element) on the three grids"""
    out = []
    for X, v in cs.convergence_grids("quad9"):
        qp, xq, wdet = em.element_points(X, v)
        x, y = xq[:, 0], xq[:, 1]
        sx, sy, cx, cy = np.sin(np.pi * x), np.sin(np.pi * y), np.cos(np.pi * x), np.cos(np.pi * y)
        k = 1.0 + x * y
        f = -(y * np.pi * cx * sy + x * np.pi * sx * cy - k * 2.0 * np.pi ** 2 * sx * sy)
        b = em.element_loads_points(X, v, f)
        w = wdet.reshape(len(v), 9)
        kavg = (w * k.reshape(len(v), 9)).sum(axis=1) / w.sum(axis=1)
        errs = []
        for K in (em.element_matrices_points(X, v, 0, k), em.element_matrices(X, v, 0, kavg)):
            E = em.element_errors(X, v, _solve(X, v, K, b), sx * sy)
            errs.append(math.sqrt(math.fsum(E[:, 0])))
        out.append(errs)
    return np.array(out)


def test_a_smooth_coefficient_converges_at_the_order_of_the_element():
    e = convergence_errors()
    got_kq = (e[0, 0] / e[1, 0], e[1, 0] / e[2, 0])
    got_avg = (e[0, 1] / e[1, 1], e[1, 1] / e[2, 1])
    print("L2 ratios: k at the points %.3f %.3f, k averaged per element %.3f %.3f" % (got_kq + got_avg))
    assert np.abs(np.array(got_kq) - np.array(KQ_RATIOS)).max() <= RATIO_MARGIN
    assert np.abs(np.array(got_avg) - np.array(AVG_RATIOS)).max() <= RATIO_MARGIN
    for with_kq, averaged in zip(got_kq, got_avg):
        assert abs(with_kq - 8.0) < abs(averaged - 8.0)             # nearer to the order of the element; 8 itself is not asserted
