"""The definition of the order-2 simplices (saamge_amd/elmat_model.py: the 6-node triangle, the 10-node tetrahedron and the
6-node triangular face) against what is known independently of the model's rules: on straight-sided jittered elements the exact
integrals of products of barycentric monomials, int L^alpha = d! alpha! / (|alpha| + d)! * measure, in rational arithmetic with
the measure in extended precision (mpmath, 50 digits); on every mesh, curved included, the identities that hold for any rule.

Every bound is MEASURED on the model, in units of 2^-52 of the largest entry of the element's matrix (times max|u|^2 for the
quadratic form, max|src| for the loads), written down here and in DESIGN.md section 4.9.4, and asserted with the project's
margin of 8:
  affine mass       8.81  (tet10; 8.76 tri6)          quadratic form    1.74  (tet10; 1.44 tri6)
  row sums K 1      1.80  (tet10; 1.65 tri6)          rigid-body modes  2.08  (tet10; 1.56 tri6)
  rule sums        38.73  (the sum of 100 entries of both signs, tet10)       loads, src = 1  11.03     loads, random src  5.54
  face matrix       5.99  (6-node triangle)           surface of the box  0.67 (units of 2^-52 of the surface)
(the straight-sided elements' midside nodes are 0.5 * (a + b) rounded to double, so they are affine up to that rounding; the
references take the vertices alone)
"""
from fractions import Fraction
from itertools import product
from math import factorial, fsum

import mpmath as mp
import numpy as np
import pytest

from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import elmat_cases as ec
import elmat_p2_cases as pc
from test_elmat_model import _check, _rigid_modes

mp.mp.dps = 50
EPS = ec.EPS
AFFINE_MASS, QUADRATIC, ROWSUM, RIGID, RULESUM, LOADS_ONE, LOADS_SRC, FACE, SURFACE = 8.81, 1.74, 1.80, 2.08, 38.73, 11.03, 5.54, 5.99, 0.67
SMALL = {2: "tri6_4x3", 3: "tet10_3x2x2"}      # the meshes the extended-precision references run on


# ---- exact integrals on the reference simplex ----
def _polys(dim):
    """the shape functions as polynomials in the barycentric coordinates: {exponents: coefficient}"""
    unit = lambda i: tuple(int(k == i) for k in range(dim + 1))
    add = lambda a, b: tuple(x + y for x, y in zip(a, b))
    out = [{add(unit(i), unit(i)): Fraction(2), unit(i): Fraction(-1)} for i in range(dim + 1)]
    return out + [{add(unit(i), unit(j)): Fraction(4)} for (i, j) in em.P2_EDGES[dim]]


def _integral(poly, dim):
    """of a polynomial in the barycentric coordinates over a simplex of measure 1"""
    total = Fraction(0)
    for alpha, c in poly.items():
        num = factorial(dim)
        for a in alpha:
            num *= factorial(a)
        total += c * Fraction(num, factorial(sum(alpha) + dim))
    return total


def _times(p, q):
    out = {}
    for (a, c), (b, d) in product(p.items(), q.items()):
        key = tuple(x + y for x, y in zip(a, b))
        out[key] = out.get(key, Fraction(0)) + c * d
    return out


def _mass_table(dim):
    P = _polys(dim)
    return [[_integral(_times(p, q), dim) for q in P] for p in P]


def _measure(V):
    """of the simplex with the vertices V (dim + 1, dim), in extended precision"""
    d = V.shape[1]
    return mp.det(mp.matrix([[mp.mpf(float(V[k + 1, i])) - mp.mpf(float(V[0, i])) for k in range(d)] for i in range(d)])) / factorial(d)


def _units(err, scale):
    return float(err) / float(scale) / EPS


def test_the_exact_mass_tables_are_the_textbook_ones():
    T = np.array([[int(v * 180) for v in row] for row in _mass_table(2)])
    assert all(v * 180 == int(v * 180) for row in _mass_table(2) for v in row)
    E = em.P2_EDGES[2]
    for a in range(3):
        assert T[a, a] == 6 and all(T[a, b] == -1 for b in range(3) if b != a)
        for k, e in enumerate(E):
            assert T[a, 3 + k] == (0 if a in e else -4)                      # adjacent edge 0, opposite edge -4
    for k in range(3):
        assert T[3 + k, 3 + k] == 32 and all(T[3 + k, 3 + l] == 16 for l in range(3) if l != k)
    T = np.array([[int(v * 420) for v in row] for row in _mass_table(3)])
    assert all(v * 420 == int(v * 420) for row in _mass_table(3) for v in row)
    E = em.P2_EDGES[3]
    for a in range(4):
        assert T[a, a] == 6 and all(T[a, b] == 1 for b in range(4) if b != a)
        for k, e in enumerate(E):
            assert T[a, 4 + k] == (-4 if a in e else -6)
    for k, e in enumerate(E):
        for l, f in enumerate(E):
            assert T[4 + k, 4 + l] == (32 if k == l else (16 if set(e) & set(f) else 8))
    assert np.array_equal(T, T.T)


def test_both_mass_rules_integrate_the_monomials_they_claim():
    """positive weights, interior points, the weights sum to the reference measure, exact to degree 4 / 5"""
    for dim, pts, w, deg in ((2, em.P2_TRI_POINTS, em.P2_TRI_W, 4), (3, em.P2_TET_POINTS, em.P2_TET_W, 5)):
        assert len(pts) == len(w) == em.MASS_NPOINTS[(dim, (6, 10)[dim - 2])]
        assert all(x > 0.0 for x in w) and all(min(p) > 0.0 and sum(p) < 1.0 for p in pts)
        worst = 0.0
        for alpha in product(range(deg + 1), repeat=dim):
            if sum(alpha) > deg:
                continue
            exact = Fraction(int(np.prod([factorial(a) for a in alpha])), factorial(sum(alpha) + dim))
            got = sum(mp.mpf(wq) * mp.fprod([mp.mpf(p[k]) ** alpha[k] for k in range(dim)]) for p, wq in zip(pts, w))
            worst = max(worst, abs(float(got / mp.mpf(exact.numerator) * exact.denominator - 1)))
        print("%dD: largest relative error of a monomial up to degree %d: %.2e" % (dim, deg, worst))
        assert worst <= 8 * (3.1e-16 if dim == 2 else 5.5e-16)


# ---- straight-sided elements against the exact integrals ----
@pytest.mark.parametrize("dim", [2, 3])
def test_affine_mass_matrices_against_the_exact_integrals(dim):
    X, e2n, _ = pc.mesh(SMALL[dim], "straight")
    c = ec.coefficients(len(e2n), dim, 0, 1)[:, 0]
    M = em.element_mass(X, e2n, c)
    T = _mass_table(dim)
    nd = e2n.shape[1]
    worst = 0.0
    for e in range(len(e2n)):
        vol = _measure(X[e2n[e, :dim + 1]]) * mp.mpf(float(c[e]))
        ref = [[vol * T[a][b].numerator / T[a][b].denominator for b in range(nd)] for a in range(nd)]
        scale = max(abs(v) for row in ref for v in row)
        worst = max(worst, max(_units(abs(mp.mpf(float(M[e, a, b])) - ref[a][b]), scale) for a in range(nd) for b in range(nd)))
    _check("affine mass", worst, AFFINE_MASS)


def _quadratic(dim):
    A = np.array([[0.7, -0.3, 0.2], [-0.3, 1.1, 0.4], [0.2, 0.4, -0.9]])[:dim, :dim]
    return A, np.array([0.5, -1.2, 0.8])[:dim], 0.3


@pytest.mark.parametrize("dim", [2, 3])
def test_affine_stiffness_against_the_closed_form_of_a_quadratic(dim):
    """K 1 = 0, and u^T K u = int |grad u|^2 for u = x^T A x + b . x + c: |grad u|^2 is quadratic, its integral is
    measure * sum over the P2 nodes of its value times the exact integral of the node's shape function"""
    X, e2n, _ = pc.mesh(SMALL[dim], "straight")
    NE, nd = e2n.shape
    K = em.element_matrices(X, e2n, 0, np.ones(NE))
    _check("row sums", max(np.abs(k.sum(axis=1)).max() / np.abs(k).max() for k in K) / EPS, ROWSUM)
    A, b, c0 = _quadratic(dim)
    Am, bm = mp.matrix(A.tolist()), mp.matrix(b.tolist())
    weights = [_integral(p, dim) for p in _polys(dim)]
    worst = 0.0
    for e in range(NE):
        V = [mp.matrix([mp.mpf(float(v)) for v in X[n]]) for n in e2n[e, :dim + 1]]
        nodes = V + [(V[i] + V[j]) / 2 for (i, j) in em.P2_EDGES[dim]]
        vol = _measure(X[e2n[e, :dim + 1]])
        ref = mp.mpf(0)
        for x, w in zip(nodes, weights):
            g = 2 * (Am * x) + bm
            ref += (g.T * g)[0] * w.numerator / w.denominator
        ref *= vol
        u = [float((x.T * Am * x)[0] + (bm.T * x)[0] + c0) for x in nodes]      # (at the exact midpoints, rounded once)
        got = mp.mpf(0)
        for a in range(nd):
            for bb in range(nd):
                got += mp.mpf(u[a]) * mp.mpf(float(K[e, a, bb])) * mp.mpf(u[bb])
        worst = max(worst, _units(abs(got - ref), np.abs(K[e]).max() * max(abs(v) for v in u) ** 2))
    _check("quadratic form", worst, QUADRATIC)


@pytest.mark.parametrize("dim", [2, 3])
def test_elasticity_annihilates_the_rigid_body_modes(dim):
    X, e2n, _ = pc.mesh(SMALL[dim], "straight")
    K, _ = pc.model(SMALL[dim], "straight", 1, 2)
    dptr, dofs = em.dof_lists(dim, e2n, 1)
    assert len(_rigid_modes(X)) == (3, 6)[dim - 2]
    worst = 0.0
    for r in _rigid_modes(X):
        for e, k in enumerate(K):
            worst = max(worst, np.abs(k @ r[dofs[dptr[e]:dptr[e + 1]]]).max() / (np.abs(k).max() * np.abs(r).max()))
    _check("rigid-body modes", worst / EPS, RIGID)


# ---- identities of any rule, on every mesh ----
def test_the_model_accepts_every_jittered_mesh():
    """no element of any mesh has a non-positive determinant at a point of either rule, at CURVED and the seed of the cases"""
    assert pc.CURVED == 0.1
    for name in pc.MESHES:
        for jitter in pc.JITTERS:
            X, e2n, ep = pc.mesh(name, jitter)
            NE = ec.num_elements(e2n, ep)
            em.element_matrices(X, e2n, 0, np.ones(NE), elem_ptr=ep)      # raises ElementError otherwise
            em.element_mass(X, e2n, np.ones(NE), elem_ptr=ep)


_PURE_P2 = [n for n in pc.MESHES if n in pc.PURE]


@pytest.mark.parametrize("jitter", pc.JITTERS)
@pytest.mark.parametrize("name", _PURE_P2)
def test_rule_sums_and_loads(name, jitter):
    """the sum of all mass entries is sum_q (w det) c; with src = 1 the loads are the row sums of M_e, with a random src M_e src_e"""
    X, e2n, _ = pc.mesh(name, jitter)
    NE, nd = e2n.shape
    dim = X.shape[1]
    c = ec.coefficients(NE, dim, 0, 1)[:, 0]
    M = em.element_mass(X, e2n, c)
    points, bad = em._mass_points(X[e2n], dim, nd, c)
    assert not bad.any()
    scale = np.abs(M).max(axis=(1, 2))
    want = np.array([fsum(s[e] for _, s in points) for e in range(NE)])
    got = np.array([fsum(M[e].ravel()) for e in range(NE)])
    _check("rule sums", (np.abs(got - want) / scale).max() / EPS, RULESUM)
    one = em.element_loads(X, e2n, np.ones(len(X)), coef=c)
    rows = np.array([[fsum(M[e, a]) for a in range(nd)] for e in range(NE)])
    _check("loads, src = 1", (np.abs(one - rows).max(axis=1) / scale).max() / EPS, LOADS_ONE)
    src, srcd = pc.nodal_data(len(X), dim)
    got = em.element_loads(X, e2n, src, coef=c)
    want = np.array([[fsum(M[e, a] * src[e2n[e]]) for a in range(nd)] for e in range(NE)])
    _check("loads, random src", (np.abs(got - want).max(axis=1) / scale).max() / EPS, LOADS_SRC)
    gotd = em.element_loads(X, e2n, srcd, vdim=dim, coef=c)                    # the vector form: component by component
    for i in range(dim):
        assert np.array_equal(gotd.reshape(NE, nd, dim)[:, :, i], em.element_loads(X, e2n, np.ascontiguousarray(srcd[:, i]), coef=c))


def test_face_matrices_against_the_exact_integrals_and_the_surface_of_the_box():
    name = SMALL[3]
    X, e2n, _ = pc.mesh(name, "straight")
    fe, fl = pc.faces(name, "all")
    T = _mass_table(2)
    worst = 0.0
    for f in range(len(fe)):
        got = em.boundary_mass(X, e2n, fe[f:f + 1], fl[f:f + 1], np.ones(1), add_to=np.zeros((len(e2n), 10, 10)))[fe[f]]
        nodes = np.array(em.FACE_NODES[(3, 10)][fl[f]])
        V = [mp.matrix([mp.mpf(float(v)) for v in X[e2n[fe[f], n]]]) for n in nodes[:3]]
        a, b = V[1] - V[0], V[2] - V[0]
        n = mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        area = mp.sqrt((n.T * n)[0]) / 2
        sub = got[np.ix_(nodes, nodes)]
        assert np.count_nonzero(got) == np.count_nonzero(sub)                  # nothing outside the face's nodes
        scale = area * 32 / 180
        worst = max(worst, max(_units(abs(mp.mpf(float(sub[i, j])) - area * T[i][j].numerator / T[i][j].denominator), scale)
                               for i in range(6) for j in range(6)))
    _check("face matrix", worst, FACE)
    for name in ("tet10_3x2x2", "tet10_5x4x3", "tri6_4x3", "tri6_9x8"):
        X, e2n, _ = pc.mesh(name)
        fe, fl = pc.faces(name, "all")
        ext = X.max(axis=0) - X.min(axis=0)
        surface = 2.0 * (ext[0] + ext[1]) if X.shape[1] == 2 else 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2])
        got = em.boundary_mass(X, e2n, fe, fl, np.ones(len(fe)), add_to=np.zeros((len(e2n),) + (e2n.shape[1],) * 2))
        _check("surface of the box", abs(fsum(got.ravel()) - surface) / surface / EPS, SURFACE)


# ---- what holds exactly ----
def _touched(dim, e2n, ep, fe, fl, shape):
    """which entries of the scalar matrices the listed faces add to (a face's exact zeros included)"""
    nd = np.diff(ep).astype(np.int64) if ep is not None else np.full(e2n.shape[0], e2n.shape[1], np.int64)
    moff = np.concatenate([[0], np.cumsum(nd * nd)])
    mask = np.zeros(int(moff[-1]), bool)
    for e, l in zip(fe, fl):
        nodes = np.array(em.FACE_NODES[(dim, int(nd[e]))][l])
        mask[moff[e] + (nodes[:, None] * nd[e] + nodes[None, :]).ravel()] = True
    return mask.reshape(shape)


@pytest.mark.parametrize("jitter", pc.JITTERS)
@pytest.mark.parametrize("name", pc.MESHES)
def test_exact_properties(name, jitter):
    X, e2n, ep = pc.mesh(name, jitter)
    dim, NE = X.shape[1], ec.num_elements(e2n, ep)
    c = ec.coefficients(NE, dim, 0, 1, seed=9)[:, 0]
    M = em.element_mass(X, e2n, c, elem_ptr=ep)
    Ms = ec.per_element(M, e2n, ep, 1)
    assert all(np.array_equal(m, m.T) for m in Ms)
    for kind in (0, 1):
        K, _ = pc.model(name, jitter, kind, 2 if kind else 1)
        assert all(np.array_equal(k, k.T) for k in ec.per_element(K, e2n, ep, dim if kind else 1))
    # the vector form: the scalar matrix in the diagonal blocks, +0.0 elsewhere
    Mv = ec.per_element(em.element_mass(X, e2n, c, vdim=dim, elem_ptr=ep), e2n, ep, dim)
    for m, mv in zip(Ms, Mv):
        nd = m.shape[0]
        full = mv.reshape(nd, dim, nd, dim)
        for i in range(dim):
            for j in range(dim):
                blk = full[:, i, :, j]
                assert np.array_equal(blk, m) if i == j else (np.all(blk == 0.0) and not np.signbit(blk).any())
    # add_to: one addition per entry
    K, _ = pc.model(name, jitter, 0, 1)
    assert np.array_equal(em.element_mass(X, e2n, c, elem_ptr=ep, add_to=K), K + M)
    E, _ = pc.model(name, jitter, 1, 2)
    assert np.array_equal(em.element_mass(X, e2n, c, vdim=dim, elem_ptr=ep, add_to=E), E + em.element_mass(X, e2n, c, vdim=dim, elem_ptr=ep))
    # a permuted face list gives the same bits; entries no face touches keep theirs
    rng = np.random.default_rng(31)
    fe, fl = pc.faces(name, "all")
    pe, pl = pc.faces(name, "shuffled")
    cf, cp = pc.face_coefficients(NE, fe, fl), pc.face_coefficients(NE, pe, pl)
    base = rng.uniform(-1.0, 1.0, K.shape)
    touched = _touched(dim, e2n, ep, fe, fl, K.shape)
    base[~touched] = np.where(rng.random((~touched).sum()) < 0.5, -0.0, np.nan)
    got = em.boundary_mass(X, e2n, fe, fl, cf, elem_ptr=ep, add_to=base)
    assert got.tobytes() == em.boundary_mass(X, e2n, pe, pl, cp, elem_ptr=ep, add_to=base).tobytes()
    assert got[~touched].tobytes() == base[~touched].tobytes() and touched.any() and not touched.all()
    g = pc.nodal_data(len(X), dim)[0]
    vec = rng.uniform(-1.0, 1.0, em.element_loads(X, e2n, g, elem_ptr=ep).shape)
    assert np.array_equal(em.boundary_loads(X, e2n, fe, fl, g, coef=cf, elem_ptr=ep, add_to=vec),
                          em.boundary_loads(X, e2n, pe, pl, g, coef=cp, elem_ptr=ep, add_to=vec))


@pytest.mark.parametrize("name", sorted(pc.MIXED))
def test_a_mixed_list_equals_the_per_type_calls(name):
    X, lists, ep = pc.mesh(name, "curved")
    dim = X.shape[1]
    nd = np.diff(ep)
    assert len(np.unique(nd)) == 3
    c = ec.coefficients(len(nd), dim, 0, 1)[:, 0]
    src = pc.nodal_data(len(X), dim)[0]
    K = ec.per_element(em.element_matrices(X, lists, 0, c, elem_ptr=ep), lists, ep, 1)
    M = ec.per_element(em.element_mass(X, lists, c, elem_ptr=ep), lists, ep, 1)
    L = em.element_loads(X, lists, src, coef=c, elem_ptr=ep)
    for k in np.unique(nd):
        ids = np.flatnonzero(nd == k)
        own = np.stack([lists[ep[e]:ep[e + 1]] for e in ids])
        assert np.array_equal(em.element_matrices(X, own, 0, c[ids]), np.stack([K[e] for e in ids]))
        assert np.array_equal(em.element_mass(X, own, c[ids]), np.stack([M[e] for e in ids]))
        assert np.array_equal(em.element_loads(X, own, src, coef=c[ids]), np.stack([L[ep[e]:ep[e + 1]] for e in ids]))
    counts = em.type_counts(dim, lists, ep)
    assert counts == ([12, 0, 0, 0, 0] if dim == 2 else [0, 0, 12, 0, 0])
    assert em.order2_count(dim, lists, ep) == (13 if dim == 2 else 14)


def test_what_the_model_refuses():
    X, e2n, _ = pc.mesh("tet10_3x2x2")
    X2, t6, _ = pc.mesh("tri6_4x3")
    NE = len(e2n)
    with pytest.raises(ValueError, match="5 nodes are no supported element type in 3D"):
        em.element_matrices(X, e2n[:, :5], 0, np.ones(NE))
    with pytest.raises(ValueError, match="10 nodes are no supported element type in 2D"):
        em.element_matrices(X2, np.arange(20).reshape(2, 10), 0, np.ones(2))
    with pytest.raises(ValueError, match="element 1: 7 nodes"):
        em.element_mass(X, np.concatenate([e2n[0], e2n[1, :7], e2n[2]]), np.ones(3), elem_ptr=np.array([0, 10, 17, 27]))
    twice = e2n.copy()
    twice[5, 9] = twice[5, 4]
    with pytest.raises(ValueError, match="twice"):
        em.element_loads(X, twice, np.ones(len(X)))
    with pytest.raises(ValueError, match="out of range"):
        em.element_matrices(X, np.where(e2n == 0, len(X), e2n), 0, np.ones(NE))
    bad = e2n.copy()
    bad[[17, 41]] = e2n[[17, 41]][:, pc.INVERTED]                                   # two elements mirrored
    for call in (lambda: em.element_matrices(X, bad, 0, np.ones(NE)), lambda: em.element_matrices(X, bad, 1, np.ones((NE, 2))),
                 lambda: em.element_mass(X, bad, np.ones(NE)), lambda: em.element_loads(X, bad, np.ones(len(X)))):
        with pytest.raises(em.ElementError) as err:
            call()
        assert err.value.element == 17
    Y, moved = pc.mass_only_inversion()
    em.element_matrices(Y, moved, 0, np.ones(NE))                                # accepted: the stiffness points are fine
    with pytest.raises(em.ElementError) as err:
        em.element_mass(Y, moved, np.ones(NE))
    assert err.value.element == 5
    # faces
    fe, fl = pc.faces("tet10_3x2x2", "all")
    K = np.zeros((NE, 10, 10))
    wrong = fl.copy()
    wrong[7] = 4
    with pytest.raises(em.FaceError, match="face 7: face_local is outside") as err:
        em.boundary_mass(X, e2n, fe, wrong, np.ones(len(fe)), add_to=K)
    assert err.value.face == 7
    f2, l2 = pc.faces("tri6_4x3", "all")
    wrong = l2.copy()
    wrong[3] = 3
    with pytest.raises(em.FaceError, match="face 3: face_local is outside"):
        em.boundary_loads(X2, t6, f2, wrong, np.ones(len(X2)), add_to=np.zeros((len(t6), 6)))
    with pytest.raises(em.FaceError, match="face 2: the same"):
        em.boundary_mass(X, e2n, np.concatenate([fe[:5], fe[2:3]]), np.concatenate([fl[:5], fl[2:3]]), np.ones(6), add_to=K)
    flat = np.array(X)
    flat[e2n[fe[4], list(em.FACE_NODES[(3, 10)][fl[4]])]] = X[e2n[fe[4], em.FACE_NODES[(3, 10)][fl[4]][0]]]
    with pytest.raises(em.FaceError, match="the measure is not positive"):
        em.boundary_mass(flat, e2n, fe[4:5], fl[4:5], np.ones(1), add_to=K)


# ---- tables, counts and the mesh helpers of problems.py ----
def test_tables_counts_and_dof_lists():
    assert em.ALL_TYPE_INDEX[(2, 6)] == 7 and em.ALL_TYPE_INDEX[(3, 10)] == 8 and em.FACE_TYPE_INDEX[(3, 6)] == 5
    assert em.face_info_index(3, 6) == em.face_info_index(3, 3) == 2 and em.face_info_index(2, 3) == 1
    assert em.NPOINTS[(2, 6)] == 3 and em.NPOINTS[(3, 10)] == 4 and em.MASS_NPOINTS[(2, 6)] == 6 and em.MASS_NPOINTS[(3, 10)] == 14
    assert set(em.P2_SIMPLEX) <= set(em.ORDER2)
    for (dim, nd) in em.P2_SIMPLEX:                                              # every face lists vertices, then their midpoints
        for face in em.FACE_NODES[(dim, nd)]:
            if dim == 2:
                assert face[1] == dim + 1 + em.P2_EDGES[2].index((face[0], face[2]))
            else:
                for k in range(3):
                    pair = tuple(sorted((face[k], face[(k + 1) % 3])))
                    assert face[3 + k] == 4 + em.P2_EDGES[3].index(pair)
        assert [f[:dim] if dim == 3 else (f[0], f[2]) for f in em.FACE_NODES[(dim, nd)]] == \
               [tuple(f) for f in em.FACE_NODES[(dim, dim + 1)]]
    X, e2n, _ = pc.mesh("tet10_3x2x2")
    assert em.type_counts(3, e2n) == [0] * 5 and em.order2_count(3, e2n) == 72
    dptr, dofs = em.dof_lists(3, e2n, 1)
    assert np.array_equal(dptr, 30 * np.arange(73)) and np.array_equal(dofs.reshape(72, 10, 3), 3 * e2n[:, :, None] + np.arange(3))
    assert em.order2_count(2, pc.mesh("tri6_9x8")[1]) == 144


def test_p2_mesh_helpers():
    n = (3, 2, 2)
    V, tets = pr.grid_coords(n), pr.hex_to_tets(n)
    X, e2n = pr.p2_simplex_nodes(V, tets)
    assert e2n.shape == (72, 10) and e2n.dtype == np.int32 and np.array_equal(e2n[:, :4], tets) and np.array_equal(X[:len(V)], V)
    edges = sorted({(min(t[i], t[j]), max(t[i], t[j])) for t in tets.tolist() for (i, j) in em.P2_EDGES[3]})
    assert len(X) == len(V) + len(edges)
    for t in e2n[::7]:
        for k, (i, j) in enumerate(em.P2_EDGES[3]):
            assert t[4 + k] == len(V) + edges.index((min(t[i], t[j]), max(t[i], t[j])))
            assert np.array_equal(X[t[4 + k]], 0.5 * (X[t[i]] + X[t[j]]))
    assert np.array_equal(pr.p2_simplex_straight_sided(X, e2n), X)
    Xj = pr.jitter(X, n, 0.2, seed=3)
    Xs = pr.p2_simplex_straight_sided(Xj, e2n)
    assert np.array_equal(Xs[:len(V)], Xj[:len(V)])
    assert np.array_equal(Xs[e2n[:, 7]], 0.5 * (Xs[e2n[:, 1]] + Xs[e2n[:, 2]]))
    X2, t6 = pr.p2_simplex_nodes(pr.grid_coords((4, 3)), pr.quads_to_tris(4, 3))
    assert t6.shape == (24, 6) and len(X2) == 20 + (4 * 4 + 5 * 3 + 12)
    assert np.array_equal(X2[t6[:, 5]], 0.5 * (X2[t6[:, 2]] + X2[t6[:, 0]]))
    fe, fl = pr.boundary_faces(2, t6)
    assert len(fe) == 14
    fe, fl = pr.boundary_faces(3, e2n)
    assert len(fe) == 2 * 2 * (3 * 2 + 2 * 2 + 3 * 2)
