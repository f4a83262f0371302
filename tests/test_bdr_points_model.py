"""The model of the boundary data at the face points (saamge_amd/elmat_model.py: boundary_points, boundary_eval,
boundary_mass_points, boundary_loads_points) on the CPU: the normals point out of the owning element for all nine element types,
the surface of every mesh is closed and encloses the mesh's volume, a linear field has its gradient and its trace on affine
elements, the calls at the points reduce to the calls per face bit for bit, a permuted list permutes the point arrays by whole
faces, and every refusal names its face.

The bounds.  EPS = 2^-52 is twice the unit roundoff u.  A quantity computed as sums of products of the inputs differs from its exact
value by at most (d u) / (1 - d u) times THE SAME EXPRESSION WITH EVERY PRODUCT TAKEN IN ABSOLUTE VALUE, d the number of roundings on
the longest path from an input to the result (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 and Lemma 3.3);
the tests form that expression (`_abs_faces`, `_abs_volume`) and use d EPS times it, which is twice the bound.  Totals are formed
with math.fsum, which adds one rounding."""
import math

import numpy as np
import pytest

from saamge_amd import elmat_model as em

import bdr_forms_cases as bc
import bdr_points_cases as bp
import elmat_cases as ec

EPS = 2.0 ** -52


def _lists(X, e2v, ep):
    """(nd, offsets, flat vertex lists) as int64"""
    _, _, ep64, flat, nd = em._mesh(X, e2v, ep)
    return nd, ep64, flat


def _abs_faces(X, e2v, ep, fe, fl, fp):
    """Per face point, with every product in absolute value: w * n (NFQ, dim), the expression of wmeas * normal without the two
    roundings of meas that cancel; x_q (NFQ, dim); and the largest node count of a listed face."""
    dim = X.shape[1]
    nd, off, flat = _lists(X, e2v, ep)
    A = np.abs(X)
    wn, xa, fnmax = np.zeros((fp[-1], dim)), np.zeros((fp[-1], dim)), 0
    fe, fl = fe.astype(np.int64), fl.astype(np.int64)
    for lf, c, ids in em._face_buckets(dim, nd, fe, fl):
        nodes = np.array(em.FACE_NODES[(dim, c)][lf])
        fnmax = max(fnmax, len(nodes))
        Af = A[flat[off[fe[ids]][:, None] + nodes]]
        for q, (N, dN, w) in enumerate(em.face_rule(dim, len(nodes))):
            t = np.einsum("nci,cj->nji", Af, np.abs(np.array(dN)))
            if dim == 2:
                n = np.stack([t[:, 0, 1], t[:, 0, 0]], axis=1)
            else:
                a, b = t[:, 0], t[:, 1]
                n = np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                              a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], axis=1)
            wn[fp[ids] + q] = w * n
            xa[fp[ids] + q] = np.einsum("c,nci->ni", np.abs(np.array(N)), Af)
    return wn, xa, fnmax


def _abs_jacobians(X, e2v, ep, points):
    """yields (node count, element ids, vertex lists, q, dN, |J| (n, dim, dim) with every product in absolute value) over the
    types and `points(dim, c)` -> [(q, dN)]"""
    nd, off, flat = _lists(X, e2v, ep)
    for c, ids, v in em._types(nd, off, flat):
        A = np.abs(X[v])
        for q, dN in points(X.shape[1], c):
            yield c, ids, v, q, dN, np.einsum("nai,aj->nij", A, np.abs(np.array(dN)))


def _permanent(J):
    if J.shape[1] == 2:
        return J[:, 0, 0] * J[:, 1, 1] + J[:, 0, 1] * J[:, 1, 0]
    return sum(J[:, 0, i] * J[:, 1, j] * J[:, 2, k] for i, j, k in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)))


def _abs_volume(X, e2v, ep):
    """the sum over the points of the mass rule of w * det with every product in absolute value, and the largest node count"""
    rule = lambda dim, c: [(q, em.mass_reference_gradients(dim, c, q)) for q in range(em.MASS_NPOINTS[(dim, c)])]
    total, ndmax = [], 0
    for c, _, _, q, _, J in _abs_jacobians(X, e2v, ep, rule):
        total.append(em.mass_point_weight(X.shape[1], c, q) * _permanent(J))
        ndmax = max(ndmax, c)
    return math.fsum(np.concatenate(total)), ndmax


def _centroids(X, e2v, ep, fe):
    nd, off, flat = _lists(X, e2v, ep)
    return np.array([X[flat[off[e]:off[e + 1]]].mean(axis=0) for e in fe])


STRAIGHT = [c for c in bp.CASES if bp.is_straight(c[0], c[2])]


OUTWARD_LIST = "interior"      # the boundary faces and a few interior ones: the list both tests below run on


@pytest.mark.parametrize("family,name,jitter", STRAIGHT, ids=["%s-%s" % (c[1], c[2]) for c in STRAIGHT])
def test_normals_are_unit_and_point_out_of_the_owning_element(family, name, jitter):
    """n_q . (x_q - centroid of the owning element) > 0 at every point of every face of the OUTWARD_LIST list, boundary or
    interior; test_every_local_face_has_been_held_outward holds that these lists reach every local face of every type.  |n| = 1:
    m2 takes 2 dim - 1 roundings, the root halves them and adds one, the division one more per component, so
    | |n| - 1 | <= (dim + 2) u < (dim + 2) EPS."""
    X, e2v, ep = bp.mesh(family, name, jitter)
    dim = X.shape[1]
    fe, fl = bp.faces(family, name, OUTWARD_LIST)
    w = bp.model(family, name, jitter, OUTWARD_LIST)
    c = np.repeat(_centroids(X, e2v, ep, fe), np.diff(w["fp"]), axis=0)
    assert (((w["xq"] - c) * w["normal"]).sum(axis=1) > 0.0).all()
    assert (np.abs(np.sqrt((w["normal"] ** 2).sum(axis=1)) - 1.0) <= (dim + 2) * EPS).all()
    assert (w["wmeas"] > 0.0).all()


def test_every_local_face_has_been_held_outward():
    """The faces the outward test runs on -- the same lists, with the model's own point offsets, one rule's points per face --
    reach all 39 (dimension, nodes, local face) triples of FACE_NODES, so no line of the face tables is left to a check by hand."""
    seen = set()
    for family, name, jitter in STRAIGHT:
        X, e2v, ep = bp.mesh(family, name, jitter)
        nd = bc.node_counts(e2v, ep)
        fe, fl = bp.faces(family, name, OUTWARD_LIST)
        fp = bp.model(family, name, jitter, OUTWARD_LIST)["fp"]
        assert len(fp) == len(fe) + 1
        for f, (e, l) in enumerate(zip(fe, fl)):
            key = (X.shape[1], int(nd[e]), int(l))
            assert fp[f + 1] - fp[f] == em.FACE_NPOINTS[(key[0], len(em.FACE_NODES[key[:2]][key[2]]))]
            seen.add(key)
    assert seen == {(dim, c, lf) for (dim, c), f in em.FACE_NODES.items() for lf in range(len(f))} and len(seen) == 39


@pytest.mark.parametrize("family,name,jitter", STRAIGHT, ids=["%s-%s" % (c[1], c[2]) for c in STRAIGHT])
def test_the_two_sides_of_an_interior_face_cancel(family, name, jitter):
    """The interior faces of the "interior" list and the same faces seen from the element across: per face, sum_q wmeas n of the
    two sides is zero to rounding.  Each side: d = 2 FN (a tangent) + 2 (a product, the difference) + 3 (/ meas, w * meas, the
    product with n; the roundings of meas itself cancel) + 1 (fsum)."""
    X, e2v, ep = bp.mesh(family, name, jitter)
    dim = X.shape[1]
    nd, off, flat = _lists(X, e2v, ep)
    outer = set(zip(*[a.tolist() for a in bp.faces(family, name, "all")]))
    fe, fl = bp.faces(family, name, "interior")
    inner = [(int(e), int(l)) for e, l in zip(fe, fl) if (int(e), int(l)) not in outer]
    assert inner
    by_vertices = {}
    for e in range(len(nd)):
        for l, nodes in enumerate(em.FACE_NODES[(dim, int(nd[e]))]):
            by_vertices.setdefault(tuple(sorted(flat[off[e] + np.array(nodes)].tolist())), []).append((e, l))
    pairs = []
    for e, l in inner:
        both = by_vertices[tuple(sorted(flat[off[e] + np.array(em.FACE_NODES[(dim, int(nd[e]))][l])].tolist()))]
        if len(both) == 2:      # (a 4-node face against a 9-node face of the mixed mesh has other nodes: no twin by this key)
            pairs.append(((e, l), [p for p in both if p != (e, l)][0]))
    assert pairs
    sides = []
    for k in (0, 1):
        se, sl = np.array([p[k][0] for p in pairs], np.int32), np.array([p[k][1] for p in pairs], np.int32)
        fp, _, wmeas, normal = em.boundary_points(X, e2v, se, sl, elem_ptr=ep)
        wn, _, fnmax = _abs_faces(X, e2v, ep, se, sl, fp)
        sides.append((fp, wmeas[:, None] * normal, wn, fnmax))
    for f in range(len(pairs)):
        for i in range(dim):
            terms, bound = [], 0.0
            for fp, v, wn, fnmax in sides:
                terms += v[fp[f]:fp[f + 1], i].tolist()
                bound += (2 * fnmax + 6) * EPS * math.fsum(wn[fp[f]:fp[f + 1], i])
            assert abs(math.fsum(terms)) <= bound, (pairs[f], i)


@pytest.mark.parametrize("family,name,jitter", bp.CASES, ids=bp.IDS)
def test_the_surface_is_closed_and_encloses_the_volume(family, name, jitter):
    """sum wmeas n = 0 and sum wmeas (x_q . n_q) = dim sum wdet, curved meshes included: the rules integrate both integrands
    exactly (2-point Gauss on bilinear faces, 3-point on 9-node faces and 3-node segments, the degree-4 rule on 6-node triangles).
    Roundings: wmeas n takes d1 = 2 FN + 6 (above); x_q . n_q adds FN + 1 (x_q) and dim (the dot): d2 = 3 FN + dim + 7; w det takes
    2 ND (an entry of J) + 5 (cofactor, the det's products and sums) + 1 (w) + 1 (fsum) + 1 (times dim): d3 = 2 ND + 8."""
    X, e2v, ep = bp.mesh(family, name, jitter)
    dim = X.shape[1]
    fe, fl = bp.faces(family, name, "all")
    w = bp.model(family, name, jitter, "all")
    wn, xa, fn = _abs_faces(X, e2v, ep, fe, fl, w["fp"])
    flux = w["wmeas"][:, None] * w["normal"]
    for i in range(dim):
        assert abs(math.fsum(flux[:, i])) <= (2 * fn + 6) * EPS * math.fsum(wn[:, i]), i
    _, _, wdet = em.element_points(X, e2v, elem_ptr=ep)
    vol_abs, ndmax = _abs_volume(X, e2v, ep)
    lhs = math.fsum((w["wmeas"] * (w["xq"] * w["normal"]).sum(axis=1)).tolist())
    rhs = dim * math.fsum(wdet.tolist())
    bound = (3 * fn + dim + 7) * EPS * math.fsum((xa * wn).sum(axis=1).tolist()) + (2 * ndmax + 8) * EPS * dim * vol_abs
    assert abs(lhs - rhs) <= bound and rhs > 0.0


BOX = [c for c in bp.CASES if bp.is_box(c[0], c[2])]


@pytest.mark.parametrize("family,name,jitter", BOX, ids=["%s-%s" % (c[1], c[2]) for c in BOX])
def test_linear_field_on_affine_elements(family, name, jitter):
    """u = a . x + b at the nodes: gradq = a and the trace is a . x_q + b.  The gradient's entry j is (sum_k r[k] C[j][k]) / det:
    r[k] takes 2 ND roundings and dim + 1 more from forming u at the nodes, C[j][k] 2 ND + 2, the dot dim, the division 1, and the
    relative error of det (2 ND + 8) enters once more: d = 6 ND + 2 dim + 12, against the same expression in absolute values
    divided by det.  The trace takes FN + 1 roundings on each side and dim + 1 for u: d = 2 FN + dim + 3 against
    sum_c |N_c| (sum_i |a_i x_c[i]| + |b|)."""
    X, e2v, ep = bp.mesh(family, name, jitter)
    dim = X.shape[1]
    a, b = np.array([1.25, -0.75, 0.5])[:dim], 0.375
    u = X @ a + b
    uabs = np.abs(X) @ np.abs(a) + abs(b)
    fe, fl = bp.faces(family, name, "all")
    fp = bp.model(family, name, jitter, "all")["fp"]
    xq = bp.model(family, name, jitter, "all")["xq"]
    uq, gq = em.boundary_eval(X, e2v, fe, fl, u, elem_ptr=ep)
    nd, off, flat = _lists(X, e2v, ep)
    fe64, fl64 = fe.astype(np.int64), fl.astype(np.int64)
    checked = 0
    for lf, c, ids in em._face_buckets(dim, nd, fe64, fl64):
        nodes = np.array(em.FACE_NODES[(dim, c)][lf])
        ve = flat[off[fe64[ids]][:, None] + np.arange(c)]
        A, U = np.abs(X[ve]), uabs[ve]
        for q, (N, _, _) in enumerate(em.face_rule(dim, len(nodes))):
            dN = np.abs(np.array(em.face_gradients(dim, c, lf, q)))
            J = np.einsum("nai,aj->nij", A, dN)
            r = np.einsum("na,ak->nk", U, dN)
            if dim == 2:
                C = np.stack([np.stack([J[:, 1, 1], J[:, 1, 0]], 1), np.stack([J[:, 0, 1], J[:, 0, 0]], 1)], 1)
            else:
                C = np.zeros_like(J)
                for i in range(3):
                    for j in range(3):
                        (i1, i2), (j1, j2) = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
                        C[:, i, j] = J[:, i1, j1] * J[:, i2, j2] + J[:, i1, j2] * J[:, i2, j1]
            det = _det(X[ve], dim, c, lf, q)
            gabs = np.einsum("nk,njk->nj", r, C) / det[:, None]
            tol = (6 * c + 2 * dim + 12) * EPS * gabs
            assert (np.abs(gq[fp[ids] + q, 0, :] - a[None, :]) <= tol).all(), (lf, c, q)
            tabs = np.abs(np.array(N)) @ uabs[flat[off[fe64[ids]][:, None] + nodes]].T
            assert (np.abs(uq[fp[ids] + q, 0] - (xq[fp[ids] + q] @ a + b)) <= (2 * len(nodes) + dim + 3) * EPS * tabs).all()
            checked += len(ids)
    assert checked == fp[-1]


def _det(Xe, dim, c, lf, q):
    """the model's determinant of the elements Xe (n, c, dim) at point q of local face lf"""
    dN = em.face_gradients(dim, c, lf, q)
    J = [[sum(Xe[:, a, i] * dN[a][j] for a in range(c)) for j in range(dim)] for i in range(dim)]
    return em._cofactors(J, dim)[1]


@pytest.mark.parametrize("family,name,jitter", bp.CASES, ids=bp.IDS)
def test_bit_identities(family, name, jitter):
    X, e2v, ep = bp.mesh(family, name, jitter)
    dim, NE = X.shape[1], ec.num_elements(e2v, ep)
    g1, gd = bc.nodal_data(len(X), dim)
    rng = np.random.default_rng(41)
    got = {}
    for variant in bp.VARIANTS:
        fe, fl = bp.faces(family, name, variant)
        w = bp.model(family, name, jitter, variant)
        fp = w["fp"]
        assert np.array_equal(fp, bp.offsets(dim, e2v, ep, fe, fl)) and fp.dtype == np.int64
        c = bc.face_coefficients(NE, fe, fl)
        for vdim, g, uq in ((1, g1, w["uq1"]), (dim, gd, w["uqd"])):
            # equal coefficients at the points of each face: the bits of boundary_mass
            K = rng.uniform(-1.0, 1.0, bc.zeros(e2v, ep, vdim, True).shape)
            want = em.boundary_mass(X, e2v, fe, fl, c, vdim=vdim, elem_ptr=ep, add_to=K)
            assert np.array_equal(em.boundary_mass_points(X, e2v, fe, fl, np.repeat(c, np.diff(fp)), vdim=vdim, elem_ptr=ep, add_to=K), want)
            # the trace of a nodal g as point data: the bits of boundary_loads
            b = rng.uniform(-1.0, 1.0, bc.zeros(e2v, ep, vdim, False).shape)
            want = em.boundary_loads(X, e2v, fe, fl, g, vdim=vdim, coef=c, elem_ptr=ep, add_to=b)
            assert np.array_equal(em.boundary_loads_points(X, e2v, fe, fl, uq, vdim=vdim, coef=c, elem_ptr=ep, add_to=b), want)
        # point data of its own
        K0, b0 = bc.zeros(e2v, ep, 1, True), bc.zeros(e2v, ep, dim, False)
        got[variant] = (em.boundary_mass_points(X, e2v, fe, fl, w["cq"], elem_ptr=ep, add_to=K0),
                        em.boundary_loads_points(X, e2v, fe, fl, w["gqd"], vdim=dim, coef=c, elem_ptr=ep, add_to=b0))
    # a permuted list: the point arrays move by whole faces, the matrices and the vectors keep their bits
    a, s = bp.model(family, name, jitter, "all"), bp.model(family, name, jitter, "shuffled")
    at = bp.whole_faces(*bp.faces(family, name, "all"), a["fp"], *bp.faces(family, name, "shuffled"), s["fp"])
    assert len(at) == a["fp"][-1] and not np.array_equal(at, np.arange(len(at)))
    for key in ("xq", "wmeas", "normal", "uq1", "gradq1", "uqd", "gradqd", "cq", "gqd"):
        assert a[key][at].tobytes() == s[key].tobytes(), key
    assert got["all"][0].tobytes() == got["shuffled"][0].tobytes() and got["all"][1].tobytes() == got["shuffled"][1].tobytes()
    assert np.any(got["all"][0] != 0.0) and np.any(got["all"][1] != 0.0)


def test_refusals_name_the_face():
    X, e2v, _ = ec.mesh("hex_5x4x3")
    NE, NV = len(e2v), len(X)
    fe, fl = bc.faces("q1", "hex_5x4x3", "shuffled")
    NF = len(fe)
    fp = bp.offsets(3, e2v, None, fe, fl)
    cq, gq, u = np.ones(fp[-1]), np.ones(fp[-1]), np.ones(NV)
    K, b = np.zeros((NE, 8, 8)), np.zeros((NE, 8))

    def calls(coords=X, lists=e2v, face_elem=fe, face_local=fl, n=None):
        n = fp[-1] if n is None else n
        return [lambda: em.boundary_points(coords, lists, face_elem, face_local),
                lambda: em.boundary_eval(coords, lists, face_elem, face_local, u),
                lambda: em.boundary_eval(coords, lists, face_elem, face_local, u, grad=False),
                lambda: em.boundary_mass_points(coords, lists, face_elem, face_local, cq[:n], add_to=K),
                lambda: em.boundary_loads_points(coords, lists, face_elem, face_local, gq[:n], add_to=b)]

    def all_refuse(match, face, **kw):
        for call in calls(**kw):
            with pytest.raises(em.FaceError, match=match) as err:
                call()
            assert err.value.face == face
    # the arguments alone, before the mesh is looked at
    bad_mesh = np.where(e2v == 7, NV, e2v)
    for call in (lambda: em.boundary_eval(X, bad_mesh, fe, fl, u, vdim=2),
                 lambda: em.boundary_mass_points(X, bad_mesh, fe, fl, cq, vdim=2, add_to=K),
                 lambda: em.boundary_loads_points(X, bad_mesh, fe, fl, gq, vdim=2, add_to=b)):
        with pytest.raises(ValueError, match="vdim"):
            call()
    for call, what in ((lambda: em.boundary_points(X, bad_mesh, fe, None), "face_elem and face_local"),
                       (lambda: em.boundary_eval(X, bad_mesh, fe, fl, None), "u: "),
                       (lambda: em.boundary_mass_points(X, bad_mesh, fe, fl, None, add_to=K), "coefq: "),
                       (lambda: em.boundary_loads_points(X, bad_mesh, fe, fl, None, add_to=b), "gq: ")):
        with pytest.raises(ValueError, match=what):
            call()
    # the mesh
    for call in calls(lists=bad_mesh):
        with pytest.raises(ValueError, match="out of range"):
            call()
    # the face list: the lowest offending index of the list
    wrong = fe.copy()
    wrong[[40, 11, 77]] = [NE, -1, NE + 5]
    all_refuse(r"face 11: face_elem is outside \[0, NE\)", 11, face_elem=wrong)
    wrong = fl.copy()
    wrong[[60, 9]] = [6, -1]
    all_refuse("face 9: face_local is outside the element type's range", 9, face_local=wrong)
    twice_e, twice_l = fe.copy(), fl.copy()
    twice_e[[50, 81]], twice_l[[50, 81]] = [fe[20], fe[33]], [fl[20], fl[33]]
    all_refuse("face 20: the same \\(element, local face\\) is listed twice", 20, face_elem=twice_e, face_local=twice_l)
    # data of the wrong size, after the list
    for call in calls(n=fp[-1] - 1)[3:]:
        with pytest.raises(ValueError, match="is needed"):
            call()
    # a measure that is not positive: faces 31 and 12 shrink to a point each; the lower index is named
    flat = X.copy()
    for f in (31, 12):
        v = bc.face_vertices(3, e2v, None, fe[f:f + 1], fl[f:f + 1])[0]
        flat[v] = flat[v[0]]
    all_refuse("face 12: the measure is not positive", 12, coords=flat)
    # an element turned inside out keeps the measures of its faces: only eval refuses, with or without the gradient, and names
    # the lowest face of the list that the element owns
    turned = e2v.copy()
    e = int(fe[25])
    turned[e] = e2v[e][[4, 5, 6, 7, 0, 1, 2, 3]]
    owned = int(np.flatnonzero(fe == e)[0])
    em.boundary_points(X, turned, fe, fl)
    em.boundary_mass_points(X, turned, fe, fl, cq, add_to=K)
    for grad in (True, False):
        with pytest.raises(em.FaceError, match="face %d: the Jacobian determinant of the element is not positive" % owned) as err:
            em.boundary_eval(X, turned, fe, fl, u, grad=grad)
        assert err.value.face == owned
    # the measure is refused before the determinant
    with pytest.raises(em.FaceError, match="face 12: the measure is not positive"):
        em.boundary_eval(flat, turned, fe, fl, u)
