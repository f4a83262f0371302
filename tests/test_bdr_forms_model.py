"""The definition of the device boundary forms (saamge_amd/elmat_model.py FACE_NODES, boundary_mass, boundary_loads) against
what is known independently of it, and problems.boundary_faces.

Errors are in units of 2^-52 of max |M_f| of the face matrix (for the loads too), the convention of test_mass_model.py.
Measured on the CPU with the meshes below, asserted with the margin of 8:

  check                                                          measured   asserted
  2-node segment = len [[1/3, 1/6], [1/6, 1/3]]                     0.50       4.0
  3-node segment = len / 30 [[4, 2, -1], [2, 16, 2], [-1, 2, 4]]    4.20      33.6
  triangle face = area / 12 (1 + delta)                             3.12      25.0
  4-node quadrilateral face = tensor product of the 2-node one      2.53      20.2
  9-node quadrilateral face = tensor product of the 3-node one      2.13      17.0
  all contributions with coef 1 sum to the surface of the box       1.33      10.6  (units of 2^-52 of the surface)
  loads with g = 1 = row sums of M_f                                3.69      29.5
  loads with random g = M_f g_f                                     3.44      27.5

The references are formed in extended precision (numpy longdouble, math.fsum), so a figure is the model's own error."""
import math

import numpy as np
import pytest

from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import bdr_forms_cases as bc
import elmat_cases as ec

MARGIN = 8
# measured (see the table above); the assertion is MARGIN times the figure
UNITS_SEG2, UNITS_SEG3, UNITS_TRI, UNITS_QUAD4, UNITS_QUAD9, UNITS_AREA, UNITS_ROW, UNITS_LOAD = 0.50, 4.20, 3.12, 2.53, 2.13, 1.33, 3.69, 3.44

SEG2_1D = np.array([[1.0, 0.5], [0.5, 1.0]], np.longdouble) / 3
SEG3_1D = np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]], np.longdouble) / 30


def _units(err, scale):
    return float(np.max(err / scale)) / ec.EPS


def _check(label, units, measured):
    print("%s: %.2f units of 2^-52 (asserted: %g)" % (label, units, MARGIN * measured))
    assert units <= MARGIN * measured


def _face_matrices(family, name, jitter, coef=None, variant="all"):
    """[(face index in the list, vertex ids of the face, its matrix M_f)]: one model call per local face index into zeros, where
    an element holds one face at most, so that the entries of the element's matrix at the face's nodes are M_f"""
    X, e2v, ep = bc.mesh(family, name, jitter)
    dim = X.shape[1]
    fe, fl = bc.faces(family, name, variant)
    c = np.ones(len(fe)) if coef is None else coef
    nd = bc.node_counts(e2v, ep)
    out = []
    for lf in np.unique(fl):
        ids = np.flatnonzero(fl == lf)
        M = em.boundary_mass(X, e2v, fe[ids], fl[ids], c[ids], elem_ptr=ep, add_to=bc.zeros(e2v, ep, 1, True))
        mats = ec.per_element(M, e2v, ep, 1)
        for f in ids:
            nodes = np.array(em.FACE_NODES[(dim, int(nd[fe[f]]))][lf])
            m = mats[fe[f]]
            rest = np.ones(m.shape, bool)
            rest[np.ix_(nodes, nodes)] = False
            assert not m[rest].any()                                 # nothing outside the face's nodes
            out.append((f, bc.face_vertices(dim, e2v, ep, fe[f:f + 1], fl[f:f + 1])[0], m[np.ix_(nodes, nodes)]))
    return X, out


def _tensor_face(p, one_d, nodes_1d):
    """the tensor-product mass of the axis-aligned segment / rectangle with the nodes p, whatever their order"""
    p = p.astype(np.longdouble)
    h = p.max(axis=0) - p.min(axis=0)
    axes = [d for d in range(p.shape[1]) if h[d] > 0]
    assert len(axes) == p.shape[1] - 1, "not an axis-aligned face"
    want = np.ones((len(p), len(p)), np.longdouble)
    for d in axes:
        idx = np.rint((p[:, d] - p[:, d].min()) / h[d] * (nodes_1d - 1)).astype(int)
        want = want * (h[d] * one_d)[np.ix_(idx, idx)]
    return want


# ---- closed forms on undeformed grids ----
@pytest.mark.parametrize("family,name,one_d,nodes_1d,fn,measured", [
    ("q1", "quads_4x3", SEG2_1D, 2, 2, "UNITS_SEG2"), ("q1", "tris_4x3", SEG2_1D, 2, 2, "UNITS_SEG2"),
    ("q2", "quad9_9x8", SEG3_1D, 3, 3, "UNITS_SEG3"), ("q2", "quad9_4x3", SEG3_1D, 3, 3, "UNITS_SEG3"),
    ("q1", "hex_5x4x3", SEG2_1D, 2, 4, "UNITS_QUAD4"), ("q1", "mixed_4", SEG2_1D, 2, 4, "UNITS_QUAD4"),
    ("q2", "hex27_5x4x3", SEG3_1D, 3, 9, "UNITS_QUAD9"), ("q2", "mixed_hex8_hex27", SEG3_1D, 3, 9, "UNITS_QUAD9")])
def test_box_faces_are_tensor_products(family, name, one_d, nodes_1d, fn, measured):
    X, faces = _face_matrices(family, name, False if family == "q1" else "box")
    worst, seen = 0.0, 0
    for _, v, m in faces:
        if len(v) != fn:
            continue
        seen += 1
        assert np.array_equal(m, m.T)
        worst = max(worst, _units(np.abs(m - _tensor_face(X[v], one_d, nodes_1d)), np.abs(m).max()))
    assert seen
    _check("%d-node face %s" % (fn, name), worst, globals()[measured])


@pytest.mark.parametrize("name,jitter", [("tets_3x2x2", False), ("tets_3x2x2", True), ("mixed_4", False)])
def test_triangle_face_is_area_over_12(name, jitter):
    """(a flat triangle: the jittered tetrahedra qualify too)"""
    X, faces = _face_matrices("q1", name, jitter)
    worst, seen = 0.0, 0
    for _, v, m in faces:
        if len(v) != 3:
            continue
        seen += 1
        p = X[v].astype(np.longdouble)
        n = np.cross(p[1] - p[0], p[2] - p[0])
        area = np.sqrt(n @ n) / 2
        worst = max(worst, _units(np.abs(m - area / 12 * (np.ones((3, 3)) + np.eye(3))), np.abs(m).max()))
    assert seen
    _check("triangle face %s %s" % (name, jitter), worst, UNITS_TRI)


@pytest.mark.parametrize("family,name,jitter", [c for c in bc.CASES if c[2] in (False, "box")],
                         ids=[i for c, i in zip(bc.CASES, bc.IDS) if c[2] in (False, "box")])
def test_contributions_sum_to_the_surface_of_the_box(family, name, jitter):
    X, faces = _face_matrices(family, name, jitter)
    ext = X.max(axis=0) - X.min(axis=0)
    blocks = 2 if name == "mixed_hex8_hex27" else 1                  # (two unit cubes side by side in one list)
    surface = blocks * (2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]) if len(ext) == 3 else 2.0 * (ext[0] + ext[1]))
    total = math.fsum(float(x) for _, _, m in faces for x in m.ravel())
    _check("surface %s" % name, abs(total - surface) / surface / ec.EPS, UNITS_AREA)


# ---- exact properties on every mesh ----
@pytest.mark.parametrize("family,name,jitter", bc.CASES, ids=bc.IDS)
def test_exact_properties(family, name, jitter):
    X, e2v, ep = bc.mesh(family, name, jitter)
    dim, NE = X.shape[1], ec.num_elements(e2v, ep)
    fe, fl = bc.faces(family, name, "interior")
    c = bc.face_coefficients(NE, fe, fl)
    rng = np.random.default_rng(31)
    # ---- symmetry, scalar and vector form
    zero1, zerod = bc.zeros(e2v, ep, 1, True), bc.zeros(e2v, ep, dim, True)
    M1 = em.boundary_mass(X, e2v, fe, fl, c, elem_ptr=ep, add_to=zero1)
    Md = em.boundary_mass(X, e2v, fe, fl, c, vdim=dim, elem_ptr=ep, add_to=zerod)
    for m, v in zip(ec.per_element(M1, e2v, ep, 1), ec.per_element(Md, e2v, ep, dim)):
        assert np.array_equal(m, m.T) and np.array_equal(v, v.T)
        for i in range(dim):
            for j in range(dim):
                blk = v[i::dim, j::dim]
                assert np.array_equal(blk, m) if i == j else (not blk.any() and not np.signbit(blk).any())
    # ---- a permuted list gives the same array (here: the list reversed and shuffled)
    for p in (np.arange(len(fe))[::-1], rng.permutation(len(fe))):
        assert np.array_equal(em.boundary_mass(X, e2v, fe[p], fl[p], c[p], elem_ptr=ep, add_to=zero1), M1)
    sa, ss = bc.faces(family, name, "all"), bc.faces(family, name, "shuffled")
    base = rng.uniform(-1.0, 1.0, zero1.shape)
    assert np.array_equal(em.boundary_mass(X, e2v, sa[0], sa[1], bc.face_coefficients(NE, *sa), elem_ptr=ep, add_to=base),
                          em.boundary_mass(X, e2v, ss[0], ss[1], bc.face_coefficients(NE, *ss), elem_ptr=ep, add_to=base))
    # ---- untouched entries keep their bits: -0.0 and NaN where no face reaches, between two components too
    touched = np.asarray(Md).ravel() != 0.0
    seeded = rng.uniform(-1.0, 1.0, zerod.shape)
    seeded[~touched] = np.where(rng.random(int((~touched).sum())) < 0.5, -0.0, np.nan)
    got = np.asarray(em.boundary_mass(X, e2v, fe, fl, c, vdim=dim, elem_ptr=ep, add_to=seeded)).ravel()
    assert touched.any() and not touched.all() and got[~touched].tobytes() == seeded[~touched].tobytes()
    assert not np.isnan(got[touched]).any()
    # ---- two calls on disjoint face sets equal one call on the union.  The faces of an element are added in ascending local
    #      face index, so the sets are split by that index: the second call then continues the order of the first
    g = rng.uniform(-1.0, 1.0, (len(X), dim))
    vec = rng.uniform(-1.0, 1.0, bc.zeros(e2v, ep, dim, False).shape)
    lo, hi = fl < 2, fl >= 2
    two = em.boundary_mass(X, e2v, fe[lo], fl[lo], c[lo], elem_ptr=ep, add_to=base)
    two = em.boundary_mass(X, e2v, fe[hi], fl[hi], c[hi], elem_ptr=ep, add_to=two)
    assert np.array_equal(two, em.boundary_mass(X, e2v, fe, fl, c, elem_ptr=ep, add_to=base))
    two = em.boundary_loads(X, e2v, fe[lo], fl[lo], g, vdim=dim, coef=c[lo], elem_ptr=ep, add_to=vec)
    two = em.boundary_loads(X, e2v, fe[hi], fl[hi], g, vdim=dim, coef=c[hi], elem_ptr=ep, add_to=two)
    assert np.array_equal(two, em.boundary_loads(X, e2v, fe, fl, g, vdim=dim, coef=c, elem_ptr=ep, add_to=vec))
    # ---- the loads without a coefficient are those with coefficient 1
    assert np.array_equal(em.boundary_loads(X, e2v, fe, fl, g[:, 0], elem_ptr=ep, add_to=vec[:len(vec) // dim]),
                          em.boundary_loads(X, e2v, fe, fl, g[:, 0], coef=np.ones(len(fe)), elem_ptr=ep, add_to=vec[:len(vec) // dim]))


@pytest.mark.parametrize("family,name,jitter", [c for c in bc.CASES if c[2] not in (False, "box")],
                         ids=[i for c, i in zip(bc.CASES, bc.IDS) if c[2] not in (False, "box")])
def test_loads_are_the_face_matrix_times_g(family, name, jitter):
    X, e2v, ep = bc.mesh(family, name, jitter)
    dim, NE = X.shape[1], ec.num_elements(e2v, ep)
    fe, fl = bc.faces(family, name, "all")
    c = bc.face_coefficients(NE, fe, fl)
    _, faces = _face_matrices(family, name, jitter, coef=c)
    nd = bc.node_counts(e2v, ep)
    off = np.concatenate([[0], np.cumsum(nd)])
    g = np.random.default_rng(37).uniform(-1.0, 1.0, (len(X), dim))
    worst_row, worst_load = 0.0, 0.0
    for lf in np.unique(fl):
        ids = np.flatnonzero(fl == lf)
        ones = np.ravel(em.boundary_loads(X, e2v, fe[ids], fl[ids], np.ones(len(X)), coef=c[ids], elem_ptr=ep, add_to=bc.zeros(e2v, ep, 1, False)))
        vec = np.ravel(em.boundary_loads(X, e2v, fe[ids], fl[ids], g, vdim=dim, coef=c[ids], elem_ptr=ep, add_to=bc.zeros(e2v, ep, dim, False)))
        for f, v, m in faces:
            if fl[f] != lf:
                continue
            nodes = np.array(em.FACE_NODES[(dim, int(nd[fe[f]]))][lf])
            scale = np.abs(m).max()
            rows = np.array([math.fsum(r) for r in m])
            worst_row = max(worst_row, _units(np.abs(ones[off[fe[f]] + nodes] - rows), scale))
            for i in range(dim):
                want = np.array([math.fsum(float(x) for x in m[a].astype(np.longdouble) * g[v, i].astype(np.longdouble)) for a in range(len(v))])
                worst_load = max(worst_load, _units(np.abs(vec[(off[fe[f]] + nodes) * dim + i] - want), scale))
    _check("row sums %s %s" % (name, jitter), worst_row, UNITS_ROW)
    _check("M_f g_f %s %s" % (name, jitter), worst_load, UNITS_LOAD)


# ---- refusals of the model ----
def test_refusals():
    X, e2v, _ = ec.mesh("hex_5x4x3")
    NE, NV = len(e2v), len(X)
    fe, fl = bc.faces("q1", "hex_5x4x3", "shuffled")
    one, K, b = np.ones(len(fe)), np.zeros((NE, 8, 8)), np.zeros((NE, 8))
    with pytest.raises(ValueError, match="vdim"):
        em.boundary_mass(X, e2v, fe, fl, one, vdim=2, add_to=K)
    with pytest.raises(ValueError, match="coef"):
        em.boundary_mass(X, e2v, fe, fl, None, add_to=K)
    with pytest.raises(ValueError, match="g:"):
        em.boundary_loads(X, e2v, fe, fl, None, add_to=b)
    with pytest.raises(ValueError, match="add_to"):
        em.boundary_mass(X, e2v, fe, fl, one)
    with pytest.raises(ValueError, match="add_to"):
        em.boundary_loads(X, e2v, fe, fl, np.ones(NV), add_to=np.zeros(5))
    with pytest.raises(ValueError, match="out of range"):
        em.boundary_mass(X, np.where(e2v == 3, NV, e2v), fe, fl, one, add_to=K)
    wrong = fe.copy()
    wrong[[40, 11]] = [NE, -1]
    with pytest.raises(em.FaceError, match=r"face 11: face_elem is outside \[0, NE\)") as err:
        em.boundary_mass(X, e2v, wrong, fl, one, add_to=K)
    assert err.value.face == 11
    wrong = fl.copy()
    wrong[[60, 9]] = [6, -1]
    with pytest.raises(em.FaceError, match="face 9: face_local is outside the element type's range"):
        em.boundary_loads(X, e2v, fe, wrong, np.ones(NV), add_to=b)
    twice_e, twice_l = fe.copy(), fl.copy()
    twice_e[[50, 81]], twice_l[[50, 81]] = [fe[20], fe[33]], [fl[20], fl[33]]
    with pytest.raises(em.FaceError, match="face 20: the same") as err:
        em.boundary_mass(X, e2v, twice_e, twice_l, one, add_to=K)
    assert err.value.face == 20
    flat = X.copy()
    for f in (31, 12):
        v = bc.face_vertices(3, e2v, None, fe[f:f + 1], fl[f:f + 1])[0]
        flat[v] = flat[v[0]]
    for call in (lambda: em.boundary_mass(flat, e2v, fe, fl, one, add_to=K), lambda: em.boundary_loads(flat, e2v, fe, fl, np.ones(NV), add_to=b)):
        with pytest.raises(em.FaceError, match="face 12: the measure is not positive") as err:
            call()
        assert err.value.face == 12
    Xt, t2v, _ = ec.mesh("tets_3x2x2")
    with pytest.raises(em.FaceError, match="face 0: face_local"):                                    # a tetrahedron has four faces
        em.boundary_mass(Xt, t2v, [0], [4], [1.0], add_to=np.zeros((len(t2v), 4, 4)))


def test_hex27_faces_are_the_hexahedron_faces_with_their_nine_nodes():
    corner = {tuple(2 * np.array(l)): k for k, l in enumerate(em.HEX_LOC)}
    for face8, face27 in zip(em.FACE_NODES[(3, 8)], em.FACE_NODES[(3, 27)]):
        assert len(set(face27)) == 9
        pos = np.array([em.Q2_HEX_LOC[k] for k in face27])
        assert [corner[tuple(p)] for p in pos[:4]] == list(face8)                                    # the corners, in order
        assert np.array_equal(2 * pos[4:8], pos[[0, 1, 2, 3]] + pos[[1, 2, 3, 0]])                    # the edge midpoints
        assert np.array_equal(4 * pos[8], pos[:4].sum(axis=0))                                       # the centre
    for key, faces in em.FACE_NODES.items():                                                         # every node of a type lies on a face or inside
        assert all(0 <= k < key[1] for f in faces for k in f)


# ---- problems.boundary_faces ----
@pytest.mark.parametrize("family,name", sorted({(c[0], c[1]) for c in bc.CASES}))
def test_boundary_faces_are_the_hull(family, name):
    X, e2v, ep = bc.box_mesh(family, name)
    dim = X.shape[1]
    fe, fl = pr.boundary_faces(dim, e2v, ep)
    assert fe.dtype == np.int32 and fl.dtype == np.int32
    key = fe.astype(np.int64) * em.MAX_FACES + fl
    assert np.all(np.diff(key) > 0)                                                                  # ascending by (element, local face)
    lo, hi = X.min(axis=0), X.max(axis=0)
    for v in bc.face_vertices(dim, e2v, ep, fe, fl):
        assert any(np.all(X[v, d] == lo[d]) or np.all(X[v, d] == hi[d]) for d in range(dim))         # every face on the hull
    counts = {"hex_3x2x2": 32, "hex_5x4x3": 94, "hex_9x8x7": 382, "quads_4x3": 14, "tris_4x3": 14, "tets_3x2x2": 64,
              "hex27_3x2x2": 32, "hex27_5x4x3": 94, "hex27_7x3x3": 102, "quad9_4x3": 14, "quad9_9x8": 34,
              "mixed_hex8_hex27": 32 + 14}                                                           # 2 (ab + bc + ca), 2 (a + b); two per cell face for tets
    if name in counts:
        assert len(fe) == counts[name]
