"""The definition of the device mass matrices, load vectors and right-hand side assembly (saamge_amd/elmat_model.py
element_mass / element_loads, saamge_amd/assemble_model.py assemble_rhs) against what is known independently of it.

Errors are in units of 2^-52 of max |M_e| (of the element's mass matrix for the loads too), the convention of test_elmat_model.py.  Measured on
the CPU with the meshes below, asserted with the margin of 8:

  check                                                      measured   asserted
  P1 triangle mass = area / 12 (1 + delta), jittered            1.67      13.4
  P1 tetrahedron mass = vol / 20 (1 + delta), jittered          3.63      29.0
  Q1 box mass = tensor product of h [[1/3, 1/6], ...]           4.41      35.3
  Q2 box mass = tensor product of h / 30 [[4, 2, -1], ...]      4.01      32.1
  sum of all entries = sum_q (w det) c                         53.93     431.4
  loads with src = 1 = row sums of M_e                         11.03      88.2
  loads with random src = M_e src_e                             3.97      31.8

The references are formed in extended precision (numpy longdouble, math.fsum), so a figure is the model's own error.  The two
large ones are no accumulation of roundings: the rounded Gauss points give sum_a N_a = 1 + 2^-52 at every point of the tensor
rules, so the entries sum to (1 + 2^-52)^2 times the weighted volume, and that volume is 27 times the largest entry of a
Q1 hexahedron (hex_3x2x2: 54 units expected, 53.93 measured; a row sum is 8 / 27 of it).
"""
import math

import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import elmat_model as em

import elmat_cases as ec
import elmat_q2_cases as qc

MARGIN = 8
# measured (see the table above); the assertion is MARGIN times the figure
UNITS_TRI, UNITS_TET, UNITS_Q1, UNITS_Q2, UNITS_SUM, UNITS_ROW, UNITS_LOAD = 1.67, 3.63, 4.41, 4.01, 53.93, 11.03, 3.97

Q1_CASES = [(name, jit) for name in ec.MESHES for jit in (False, True)]
Q2_CASES = [(name, jit) for name in qc.MESHES for jit in qc.JITTERS]
ALL_CASES = [("q1",) + c for c in Q1_CASES] + [("q2",) + c for c in Q2_CASES]
ALL_IDS = ["%s-%s" % (c[1], c[2]) for c in ALL_CASES]


def _mesh(family, name, jitter):
    return ec.mesh(name, jitter) if family == "q1" else qc.mesh(name, jitter)


def _lists(e2v, ep):
    """the node lists of the elements, one array each"""
    if ep is None:
        return [np.asarray(v) for v in e2v]
    return [np.asarray(e2v[ep[e]:ep[e + 1]]) for e in range(len(ep) - 1)]


def _coef(NE, seed=11):
    return np.random.default_rng(seed).uniform(0.5, 2.0, NE)


def _units(err, scale):
    """the references are formed in extended precision, so the figure is the model's own error"""
    return float(np.max(err / scale)) / ec.EPS


def _check(label, units, measured):
    print("%s: %.2f units of 2^-52 (asserted: %g)" % (label, units, MARGIN * measured))
    assert units <= MARGIN * measured


_mass = {}


def _model_mass(family, name, jitter, vdim=1):
    key = (family, name, jitter, vdim)
    if key not in _mass:
        X, e2v, ep = _mesh(family, name, jitter)
        c = _coef(ec.num_elements(e2v, ep))
        M = em.element_mass(X, e2v, c, vdim=vdim, elem_ptr=ep)
        M.setflags(write=False)
        _mass[key] = (M, c)
    return _mass[key]


# ---- closed forms ----
def test_p1_triangle_mass_is_area_over_12():
    X, e2v, ep = ec.mesh("tris_4x3", True)
    M, c = _model_mass("q1", "tris_4x3", True)
    worst = 0.0
    for e, v in enumerate(e2v):
        p = X[v].astype(np.longdouble)
        area = 0.5 * ((p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0]))
        want = c[e] * area / 12.0 * (np.ones((3, 3)) + np.eye(3))
        worst = max(worst, _units(np.abs(M[e] - want), np.abs(M[e]).max()))
    _check("P1 triangle", worst, UNITS_TRI)


def test_p1_tetrahedron_mass_is_volume_over_20():
    X, e2v, ep = ec.mesh("tets_3x2x2", True)
    M, c = _model_mass("q1", "tets_3x2x2", True)
    worst = 0.0
    for e, v in enumerate(e2v):
        p = X[v].astype(np.longdouble)
        d = p[1:] - p[0]
        vol = (d[0, 0] * (d[1, 1] * d[2, 2] - d[1, 2] * d[2, 1]) - d[0, 1] * (d[1, 0] * d[2, 2] - d[1, 2] * d[2, 0])
               + d[0, 2] * (d[1, 0] * d[2, 1] - d[1, 1] * d[2, 0])) / 6.0
        want = c[e] * vol / 20.0 * (np.ones((4, 4)) + np.eye(4))
        worst = max(worst, _units(np.abs(M[e] - want), np.abs(M[e]).max()))
    _check("P1 tetrahedron", worst, UNITS_TET)


def _box_mass(p, loc, one_d, nodes_1d):
    """the tensor-product mass of the axis-aligned box with the nodes p in the type's order loc"""
    dim = p.shape[1]
    p = p.astype(np.longdouble)
    h = p.max(axis=0) - p.min(axis=0)
    ref = (p - p.min(axis=0)) / h * (nodes_1d - 1)
    assert np.array_equal(np.rint(ref).astype(int), np.asarray(loc)), "not an axis-aligned box in the type's node order"
    want = np.ones((len(loc), len(loc)), np.longdouble)
    for d in range(dim):
        idx = [l[d] for l in loc]
        want = want * (h[d] * one_d)[np.ix_(idx, idx)]
    return want


Q1_1D = np.array([[1.0, 0.5], [0.5, 1.0]], np.longdouble) / 3
Q2_1D = np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]], np.longdouble) / 30


@pytest.mark.parametrize("name,loc", [("hex_5x4x3", em.HEX_LOC), ("quads_4x3", em.QUAD_LOC)])
def test_q1_box_mass_is_the_tensor_product(name, loc):
    X, e2v, ep = ec.mesh(name, False)
    M, c = _model_mass("q1", name, False)
    worst = 0.0
    for e, v in enumerate(e2v):
        want = c[e] * _box_mass(X[v], loc, Q1_1D, 2)
        worst = max(worst, _units(np.abs(M[e] - want), np.abs(M[e]).max()))
    _check("Q1 box " + name, worst, UNITS_Q1)


@pytest.mark.parametrize("name,loc", [("hex27_5x4x3", em.Q2_HEX_LOC), ("quad9_9x8", em.Q2_QUAD_LOC)])
def test_q2_box_mass_is_the_tensor_product(name, loc):
    X, e2v, ep = qc.mesh(name, "box")
    M, c = _model_mass("q2", name, "box")
    worst = 0.0
    for e, v in enumerate(e2v):
        want = c[e] * _box_mass(X[v], loc, Q2_1D, 3)
        worst = max(worst, _units(np.abs(M[e] - want), np.abs(M[e]).max()))
    _check("Q2 box " + name, worst, UNITS_Q2)


# ---- properties on every mesh ----
@pytest.mark.parametrize("family,name,jitter", ALL_CASES, ids=ALL_IDS)
def test_entries_sum_to_the_weighted_volume_and_symmetry_is_exact(family, name, jitter):
    """partition of unity: sum_ab M_ab = sum_q (w det) c, curved elements included"""
    X, e2v, ep = _mesh(family, name, jitter)
    M, c = _model_mass(family, name, jitter)
    dim = X.shape[1]
    worst = 0.0
    for e, (m, v) in enumerate(zip(ec.per_element(M, e2v, ep, 1), _lists(e2v, ep))):
        assert np.array_equal(m, m.T)
        points, bad = em._mass_points(X[v][None], dim, len(v), np.array([c[e]]))
        assert not bad.any()
        want = math.fsum(float(s[0]) for _, s in points)
        worst = max(worst, abs(math.fsum(m.ravel()) - want) / np.abs(m).max() / ec.EPS)
    _check("entry sum %s %s" % (name, jitter), worst, UNITS_SUM)


@pytest.mark.parametrize("family,name,jitter", ALL_CASES, ids=ALL_IDS)
def test_vector_form_holds_the_scalar_matrix_on_its_diagonal_blocks(family, name, jitter):
    X, e2v, ep = _mesh(family, name, jitter)
    dim = X.shape[1]
    M, _ = _model_mass(family, name, jitter)
    V, _ = _model_mass(family, name, jitter, vdim=dim)
    for m, v in zip(ec.per_element(M, e2v, ep, 1), ec.per_element(V, e2v, ep, dim)):
        nd = m.shape[0]
        assert v.shape == (dim * nd, dim * nd) and np.array_equal(v, v.T)
        for i in range(dim):
            for j in range(dim):
                blk = v[i::dim, j::dim]
                if i == j:
                    assert np.array_equal(blk, m)
                else:
                    assert not blk.any() and not np.signbit(blk).any()


@pytest.mark.parametrize("family,name,jitter", [c for c in ALL_CASES if c[2] not in (False, "box")],
                         ids=[i for c, i in zip(ALL_CASES, ALL_IDS) if c[2] not in (False, "box")])
@pytest.mark.parametrize("kind", [0, 1])
def test_add_to_is_k_plus_m_bit_for_bit(family, name, jitter, kind):
    X, e2v, ep = _mesh(family, name, jitter)
    dim = X.shape[1]
    vdim = dim if kind else 1
    K, _ = (ec.model if family == "q1" else qc.model)(name, jitter, kind, 2 if kind else 1)
    M, c = _model_mass(family, name, jitter, vdim)
    got = em.element_mass(X, e2v, c, vdim=vdim, elem_ptr=ep, add_to=K)
    assert got.shape == K.shape and np.array_equal(got, K + M) and not np.array_equal(got, K)


@pytest.mark.parametrize("family,name,jitter", ALL_CASES, ids=ALL_IDS)
def test_loads_are_the_mass_matrix_times_the_nodal_source(family, name, jitter):
    X, e2v, ep = _mesh(family, name, jitter)
    dim, NV = X.shape[1], len(X)
    M, c = _model_mass(family, name, jitter)
    rng = np.random.default_rng(3)
    ones = em.element_loads(X, e2v, np.ones(NV), coef=c, elem_ptr=ep)
    src = rng.uniform(-1.0, 1.0, (NV, dim))
    vec = em.element_loads(X, e2v, src, vdim=dim, coef=c, elem_ptr=ep)
    unit = em.element_loads(X, e2v, src[:, 0], elem_ptr=ep)                 # coef None: 1.0
    one = em.element_loads(X, e2v, src[:, 0], coef=np.ones(len(c)), elem_ptr=ep)
    assert np.array_equal(unit, one)
    ones, vec = np.asarray(ones).ravel(), np.asarray(vec).ravel()
    row = load = 0.0
    at = 0
    for m, v in zip(ec.per_element(M, e2v, ep, 1), _lists(e2v, ep)):
        nd = len(v)
        scale = np.abs(m).max()
        row = max(row, _units(np.abs(ones[at:at + nd] - m.astype(np.longdouble).sum(axis=1)), scale))
        got = vec[dim * at:dim * (at + nd)].reshape(nd, dim)
        load = max(load, _units(np.abs(got - m.astype(np.longdouble) @ src[v].astype(np.longdouble)), scale))
        at += nd
    assert dim * at == len(vec)
    _check("row sums %s %s" % (name, jitter), row, UNITS_ROW)
    _check("M src %s %s" % (name, jitter), load, UNITS_LOAD)


# ---- the global right-hand side ----
@pytest.mark.parametrize("family,name", [("q1", "hex_5x4x3"), ("q1", "mixed_4"), ("q2", "mixed_hex8_hex27")])
def test_assemble_rhs_is_the_loop_in_element_order(family, name):
    X, e2v, ep = _mesh(family, name, True if family == "q1" else "curved")
    NV = len(X)
    elvec = np.asarray(em.element_loads(X, e2v, np.random.default_rng(4).uniform(-1, 1, NV), elem_ptr=ep)).ravel()
    want = [None] * NV
    at = 0
    for v in _lists(e2v, ep):
        for a, d in enumerate(v):
            t = elvec[at + a]
            want[d] = t if want[d] is None else want[d] + t
        at += len(v)
    got = am.assemble_rhs(NV, ep, e2v, elvec)
    assert got.shape == (NV,) and np.array_equal(got, np.array(want, np.float64))
    with pytest.raises(ValueError, match="elvec"):
        am.assemble_rhs(NV, ep, e2v, elvec[:-1])


# ---- refusals ----
def test_refusals():
    X, e2v, _ = ec.mesh("hex_3x2x2")
    NE, NV = len(e2v), len(X)
    one = np.ones(NE)
    with pytest.raises(ValueError, match="vdim"):
        em.element_mass(X, e2v, one, vdim=2)
    with pytest.raises(ValueError, match="vdim"):
        em.element_loads(X, e2v, np.ones((NV, 2)), vdim=2)
    with pytest.raises(ValueError, match="coef"):
        em.element_mass(X, e2v, None)
    with pytest.raises(ValueError, match="coef"):
        em.element_mass(X, e2v, np.ones(NE + 1))
    with pytest.raises(ValueError, match="src"):
        em.element_loads(X, e2v, None)
    with pytest.raises(ValueError, match="src"):
        em.element_loads(X, e2v, np.ones(NV + 1))
    with pytest.raises(ValueError, match="add_to"):
        em.element_mass(X, e2v, one, add_to=np.zeros(5))
    with pytest.raises(ValueError, match="out of range"):
        em.element_mass(X, np.where(e2v == 3, NV, e2v), one)
    twice = e2v.copy()
    twice[5, 7] = twice[5, 0]
    with pytest.raises(ValueError, match="twice"):
        em.element_loads(X, twice, np.ones(NV))
    with pytest.raises(ValueError, match="no supported element type"):
        em.element_mass(X, e2v[:, :5], one)
    bad = e2v.copy()
    bad[[4, 9], 0], bad[[4, 9], 2] = e2v[[4, 9], 2], e2v[[4, 9], 0]
    for call in (lambda: em.element_mass(X, bad, one), lambda: em.element_loads(X, bad, np.ones(NV))):
        with pytest.raises(em.ElementError) as err:
            call()
        assert err.value.element == 4
    Xt, t2v, _ = ec.mesh("tets_3x2x2")
    flipped = t2v.copy()
    flipped[3, [0, 1]] = t2v[3, [1, 0]]
    with pytest.raises(em.ElementError) as err:
        em.element_mass(Xt, flipped, np.ones(len(t2v)))
    assert err.value.element == 3
