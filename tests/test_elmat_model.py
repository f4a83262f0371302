"""The definition of the device element matrices (saamge_amd/elmat_model.py) against what the project already has: the
closed-form box matrices of problems.py, and on jittered meshes the properties every stiffness matrix has -- exact symmetry,
vanishing row sums, rigid-body modes in the null space, no negative eigenvalue, the patch test through assemble_model.

Every bound is MEASURED on the model (in units of 2^-52 of max|K_e|, or of max|A| max|u| for the patch test), written down
here and in DESIGN.md section 4.9, and asserted with a margin of 8 for other shapes:
  boxes            20.7   (hex 9 x 8 x 7, K = diag(1, 1, 1000); it grows with |x| / h, the cancellation in the Jacobian's
                           differences of vertex coordinates: 11.5 at 5 x 4 x 3, 6.0 at 3 x 2 x 2)
  row sums          2.74      rigid-body modes  3.11      smallest eigenvalue  -4.22      patch test  2.12
"""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import elmat_cases as ec

EPS = ec.EPS
MARGIN = 8.0
BOX, ROWSUM, RIGID, MINEIG, PATCH = 20.7, 2.74, 3.11, 4.22, 2.12


def _dev(K, R):
    return max(np.abs(k - r).max() / np.abs(r).max() for k, r in zip(K, R)) / EPS


def _check(what, figure, measured):
    print("%s: %.3f units of 2^-52 (measured bound %.2f, asserted at %.0f x)" % (what, figure, measured, MARGIN))
    assert figure <= MARGIN * measured, (what, figure)


# ---- boxes ----
@pytest.mark.parametrize("n", [(3, 2, 2), (5, 4, 3), (9, 8, 7)], ids=lambda n: "x".join(map(str, n)))
def test_hex_boxes_against_the_closed_forms(n):
    X, e2v = pr.grid_coords(n), ec.hex_vertices(n)
    h = tuple(1.0 / m for m in n)
    NE = len(e2v)
    cen = X[e2v].mean(axis=1)
    cb = pr.checkerboard_coef(cen[:, 0], cen[:, 1], cen[:, 2])
    Kh = pr.hex_element_matrix(h)
    _check("one", _dev(em.element_matrices(X, e2v, 0, np.ones(NE)), np.broadcast_to(Kh, (NE, 8, 8))), BOX)
    _check("checkerboard", _dev(em.element_matrices(X, e2v, 0, cb), cb[:, None, None] * Kh[None]), BOX)
    Kd = pr.hex_element_matrix(h, (1.0, 1.0, 1000.0))
    _check("diag(1, 1, 1000)", _dev(em.element_matrices(X, e2v, 0, np.tile([1.0, 1.0, 1000.0], (NE, 1))),
                                    np.broadcast_to(Kd, (NE, 8, 8))), BOX)
    # the same tensors through the longer coefficient forms: the zero entries are multiplied like any other
    full = em.element_matrices(X, e2v, 0, np.tile([1.0, 1.0, 1000.0, 0.0, 0.0, 0.0], (NE, 1)))
    assert np.array_equal(full, em.element_matrices(X, e2v, 0, np.tile([1.0, 1.0, 1000.0], (NE, 1))))
    assert np.array_equal(em.element_matrices(X, e2v, 0, np.tile(cb[:, None], (1, 3))), em.element_matrices(X, e2v, 0, cb))
    for lam, mu in ((1.0, 1.0), (2.0, 0.5)):
        Ke = pr.hex_elasticity_matrix(h, lam, mu)
        _check("elasticity %g %g" % (lam, mu),
               _dev(em.element_matrices(X, e2v, 1, np.tile([lam, mu], (NE, 1))), np.broadcast_to(Ke, (NE, 24, 24))), BOX)


@pytest.mark.parametrize("coef", [None, "checkerboard"], ids=["one", "checkerboard"])
def test_wedges_and_hexes_against_the_mixed_problem(coef):
    p = pr.poisson3d_mixed_problem(4, (2, 2, 2), wedges="half", coef=coef)
    K = em.element_matrices(pr.grid_coords(4), p.elem_to_dof, 0, p.coefs, elem_ptr=p.elem_ptr)
    assert K.shape == p.elmat.shape
    assert em.type_counts(3, p.elem_to_dof, p.elem_ptr) == [0, 0, 0, int((np.diff(p.elem_ptr) == 6).sum()),
                                                            int((np.diff(p.elem_ptr) == 8).sum())]
    _check("mixed", _dev(ec.per_element(K, p.elem_to_dof, p.elem_ptr, 1), ec.per_element(p.elmat, p.elem_to_dof, p.elem_ptr, 1)), BOX)


@pytest.mark.parametrize("coef", [1.0, "checkerboard"], ids=["one", "checkerboard"])
def test_quads_against_quad_mesh_problem(coef):
    p = pr.quad_mesh_problem(4, 3, coef=coef, vertex_y=pr.MLTEST_VERTEX_Y)
    cen = p.coords[p.elem_to_dof].mean(axis=1)
    c = np.ones(12) if coef == 1.0 else pr.checkerboard_coef(cen[:, 0], cen[:, 1])
    _check("quads", _dev(em.element_matrices(p.coords, p.elem_to_dof, 0, c), p.elmat), BOX)


def test_quad_elasticity_against_quad_elasticity_matrix():
    p, q = pr.mltest_elasticity_problem(), pr.mltest_problem()
    K = em.element_matrices(q.coords, q.elem_to_dof, 1, np.ones((12, 2)))
    _check("quad elasticity", _dev(K, p.elmat), BOX)
    dptr, dofs = em.dof_lists(2, q.elem_to_dof, 1)
    assert np.array_equal(dofs.reshape(12, 8), p.elem_to_dof) and np.array_equal(dptr, 8 * np.arange(13))


# ---- jittered meshes: all five types, both kinds ----
def _rigid_modes(X):
    NV, dim = X.shape
    o, z = np.ones(NV), np.zeros(NV)
    if dim == 2:
        return [np.stack(m, 1).ravel() for m in ([o, z], [z, o], [-X[:, 1], X[:, 0]])]
    return [np.stack(m, 1).ravel() for m in ([o, z, z], [z, o, z], [z, z, o], [z, -X[:, 2], X[:, 1]], [X[:, 2], z, -X[:, 0]],
                                             [-X[:, 1], X[:, 0], z])]


@pytest.mark.parametrize("kind", [0, 1], ids=["diffusion", "elasticity"])
@pytest.mark.parametrize("name", sorted(ec.MESHES))
def test_jittered_meshes_keep_the_properties_of_a_stiffness_matrix(name, kind):
    X, e2v, ep = ec.mesh(name, jittered=True)
    X0 = ec.mesh(name)[0]
    NV, dim = X.shape
    comp = dim if kind else 1
    K, _ = ec.model(name, True, kind, 2 if kind else dim * (dim + 1) // 2)
    Ks = ec.per_element(K, e2v, ep, comp)
    dptr, dofs = em.dof_lists(dim, e2v, kind, ep)
    assert len(Ks) == ec.num_elements(e2v, ep) and all(k.shape[0] == dptr[e + 1] - dptr[e] for e, k in enumerate(Ks))
    assert all(np.array_equal(k, k.T) for k in Ks), "not exactly symmetric"
    scale = [np.abs(k).max() for k in Ks]
    _check("smallest eigenvalue", max(-np.linalg.eigvalsh(k).min() / s for k, s in zip(Ks, scale)) / EPS, MINEIG)
    if kind == 0:
        _check("row sums", max(np.abs(k.sum(axis=1)).max() / s for k, s in zip(Ks, scale)) / EPS, ROWSUM)
    else:
        worst = 0.0
        for r in _rigid_modes(X):
            for e, (k, s) in enumerate(zip(Ks, scale)):
                worst = max(worst, np.abs(k @ r[dofs[dptr[e]:dptr[e + 1]]]).max() / (s * np.abs(r).max()))
        _check("rigid-body modes", worst / EPS, RIGID)
    # the patch test: one coefficient for the whole mesh, a linear function, the rows of the vertices inside the domain
    NE = ec.num_elements(e2v, ep)
    const = [2.0, 0.75] if kind else ([1.5, 0.8, 1.1, 0.2, -0.1, 0.15] if dim == 3 else [1.5, 0.8, 0.2])
    Kc = em.element_matrices(X, e2v, kind, np.tile(const, (NE, 1)), elem_ptr=ep)
    rowptr, col, val = am.assemble(NV * comp, dptr, dofs, Kc.ravel(), None)
    if kind == 0:
        u = 1.0 + 2.0 * X[:, 0] - 3.0 * X[:, 1] + (0.5 * X[:, 2] if dim == 3 else 0.0)
    else:
        A = np.array([[0.3, -1.0, 0.5], [2.0, 0.7, -0.4], [0.1, 0.9, -1.5]])[:dim, :dim]
        u = (X @ A.T + np.arange(1, dim + 1)[None, :]).ravel()
    Au = np.zeros(NV * comp)
    np.add.at(Au, np.repeat(np.arange(NV * comp), np.diff(rowptr)), val * u[col])
    inside = np.repeat(np.all((X0 > 1e-9) & (X0 < 1.0 - 1e-9), axis=1), comp)
    assert inside.any()
    _check("patch test", np.abs(Au[inside]).max() / (np.abs(val).max() * np.abs(u).max()) / EPS, PATCH)


# ---- refusals ----
def test_an_inverted_element_is_reported():
    X, e2v, _ = ec.mesh("hex_5x4x3", jittered=True)
    bad = e2v.copy()
    bad[[17, 41], 0], bad[[17, 41], 1] = e2v[[17, 41], 1], e2v[[17, 41], 0]      # two vertices of a hex swapped, twice
    with pytest.raises(em.ElementError) as err:
        em.element_matrices(X, bad, 0, np.ones(len(bad)))
    assert err.value.element == 17
    flat = X.copy()
    flat[:, 2] = 0.0                                                             # degenerate: every determinant is zero
    with pytest.raises(em.ElementError) as err:
        em.element_matrices(flat, e2v, 1, np.ones((len(e2v), 2)))
    assert err.value.element == 0


def test_what_the_model_refuses():
    X, e2v, _ = ec.mesh("hex_3x2x2")
    NE = len(e2v)
    with pytest.raises(ValueError, match="5 nodes are no supported element type in 3D"):
        em.element_matrices(X, e2v[:, :5], 0, np.ones(NE))
    with pytest.raises(ValueError, match="ncoef = 2 is not allowed"):
        em.element_matrices(X, e2v, 0, np.ones((NE, 2)))
    with pytest.raises(ValueError, match="ncoef = 1 is not allowed"):
        em.element_matrices(X, e2v, 1, np.ones(NE))
    with pytest.raises(ValueError, match="out of range"):
        em.element_matrices(X, np.where(e2v == 0, len(X), e2v), 0, np.ones(NE))
    with pytest.raises(ValueError, match="kind"):
        em.element_matrices(X, e2v, 2, np.ones(NE))
    ep = np.array([0, 8, 13], np.int32)                                          # a hex and a 5-node pyramid
    with pytest.raises(ValueError, match="element 1: 5 nodes"):
        em.element_matrices(X, e2v.ravel()[:13], 0, np.ones(2), elem_ptr=ep)


# ---- the mesh helpers of problems.py ----
def test_mesh_helpers():
    n = (3, 2, 2)
    p = pr.poisson3d_problem(n, blk=(2, 2, 2))
    X = pr.grid_coords(n)
    assert X.shape == (p.ND, 3) and np.array_equal(ec.hex_vertices(n), p.elem_to_dof)
    assert np.array_equal(X[p.elem_to_dof[0]], np.array(pr._HEX_LOC) / np.array(n, dtype=float))
    q = pr.mltest_problem()
    assert np.allclose(pr.grid_coords((4, 3)), q.coords, atol=1e-9, rtol=0)
    Xj = pr.jitter(X, n, 0.2, seed=3)
    assert np.array_equal(Xj, pr.jitter(X, n, 0.2, seed=3)) and not np.array_equal(Xj, pr.jitter(X, n, 0.2, seed=4))
    move = np.abs(Xj - X) * np.array(n)
    assert move.max() <= 0.2 and move.min(axis=0).max() < 0.2 and (move > 0).all()      # boundary vertices move too
    tets = pr.hex_to_tets(n)
    assert tets.shape == (6 * p.NE, 4) and tets.dtype == np.int32
    E = X[tets[:, 1:]] - X[tets[:, :1]]
    vol = np.linalg.det(E) / 6.0
    assert (vol > 0).all() and abs(vol.sum() - 1.0) < 1e-14 and np.allclose(vol, 1.0 / (6 * p.NE))
    for c in range(p.NE):                                                         # the six tetrahedra of a cell use its vertices
        assert set(tets[6 * c:6 * c + 6].ravel()) == set(p.elem_to_dof[c])
    tris = pr.quads_to_tris(4, 3)
    assert tris.shape == (24, 3) and tris.dtype == np.int32
    P = q.coords[tris]
    area = 0.5 * ((P[:, 1, 0] - P[:, 0, 0]) * (P[:, 2, 1] - P[:, 0, 1]) - (P[:, 1, 1] - P[:, 0, 1]) * (P[:, 2, 0] - P[:, 0, 0]))
    assert (area > 0).all() and abs(area.sum() - 1.0) < 1e-14
    for c in range(12):
        assert set(tris[2 * c:2 * c + 2].ravel()) == set(q.elem_to_dof[c])
