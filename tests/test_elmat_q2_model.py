"""The definition of the order-2 element matrices (saamge_amd/elmat_model.py: the 9-node quadrilateral and the 27-node
hexahedron) against what the project already has: the closed-form box matrices of problems.py, and on jittered meshes
(straight-sided and curved, elmat_q2_cases.py) the properties every stiffness matrix has -- exact symmetry, vanishing row sums,
rigid-body modes in the null space, no negative eigenvalue -- and, on the straight-sided meshes, where the rule is exact (the
integrand has degree 4 per axis), the patch test through assemble_model.  On curved elements the integrand has degree 6
against a rule exact to 5, so the patch test is not asserted there.

Every bound is MEASURED on the model (in units of 2^-52 of max|K_e|, or of max|A| max|u| for the patch test), written down
here and in DESIGN.md section 4.9.1, and asserted with the project's margin of 8:
  boxes            4.17   (hex27 5 x 4 x 3, K = diag(1, 1, 1000); 3.96 for elasticity there, 3.54 on the quad9 grid)
  row sums          2.49      rigid-body modes  2.51      smallest eigenvalue  -2.35      patch test  1.83
"""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import elmat_cases as ec
import elmat_q2_cases as qc
from test_elmat_model import _check, _dev, _rigid_modes

EPS = ec.EPS
BOX, ROWSUM, RIGID, MINEIG, PATCH = 4.17, 2.49, 2.51, 2.35, 1.83


# ---- boxes ----
@pytest.mark.parametrize("coef", [1.0, "checkerboard"], ids=["one", "checkerboard"])
def test_quad9_boxes_against_quad_mesh_problem(coef):
    p = pr.quad_mesh_problem(4, 3, order=2, coef=coef, vertex_y=pr.MLTEST_VERTEX_Y)
    cen = p.coords[p.elem_to_dof[:, 8]]
    c = np.ones(12) if coef == 1.0 else pr.checkerboard_coef(cen[:, 0], cen[:, 1])
    K = em.element_matrices(p.coords, p.elem_to_dof, 0, c)
    assert K.shape == (12, 9, 9)
    _check("quad9", _dev(K, p.elmat), BOX)


@pytest.mark.parametrize("n", [(3, 2, 2), (5, 4, 3)], ids=lambda n: "x".join(map(str, n)))
def test_hex27_boxes_against_the_closed_forms(n):
    X, e2n, _ = qc.mesh("hex27_" + "x".join(map(str, n)))
    h = tuple(1.0 / m for m in n)
    NE = len(e2n)
    for lam, mu in ((1.0, 1.0), (2.0, 0.5)):
        Ke = pr.hex_elasticity_matrix_tensor(h, 2, lam, mu)
        _check("elasticity %g %g" % (lam, mu),
               _dev(em.element_matrices(X, e2n, 1, np.tile([lam, mu], (NE, 1))), np.broadcast_to(Ke, (NE, 81, 81))), BOX)
    _check("K = I", _dev(em.element_matrices(X, e2n, 0, np.ones(NE)),
                         np.broadcast_to(pr.hex_diffusion_matrix_tensor(h, 2), (NE, 27, 27))), BOX)
    Kd = pr.hex_diffusion_matrix_tensor(h, 2, (1.0, 1.0, 1000.0))
    diag = em.element_matrices(X, e2n, 0, np.tile([1.0, 1.0, 1000.0], (NE, 1)))
    _check("diag(1, 1, 1000)", _dev(diag, np.broadcast_to(Kd, (NE, 27, 27))), BOX)
    # the same tensors through the longer coefficient forms: the zero entries are multiplied like any other
    assert np.array_equal(em.element_matrices(X, e2n, 0, np.tile([1.0, 1.0, 1000.0, 0.0, 0.0, 0.0], (NE, 1))), diag)
    c = ec.coefficients(NE, 3, 0, 1)[:, 0]
    one = em.element_matrices(X, e2n, 0, c)
    assert np.array_equal(em.element_matrices(X, e2n, 0, np.tile(c[:, None], (1, 3))), one)
    assert np.array_equal(em.element_matrices(X, e2n, 0, np.concatenate([np.tile(c[:, None], (1, 3)), np.zeros((NE, 3))], axis=1)), one)


def test_the_closed_form_q2_diffusion_matrix():
    h = (0.25, 0.5, 0.125)
    K = pr.hex_diffusion_matrix_tensor(h, 2, (1.0, 2.0, 3.0))
    assert K.shape == (27, 27) and np.allclose(K, K.T, rtol=0, atol=1e-15) and np.abs(K.sum(axis=1)).max() < 1e-13
    assert np.linalg.eigvalsh(K).min() > -1e-13
    perm = np.array([(iz * 2 + iy) * 2 + ix for (ix, iy, iz) in pr._HEX_LOC])                 # order 1: the trilinear matrix
    assert np.array_equal(pr.hex_diffusion_matrix_tensor(h, 1, (1.0, 2.0, 3.0))[np.ix_(perm, perm)],
                          pr.hex_element_matrix(h, (1.0, 2.0, 3.0)))


# ---- jittered meshes: both types and the list of two orders, both kinds, both jitters ----
def test_the_model_accepts_every_jittered_mesh():
    """no element of any mesh has a non-positive determinant at a point, at the amounts and the seed of elmat_q2_cases"""
    for name in qc.MESHES:
        for jitter in ("straight", "curved"):
            X, e2n, ep = qc.mesh(name, jitter)
            em.element_matrices(X, e2n, 0, np.ones(ec.num_elements(e2n, ep)), elem_ptr=ep)      # raises ElementError otherwise


@pytest.mark.parametrize("kind", [0, 1], ids=["diffusion", "elasticity"])
@pytest.mark.parametrize("jitter", ["straight", "curved"])
@pytest.mark.parametrize("name", qc.MESHES)
def test_jittered_meshes_keep_the_properties_of_a_stiffness_matrix(name, jitter, kind):
    X, e2n, ep = qc.mesh(name, jitter)
    X0 = qc.mesh(name)[0]
    NV, dim = X.shape
    comp = dim if kind else 1
    K, _ = qc.model(name, jitter, kind, 2 if kind else dim * (dim + 1) // 2)
    Ks = ec.per_element(K, e2n, ep, comp)
    dptr, dofs = em.dof_lists(dim, e2n, kind, ep)
    assert len(Ks) == ec.num_elements(e2n, ep) and all(k.shape[0] == dptr[e + 1] - dptr[e] for e, k in enumerate(Ks))
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
    if jitter != "straight":
        return
    # the patch test: one coefficient for the whole mesh, a linear function, the rows of the nodes inside the domain
    NE = ec.num_elements(e2n, ep)
    const = [2.0, 0.75] if kind else ([1.5, 0.8, 1.1, 0.2, -0.1, 0.15] if dim == 3 else [1.5, 0.8, 0.2])
    Kc = em.element_matrices(X, e2n, kind, np.tile(const, (NE, 1)), elem_ptr=ep)
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
def test_an_inverted_hex27_is_reported():
    X, e2n, _ = qc.mesh("hex27_5x4x3", "straight")
    bad = e2n.copy()
    bad[[17, 41], 0], bad[[17, 41], 2] = e2n[[17, 41], 2], e2n[[17, 41], 0]      # two corner nodes of a hex swapped, twice
    for kind, coef in ((0, np.ones(len(bad))), (1, np.ones((len(bad), 2)))):
        with pytest.raises(em.ElementError) as err:
            em.element_matrices(X, bad, kind, coef)
        assert err.value.element == 17


def test_what_the_model_refuses():
    X, e2n, _ = qc.mesh("hex27_3x2x2")
    X2, q2n, _ = qc.mesh("quad9_4x3")
    NE = len(e2n)
    with pytest.raises(ValueError, match="27 nodes are no supported element type in 2D"):
        em.element_matrices(X2, np.arange(54).reshape(2, 27), 0, np.ones(2))
    with pytest.raises(ValueError, match="9 nodes are no supported element type in 3D"):
        em.element_matrices(X, e2n[:, :9], 0, np.ones(NE))
    with pytest.raises(ValueError, match="element 1: 9 nodes"):
        em.element_matrices(X, np.concatenate([e2n[0], e2n[1, :9], e2n[2]]), 0, np.ones(3), elem_ptr=np.array([0, 27, 36, 63]))
    with pytest.raises(ValueError, match="element 1: 27 nodes"):
        em.element_matrices(X2, np.concatenate([q2n[0], np.arange(27)]), 0, np.ones(2), elem_ptr=np.array([0, 9, 36]))
    with pytest.raises(ValueError, match="out of range"):
        em.element_matrices(X, np.where(e2n == 0, len(X), e2n), 0, np.ones(NE))
    twice = e2n.copy()
    twice[5, 26] = twice[5, 4]
    with pytest.raises(ValueError, match="twice"):
        em.element_matrices(X, twice, 0, np.ones(NE))


# ---- dof lists, counts, the mesh helpers of problems.py ----
def test_dof_lists_and_counts():
    p = pr.quad_mesh_problem(4, 3, order=2, coef=1.0, vertex_y=pr.MLTEST_VERTEX_Y)
    X, q2n, _ = qc.mesh("quad9_4x3")
    dptr, dofs = em.dof_lists(2, q2n, 0)
    assert np.array_equal(dofs.reshape(12, 9), p.elem_to_dof) and np.array_equal(dptr, 9 * np.arange(13))
    assert em.type_counts(2, q2n) == [0] * 5 and em.order2_count(2, q2n) == 12
    n = (3, 2, 2)
    q = pr.elasticity3d_q2_problem(n, blk=(2, 2, 2))
    e2n = pr.q2_hex_nodes(n)
    dptr, dofs = em.dof_lists(3, e2n, 1)
    assert np.array_equal(dofs.reshape(12, 81), q.elem_to_dof) and np.array_equal(dptr, 81 * np.arange(13))
    assert em.type_counts(3, e2n) == [0] * 5 and em.order2_count(3, e2n) == 12
    X, lists, ep = qc.mesh("mixed_hex8_hex27")
    assert em.type_counts(3, lists, ep) == [0, 0, 0, 0, 12] and em.order2_count(3, lists, ep) == 3
    assert em.order2_count(3, ec.mesh("hex_3x2x2")[1]) == 0


def test_q2_mesh_helpers():
    n = (3, 2, 2)
    e2n = pr.q2_hex_nodes(n)
    X = pr.grid_coords((6, 4, 4))
    assert e2n.shape == (12, 27) and e2n.dtype == np.int32 and X.shape == (7 * 5 * 5, 3)
    assert np.array_equal(X[e2n[0]] * np.array([6.0, 4.0, 4.0]), np.array(pr.Q2_HEX_LOC, dtype=float))
    assert np.allclose(pr.q2_straight_sided(X, e2n), X, rtol=0, atol=1e-15)      # the grid is straight-sided already
    Xj = pr.jitter(X, n, 0.2, seed=3)
    Xs = pr.q2_straight_sided(Xj, e2n)
    corners = np.unique(e2n[:, [k for k, l in enumerate(pr.Q2_HEX_LOC) if 1 not in l]])
    assert np.array_equal(Xs[corners], Xj[corners])
    loc = {l: k for k, l in enumerate(pr.Q2_HEX_LOC)}
    P = Xs[e2n]
    assert np.allclose(P[:, loc[(1, 0, 0)]], 0.5 * (P[:, loc[(0, 0, 0)]] + P[:, loc[(2, 0, 0)]]), rtol=0, atol=1e-15)
    assert np.allclose(P[:, loc[(1, 1, 2)]], 0.25 * (P[:, loc[(0, 0, 2)]] + P[:, loc[(2, 0, 2)]] + P[:, loc[(0, 2, 2)]]
                                                      + P[:, loc[(2, 2, 2)]]), rtol=0, atol=1e-15)
    assert np.allclose(P[:, loc[(1, 1, 1)]], P[:, [loc[l] for l in loc if 1 not in l]].mean(axis=1), rtol=0, atol=1e-15)
    p = pr.quad_mesh_problem(4, 3, order=2, coef=1.0)
    Q = pr.q2_straight_sided(pr.jitter(p.coords, (4, 3), 0.2, seed=3), p.elem_to_dof)[p.elem_to_dof]
    assert np.allclose(Q[:, 5], 0.5 * (Q[:, 1] + Q[:, 2]), rtol=0, atol=1e-15)      # the right edge's midpoint
    assert np.allclose(Q[:, 8], Q[:, :4].mean(axis=1), rtol=0, atol=1e-15)
