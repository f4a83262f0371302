"""The definition of the uniform refinement (saamge_amd/mesh_refine_model.py) against facts known without it: the element
layer's positivity check and exact measures, the conformity of the refined mesh through mesh_model.FaceTable, structured grids
and problems.p2_simplex_nodes, the shape classes of a refined tetrahedron (Bey), the interpolation on linear functions, nested
stiffness matrices P^T A_fine P = A_coarse, the numbering guarantee, and the refusals.

Measures are computed in exact integer arithmetic (every float is an integer times a power of two), so the bound of the
measure test holds the coordinates of the lift alone: it is not spent on the rounding of a volume formula."""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import elmat_model as em
from saamge_amd import mesh_lift_model as lm
from saamge_amd import mesh_model as mm
from saamge_amd import mesh_refine_model as rm
from saamge_amd import problems as pr

import mesh_faces_cases as mc
import mesh_refine_cases as rc

U = 2.0 ** -53


# ---- exact measures ----
def _integers(X):
    """(object array of Python ints, K): X * 2^K, exactly"""
    X = np.asarray(X, np.float64)
    nz = X[X != 0.0]
    K = max(0, 53 - int(np.frexp(np.abs(nz))[1].min())) if len(nz) else 0
    big = np.ldexp(X, K)
    assert np.array_equal(big, np.round(big))
    return np.array([int(v) for v in big.ravel()], dtype=object).reshape(X.shape), K


def _det(a, b, c=None):
    if c is None:
        return a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0]) +
            a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]))


def _measures(Xi, dim, ep, e2v):
    """d! times the measure of every element, as Python ints in units of 2^(-K dim); a trilinear hexahedron by the
    three-determinant formula through its long diagonal 0 - 6, which is exact for it"""
    nd = np.diff(ep)
    out = np.zeros(len(nd), dtype=object)
    for c in [int(c) for c in np.unique(nd)]:
        ids = np.flatnonzero(nd == c)
        V = Xi[e2v[ep[ids][:, None] + np.arange(c)[None, :]]]                               # (elements, corners, dim)
        x = [V[:, k] for k in range(c)]
        if dim == 2 and c == 3:
            m = _det(x[1] - x[0], x[2] - x[0])
        elif dim == 2:
            m = sum(x[k][:, 0] * x[(k + 1) % 4][:, 1] - x[(k + 1) % 4][:, 0] * x[k][:, 1] for k in range(4))
        elif c == 4:
            m = _det(x[1] - x[0], x[2] - x[0], x[3] - x[0])
        else:
            d = x[6] - x[0]
            m = _det(d, x[1] - x[0], x[2] - x[5]) + _det(d, x[4] - x[0], x[5] - x[7]) + _det(d, x[3] - x[0], x[7] - x[2])
        out[ids] = m
    return out


def test_the_hexahedron_formula_on_the_unit_cube():
    X, K = _integers(pr.grid_coords((1, 1, 1))[[0, 1, 3, 2, 4, 5, 7, 6]])
    assert _measures(X, 3, np.array([0, 8]), np.arange(8))[0] == 6 * 2 ** (3 * K)


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("name", rc.GEOMETRIC)
def test_orientation_and_exact_counts(name, levels):
    NV, dim, e2v, ep = rc.case(name)
    nc = rm.NC[dim]
    R = rc.model(name, levels)
    coarse = rc.model(name, levels - 1) if levels > 1 else None
    cX, cep, ce2v = (coarse.coords, coarse.elem_ptr, coarse.elem_to_vertex) if coarse else \
        (rc.coords(name),) + tuple(np.asarray(a) for a in lm._topology(NV, dim, e2v, ep)[:2])
    assert R.NE == nc * (len(cep) - 1) and R.info[:4] == [R.NV, R.NE, len(R.elem_to_vertex), levels]
    # every child passes the element layer's positivity check
    em.element_matrices(R.coords, R.elem_to_vertex, 0, np.ones(R.NE), elem_ptr=R.elem_ptr)        # (raises ElementError otherwise)
    # the children's measures sum to the parent's: one number system for both levels
    both, _ = _integers(np.concatenate([cX, R.coords]))
    parent = _measures(both[:len(cX)], dim, np.asarray(cep, np.int64), np.asarray(ce2v, np.int64))
    child = _measures(both[len(cX):], dim, R.elem_ptr.astype(np.int64), R.elem_to_vertex.astype(np.int64))
    assert (child > 0).all() and (parent > 0).all()
    total = child.reshape(-1, nc).sum(axis=1)
    worst = max(abs(int(t) - int(p)) / int(p) for t, p in zip(total, parent))
    print("%s level %d: the largest |sum of children - parent| / parent = %.3g u" % (name, levels, worst / U))
    for t, p in zip(total, parent):
        assert abs(int(t) - int(p)) * 2 ** 53 <= 8 * int(p)
    # every parent corner k is corner k of child k
    nd = np.diff(cep)
    for k in range(int(nd.max())):
        has = np.flatnonzero(nd > k)
        assert np.array_equal(R.elem_to_vertex[R.elem_ptr[nc * has + k] + k], np.asarray(ce2v)[np.asarray(cep)[has] + k])


@pytest.mark.parametrize("name,levels", rc.CASES)
def test_conformity(name, levels):
    NV, dim, e2v, ep = rc.case(name)
    R = rc.model(name, levels)
    nc = rm.NC[dim]
    T0 = mc.table(name) if name in mc.NAMES else mm.FaceTable(NV, dim, e2v, ep)
    T = mm.FaceTable(R.NV, dim, R.elem_to_vertex, R.elem_ptr)                              # (a non-manifold face raises)
    per_face = 2 if dim == 2 else 4
    assert T.NB == per_face ** levels * T0.NB
    slots = nc ** levels * len(T0.nbr_elem)
    assert len(T.nbr_elem) == slots and int((T.nbr_elem >= 0).sum()) == slots - T.NB
    if R.NE and (np.diff(R.elem_ptr) == np.diff(R.elem_ptr)[0]).all():                     # one type: the closed form
        faces_per_element = len(em.FACE_NODES[(dim, int(np.diff(R.elem_ptr)[0]))])
        pairs = int((T.nbr_elem >= 0).sum()) // 2
        assert 2 * pairs == nc * faces_per_element * (R.NE // nc) - T.NB


def _tuples(X):
    return set(map(tuple, np.asarray(X).tolist()))


@pytest.mark.parametrize("levels", [1, 2])
def test_structured_identity(levels):
    f = 2 ** levels
    R = rc.model("hex_3x2x2", levels)
    assert _tuples(R.coords) == _tuples(pr.grid_coords((3 * f, 2 * f, 2 * f))) and R.NV == (3 * f + 1) * (2 * f + 1) ** 2
    # the quadrilaterals of the 4 x 3 unit-square grid (quads_4x3 carries the 9-digit coordinates of the mltest fixture)
    v = lambda i, j: j * 5 + i
    quads = np.array([[v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)] for j in range(3) for i in range(4)], np.int32)
    R = rm.MeshRefine(20, 2, pr.grid_coords((4, 3)), quads, levels=levels)
    assert _tuples(R.coords) == _tuples(pr.grid_coords((4 * f, 3 * f))) and R.NV == (4 * f + 1) * (3 * f + 1)
    if levels == 1:
        R = rc.model("tets_3x2x2", 1)
        X2, rows = pr.p2_simplex_nodes(rc.coords("tets_3x2x2"), rc.case("tets_3x2x2")[2])
        assert np.array_equal(R.coords.view(np.int64), X2.view(np.int64))                  # the same numbering, bit for bit
        assert _tuples(R.coords) == _tuples(X2) and R.NV == len(_tuples(X2))


def _classes(X, rows, scale):
    e = np.array([np.linalg.norm(X[rows[:, i]] - X[rows[:, j]], axis=1) for i in range(4) for j in range(i + 1, 4)]).T * scale
    vol = np.linalg.det(X[rows[:, 1:]] - X[rows[:, :1]]) * scale ** 3
    assert (vol > 0).all()
    key = np.round(np.concatenate([np.sort(e, axis=1), vol[:, None]], axis=1) / np.abs(e).max(), 9)
    return len(np.unique(key, axis=0))


@pytest.mark.parametrize("which", ["unit", "random"])
def test_shape_stability_of_the_tetrahedron(which):
    """Bey: the descendants of a tetrahedron fall into at most 3 congruence classes; with the diagonal m02 - m13 they are 3"""
    X = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    if which == "random":
        X = X + np.random.default_rng(7).uniform(-0.2, 0.2, (4, 3))
    tet = np.array([[0, 1, 2, 3]], np.int32)
    for levels in (1, 2, 3, 4):
        R = rm.MeshRefine(4, 3, X, tet, levels=levels)
        assert R.NE == 8 ** levels
        assert _classes(R.coords, R.lists(), 2.0 ** levels) == 3, levels


@pytest.mark.parametrize("name,levels", rc.CASES)
def test_interpolation_rows(name, levels):
    R = rc.model(name, levels)
    assert len(R.P) == levels and R.info[4] == sum(P.nnz for P in R.P)
    X = rc.coords(name)
    for j, P in enumerate(R.P):
        NVj, NE, _, NEd, NFq, NC, _, nnz = R.level_info[j]
        assert (P.nrows, P.ncols, P.nnz) == (R.level_info[j + 1][0], NVj, nnz)
        assert nnz == NVj + 2 * NEd + 4 * NFq + (4 if R.dim == 2 else 8) * NC
        assert P.rowptr.dtype == np.int32 and P.col.dtype == np.int32 and P.rowptr[0] == 0 and P.rowptr[-1] == nnz
        row = np.repeat(np.arange(P.nrows), np.diff(P.rowptr))
        sums = np.zeros(P.nrows)
        np.add.at(sums, row, P.val)
        assert (sums == 1.0).all()                                                        # powers of two: exact
        inner = np.ones(nnz, bool)
        inner[P.rowptr[:-1][np.diff(P.rowptr) > 0]] = False
        assert (np.diff(P.col.astype(np.int64))[inner[1:]] > 0).all()                     # columns ascend within a row
        assert np.array_equal(P.col[:NVj], np.arange(NVj)) and (P.val[:NVj] == 1.0).all()
        # P coords = coords2: the lift adds in another order, at most 8 additions
        Xn = P.dot(X)
        want = R.coords if j == levels - 1 else rc.model(name, j + 1).coords
        if len(X):
            assert np.abs(Xn - want).max() <= 8 * U * np.abs(X).max()
        X = want


@pytest.mark.parametrize("name", rc.NAMES)
def test_interpolation_is_exact_on_linear_functions(name):
    NV, dim, e2v, ep = rc.case(name)
    R = rm.MeshRefine(NV, dim, rc.dyadic_coords(name), e2v, ep, levels=2, want_interp=True)
    f = lambda X: 1.0 + 2.0 * X[:, 0] - 3.0 * X[:, 1] + (4.0 * X[:, 2] if dim == 3 else 0.0)
    mid = rm.MeshRefine(NV, dim, rc.dyadic_coords(name), e2v, ep, levels=1).coords
    assert np.array_equal(R.P[0].dot(f(rc.dyadic_coords(name))), f(mid))
    assert np.array_equal(R.P[1].dot(f(mid)), f(R.coords))


def _stiffness(X, rows):
    n = X.shape[0]
    elmat = em.element_matrices(X, rows, 0, np.ones(rows.shape[0]))
    rowptr, col, val = am.assemble(n, None, rows, elmat, eliminate=False)
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rowptr)), col] = val
    return A


@pytest.mark.parametrize("name", rc.AFFINE)
def test_nested_spaces(name):
    """on affine elements the coarse shape functions are combinations of the fine ones with the weights of P, so the Galerkin
    product of the fine stiffness matrix is the coarse one -- whatever numbering the model chose"""
    NV, dim, e2v, ep = rc.case(name)
    R = rc.model(name, 1)
    Ac, Af = _stiffness(rc.coords(name), e2v), _stiffness(R.coords, R.lists())
    P = R.P[0].dense()
    err = np.abs(P.T @ Af @ P - Ac).max()
    print("%s: |P^T A_fine P - A_coarse| = %.3e of %.3e" % (name, err, np.abs(Ac).max()))
    assert err <= 1e-12 * max(np.abs(Ac).max(), np.abs(Af).max())


@pytest.mark.parametrize("name", ["hex_3x2x2", "tets_3x2x2", "tris_and_quads", "tet_beside_hex", "double_contact"])
def test_numbering(name):
    NV, dim, e2v, ep = rc.case(name)
    nc = rm.NC[dim]
    shift = 2 if dim == 2 else 3
    nd0 = mc.node_counts(e2v, ep)
    for s in (1, 2):
        R = rc.model(name, s)
        anc = np.arange(R.NE) >> (shift * s)
        assert np.array_equal(anc, np.arange(R.NE) // nc ** s)
        assert np.array_equal(np.diff(R.elem_ptr), nd0[anc])                               # each child has its ancestor's type
        # the vertices of a descendant lie in the hull of its ancestor: its box, to rounding
        X0 = rc.coords(name)
        ep0 = np.concatenate([[0], np.cumsum(nd0)])
        flat0 = np.asarray(e2v).ravel()
        for e in range(len(nd0)):
            own = X0[flat0[ep0[e]:ep0[e + 1]]]
            sub = R.coords[R.elem_to_vertex[R.elem_ptr[e * nc ** s]:R.elem_ptr[(e + 1) * nc ** s]]]
            assert (sub >= own.min(axis=0) - 1e-14).all() and (sub <= own.max(axis=0) + 1e-14).all()
        # the descendants of one element are connected in the face graph of the refined mesh
        T = mm.FaceTable(R.NV, dim, R.elem_to_vertex, R.elem_ptr)
        for e in range(len(nd0)):
            ids = np.arange(e * nc ** s, (e + 1) * nc ** s)
            seen, front = {int(ids[0])}, [int(ids[0])]
            while front:
                c = front.pop()
                for n in T.adj[T.xadj[c]:T.xadj[c + 1]]:
                    if anc[n] == e and int(n) not in seen:
                        seen.add(int(n))
                        front.append(int(n))
            assert len(seen) == len(ids)


def test_level_info_and_hierarchical_vertices():
    R = rc.model("hex_5x4x3", 2)
    n = (5, 4, 3)
    for j in range(3):
        m = [v << j for v in n]
        NV, NE, entries = R.level_info[j][:3]
        assert NV == (m[0] + 1) * (m[1] + 1) * (m[2] + 1) and NE == m[0] * m[1] * m[2] and entries == 8 * NE
    assert R.level_info[2][3:] == [-1] * 5 and R.level_info[0][3:6] == rc.lc.model("hex_5x4x3").info[1:4]
    assert np.array_equal(R.coords[:rc.coords("hex_5x4x3").shape[0]], rc.coords("hex_5x4x3"))
    assert np.array_equal(R.coords[:rc.model("hex_5x4x3", 1).NV], rc.model("hex_5x4x3", 1).coords)
    plain = rm.MeshRefine(*rc.case("hex_5x4x3")[:2], rc.coords("hex_5x4x3"), rc.case("hex_5x4x3")[2], levels=2)
    assert plain.P == [] and plain.info[4] == 0 and [l[7] for l in plain.level_info] == [0, 0, -1]
    assert np.array_equal(plain.elem_to_vertex, R.elem_to_vertex)
    assert rm.MeshRefine(*rc.case("hex_5x4x3")[:2], None, rc.case("hex_5x4x3")[2]).coords is None


def test_refusals(monkeypatch):
    NV, dim, e2v, ep = mc.case("mixed_4")
    wedge = int(np.flatnonzero(mc.node_counts(e2v, ep) == 6)[0])
    with pytest.raises(rm.LiftError, match="element %d: a wedge" % wedge) as r:
        rm.MeshRefine(NV, dim, None, e2v, ep)
    assert r.value.element == wedge
    NV, dim, e2v, ep = mc.case("hex27_3x2x2")
    with pytest.raises(rm.LiftError, match="element 0: 27 nodes"):
        rm.MeshRefine(NV, dim, None, e2v, ep, levels=2)
    for name in ("single_2_6", "single_2_9", "single_3_10", "single_3_6"):
        NV, dim, e2v, ep = mc.case(name)
        with pytest.raises(rm.LiftError, match="element 0"):
            rm.MeshRefine(NV, dim, None, e2v, ep)
    for name, (NV, dim, e2v, ep, word) in sorted(mc.REFUSED_MESHES.items()):
        with pytest.raises(ValueError, match=word):
            rm.MeshRefine(NV, dim, None, e2v, ep)
    NV, dim, e2v, ep = rc.case("hex_3x2x2")
    with pytest.raises(ValueError, match="levels must be at least 1"):
        rm.MeshRefine(NV, dim, None, e2v, ep, levels=0)
    with pytest.raises(ValueError, match="levels above"):
        rm.MeshRefine(NV, dim, None, e2v, ep, levels=rm.MAX_LEVELS + 1)
    # the overflow refusals, reached by counts only: the limits lowered to what level 2 passes
    two = rc.model("hex_3x2x2", 2)
    monkeypatch.setattr(rm, "LIMIT", len(two.elem_to_vertex) - 1)
    with pytest.raises(ValueError, match="level 2: the element -> vertex lists are beyond 32 bits"):
        rm.MeshRefine(NV, dim, None, e2v, ep, levels=2)
    assert rm.MeshRefine(NV, dim, None, e2v, ep, levels=1).NE == 96
    # nnz of P counts every vertex, listed or not, so it passes the limit before the lists do where many are unlisted
    many = rm.MeshRefine(NV + 2000, dim, None, e2v, ep, want_interp=True)
    assert many.P[0].nnz > len(many.elem_to_vertex) and many.info[7] == 2000
    monkeypatch.setattr(rm, "LIMIT", many.P[0].nnz - 1)
    assert rm.MeshRefine(NV + 2000, dim, None, e2v, ep).NE == 96                           # (asked for without the interpolation)
    with pytest.raises(ValueError, match="level 0: nnz = %d entries of the interpolation" % many.P[0].nnz):
        rm.MeshRefine(NV + 2000, dim, None, e2v, ep, want_interp=True)
    monkeypatch.setattr(rm, "LIMIT", 2 ** 31 - 1)
    monkeypatch.setattr(lm, "_MAX_INT", two.NV - 1)
    with pytest.raises(ValueError, match="NV2 = %d nodes are beyond 32 bits" % two.NV):
        rm.MeshRefine(NV, dim, None, e2v, ep, levels=2)
