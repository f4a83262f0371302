"""CPU model of the device element matrices (csrc/elmat.hip) -- numpy only, test infrastructure like capi.py.

This file is the DEFINITION of the result: the device code restates it and must give the same bits.  Everything is written
as single IEEE operations in a fixed order (no fused multiply-add, no library sums), vectorised over the elements and, where
every lane of the vector does the same operation, over the nodes and node pairs of an element (elementwise, so the roundings
are those of the scalar formulas).

  types        (dim, nodes): (2, 3) P1 triangle, (2, 4) Q1 quadrilateral (v00, v10, v11, v01), (3, 4) P1 tetrahedron,
               (3, 6) P1 x P1 wedge (node a * 3 + i: triangle vertex i on the bottom a = 0 / top a = 1 face), (3, 8) Q1
               hexahedron (vertex order HEX_LOC); order 2: (2, 9) Q2 quadrilateral (MFEM's H1 order: the vertices v00, v10,
               v11, v01, the edge midpoints bottom, right, top, left, the centre -- tensor positions Q2_QUAD_LOC) and (3, 27)
               Q2 hexahedron (lexicographic: node (iz * 3 + iy) * 3 + ix); order-2 simplices: (2, 6) P2 triangle (the vertices
               0, 1, 2, then the midpoints of the edges (0,1), (1,2), (2,0)) and (3, 10) P2 tetrahedron (the vertices 0 .. 3,
               then the midpoints of the edges (0,1), (0,2), (0,3), (1,2), (1,3), (2,3)) -- P2_EDGES; believed to be MFEM's H1
               order-2 orders, which could not be verified against MFEM itself: the table is the definition.  Anything else
               is refused.
  geometry     isoparametric: the Jacobian below runs over ALL nodes of the element, so an order-2 element may be curved; a
               straight-sided one has its extra nodes at the multilinear image of its corners.
  rule         reference elements [0, 1]^dim and the unit simplex; triangle, tetrahedron: 1 point; quadrilateral, hexahedron:
               2 Gauss points per axis (point q: axis d takes GAUSS[(q >> d) & 1]); wedge: point q = 3 * qz + qt, the 3-point
               degree-2 triangle rule times 2 Gauss points.  The points and the weight of a point are the literals below.
  order 2      3 Gauss points per axis, GAUSS3 with the 1-D weights GAUSS3_W; point q = (qz * 3 + qy) * 3 + qx, its weight
               (wx * wy) * wz (wx * wy in 2D).  The 1-D shape functions on the nodes 0, 1/2, 1 and their derivatives are the
               expressions of _n2 and _d2; the gradient of node (ix, iy, iz) is (d(ix, px) * (n(iy, py) * n(iz, pz)),
               d(iy, py) * (n(ix, px) * n(iz, pz)), d(iz, pz) * (n(ix, px) * n(iy, py))), in 2D (d(ix, px) * n(iy, py),
               n(ix, px) * d(iy, py)).
  simplices    order 2 on the barycentric coordinates L_0 = ((1 - x) - y) - z (2D: (1 - x) - y), L_1 = x, L_2 = y, L_3 = z with
               the constant gradients dL_i = TRI_D[i] / TET_D[i]: vertex node i: N = L_i * (2.0 * L_i - 1.0), gradient component
               k (4.0 * L_i - 1.0) * dL_i[k]; edge node (i, j): N = (4.0 * L_i) * L_j, gradient component k
               (4.0 * L_i) * dL_j[k] + (4.0 * L_j) * dL_i[k] (_p2_simplex).  Stiffness rules (degree 2): triangle the three
               points of WEDGE_TRI, weight 1/6 each; tetrahedron TET_POINTS, weight 1/24 each.  Mass, loads and faces:
               P2_TRI_POINTS (6 points, degree 4) and P2_TET_POINTS (14 points, degree 5) with the weights P2_TRI_W, P2_TET_W
               (the reference measure included), further down.
  point        J[i][j] = sum over the nodes a, ascending, of x_a[i] * dN_a[j], the first product taken as it is; the cofactors
               C[i][j] and det from the explicit formulas of _cofactors; G_a[i] = sum_j dN_a[j] * C[i][j] (the physical
               gradient times det); s = weight / det (one division per point).
  kind 0       diffusion.  K of the element as (xx, yy, zz, xy, yz, xz) in 3D, (xx, yy, xy) in 2D: ncoef = 1 fills the
               diagonal with c, ncoef = dim gives the diagonal, the missing entries are 0.0 and are multiplied like any
               other.  F_a = K G_a; entry (a, b) with a <= b gets s * (F_a . G_b) per point, (b, a) is the same double.
  kind 1       elasticity, ncoef = 2 (lambda, mu), dof dim * a + i:  entry ((a, i), (b, j)) gets per point
               s * (lambda * (G_a[i] * G_b[j]) + mu * (G_a[j] * G_b[i]) [+ mu * (G_a . G_b) when i == j]).
  sums         over the points in ascending order, starting from 0.0.
  layout       packed in element order, row-major, element e at sum_{f<e} size_f^2; (NE, size, size) when elem_ptr is None.
  refused      dim, kind, ncoef out of range, a node count that is no type of the dimension, malformed offsets, a vertex id
               outside [0, NV), an element that lists a vertex twice, and an element whose det is not positive at a point
               (ElementError, .element the smallest such id).
  zeroth order element_mass and element_loads, on the same types, node orders and geometry: defined further down in this file.
  points       element_points, element_eval, element_loads_points and element_errors: the points of the mass rule, a nodal field
               and its gradient there, the loads of a source given there and the squared errors per element: defined after the
               boundary forms.
  point coef   element_matrices_points and element_mass_points: the stiffness forms and the mass with a coefficient per point of
               the mass rule in the place of the coefficient per element: defined at the end of this file.
  boundary    FACE_NODES, boundary_mass and boundary_loads: the face mass and the face loads of a list of (element, local face)
               pairs, added into the owning elements' matrices and vectors: defined at the end of this file.
  face points  boundary_points, boundary_eval, boundary_mass_points and boundary_loads_points: the points of the listed faces with
               weight * measure and the outward unit normal, the trace and the whole gradient of a nodal field there, the face mass
               with a coefficient per point and the face loads of data given there: defined at the end of this file.
"""
import numpy as np

GAUSS = (0.21132486540518713, 0.7886751345948129)        # 1/2 -+ 1/(2 sqrt 3)
TRI_A, TRI_B = 0.16666666666666666, 0.6666666666666666   # the triangle rule's coordinates 1/6 and 2/3
QUAD_LOC = [(0, 0), (1, 0), (1, 1), (0, 1)]
HEX_LOC = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
TRI_D = [(-1.0, -1.0), (1.0, 0.0), (0.0, 1.0)]
TET_D = [(-1.0, -1.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
WEDGE_TRI = [(TRI_A, TRI_A), (TRI_B, TRI_A), (TRI_A, TRI_B)]
# weight of one point (all points of a rule weigh the same)
WEIGHT = {(2, 3): 0.5, (2, 4): 0.25, (3, 4): 0.16666666666666666, (3, 6): 0.08333333333333333, (3, 8): 0.125}
NPOINTS = {(2, 3): 1, (2, 4): 4, (3, 4): 1, (3, 6): 6, (3, 8): 8}
TYPE_INDEX = {(2, 3): 0, (2, 4): 1, (3, 4): 2, (3, 6): 3, (3, 8): 4}      # info[0..4] of saamge_amd_element_matrices
# ---- order 2 (their number is info[7])
GAUSS3 = (0.11270166537925831, 0.5, 0.8872983346207417)  # 1/2 - sqrt(15)/10, 1/2, 1/2 + sqrt(15)/10
GAUSS3_W = (0.2777777777777778, 0.4444444444444444, 0.2777777777777778)      # 5/18, 4/9, 5/18
Q2_QUAD_LOC = [(0, 0), (2, 0), (2, 2), (0, 2), (1, 0), (2, 1), (1, 2), (0, 1), (1, 1)]
Q2_HEX_LOC = [(ix, iy, iz) for iz in range(3) for iy in range(3) for ix in range(3)]
ORDER2 = ((2, 9), (3, 27), (2, 6), (3, 10))
NPOINTS.update({(2, 9): 9, (3, 27): 27})
# the order-2 simplices: edge (i, j) of midside node dim + 1 + k; their stiffness rules are the order-1 mass rules
P2_EDGES = {2: ((0, 1), (1, 2), (2, 0)), 3: ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))}
P2_SIMPLEX = ((2, 6), (3, 10))
NPOINTS.update({(2, 6): 3, (3, 10): 4})
WEIGHT.update({(2, 6): 0.16666666666666666, (3, 10): 0.041666666666666664})
# every type by the device's internal index (csrc/elmat.hip em_type_index); TYPE_INDEX stays the order-1 part, info[0..4]
ALL_TYPE_INDEX = dict(TYPE_INDEX)
ALL_TYPE_INDEX.update({(2, 9): 5, (3, 27): 6, (2, 6): 7, (3, 10): 8})


class ElementError(ValueError):
    """An element with a non-positive Jacobian determinant; .element is the smallest such id."""

    def __init__(self, element):
        ValueError.__init__(self, "element %d: the Jacobian determinant is not positive" % element)
        self.element = int(element)


def _f(l, p):
    return p if l else 1.0 - p


def _df(l):
    return 1.0 if l else -1.0


def _n2(l, p):
    """1-D order-2 shape function of node l (at 0, 1/2, 1) at p"""
    if l == 0:
        return (2.0 * p - 1.0) * (p - 1.0)
    if l == 1:
        return (4.0 * p) * (1.0 - p)
    return p * (2.0 * p - 1.0)


def _d2(l, p):
    """its derivative"""
    if l == 0:
        return 4.0 * p - 3.0
    if l == 1:
        return 4.0 - 8.0 * p
    return 4.0 * p - 1.0


def _p2_simplex(dim, pt):
    """(N[a], dN[a][k]) of the order-2 simplex at the reference point pt, as Python floats."""
    L = [(1.0 - pt[0]) - pt[1], pt[0], pt[1]] if dim == 2 else [((1.0 - pt[0]) - pt[1]) - pt[2], pt[0], pt[1], pt[2]]
    D = TRI_D if dim == 2 else TET_D
    N = [L[i] * (2.0 * L[i] - 1.0) for i in range(dim + 1)]
    dN = [tuple((4.0 * L[i] - 1.0) * D[i][k] for k in range(dim)) for i in range(dim + 1)]
    for (i, j) in P2_EDGES[dim]:
        N.append((4.0 * L[i]) * L[j])
        dN.append(tuple((4.0 * L[i]) * D[j][k] + (4.0 * L[j]) * D[i][k] for k in range(dim)))
    return N, dN


def point_weight(dim, nd, q):
    """weight of point q of the type's rule"""
    if (dim, nd) == (2, 9):
        return GAUSS3_W[q % 3] * GAUSS3_W[q // 3]
    if (dim, nd) == (3, 27):
        return (GAUSS3_W[q % 3] * GAUSS3_W[(q // 3) % 3]) * GAUSS3_W[q // 9]
    return WEIGHT[(dim, nd)]


def rule_point(dim, nd, q):
    """the reference point q of the type's stiffness rule; None for the order-1 simplices, whose gradients are the same everywhere"""
    if (dim, nd) == (2, 9):
        return (GAUSS3[q % 3], GAUSS3[q // 3])
    if (dim, nd) == (3, 27):
        return (GAUSS3[q % 3], GAUSS3[(q // 3) % 3], GAUSS3[q // 9])
    if (dim, nd) == (2, 6):
        return WEDGE_TRI[q]
    if (dim, nd) == (3, 10):
        return TET_POINTS[q]
    if (dim, nd) in ((2, 3), (3, 4)):
        return None
    if (dim, nd) == (2, 4):
        return (GAUSS[q & 1], GAUSS[(q >> 1) & 1])
    if (dim, nd) == (3, 8):
        return (GAUSS[q & 1], GAUSS[(q >> 1) & 1], GAUSS[(q >> 2) & 1])
    if (dim, nd) == (3, 6):
        return WEDGE_TRI[q % 3] + (GAUSS[q // 3],)
    raise ValueError("%d nodes: no supported element type in %dD" % (nd, dim))


def gradients_at(dim, nd, pt):
    """dN[a][j] of the type at the reference point pt, as Python floats: the one statement of every type's gradients (the rules'
    tables and the tables at the face points are this function at their points)."""
    if (dim, nd) == (2, 9):
        px, py = pt
        return [(_d2(ix, px) * _n2(iy, py), _n2(ix, px) * _d2(iy, py)) for (ix, iy) in Q2_QUAD_LOC]
    if (dim, nd) == (3, 27):
        px, py, pz = pt
        return [(_d2(ix, px) * (_n2(iy, py) * _n2(iz, pz)), _d2(iy, py) * (_n2(ix, px) * _n2(iz, pz)),
                 _d2(iz, pz) * (_n2(ix, px) * _n2(iy, py))) for (ix, iy, iz) in Q2_HEX_LOC]
    if (dim, nd) in P2_SIMPLEX:
        return _p2_simplex(dim, pt)[1]
    if (dim, nd) == (2, 3):
        return [tuple(d) for d in TRI_D]
    if (dim, nd) == (3, 4):
        return [tuple(d) for d in TET_D]
    if (dim, nd) == (2, 4):
        px, py = pt
        return [(_df(lx) * _f(ly, py), _f(lx, px) * _df(ly)) for (lx, ly) in QUAD_LOC]
    if (dim, nd) == (3, 8):
        px, py, pz = pt
        return [(_df(lx) * (_f(ly, py) * _f(lz, pz)), _df(ly) * (_f(lx, px) * _f(lz, pz)), _df(lz) * (_f(lx, px) * _f(ly, py)))
                for (lx, ly, lz) in HEX_LOC]
    if (dim, nd) == (3, 6):
        xi, eta, zeta = pt
        T = ((1.0 - xi) - eta, xi, eta)
        L = (1.0 - zeta, zeta)
        return [(TRI_D[i][0] * L[a], TRI_D[i][1] * L[a], T[i] * _df(a)) for a in (0, 1) for i in (0, 1, 2)]
    raise ValueError("%d nodes: no supported element type in %dD" % (nd, dim))


def reference_gradients(dim, nd, q):
    """dN[a][j] at point q of the type's rule, as Python floats."""
    return gradients_at(dim, nd, rule_point(dim, nd, q))


def _cofactors(J, dim):
    """(C, det): C[i][j] the cofactor of J[i][j]."""
    if dim == 2:
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
        return [[J[1][1], -J[1][0]], [-J[0][1], J[0][0]]], det
    C = [[J[1][1] * J[2][2] - J[1][2] * J[2][1], J[1][2] * J[2][0] - J[1][0] * J[2][2], J[1][0] * J[2][1] - J[1][1] * J[2][0]],
         [J[0][2] * J[2][1] - J[0][1] * J[2][2], J[0][0] * J[2][2] - J[0][2] * J[2][0], J[0][1] * J[2][0] - J[0][0] * J[2][1]],
         [J[0][1] * J[1][2] - J[0][2] * J[1][1], J[0][2] * J[1][0] - J[0][0] * J[1][2], J[0][0] * J[1][1] - J[0][1] * J[1][0]]]
    det = (J[0][0] * C[0][0] + J[0][1] * C[0][1]) + J[0][2] * C[0][2]
    return C, det


def _dot(u, v, dim):
    s = u[0] * v[0] + u[1] * v[1]
    return s + u[2] * v[2] if dim == 3 else s


def _tensor(coef, dim):
    """The symmetric tensor's entries K[i][j] as arrays over the elements."""
    n, ncoef = coef.shape
    zero = np.zeros(n)
    if ncoef == 1:
        d = [coef[:, 0]] * dim
        o = [zero] * 3
    elif ncoef == dim:
        d = [coef[:, i] for i in range(dim)]
        o = [zero] * 3
    else:                                    # xx, yy, zz, xy, yz, xz / xx, yy, xy
        d = [coef[:, i] for i in range(dim)]
        o = [coef[:, dim + i] for i in range(ncoef - dim)]
    if dim == 2:
        return [[d[0], o[0]], [o[0], d[1]]]
    return [[d[0], o[0], o[2]], [o[0], d[1], o[1]], [o[2], o[1], d[2]]]


def _block(X, dim, nd, kind, coef, rows=None):
    """Matrices (n, size, size) of n elements of one type, and per element whether a det was not positive.  The node pairs
    (a, b) with a <= b are the lanes of one vector: every line below is the scalar formula of the entry, elementwise.
    rows None: coef holds one row per element and the rule is the type's stiffness rule.  Otherwise (element_matrices_points)
    the rule is the type's MASS rule and point q of element k takes the row rows[k] + q of coef; nothing else differs."""
    n = X.shape[0]
    size = nd if kind == 0 else dim * nd
    bad = np.zeros(n, bool)
    pa, pb = np.triu_indices(nd)                                     # the pairs a <= b
    acc = np.zeros((n, len(pa)) if kind == 0 else (n, len(pa), dim, dim))
    npoints, gradients, weight = (NPOINTS, reference_gradients, point_weight) if rows is None else \
        (MASS_NPOINTS, mass_reference_gradients, mass_point_weight)
    with np.errstate(all="ignore"):
        for q in range(npoints[(dim, nd)]):
            cq = coef if rows is None else coef[rows + q]
            K = _tensor(cq, dim) if kind == 0 else None
            dN = gradients(dim, nd, q)
            J = [[None] * dim for _ in range(dim)]
            for i in range(dim):
                for j in range(dim):
                    s = X[:, 0, i] * dN[0][j]
                    for a in range(1, nd):
                        s = s + X[:, a, i] * dN[a][j]
                    J[i][j] = s
            C, det = _cofactors(J, dim)
            bad |= ~(det > 0.0)
            s = (weight(dim, nd, q) / det)[:, None]
            dA = np.array(dN)                                        # (nd, dim)
            G = []                                                   # G[i]: (n, nd), component i of every node's gradient
            for i in range(dim):
                t = dA[None, :, 0] * C[i][0][:, None] + dA[None, :, 1] * C[i][1][:, None]
                if dim == 3:
                    t = t + dA[None, :, 2] * C[i][2][:, None]
                G.append(t)
            Ga, Gb = [g[:, pa] for g in G], [g[:, pb] for g in G]
            if kind == 0:
                F = []
                for i in range(dim):
                    t = K[i][0][:, None] * G[0] + K[i][1][:, None] * G[1]
                    if dim == 3:
                        t = t + K[i][2][:, None] * G[2]
                    F.append(t[:, pa])
                term = s * _dot(F, Gb, dim)
                acc = acc + term
            else:
                lam, mu = cq[:, 0][:, None], cq[:, 1][:, None]
                md = mu * _dot(Ga, Gb, dim)
                for i in range(dim):
                    for j in range(dim):                             # (on a == b the entries with i > j are not used)
                        t = lam * (Ga[i] * Gb[j]) + mu * (Ga[j] * Gb[i])
                        if i == j:
                            t = t + md
                        term = s * t
                        acc[:, :, i, j] = acc[:, :, i, j] + term
    out = np.zeros((n, size, size))
    if kind == 0:
        out[:, pa, pb] = acc
    else:
        for i in range(dim):
            for j in range(dim):
                out[:, dim * pa + i, dim * pb + j] = acc[:, :, i, j]
    iu = np.triu_indices(size, 1)
    out[:, iu[1], iu[0]] = out[:, iu[0], iu[1]]
    return out, bad


def allowed_ncoef(dim, kind):
    return (2,) if kind == 1 else tuple(sorted({1, dim, dim * (dim + 1) // 2}))


def _mesh(coords, elem_to_vertex, elem_ptr):
    X = np.asarray(coords, np.float64)
    if X.ndim != 2 or X.shape[1] not in (2, 3):
        raise ValueError("coords: (NV, dim) with dim 2 or 3 is needed")
    NV, dim = X.shape
    e2v = np.asarray(elem_to_vertex)
    if elem_ptr is None:
        if e2v.ndim != 2:
            raise ValueError("elem_to_vertex: (NE, nodes) is needed without elem_ptr")
        ep = np.arange(e2v.shape[0] + 1, dtype=np.int64) * e2v.shape[1]
    else:
        ep = np.asarray(elem_ptr, np.int64)
        if ep.ndim != 1 or len(ep) < 1 or ep[0] != 0:
            raise ValueError("elem_ptr: must start at 0")
        if (np.diff(ep) <= 0).any():
            raise ValueError("elem_ptr: every element needs a vertex")
    e2v = e2v.astype(np.int64).ravel()
    if len(e2v) != ep[-1]:
        raise ValueError("elem_to_vertex: elem_ptr[NE] entries are needed")
    if len(e2v) and (e2v.min() < 0 or e2v.max() >= NV):
        raise ValueError("elem_to_vertex entry out of range")
    nd = np.diff(ep)
    elem = np.repeat(np.arange(len(nd), dtype=np.int64), nd)
    if len(np.unique(elem * max(int(NV), 1) + e2v)) != len(e2v):
        raise ValueError("an element lists a vertex twice")
    for e in np.flatnonzero(~np.isin(nd, [k[1] for k in ALL_TYPE_INDEX if k[0] == dim])):
        raise ValueError("element %d: %d nodes are no supported element type in %dD" % (e, nd[e], dim))
    return X, dim, ep, e2v, nd


def element_matrices(coords, elem_to_vertex, kind, coef, elem_ptr=None):
    """The element matrices: (NE, size, size) when elem_ptr is None, else packed.  coef: (NE,) or (NE, ncoef)."""
    if kind not in (0, 1):
        raise ValueError("kind: 0 (diffusion) or 1 (elasticity)")
    X, dim, ep, e2v, nd = _mesh(coords, elem_to_vertex, elem_ptr)
    NE = len(nd)
    coef = np.asarray(coef, np.float64).reshape(NE, -1) if NE else np.zeros((0, allowed_ncoef(dim, kind)[0]))
    if coef.shape[1] not in allowed_ncoef(dim, kind):
        raise ValueError("ncoef = %d is not allowed for kind %d in %dD" % (coef.shape[1], kind, dim))
    comp = 1 if kind == 0 else dim
    moff = np.concatenate([[0], np.cumsum((nd * comp) ** 2)])
    out = np.zeros(int(moff[-1]))
    bad = np.zeros(NE, bool)
    for c in np.unique(nd):
        ids = np.flatnonzero(nd == c)
        blk, bad[ids] = _block(X[e2v[ep[ids][:, None] + np.arange(c)]], dim, int(c), kind, coef[ids])
        out[moff[ids][:, None] + np.arange((c * comp) ** 2)] = blk.reshape(len(ids), -1)
    if bad.any():
        raise ElementError(np.flatnonzero(bad)[0])
    if elem_ptr is None:
        return out.reshape(NE, nd[0] * comp, nd[0] * comp) if NE else out.reshape(0, 0, 0)
    return out


def type_counts(dim, elem_to_vertex, elem_ptr=None):
    """[triangles, quadrilaterals, tetrahedra, wedges, hexahedra]"""
    nd = np.diff(np.asarray(elem_ptr, np.int64)) if elem_ptr is not None else \
        np.full(np.asarray(elem_to_vertex).shape[0], np.asarray(elem_to_vertex).shape[1])
    out = [0] * 5
    for (d, k), t in TYPE_INDEX.items():
        if d == dim:
            out[t] = int((nd == k).sum())
    return out


def order2_count(dim, elem_to_vertex, elem_ptr=None):
    """the number of order-2 elements of all four types (info[7] of saamge_amd_element_matrices)"""
    nd = np.diff(np.asarray(elem_ptr, np.int64)) if elem_ptr is not None else \
        np.full(np.asarray(elem_to_vertex).shape[0], np.asarray(elem_to_vertex).shape[1])
    return int(sum((nd == k).sum() for (d, k) in ORDER2 if d == dim))


def dof_lists(dim, elem_to_vertex, kind, elem_ptr=None):
    """(dof_ptr, elem_to_dof), both int32 and flat: the dofs the matrices are indexed by -- kind 0 the vertex lists, kind 1
    dim * vertex + component."""
    e2v = np.asarray(elem_to_vertex)
    ep = np.arange(e2v.shape[0] + 1, dtype=np.int64) * e2v.shape[1] if elem_ptr is None else np.asarray(elem_ptr, np.int64)
    e2v = e2v.astype(np.int64).ravel()
    if kind == 0:
        return ep.astype(np.int32), e2v.astype(np.int32)
    return (ep * dim).astype(np.int32), (dim * e2v[:, None] + np.arange(dim)[None, :]).ravel().astype(np.int32)


# ---- mass matrices and load vectors (zeroth-order forms) ---------------------------------------------------------------------
#   rule         the type's rule above, except the simplices (one point is not enough for a product of two shape functions):
#                triangle: the three points of WEDGE_TRI, weight 1/6 each; tetrahedron: four points, weight 1/24 each, point 0
#                (TET_A, TET_A, TET_A) and point q = 1 .. 3 with coordinate q - 1 replaced by TET_B.  Order-2 simplices:
#                triangle 6 points in two orbits (a, a), (b, a), (a, b) with b = 1.0 - 2.0 * a; tetrahedron 14 points: two
#                orbits (a, a, a), (b, a, a), (a, b, a), (a, a, b) with b = 1.0 - 3.0 * a, then one point per edge (i, j) in
#                the order of P2_EDGES whose barycentric coordinates i and j are b = 0.5 - a and the other two a, the point
#                being (L_1, L_2, L_3).  Their shape values and gradients are _p2_simplex's AT THE MASS POINTS
#                (mass_reference_gradients: the gradients are not constant).
#   shapes       N_a at a point, written out like the gradients (shape_values).
#   point        J, the cofactors and det exactly as above, from the type's gradients at that point (constant for the
#                simplices, formed per point all the same); a det that is not positive refuses the element;
#                s = (weight * det) * c_e -- no division.
#   mass         entry (a, b) with a <= b gets s * (N_a * N_b) per point, summed over the points in ascending order from 0.0;
#                (b, a) is the same double.  vdim = dim: dof dim * a + i, entry ((a, i), (b, j)) the scalar entry when i == j
#                and +0.0 otherwise.  add_to: the result is add_to + m, one addition per entry after m is complete.
#   loads        src nodal (NV, vdim): per point fq_i = sum_c N_c * src[c][i], nodes ascending, the first product as it is;
#                dof (a, i) gets (s * fq_i) * N_a, summed over the points from 0.0.  coef None: 1.0.  Packed: element e at
#                sum_{f<e} size_f; (NE, size) when elem_ptr is None.
TET_A, TET_B = 0.1381966011250105, 0.5854101966249685    # (5 - sqrt 5) / 20, (5 + 3 sqrt 5) / 20
TET_POINTS = [(TET_A, TET_A, TET_A), (TET_B, TET_A, TET_A), (TET_A, TET_B, TET_A), (TET_A, TET_A, TET_B)]
MASS_NPOINTS = dict(NPOINTS)
MASS_NPOINTS.update({(2, 3): 3, (3, 4): 4})
MASS_WEIGHT = {(2, 3): 0.16666666666666666, (3, 4): 0.041666666666666664}
P2_TRI_A = (0.44594849091596483, 0.09157621350977073)
P2_TRI_W = tuple(w for w in (0.11169079483900572, 0.054975871827660935) for _ in range(3))
P2_TRI_POINTS = [p for a in P2_TRI_A for b in (1.0 - 2.0 * a,) for p in ((a, a), (b, a), (a, b))]
P2_TET_A = (0.3108859192633006, 0.09273525031089122)
P2_TET_EDGE_A = 0.04550370412564965
P2_TET_W = tuple(w for w in (0.018781320953002643, 0.012248840519393659) for _ in range(4)) + (0.007091003462846911,) * 6
P2_TET_POINTS = [p for a in P2_TET_A for b in (1.0 - 3.0 * a,) for p in ((a, a, a), (b, a, a), (a, b, a), (a, a, b))] + \
    [tuple((0.5 - P2_TET_EDGE_A) if k in e else P2_TET_EDGE_A for k in (1, 2, 3)) for e in P2_EDGES[3]]
MASS_NPOINTS.update({(2, 6): 6, (3, 10): 14})


def mass_point_weight(dim, nd, q):
    """weight of point q of the type's mass rule"""
    if (dim, nd) == (2, 6):
        return P2_TRI_W[q]
    if (dim, nd) == (3, 10):
        return P2_TET_W[q]
    return MASS_WEIGHT[(dim, nd)] if (dim, nd) in MASS_WEIGHT else point_weight(dim, nd, q)


def mass_reference_gradients(dim, nd, q):
    """dN[a][j] at point q of the type's MASS rule: the stiffness rule's, except for the order-2 simplices"""
    if (dim, nd) == (2, 6):
        return gradients_at(2, 6, P2_TRI_POINTS[q])
    if (dim, nd) == (3, 10):
        return gradients_at(3, 10, P2_TET_POINTS[q])
    return reference_gradients(dim, nd, q)


def shape_values(dim, nd, q):
    """N[a] at point q of the type's mass rule, as Python floats."""
    if (dim, nd) == (2, 9):
        px, py = GAUSS3[q % 3], GAUSS3[q // 3]
        return [_n2(ix, px) * _n2(iy, py) for (ix, iy) in Q2_QUAD_LOC]
    if (dim, nd) == (3, 27):
        px, py, pz = GAUSS3[q % 3], GAUSS3[(q // 3) % 3], GAUSS3[q // 9]
        return [_n2(ix, px) * (_n2(iy, py) * _n2(iz, pz)) for (ix, iy, iz) in Q2_HEX_LOC]
    if (dim, nd) == (2, 6):
        return _p2_simplex(2, P2_TRI_POINTS[q])[0]
    if (dim, nd) == (3, 10):
        return _p2_simplex(3, P2_TET_POINTS[q])[0]
    if (dim, nd) == (2, 3):
        x, y = WEDGE_TRI[q]
        return [(1.0 - x) - y, x, y]
    if (dim, nd) == (3, 4):
        x, y, z = TET_POINTS[q]
        return [((1.0 - x) - y) - z, x, y, z]
    if (dim, nd) == (2, 4):
        px, py = GAUSS[q & 1], GAUSS[(q >> 1) & 1]
        return [_f(lx, px) * _f(ly, py) for (lx, ly) in QUAD_LOC]
    if (dim, nd) == (3, 8):
        px, py, pz = GAUSS[q & 1], GAUSS[(q >> 1) & 1], GAUSS[(q >> 2) & 1]
        return [_f(lx, px) * (_f(ly, py) * _f(lz, pz)) for (lx, ly, lz) in HEX_LOC]
    if (dim, nd) == (3, 6):
        xi, eta = WEDGE_TRI[q % 3]
        zeta = GAUSS[q // 3]
        T = ((1.0 - xi) - eta, xi, eta)
        L = (1.0 - zeta, zeta)
        return [T[i] * L[a] for a in (0, 1) for i in (0, 1, 2)]
    raise ValueError("%d nodes: no supported element type in %dD" % (nd, dim))


def _mass_points(X, dim, nd, c, rows=None):
    """Per point of the mass rule: (N, s) with s = (weight * det) * c over the n elements of X, and per element whether a det
    was not positive.  rows (element_mass_points): c holds one coefficient per point, point q of element k takes c[rows[k] + q]."""
    bad = np.zeros(X.shape[0], bool)
    out = []
    with np.errstate(all="ignore"):
        for q in range(MASS_NPOINTS[(dim, nd)]):
            dN = mass_reference_gradients(dim, nd, q)                # (the order-1 simplices': the same at every point)
            J = [[None] * dim for _ in range(dim)]
            for i in range(dim):
                for j in range(dim):
                    t = X[:, 0, i] * dN[0][j]
                    for a in range(1, nd):
                        t = t + X[:, a, i] * dN[a][j]
                    J[i][j] = t
            _, det = _cofactors(J, dim)
            bad |= ~(det > 0.0)
            cq = c if rows is None else c[rows + q]
            out.append((shape_values(dim, nd, q), (mass_point_weight(dim, nd, q) * det) * cq))
    return out, bad


def _mass_block(X, dim, nd, c, rows=None):
    """Scalar mass matrices (n, nd, nd) of n elements of one type; rows: as in _mass_points."""
    n = X.shape[0]
    pa, pb = np.triu_indices(nd)
    acc = np.zeros((n, len(pa)))
    points, bad = _mass_points(X, dim, nd, c, rows)
    with np.errstate(all="ignore"):
        for N, s in points:
            NN = np.array([N[a] * N[b] for a, b in zip(pa, pb)])
            term = s[:, None] * NN[None, :]
            acc = acc + term
    out = np.zeros((n, nd, nd))
    out[:, pa, pb] = acc
    out[:, pb, pa] = acc
    return out, bad


def _load_block(X, dim, nd, c, F):
    """Load vectors (n, nd, vdim) of n elements of one type; F: (n, nd, vdim) the nodal source."""
    n, vdim = X.shape[0], F.shape[2]
    acc = np.zeros((n, nd, vdim))
    points, bad = _mass_points(X, dim, nd, c)
    with np.errstate(all="ignore"):
        for N, s in points:
            fq = N[0] * F[:, 0, :]
            for a in range(1, nd):
                fq = fq + N[a] * F[:, a, :]
            sf = s[:, None] * fq
            term = sf[:, None, :] * np.array(N)[None, :, None]
            acc = acc + term
    return acc, bad


def _vdim(vdim, dim):
    if vdim not in (1, dim):
        raise ValueError("vdim: 1 or dim")
    return int(vdim)


def element_mass(coords, elem_to_vertex, coef, vdim=1, elem_ptr=None, add_to=None):
    """The mass matrices with the per-element coefficient coef (NE,): (NE, size, size) when elem_ptr is None, else packed;
    size = vdim * nodes.  add_to: matrices of the same layout (diffusion for vdim 1, elasticity for vdim dim) the result is
    added to."""
    X, dim, ep, e2v, nd = _mesh(coords, elem_to_vertex, elem_ptr)
    vdim = _vdim(vdim, dim)
    NE = len(nd)
    if coef is None:
        raise ValueError("coef: (NE,) is needed")
    coef = np.asarray(coef, np.float64).reshape(-1)
    if len(coef) != NE:
        raise ValueError("coef: (NE,) is needed")
    moff = np.concatenate([[0], np.cumsum((nd * vdim) ** 2)])
    out = np.zeros(int(moff[-1]))
    bad = np.zeros(NE, bool)
    for c in np.unique(nd):
        ids = np.flatnonzero(nd == c)
        c = int(c)
        m, bad[ids] = _mass_block(X[e2v[ep[ids][:, None] + np.arange(c)]], dim, c, coef[ids])
        if vdim > 1:
            full = np.zeros((len(ids), c, vdim, c, vdim))
            for i in range(vdim):
                full[:, :, i, :, i] = m
            m = full
        out[moff[ids][:, None] + np.arange((c * vdim) ** 2)] = m.reshape(len(ids), -1)
    if bad.any():
        raise ElementError(np.flatnonzero(bad)[0])
    if add_to is not None:
        base = np.asarray(add_to, np.float64).ravel()
        if len(base) != len(out):
            raise ValueError("add_to: the layout of the result is needed")
        out = base + out
    if elem_ptr is None:
        return out.reshape(NE, nd[0] * vdim, nd[0] * vdim) if NE else out.reshape(0, 0, 0)
    return out


def element_loads(coords, elem_to_vertex, src, vdim=1, coef=None, elem_ptr=None):
    """The load vectors of the nodal source src (NV, vdim) (or (NV,) for vdim 1) with the per-element coefficient coef (NE,),
    None: 1.0.  (NE, size) when elem_ptr is None, else packed."""
    X, dim, ep, e2v, nd = _mesh(coords, elem_to_vertex, elem_ptr)
    vdim = _vdim(vdim, dim)
    NE, NV = len(nd), X.shape[0]
    if src is None:
        raise ValueError("src: (NV, vdim) is needed")
    F = np.asarray(src, np.float64)
    if F.size != NV * vdim:
        raise ValueError("src: (NV, vdim) is needed")
    F = F.reshape(NV, vdim)
    coef = np.ones(NE) if coef is None else np.asarray(coef, np.float64).reshape(-1)
    if len(coef) != NE:
        raise ValueError("coef: (NE,) is needed")
    voff = np.concatenate([[0], np.cumsum(nd * vdim)])
    out = np.zeros(int(voff[-1]))
    bad = np.zeros(NE, bool)
    for c in np.unique(nd):
        ids = np.flatnonzero(nd == c)
        c = int(c)
        v = e2v[ep[ids][:, None] + np.arange(c)]
        blk, bad[ids] = _load_block(X[v], dim, c, coef[ids], F[v])
        out[voff[ids][:, None] + np.arange(c * vdim)] = blk.reshape(len(ids), -1)
    if bad.any():
        raise ElementError(np.flatnonzero(bad)[0])
    if elem_ptr is None:
        return out.reshape(NE, nd[0] * vdim) if NE else out.reshape(0, 0)
    return out


# ---- boundary forms: the face mass (Robin) and the face loads (Neumann) ---------------------------------------------------------
#   face         a pair (element id, local face index); FACE_NODES[(dim, nodes)][local face] lists the element's local node ids of
#                the face in the node order of the face's own type: the 2-node / 3-node segment (start, end / start, middle, end),
#                the triangle, the 4-node quadrilateral (QUAD_LOC order), the 9-node quadrilateral (Q2_QUAD_LOC order) and the
#                6-node triangle (the three vertices, then the midpoints of (v0, v1), (v1, v2), (v2, v0): the order of (2, 6)).
#                The P2 triangle's faces are 3-node segments, the P2 tetrahedron's four faces are those of the tetrahedron as
#                6-node triangles (believed to be MFEM's orientation, like the rest of the table; the table is the definition).
#   rule         of the face type (face_rule): the 2-node segment has the 2 GAUSS points, weight 0.5 each, shapes _f, derivatives
#                _df; the 3-node segment GAUSS3 / GAUSS3_W, _n2, _d2; a triangle, 4-node or 9-node quadrilateral face has the mass
#                rule, shape values and reference gradients of the element type (2, 3), (2, 4), (2, 9); a 6-node triangle
#                those of (2, 6): the 6-point rule.
#   point        tangents t_j[i] = sum over the face nodes c, ascending, of x_c[i] * dN_c[j], the first product as it is;
#                dim 2: m2 = t[0] * t[0] + t[1] * t[1]; dim 3: n = t_0 x t_1 (n0 = t0y * t1z - t0z * t1y, n1 = t0z * t1x - t0x * t1z,
#                n2 = t0x * t1y - t0y * t1x), m2 = (n0 * n0 + n1 * n1) + n2 * n2; meas = sqrt(m2), correctly rounded;
#                s = (w * meas) * c_f with the coefficient c_f of the face.  A face with a point where not (meas > 0) is refused.
#   mass         face entry (a, b), a <= b in face-node order, is the sum over the points, ascending from 0.0, of s * (N_a * N_b);
#                (b, a) is the same double.  The complete face matrix is added to the owning element's packed matrix, one addition
#                per entry: vdim 1 at (node a, node b), vdim = dim at ((a, i), (b, i)) for every component i.  Entries no listed
#                face touches keep their bits.  The faces of one element are added in ascending local face index, whatever the
#                order of the list.
#   loads        g nodal (NV, vdim): per point gq_i = sum over the face nodes c, ascending, of N_c * g[c][i]; face dof (a, i) gets
#                the sum over the points from 0.0 of (s * gq_i) * N_a, added to the element's packed vector at the dof of local
#                node a, same face order.  coef None: 1.0.
#   refused      vdim, missing arguments, what _mesh refuses, then the first face (lowest index in the list) with face_elem outside
#                [0, NE) or face_local outside the type's range, then the first face whose (element, local face) the list holds
#                more than once, then the first face with a non-positive measure (FaceError, .face).
def _hex27_faces(hex_faces):
    out = []
    for c in hex_faces:
        P = [np.array(HEX_LOC[k]) * 2 for k in c]
        face = []
        for (u, v) in Q2_QUAD_LOC:
            ix, iy, iz = P[0] + u * (P[1] - P[0]) // 2 + v * (P[3] - P[0]) // 2
            face.append(int((iz * 3 + iy) * 3 + ix))
        out.append(tuple(face))
    return tuple(out)


_HEX_FACES = ((3, 2, 1, 0), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7), (4, 5, 6, 7))
FACE_NODES = {
    (2, 3): ((0, 1), (1, 2), (2, 0)),
    (2, 4): ((0, 1), (1, 2), (2, 3), (3, 0)),
    (2, 9): ((0, 4, 1), (1, 5, 2), (2, 6, 3), (3, 7, 0)),
    (2, 6): ((0, 3, 1), (1, 4, 2), (2, 5, 0)),
    (3, 10): ((1, 2, 3, 7, 9, 8), (0, 3, 2, 6, 9, 5), (0, 1, 3, 4, 8, 6), (0, 2, 1, 5, 7, 4)),
    (3, 4): ((1, 2, 3), (0, 3, 2), (0, 1, 3), (0, 2, 1)),
    (3, 6): ((0, 2, 1), (3, 4, 5), (0, 1, 4, 3), (1, 2, 5, 4), (2, 0, 3, 5)),
    (3, 8): _HEX_FACES,
    (3, 27): _hex27_faces(_HEX_FACES),
}
# (dim, face nodes) -> info[0..4] of saamge_amd_boundary_mass / _loads: 2-node segments, 3-node segments, triangles, 4-node
# quadrilaterals, 9-node quadrilaterals.  The 6-node triangle is face type 5; info counts it with the triangles
# (face_info_index): info[1] counts the 3-node segments whichever element type owns them, info[2] the triangular faces of 3
# and of 6 nodes.
FACE_TYPE_INDEX = {(2, 2): 0, (2, 3): 1, (3, 3): 2, (3, 4): 3, (3, 9): 4, (3, 6): 5}


def face_info_index(dim, fn):
    """the entry of info[0..4] of saamge_amd_boundary_mass / _loads that counts the faces of this type"""
    t = FACE_TYPE_INDEX[(dim, fn)]
    return 2 if t == 5 else t

MAX_FACES = 6


class FaceError(ValueError):
    """A refused face of a face list; .face is its index in the list (the smallest such index)."""

    def __init__(self, face, what):
        ValueError.__init__(self, "face %d: %s" % (face, what))
        self.face = int(face)


def face_rule(dim, fn):
    """The rule of the face type with fn nodes of a dim-dimensional element: per point (N[a], dN[a][j], weight)."""
    if (dim, fn) == (2, 2):
        return [([_f(0, p), _f(1, p)], [(_df(0),), (_df(1),)], 0.5) for p in GAUSS]
    if (dim, fn) == (2, 3):
        return [([_n2(k, p) for k in range(3)], [(_d2(k, p),) for k in range(3)], GAUSS3_W[q]) for q, p in enumerate(GAUSS3)]
    if (dim, fn) not in FACE_TYPE_INDEX:
        raise ValueError("%d nodes: no face type of a %dD element" % (fn, dim))
    return [(shape_values(2, fn, q), mass_reference_gradients(2, fn, q), mass_point_weight(2, fn, q))
            for q in range(MASS_NPOINTS[(2, fn)])]


def _face_points(X, dim, fn, c, rows=None, geom=False):
    """Per point of the face rule: (N, s) with s = (weight * meas) * c over the n faces of X (n, fn, dim), and per face whether
    a measure was not positive.  rows (boundary_mass_points): c holds one coefficient per point, point q of face k takes
    c[rows[k] + q].  geom (boundary_points): (N, s, normal) with the unit normal, its dim components each divided by meas."""
    bad = np.zeros(X.shape[0], bool)
    out = []
    with np.errstate(all="ignore"):
        for q, (N, dN, w) in enumerate(face_rule(dim, fn)):
            t = [[None] * dim for _ in range(dim - 1)]
            for j in range(dim - 1):
                for i in range(dim):
                    v = X[:, 0, i] * dN[0][j]
                    for a in range(1, fn):
                        v = v + X[:, a, i] * dN[a][j]
                    t[j][i] = v
            if dim == 2:
                m2 = t[0][0] * t[0][0] + t[0][1] * t[0][1]
                nrm = (t[0][1], -t[0][0])
            else:
                (ax, ay, az), (bx, by, bz) = t
                n0, n1, n2 = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
                m2 = (n0 * n0 + n1 * n1) + n2 * n2
                nrm = (n0, n1, n2)
            meas = np.sqrt(m2)
            bad |= ~(meas > 0.0)
            s = (w * meas) * (c if rows is None else c[rows + q])
            out.append((N, s, np.stack([v / meas for v in nrm], axis=1)) if geom else (N, s))
    return out, bad


def _face_list(dim, nd, face_elem, face_local):
    """The checked face list as int64 arrays."""
    if face_elem is None or face_local is None:
        raise ValueError("face_elem and face_local: (NF,) are needed")
    fe, fl = np.asarray(face_elem).astype(np.int64).ravel(), np.asarray(face_local).astype(np.int64).ravel()
    if len(fe) != len(fl):
        raise ValueError("face_elem and face_local: (NF,) are needed")
    NE = len(nd)
    wrong_e = (fe < 0) | (fe >= NE)
    nfaces = np.zeros(len(fe), np.int64)
    counts = {k[1]: len(v) for k, v in FACE_NODES.items() if k[0] == dim}
    if NE:
        nfaces[~wrong_e] = np.array([counts[int(c)] for c in nd[fe[~wrong_e]]], np.int64)
    wrong = wrong_e | (fl < 0) | (fl >= nfaces)
    if wrong.any():
        f = int(np.flatnonzero(wrong)[0])
        raise FaceError(f, "face_elem is outside [0, NE)" if wrong_e[f] else "face_local is outside the element type's range")
    key = fe * MAX_FACES + fl
    uniq, first, count = np.unique(key, return_index=True, return_counts=True)
    if (count > 1).any():
        raise FaceError(int(first[count > 1].min()), "the same (element, local face) is listed twice")
    return fe, fl


def _face_buckets(dim, nd, fe, fl):
    """(local face, nodes of the element type, the faces of the list): by ascending local face, then node count."""
    for lf in range(MAX_FACES):
        sel = np.flatnonzero(fl == lf)
        for c in np.unique(nd[fe[sel]]):
            yield lf, int(c), sel[nd[fe[sel]] == c]


def _face_coef(coef, NF, needed):
    if coef is None:
        if needed:
            raise ValueError("coef: (NF,) is needed")
        return np.ones(NF)
    coef = np.asarray(coef, np.float64).reshape(-1)
    if len(coef) != NF:
        raise ValueError("coef: (NF,) is needed")
    return coef


def _refuse_measure(bad):
    if bad.any():
        raise FaceError(int(np.flatnonzero(bad)[0]), "the measure is not positive")


def boundary_mass(coords, elem_to_vertex, face_elem, face_local, coef, vdim=1, elem_ptr=None, add_to=None):
    """add_to plus the face mass matrices (coef_f u, v)_face of the listed faces, coef (NF,): a new array in the layout of
    add_to, which is that of element_matrices / element_mass ((NE, size, size) when elem_ptr is None, else packed)."""
    X, dim, ep, e2v, nd = _mesh(coords, elem_to_vertex, elem_ptr)
    vdim = _vdim(vdim, dim)
    if coef is None:
        raise ValueError("coef: (NF,) is needed")
    fe, fl = _face_list(dim, nd, face_elem, face_local)
    coef = _face_coef(coef, len(fe), True)
    return _add_face_mass(X, dim, ep, e2v, nd, vdim, fe, fl, coef, None, add_to, elem_ptr is None)


def _add_face_mass(X, dim, ep, e2v, nd, vdim, fe, fl, coef, fp, add_to, square):
    """boundary_mass after its checks.  fp None: coef (NF,) per face; else (boundary_mass_points) coef (NFQ,) per point, point q
    of face f at fp[f] + q."""
    if add_to is None:
        raise ValueError("add_to: the matrices the faces are added to are needed")
    moff = np.concatenate([[0], np.cumsum((nd * vdim) ** 2)])
    out = np.array(add_to, np.float64).ravel()
    if len(out) != moff[-1]:
        raise ValueError("add_to: the layout of element_matrices is needed")
    bad = np.zeros(len(fe), bool)
    with np.errstate(all="ignore"):
        for lf, c, ids in _face_buckets(dim, nd, fe, fl):
            nodes = np.array(FACE_NODES[(dim, c)][lf])
            fn, S = len(nodes), c * vdim
            points, bad[ids] = _face_points(X[e2v[ep[fe[ids]][:, None] + nodes]], dim, fn, coef[ids] if fp is None else coef,
                                            None if fp is None else fp[ids])
            pa, pb = np.triu_indices(fn)
            acc = np.zeros((len(ids), len(pa)))
            for N, s in points:
                NN = np.array([N[a] * N[b] for a, b in zip(pa, pb)])
                term = s[:, None] * NN[None, :]
                acc = acc + term
            base = moff[fe[ids]]
            for k, (a, b) in enumerate(zip(pa, pb)):
                for i in range(vdim):
                    r, cc = vdim * nodes[a] + i, vdim * nodes[b] + i
                    for idx in ([base + r * S + cc] if a == b else [base + r * S + cc, base + cc * S + r]):
                        out[idx] = out[idx] + acc[:, k]          # (an element occurs once in a bucket: no index twice)
    _refuse_measure(bad)
    if square:
        return out.reshape(len(nd), nd[0] * vdim, nd[0] * vdim) if len(nd) else out.reshape(0, 0, 0)
    return out


def boundary_loads(coords, elem_to_vertex, face_elem, face_local, g, vdim=1, coef=None, elem_ptr=None, add_to=None):
    """add_to plus the face load vectors (coef_f g, v)_face of the listed faces, g nodal (NV, vdim) or (NV,), coef (NF,) or None
    (1.0): a new array in the layout of add_to, which is that of element_loads."""
    X, dim, ep, e2v, nd = _mesh(coords, elem_to_vertex, elem_ptr)
    vdim = _vdim(vdim, dim)
    NV = X.shape[0]
    if g is None:
        raise ValueError("g: (NV, vdim) is needed")
    G = np.asarray(g, np.float64)
    if G.size != NV * vdim:
        raise ValueError("g: (NV, vdim) is needed")
    G = G.reshape(NV, vdim)
    fe, fl = _face_list(dim, nd, face_elem, face_local)
    coef = _face_coef(coef, len(fe), False)
    return _add_face_loads(X, dim, ep, e2v, nd, vdim, fe, fl, coef, G, None, add_to, elem_ptr is None)


def _add_face_loads(X, dim, ep, e2v, nd, vdim, fe, fl, coef, G, fp, add_to, rows):
    """boundary_loads after its checks.  fp None: G (NV, vdim) at the nodes; else (boundary_loads_points) G (NFQ, vdim) at the
    points, point q of face f at fp[f] + q, read where the nodal data is interpolated."""
    if add_to is None:
        raise ValueError("add_to: the vectors the faces are added to are needed")
    out = np.array(add_to, np.float64).ravel()
    if len(out) != ep[-1] * vdim:
        raise ValueError("add_to: the layout of element_loads is needed")
    bad = np.zeros(len(fe), bool)
    with np.errstate(all="ignore"):
        for lf, c, ids in _face_buckets(dim, nd, fe, fl):
            nodes = np.array(FACE_NODES[(dim, c)][lf])
            fn = len(nodes)
            v = e2v[ep[fe[ids]][:, None] + nodes]
            points, bad[ids] = _face_points(X[v], dim, fn, coef[ids])
            F = G[v] if fp is None else None                         # (n, fn, vdim)
            acc = np.zeros((len(ids), fn, vdim))
            for q, (N, s) in enumerate(points):
                if fp is None:
                    gq = N[0] * F[:, 0, :]
                    for a in range(1, fn):
                        gq = gq + N[a] * F[:, a, :]
                else:
                    gq = G[fp[ids] + q]
                sg = s[:, None] * gq
                term = sg[:, None, :] * np.array(N)[None, :, None]
                acc = acc + term
            idx = (ep[fe[ids]] * vdim)[:, None, None] + (vdim * nodes)[None, :, None] + np.arange(vdim)[None, None, :]
            out[idx] = out[idx] + acc
    _refuse_measure(bad)
    if rows:
        return out.reshape(len(nd), nd[0] * vdim) if len(nd) else out.reshape(0, 0)
    return out


# ---- data at the points of the mass rule: the points, evaluation, loads of point data, errors ----------------------------------------
#   points       the points of an element are those of its type's MASS rule (MASS_NPOINTS, shape_values, mass_reference_gradients,
#                mass_point_weight), in the rule's order; point q of element e has the global index qp_ptr[e] + q, qp_ptr (NE + 1,
#                int64), NQ = qp_ptr[NE].  xq[q][i] = sum over the nodes a, ascending, of N_a * x_a[i], the first product as it is;
#                wdet[q] = weight_q * det_q: the bits of s of _mass_points with the coefficient 1.0.
#   eval         u nodal (NV, vdim): uq[q][i] = sum over the nodes, ascending, of N_a * u_a[i] (fq of _load_block).  Gradient:
#                r[i][k] = sum over the nodes, ascending, of u_a[i] * dN_a[k], the first product as it is (J with u in the place of
#                x); t[i][j] = r[i][0] * C[j][0] + r[i][1] * C[j][1] (+ r[i][2] * C[j][2]) with the cofactors C of _cofactors;
#                gradq[q][i][j] = t[i][j] / det: the derivative of component i along x_j, the division last.
#   loads        fq (NQ, vdim) at the points: dof (a, i) gets the sum over the points, ascending from 0.0, of (s * fq[q][i]) * N_a,
#                s = (weight * det) * coef_e (coef None: 1.0); the packed layout of element_loads.
#   errors       (NE, 2).  Column 0: the sum over the points, ascending from 0.0, of wdet_q * d_q, d_q = the sum over i, ascending, of
#                (uq_i - exq_i) * (uq_i - exq_i), the first square as it is; column 1 the same with gradq - exgradq over (i, j), i
#                outermost.  A column whose exact data is None is 0.0.
#   refused      vdim, then what _mesh refuses; then a missing u / fq (or one of the wrong size; then exact data of the wrong
#                size); then the first element with a non-positive determinant (ElementError).
def _points_block(X, dim, nd):
    """Per point of the mass rule of n elements of one type: (N, dN, C, det), and per element whether a det was not positive."""
    bad = np.zeros(X.shape[0], bool)
    out = []
    with np.errstate(all="ignore"):
        for q in range(MASS_NPOINTS[(dim, nd)]):
            dN = mass_reference_gradients(dim, nd, q)
            J = [[None] * dim for _ in range(dim)]
            for i in range(dim):
                for j in range(dim):
                    t = X[:, 0, i] * dN[0][j]
                    for a in range(1, nd):
                        t = t + X[:, a, i] * dN[a][j]
                    J[i][j] = t
            C, det = _cofactors(J, dim)
            bad |= ~(det > 0.0)
            out.append((shape_values(dim, nd, q), dN, C, det))
    return out, bad


def _eval_point(N, dN, C, det, F, dim, grad):
    """(uq (n, vdim), gradq (n, vdim, dim) or None) at one point; F: (n, nd, vdim) the nodal field."""
    nd = F.shape[1]
    uq = N[0] * F[:, 0, :]
    for a in range(1, nd):
        uq = uq + N[a] * F[:, a, :]
    if not grad:
        return uq, None
    g = np.zeros(F.shape[:1] + (F.shape[2], dim))
    r = []
    for k in range(dim):
        t = F[:, 0, :] * dN[0][k]
        for a in range(1, nd):
            t = t + F[:, a, :] * dN[a][k]
        r.append(t)
    for j in range(dim):
        t = r[0] * C[j][0][:, None] + r[1] * C[j][1][:, None]
        if dim == 3:
            t = t + r[2] * C[j][2][:, None]
        g[:, :, j] = t / det[:, None]
    return uq, g


def _points_mesh(coords, elem_to_vertex, elem_ptr, vdim):
    shape = np.shape(coords)
    if len(shape) == 2 and shape[1] in (2, 3):
        _vdim(vdim, shape[1])                                        # (refused before the mesh is looked at)
    X, dim, ep, e2v, nd = _mesh(coords, elem_to_vertex, elem_ptr)
    vdim = _vdim(vdim, dim)
    npts = np.array([MASS_NPOINTS[(dim, int(c))] for c in nd], np.int64)
    qp = np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)
    return X, dim, ep, e2v, nd, vdim, qp


def _point_data(a, n, what, needed=True):
    if a is None:
        if needed:
            raise ValueError("%s is needed" % what)
        return None
    a = np.asarray(a, np.float64)
    if a.size != int(np.prod(n)):
        raise ValueError("%s is needed" % what)
    return a.reshape(n)


def _types(nd, ep, e2v):
    """(node count, element ids, their vertex lists (n, nodes)) per type, ascending node count"""
    for c in np.unique(nd):
        ids = np.flatnonzero(nd == c)
        yield int(c), ids, e2v[ep[ids][:, None] + np.arange(int(c))]


def _refuse_det(bad):
    if bad.any():
        raise ElementError(np.flatnonzero(bad)[0])


def element_points(coords, elem_to_vertex, elem_ptr=None):
    """(qp_ptr (NE + 1,) int64, xq (NQ, dim), wdet (NQ,)): the points of the mass rule of every element and weight * det there."""
    X, dim, ep, e2v, nd, _, qp = _points_mesh(coords, elem_to_vertex, elem_ptr, 1)
    NQ = int(qp[-1])
    xq, wdet = np.zeros((NQ, dim)), np.zeros(NQ)
    bad = np.zeros(len(nd), bool)
    with np.errstate(all="ignore"):
        for c, ids, v in _types(nd, ep, e2v):
            points, bad[ids] = _points_block(X[v], dim, c)
            for q, (N, dN, C, det) in enumerate(points):
                xq[qp[ids] + q] = _eval_point(N, dN, C, det, X[v], dim, False)[0]
                wdet[qp[ids] + q] = mass_point_weight(dim, c, q) * det
    _refuse_det(bad)
    return qp, xq, wdet


def element_eval(coords, elem_to_vertex, u, vdim=1, elem_ptr=None, grad=True):
    """(uq (NQ, vdim), gradq (NQ, vdim, dim)) of the nodal field u (NV, vdim) or (NV,) at the points; grad=False: gradq is None."""
    X, dim, ep, e2v, nd, vdim, qp = _points_mesh(coords, elem_to_vertex, elem_ptr, vdim)
    U = _point_data(u, (X.shape[0], vdim), "u: (NV, vdim)")
    NQ = int(qp[-1])
    uq, gq = np.zeros((NQ, vdim)), np.zeros((NQ, vdim, dim)) if grad else None
    bad = np.zeros(len(nd), bool)
    with np.errstate(all="ignore"):
        for c, ids, v in _types(nd, ep, e2v):
            points, bad[ids] = _points_block(X[v], dim, c)
            for q, (N, dN, C, det) in enumerate(points):
                a, g = _eval_point(N, dN, C, det, U[v], dim, grad)
                uq[qp[ids] + q] = a
                if grad:
                    gq[qp[ids] + q] = g
    _refuse_det(bad)
    return uq, gq


def element_loads_points(coords, elem_to_vertex, fq, vdim=1, coef=None, elem_ptr=None):
    """The load vectors of the source fq (NQ, vdim) or (NQ,) given at the points, with the per-element coefficient coef (NE,), None:
    1.0, in the layout of element_loads."""
    X, dim, ep, e2v, nd, vdim, qp = _points_mesh(coords, elem_to_vertex, elem_ptr, vdim)
    NE = len(nd)
    F = _point_data(fq, (int(qp[-1]), vdim), "fq: (NQ, vdim)")
    coef = np.ones(NE) if coef is None else np.asarray(coef, np.float64).reshape(-1)
    if len(coef) != NE:
        raise ValueError("coef: (NE,) is needed")
    voff = np.concatenate([[0], np.cumsum(nd * vdim)])
    out = np.zeros(int(voff[-1]))
    bad = np.zeros(NE, bool)
    with np.errstate(all="ignore"):
        for c, ids, v in _types(nd, ep, e2v):
            points, bad[ids] = _mass_points(X[v], dim, c, coef[ids])
            acc = np.zeros((len(ids), c, vdim))
            for q, (N, s) in enumerate(points):
                sf = s[:, None] * F[qp[ids] + q]
                term = sf[:, None, :] * np.array(N)[None, :, None]
                acc = acc + term
            out[voff[ids][:, None] + np.arange(c * vdim)] = acc.reshape(len(ids), -1)
    _refuse_det(bad)
    if elem_ptr is None:
        return out.reshape(NE, nd[0] * vdim) if NE else out.reshape(0, 0)
    return out


def element_errors(coords, elem_to_vertex, u, exq=None, exgradq=None, vdim=1, elem_ptr=None):
    """(NE, 2): per element the squared L2 error of the nodal u against the exact values exq (NQ, vdim) at the points, and the
    squared error of its gradient against exgradq (NQ, vdim, dim); a column whose exact data is None is 0.0."""
    X, dim, ep, e2v, nd, vdim, qp = _points_mesh(coords, elem_to_vertex, elem_ptr, vdim)
    NE, NQ = len(nd), int(qp[-1])
    U = _point_data(u, (X.shape[0], vdim), "u: (NV, vdim)")
    E = _point_data(exq, (NQ, vdim), "exq: (NQ, vdim)", False)
    EG = _point_data(exgradq, (NQ, vdim, dim), "exgradq: (NQ, vdim, dim)", False)
    out = np.zeros((NE, 2))
    bad = np.zeros(NE, bool)
    with np.errstate(all="ignore"):
        for c, ids, v in _types(nd, ep, e2v):
            points, bad[ids] = _points_block(X[v], dim, c)
            acc0, acc1 = np.zeros(len(ids)), np.zeros(len(ids))
            for q, (N, dN, C, det) in enumerate(points):
                wdet = mass_point_weight(dim, c, q) * det
                a, g = _eval_point(N, dN, C, det, U[v], dim, EG is not None)
                if E is not None:
                    d = (a - E[qp[ids] + q]).reshape(len(ids), -1)
                    t = d[:, 0] * d[:, 0]
                    for k in range(1, d.shape[1]):
                        t = t + d[:, k] * d[:, k]
                    term = wdet * t
                    acc0 = acc0 + term
                if EG is not None:
                    d = (g - EG[qp[ids] + q]).reshape(len(ids), -1)
                    t = d[:, 0] * d[:, 0]
                    for k in range(1, d.shape[1]):
                        t = t + d[:, k] * d[:, k]
                    term = wdet * t
                    acc1 = acc1 + term
            out[ids, 0], out[ids, 1] = acc0, acc1
    _refuse_det(bad)
    return out


# ---- coefficients at the points: the stiffness forms and the mass with one coefficient per point of the mass rule ----------------------
#   points       those of the type's MASS rule for both forms (MASS_NPOINTS, mass_reference_gradients, mass_point_weight), so that
#                one point index serves all point data: row qp_ptr[e] + q of coefq belongs to point q of element e, the indexing of
#                element_points and element_eval.  For the quadrilateral, hexahedron, wedge and their order-2 relatives this is the
#                stiffness rule of element_matrices; the triangle has 3 points here against 1, the tetrahedron 4 against 1, the
#                6-node triangle 6 against 3 and the 10-node tetrahedron 14 against 4.
#   stiffness    per point everything is _block's: J over the nodes ascending, _cofactors, s = weight / det, G_a, then kind 0
#                F_a = K_q G_a with K_q = _tensor of the POINT's row (ncoef 1, dim or dim (dim + 1) / 2, the missing entries 0.0 and
#                multiplied like any other), kind 1 the term with lambda_q, mu_q of the point's row; the terms are added over the
#                points ascending from 0.0.  The packed layout and dof_lists are element_matrices'.
#   mass         element_mass with s = (weight * det) * coefq[qp_ptr[e] + q] in _mass_points; coefq (NQ,).
#   refused      what the form they parallel refuses, in its order, with coefq (of the wrong size) in the place of coef; ElementError
#                names the smallest element whose det is not positive at a point of the MASS rule: a curved 6-node triangle or
#                10-node tetrahedron can be refused here at a point element_matrices does not have.
def element_matrices_points(coords, elem_to_vertex, kind, coefq, elem_ptr=None):
    """The element matrices with the coefficients coefq (NQ, ncoef) or (NQ,) given at the points of element_points: (NE, size, size)
    when elem_ptr is None, else packed."""
    if kind not in (0, 1):
        raise ValueError("kind: 0 (diffusion) or 1 (elasticity)")
    X, dim, ep, e2v, nd, _, qp = _points_mesh(coords, elem_to_vertex, elem_ptr, 1)
    NE, NQ = len(nd), int(qp[-1])
    if coefq is None:
        raise ValueError("coefq: (NQ, ncoef) is needed")
    coefq = np.asarray(coefq, np.float64)
    if NQ == 0:
        coefq = np.zeros((0, allowed_ncoef(dim, kind)[0]))
    elif coefq.size % NQ or coefq.size == 0:
        raise ValueError("coefq: (NQ, ncoef) is needed")
    else:
        coefq = coefq.reshape(NQ, -1)
    if coefq.shape[1] not in allowed_ncoef(dim, kind):
        raise ValueError("ncoef = %d is not allowed for kind %d in %dD" % (coefq.shape[1], kind, dim))
    comp = 1 if kind == 0 else dim
    moff = np.concatenate([[0], np.cumsum((nd * comp) ** 2)])
    out = np.zeros(int(moff[-1]))
    bad = np.zeros(NE, bool)
    for c, ids, v in _types(nd, ep, e2v):
        blk, bad[ids] = _block(X[v], dim, c, kind, coefq, qp[ids])
        out[moff[ids][:, None] + np.arange((c * comp) ** 2)] = blk.reshape(len(ids), -1)
    _refuse_det(bad)
    if elem_ptr is None:
        return out.reshape(NE, nd[0] * comp, nd[0] * comp) if NE else out.reshape(0, 0, 0)
    return out


def element_mass_points(coords, elem_to_vertex, coefq, vdim=1, elem_ptr=None, add_to=None):
    """The mass matrices with the coefficient coefq (NQ,) given at the points of element_points, in the layout of element_mass;
    add_to as there."""
    X, dim, ep, e2v, nd, vdim, qp = _points_mesh(coords, elem_to_vertex, elem_ptr, vdim)
    NE, NQ = len(nd), int(qp[-1])
    if coefq is None:
        raise ValueError("coefq: (NQ,) is needed")
    coefq = np.asarray(coefq, np.float64).reshape(-1)
    if len(coefq) != NQ:
        raise ValueError("coefq: (NQ,) is needed")
    moff = np.concatenate([[0], np.cumsum((nd * vdim) ** 2)])
    out = np.zeros(int(moff[-1]))
    bad = np.zeros(NE, bool)
    for c, ids, v in _types(nd, ep, e2v):
        m, bad[ids] = _mass_block(X[v], dim, c, coefq, qp[ids])
        if vdim > 1:
            full = np.zeros((len(ids), c, vdim, c, vdim))
            for i in range(vdim):
                full[:, :, i, :, i] = m
            m = full
        out[moff[ids][:, None] + np.arange((c * vdim) ** 2)] = m.reshape(len(ids), -1)
    _refuse_det(bad)
    if add_to is not None:
        base = np.asarray(add_to, np.float64).ravel()
        if len(base) != len(out):
            raise ValueError("add_to: the layout of the result is needed")
        out = base + out
    if elem_ptr is None:
        return out.reshape(NE, nd[0] * vdim, nd[0] * vdim) if NE else out.reshape(0, 0, 0)
    return out


# ---- boundary data at the face points: the points and the normals, traces, the Robin and Neumann terms of point data ------------------
#   points       the points of face f of the list are those of its face type's rule (face_rule), in the rule's order; point q of
#                face f has the global index fp_ptr[f] + q, fp_ptr (NF + 1,) int64, NFQ = fp_ptr[NF]: the index follows the LIST, not
#                the buckets the faces are worked in, so a permuted list permutes the point arrays by whole faces.
#                xq[q][i] = sum over the face nodes c, ascending, of N_c * x_c[i], the first product as it is; wmeas[q] = w_q * meas_q:
#                the bits of s of _face_points with the coefficient 1.0; normal[q] = (n0, n1, n2) / meas with n = t_0 x t_1 of
#                _face_points in 3D, (t_y, -t_x) / meas in 2D, the division last: the unit normal that points out of the owning
#                element (FACE_NODES orders every face of every type so; tests/test_bdr_points_model.py holds it to that).
#   eval         u nodal (NV, vdim).  uq[q][i] = sum over the FACE nodes, ascending, of N_c * u_c[i]: gq of boundary_loads.  gradq is
#                the whole gradient of the ELEMENT's field at the face point: the reference position of the point in the element is
#                xi[k] = sum over the face nodes c, ascending, of N_c * REF_NODES[node c][k], the first product as it is
#                (face_ref_point); dN_a = gradients_at(xi) of ALL nodes of the element (face_gradients); J[i][j] = sum over the nodes,
#                ascending, of x_a[i] * dN_a[j]; _cofactors; then everything is _eval_point's: r[i][k], (sum_k r[i][k] C[j][k]) / det.
#   mass         boundary_mass with s = (w * meas) * coefq[fp_ptr[f] + q]; coefq (NFQ,).
#   loads        gq (NFQ, vdim) at the points: face dof (a, i) gets the sum over the points, ascending from 0.0, of
#                (s * gq[q][i]) * N_a, s = (w * meas) * coef_f (coef None: 1.0); added as boundary_loads adds.
#   refused      vdim; missing face lists, u, coefq, gq; what _mesh refuses; what _face_list refuses; data of the wrong size; the
#                first face with a non-positive measure; for eval, then the first face (lowest index of the list) with a point
#                where the element's determinant is not positive -- whether or not the gradient is asked for (FaceError, .face).
def _ref_nodes():
    tri, tet = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    out = {(2, 3): tri, (3, 4): tet,
           (2, 4): [(float(x), float(y)) for (x, y) in QUAD_LOC],
           (3, 8): [(float(x), float(y), float(z)) for (x, y, z) in HEX_LOC],
           (3, 6): [(x, y, float(a)) for a in (0, 1) for (x, y) in tri],
           (2, 9): [(0.5 * x, 0.5 * y) for (x, y) in Q2_QUAD_LOC],
           (3, 27): [(0.5 * x, 0.5 * y, 0.5 * z) for (x, y, z) in Q2_HEX_LOC]}
    for (dim, nd), V in (((2, 6), tri), ((3, 10), tet)):
        out[(dim, nd)] = V + [tuple(0.5 * (V[i][k] + V[j][k]) for k in range(dim)) for (i, j) in P2_EDGES[dim]]
    return out


REF_NODES = _ref_nodes()                     # the reference position of every node of every type (exact doubles)
FACE_NPOINTS = {k: len(face_rule(*k)) for k in FACE_TYPE_INDEX}


def face_ref_point(dim, nd, lf, q):
    """the reference position, in the element (dim, nd), of point q of its local face lf"""
    nodes = FACE_NODES[(dim, nd)][lf]
    N, R = face_rule(dim, len(nodes))[q][0], REF_NODES[(dim, nd)]
    xi = []
    for k in range(dim):
        t = N[0] * R[nodes[0]][k]
        for c in range(1, len(nodes)):
            t = t + N[c] * R[nodes[c]][k]
        xi.append(t)
    return tuple(xi)


def face_gradients(dim, nd, lf, q):
    """dN[a][k] of all nd nodes of the element type at point q of its local face lf, as Python floats"""
    return gradients_at(dim, nd, face_ref_point(dim, nd, lf, q))


def _face_mesh(coords, elem_to_vertex, elem_ptr, vdim, face_elem, face_local, needed=()):
    """The checks the four calls share, in their order; needed: (array, what) pairs that must not be None.  Returns the mesh, the
    checked face list and fp_ptr."""
    shape = np.shape(coords)
    if len(shape) == 2 and shape[1] in (2, 3):
        _vdim(vdim, shape[1])                                        # (refused before the mesh is looked at)
    if face_elem is None or face_local is None:
        raise ValueError("face_elem and face_local: (NF,) are needed")
    for a, what in needed:
        if a is None:
            raise ValueError("%s is needed" % what)
    X, dim, ep, e2v, nd = _mesh(coords, elem_to_vertex, elem_ptr)
    vdim = _vdim(vdim, dim)
    fe, fl = _face_list(dim, nd, face_elem, face_local)
    npts = np.array([FACE_NPOINTS[(dim, len(FACE_NODES[(dim, int(nd[e]))][l]))] for e, l in zip(fe, fl)], np.int64)
    fp = np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)
    return X, dim, ep, e2v, nd, vdim, fe, fl, fp


def _refuse_face_det(bad):
    if bad.any():
        raise FaceError(int(np.flatnonzero(bad)[0]), "the Jacobian determinant of the element is not positive")


def boundary_points(coords, elem_to_vertex, face_elem, face_local, elem_ptr=None):
    """(fp_ptr (NF + 1,) int64, xq (NFQ, dim), wmeas (NFQ,), normal (NFQ, dim)): the points of the face rule of every listed face,
    weight * measure there and the unit normal that points out of the owning element."""
    X, dim, ep, e2v, nd, _, fe, fl, fp = _face_mesh(coords, elem_to_vertex, elem_ptr, 1, face_elem, face_local)
    NFQ = int(fp[-1])
    xq, wmeas, normal = np.zeros((NFQ, dim)), np.zeros(NFQ), np.zeros((NFQ, dim))
    bad = np.zeros(len(fe), bool)
    with np.errstate(all="ignore"):
        for lf, c, ids in _face_buckets(dim, nd, fe, fl):
            nodes = np.array(FACE_NODES[(dim, c)][lf])
            Xf = X[e2v[ep[fe[ids]][:, None] + nodes]]
            points, bad[ids] = _face_points(Xf, dim, len(nodes), 1.0, geom=True)
            for q, (N, s, n) in enumerate(points):
                xq[fp[ids] + q] = _eval_point(N, None, None, None, Xf, dim, False)[0]
                wmeas[fp[ids] + q] = s
                normal[fp[ids] + q] = n
    _refuse_measure(bad)
    return fp, xq, wmeas, normal


def boundary_eval(coords, elem_to_vertex, face_elem, face_local, u, vdim=1, elem_ptr=None, grad=True):
    """(uq (NFQ, vdim), gradq (NFQ, vdim, dim)) of the nodal field u (NV, vdim) or (NV,) at the face points: the trace through the
    face's shape functions and the whole gradient of the owning element's field; grad=False: gradq is None (the determinants are
    checked all the same)."""
    X, dim, ep, e2v, nd, vdim, fe, fl, fp = _face_mesh(coords, elem_to_vertex, elem_ptr, vdim, face_elem, face_local,
                                                       [(u, "u: (NV, vdim)")])
    U = _point_data(u, (X.shape[0], vdim), "u: (NV, vdim)")
    NFQ = int(fp[-1])
    uq, gq = np.zeros((NFQ, vdim)), np.zeros((NFQ, vdim, dim)) if grad else None
    bad, bad_det = np.zeros(len(fe), bool), np.zeros(len(fe), bool)
    with np.errstate(all="ignore"):
        for lf, c, ids in _face_buckets(dim, nd, fe, fl):
            nodes = np.array(FACE_NODES[(dim, c)][lf])
            v = e2v[ep[fe[ids]][:, None] + nodes]
            ve = e2v[ep[fe[ids]][:, None] + np.arange(c)]
            points, bad[ids] = _face_points(X[v], dim, len(nodes), 1.0)
            Xe, Ue, Uf = X[ve], U[ve], U[v]
            for q, (N, _) in enumerate(points):
                uq[fp[ids] + q] = _eval_point(N, None, None, None, Uf, dim, False)[0]
                dN = face_gradients(dim, c, lf, q)
                J = [[None] * dim for _ in range(dim)]
                for i in range(dim):
                    for j in range(dim):
                        t = Xe[:, 0, i] * dN[0][j]
                        for a in range(1, c):
                            t = t + Xe[:, a, i] * dN[a][j]
                        J[i][j] = t
                C, det = _cofactors(J, dim)
                bad_det[ids] |= ~(det > 0.0)
                if grad:
                    gq[fp[ids] + q] = _eval_point([0.0] * c, dN, C, det, Ue, dim, True)[1]
    _refuse_measure(bad)
    _refuse_face_det(bad_det)
    return uq, gq


def boundary_mass_points(coords, elem_to_vertex, face_elem, face_local, coefq, vdim=1, elem_ptr=None, add_to=None):
    """boundary_mass with the coefficient coefq (NFQ,) given at the face points of boundary_points."""
    X, dim, ep, e2v, nd, vdim, fe, fl, fp = _face_mesh(coords, elem_to_vertex, elem_ptr, vdim, face_elem, face_local,
                                                       [(coefq, "coefq: (NFQ,)")])
    coefq = _point_data(coefq, (int(fp[-1]),), "coefq: (NFQ,)")
    return _add_face_mass(X, dim, ep, e2v, nd, vdim, fe, fl, coefq, fp, add_to, elem_ptr is None)


def boundary_loads_points(coords, elem_to_vertex, face_elem, face_local, gq, vdim=1, coef=None, elem_ptr=None, add_to=None):
    """boundary_loads of data given AT THE FACE POINTS of boundary_points, gq (NFQ, vdim) or (NFQ,); coef (NF,) or None (1.0)."""
    X, dim, ep, e2v, nd, vdim, fe, fl, fp = _face_mesh(coords, elem_to_vertex, elem_ptr, vdim, face_elem, face_local,
                                                       [(gq, "gq: (NFQ, vdim)")])
    G = _point_data(gq, (int(fp[-1]), vdim), "gq: (NFQ, vdim)")
    coef = _face_coef(coef, len(fe), False)
    return _add_face_loads(X, dim, ep, e2v, nd, vdim, fe, fl, coef, G, fp, add_to, elem_ptr is None)
