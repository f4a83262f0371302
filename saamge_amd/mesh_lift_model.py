"""CPU model of the lift of an order-1 mesh to order 2 (csrc/mesh_lift.hip) -- numpy only, test infrastructure like mesh_model.py.

This file is the DEFINITION of the result: every integer and every coordinate bit, and the device gives the same.

  lifts        by (dim, nodes): (2, 3) -> (2, 6), (2, 4) -> (2, 9), (3, 4) -> (3, 10), (3, 8) -> (3, 27); with elem_ptr one list
               may mix them, each element lifts by its own type.
  refused      what mesh_model._topology refuses; then the lowest element that is a wedge (there is no 18-node type) or already
               of order 2 (LiftError, .element, info[6]); then what the face table of a mesh with a hexahedron refuses
               (mesh_model.MeshError); then NV2 beyond 2^31 - 1.
  edges        the local edges LOCAL_EDGES of a type are pairs of local corner nodes; an edge is the unordered vertex pair
               {a, b}, a < b, and a OWNS it.  edge_ptr (int64, NV + 1) counts the owned edges per vertex, edge_hi (int32, NEd)
               holds the b of each edge, ascending within each owner: edge k is the k-th pair in ascending (a, b) order, the
               numbering of problems.p2_simplex_nodes.
  node ids     vertices keep [0, NV), listed by an element or not; edge k is node NV + k; each distinct quadrilateral face of a
               hexahedron is node NV + NEd + f, f the rank of its REPRESENTATIVE slot of the face table of the order-1 mesh (the
               lower slot of an interior pair, the slot itself on the boundary) among representative slots in slot order,
               face_slot[f] (int64) that slot; the centre of the c-th quadrilateral (2D) / hexahedron (3D) in element order is
               node NV + NEd + NFq + c.
  local order  tri6, tet10: the vertices, then the edges in the order of LOCAL_EDGES; quad9: elmat_model.Q2_QUAD_LOC; hex27:
               lexicographic (iz * 3 + iy) * 3 + ix -- a position without a 1 is the corner HEX_LOC = position / 2, with one 1
               the edge between its two corners, with two the local face (FACE_NODES[(3, 8)]) of its four corners, (1, 1, 1) the
               centre.
  coordinates  None without coords.  Vertices are copied; an edge node is 0.5 * (X[a] + X[b]); a face node
               0.25 * ((X[v0] + X[v1]) + (X[v2] + X[v3])) with v0 < v1 < v2 < v3 the face's vertex ids ascending, so both elements
               at the face compute the same bits; a quadrilateral's centre 0.25 * ((c0 + c1) + (c2 + c3)) and a hexahedron's
               0.125 * (((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7))) in the element's local order.  Additions and
               multiplications by powers of two only: nothing can be contracted into an FMA.
  info         [0] NV2 = NV + [1] + [2] + [3], [1] NEd, [2] NFq, [3] NC, [4] entries of elem_to_node, [5] the most edges one
               vertex owns, [6] -1 or the lowest refused element, [7] vertices that no element lists.
"""
import numpy as np

from .elmat_model import FACE_NODES, HEX_LOC, Q2_HEX_LOC, Q2_QUAD_LOC
from .mesh_model import FaceTable, MeshError, _topology

LIFT = {(2, 3): 6, (2, 4): 9, (3, 4): 10, (3, 8): 27}
LOCAL_EDGES = {
    (2, 3): ((0, 1), (1, 2), (2, 0)),
    (2, 4): ((0, 1), (1, 2), (2, 3), (3, 0)),
    (3, 4): ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)),
    (3, 8): tuple((i, j) for i in range(8) for j in range(i + 1, 8)
                  if sum(int(p != q) for p, q in zip(HEX_LOC[i], HEX_LOC[j])) == 1),
}
assert Q2_QUAD_LOC[4:8] == [(1, 0), (2, 1), (1, 2), (0, 1)]      # quad9: the edge nodes follow LOCAL_EDGES[(2, 4)]


def _hex27_plan():
    """per lexicographic position: ("v", corner), ("e", local edge), ("f", local face) or ("c", 0)"""
    corner = {tuple(2 * c for c in l): k for k, l in enumerate(HEX_LOC)}
    plan = []
    for pos in Q2_HEX_LOC:
        ends = [[]]
        for v in pos:
            ends = [c + [o] for c in ends for o in ((0, 2) if v == 1 else (v,))]
        cs = sorted(corner[tuple(c)] for c in ends)
        if len(cs) == 1:
            plan.append(("v", cs[0]))
        elif len(cs) == 2:
            plan.append(("e", LOCAL_EDGES[(3, 8)].index(tuple(cs))))
        elif len(cs) == 4:
            plan.append(("f", [sorted(f) for f in FACE_NODES[(3, 8)]].index(cs)))
        else:
            plan.append(("c", 0))
    return tuple(plan)


HEX27_PLAN = _hex27_plan()
_MAX_INT = 2 ** 31 - 1


class LiftError(ValueError):
    """An element that has no lift; .element is the lowest such element."""

    def __init__(self, element, what, info):
        ValueError.__init__(self, "element %d: %s" % (element, what))
        self.element = int(element)
        self.info = list(info)


class MeshLift(object):
    """NV2, coords2 (or None), elem_ptr2 (int32), elem_to_node (int32, flat), edge_ptr (int64), edge_hi (int32), face_slot
    (int64), info of a mesh (the module's docstring).  faces: the mesh_model.FaceTable of the same mesh, or None."""

    def __init__(self, NV, dim, coords, elem_to_vertex, elem_ptr=None, faces=None):
        NV, dim = int(NV), int(dim)
        ep, e2v, nd = _topology(NV, dim, elem_to_vertex, elem_ptr)
        NE = len(nd)
        info = [0, 0, 0, 0, 0, 0, -1, 0]
        for e in np.flatnonzero(~np.isin(nd, [k[1] for k in LIFT if k[0] == dim])):
            info[6] = int(e)
            self.info = info
            raise LiftError(e, "a wedge has no order-2 type" if nd[e] == 6 and dim == 3 else
                            "%d nodes: the element is of order 2 already" % nd[e], info)
        if faces is not None and (faces.NE != NE or len(faces.nbr_elem) != sum(len(FACE_NODES[(dim, int(c))]) for c in nd)):
            raise ValueError("faces: the face table does not fit the mesh")
        X = None
        if coords is not None:
            X = np.ascontiguousarray(coords, dtype=np.float64)
            if X.shape != (NV, dim):
                raise ValueError("coords: (NV, dim) is needed")
        types = [int(c) for c in np.unique(nd)]
        ids = {c: np.flatnonzero(nd == c) for c in types}
        corner = {c: e2v[ep[ids[c]][:, None] + np.arange(c)[None, :]] for c in types}      # (elements of the type, corners)
        # ---- edges
        lo, hi = {}, {}
        for c in types:
            a = np.stack([corner[c][:, i] for (i, j) in LOCAL_EDGES[(dim, c)]], axis=1)
            b = np.stack([corner[c][:, j] for (i, j) in LOCAL_EDGES[(dim, c)]], axis=1)
            lo[c], hi[c] = np.minimum(a, b), np.maximum(a, b)
        M = max(NV, 1)
        keys = np.concatenate([(lo[c] * M + hi[c]).ravel() for c in types]) if types else np.zeros(0, np.int64)
        uniq = np.unique(keys)
        NEd = len(uniq)
        owned = np.bincount(uniq // M, minlength=NV)[:NV] if NV else np.zeros(0, np.int64)
        self.edge_ptr = np.concatenate([[0], np.cumsum(owned)]).astype(np.int64)
        self.edge_hi = (uniq % M).astype(np.int32)
        # ---- quadrilateral faces of hexahedra, through the face table of the order-1 mesh
        hexes = dim == 3 and 8 in types
        rep = None
        self.face_slot = np.zeros(0, np.int64)
        if hexes:
            T = faces
            if T is None:
                try:
                    T = FaceTable(NV, dim, elem_to_vertex, elem_ptr)
                except MeshError as err:
                    info[6] = err.element
                    self.info = info
                    raise
            S = len(T.nbr_elem)
            selem = np.repeat(np.arange(NE, dtype=np.int64), np.diff(T.slot_ptr))
            other = np.where(T.nbr_elem >= 0, T.slot_ptr[np.maximum(T.nbr_elem, 0)] + T.nbr_local, np.arange(S))
            rep = np.minimum(np.arange(S, dtype=np.int64), other)
            flag = (nd[selem] == 8) & (rep == np.arange(S))
            self.face_slot = np.flatnonzero(flag).astype(np.int64)
            rank = np.cumsum(flag) - flag                                                 # exclusive scan over the slots
            slot_ptr = T.slot_ptr
        NFq = len(self.face_slot)
        cc = 4 if dim == 2 else 8
        NC = len(ids[cc]) if cc in ids else 0
        NV2 = NV + NEd + NFq + NC
        nd2 = np.array([LIFT[(dim, int(c))] for c in nd], np.int64)
        info[:6] = [NV2, NEd, NFq, NC, int(nd2.sum()), int(owned.max()) if NV else 0]
        info[7] = NV - len(np.unique(e2v))
        self.info = info
        if NV2 > _MAX_INT:
            raise ValueError("NV2 = %d nodes are beyond 32 bits" % NV2)
        self.NV, self.NV2, self.NE, self.dim = NV, NV2, NE, dim
        ep2 = np.concatenate([[0], np.cumsum(nd2)]).astype(np.int64)
        self.elem_ptr2 = ep2.astype(np.int32)
        e2n = np.zeros(int(ep2[-1]), np.int64)
        X2 = None
        if X is not None:
            X2 = np.zeros((NV2, dim))
            X2[:NV] = X
            X2[NV:NV + NEd] = 0.5 * (X[uniq // M] + X[uniq % M])
        for c in types:
            base = ep2[ids[c]]
            V = corner[c]
            edge = NV + np.searchsorted(uniq, lo[c] * M + hi[c])                          # (elements, local edges)
            centre = NV + NEd + NFq + np.arange(len(ids[c]))
            if c in (3, 4) and (dim, c) != (2, 4):                                        # tri6, tet10
                e2n[base[:, None] + np.arange(c)[None, :]] = V
                e2n[base[:, None] + c + np.arange(edge.shape[1])[None, :]] = edge
            elif dim == 2:                                                                # quad9
                e2n[base[:, None] + np.arange(4)[None, :]] = V
                e2n[base[:, None] + 4 + np.arange(4)[None, :]] = edge
                e2n[base + 8] = centre
                if X is not None:
                    X2[centre] = 0.25 * ((X[V[:, 0]] + X[V[:, 1]]) + (X[V[:, 2]] + X[V[:, 3]]))
            else:                                                                         # hex27
                s = slot_ptr[ids[c]][:, None] + np.arange(6)[None, :]
                fnode = NV + NEd + rank[rep[s]]
                for p, (kind, k) in enumerate(HEX27_PLAN):
                    e2n[base + p] = {"v": lambda: V[:, k], "e": lambda: edge[:, k], "f": lambda: fnode[:, k],
                                     "c": lambda: centre}[kind]()
                if X is not None:
                    for lf, f in enumerate(FACE_NODES[(3, 8)]):
                        v = np.sort(V[:, list(f)], axis=1)
                        X2[fnode[:, lf]] = 0.25 * ((X[v[:, 0]] + X[v[:, 1]]) + (X[v[:, 2]] + X[v[:, 3]]))
                    X2[centre] = 0.125 * (((X[V[:, 0]] + X[V[:, 1]]) + (X[V[:, 2]] + X[V[:, 3]])) +
                                          ((X[V[:, 4]] + X[V[:, 5]]) + (X[V[:, 6]] + X[V[:, 7]])))
        self.elem_to_node = e2n.astype(np.int32)
        self.coords2 = X2

    def arrays(self):
        return (self.coords2, self.elem_ptr2, self.elem_to_node, self.edge_ptr, self.edge_hi, self.face_slot)

    def lists(self):
        """elem_to_node as (NE, nodes) of a mesh of one type"""
        n = np.diff(self.elem_ptr2)
        assert len(n) and (n == n[0]).all()
        return self.elem_to_node.reshape(self.NE, int(n[0]))


def lift_order2(NV, dim, coords, elem_to_vertex, elem_ptr=None, faces=None):
    return MeshLift(NV, dim, coords, elem_to_vertex, elem_ptr, faces)


__all__ = ["LIFT", "LOCAL_EDGES", "HEX27_PLAN", "LiftError", "MeshError", "MeshLift", "lift_order2"]
