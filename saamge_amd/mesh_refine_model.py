"""CPU model of the uniform refinement of an order-1 mesh (csrc/mesh_refine.hip) -- numpy only, test infrastructure like
mesh_lift_model.py.

This file is the DEFINITION of the result: every integer and every coordinate bit, and the device gives the same.  One
refinement step is mesh_lift_model.MeshLift of the mesh plus the child tables below; `levels` repeats the step.

  types        a triangle gives 4 triangles, a quadrilateral 4 quadrilaterals, a tetrahedron 8 tetrahedra, a hexahedron 8
               hexahedra; with elem_ptr one list may mix them and each child has its parent's type.  Wedges and order-2 elements
               are refused as the lift refuses them, so the child count nc is 4 in 2D and 8 in 3D.
  elements     GUARANTEED: child k of element e is element nc * e + k of the next level, so the parent of c is c // nc and the
               ancestor s levels up is c >> (2 s) in 2D, c >> (3 s) in 3D.  The nested partitions arange(NE) >> (2 s | 3 s) are
               connected agglomerates of the refined mesh's face graph.
  vertices     the vertex ids of level j + 1 are the node ids of the lift of level j: the vertices of level j keep their ids, then
               the edges, then the quadrilateral faces of hexahedra, then the centres.  coords of level j + 1 is coords2 of the
               lift, bit for bit.
  children     CHILDREN[(dim, nodes)][k][j]: local corner j of child k as an index into the parent's lifted local node list.
               Triangle (tri6: 3 = m01, 4 = m12, 5 = m20): three corner children and the inner one.  Quadrilateral, hexahedron:
               the lifted node at reference position LOC[k] + LOC[j], so child k holds the parent's corner k at its own local
               position k.  Tetrahedron (tet10: 4 = m01, 5 = m02, 6 = m03, 7 = m12, 8 = m13, 9 = m23): four corner children, and
               the inner octahedron cut along m02 - m13 (Bey's choice) into (4,5,6,8) (7,5,4,8) (5,6,8,9) (8,7,5,9) -- the second
               and fourth are Bey's [m01,m02,m12,m13] and [m02,m12,m13,m23] with local positions 0 and 2 exchanged, which makes
               them positive and keeps the pairing that selects the next diagonal: every descendant falls into one of 3
               congruence classes.  Every child has a positive Jacobian determinant where its parent has one.
  elem_ptr     always given (int32): element c of the result is elem_to_vertex[elem_ptr[c]:elem_ptr[c + 1]].
  interp       P_j (want_interp): CSR, one row per vertex of level j + 1, one column per vertex of level j, rowptr and col int32,
               columns ascending within a row.  A kept vertex v: (v, 1.0); an edge node: (a, 0.5) (b, 0.5); a face node: its four
               face vertices at 0.25; a quadrilateral's centre its four corners at 0.25, a hexahedron's its eight at 0.125.
               nnz = NV + 2 NEd + 4 NFq + (4 | 8) NC.
  refused      levels < 1, levels > MAX_LEVELS; then per level j: what the lift of level j refuses (at level 0 the refusals of
               mesh_lift_model, in their order; NV of level j + 1 beyond 2^31 - 1), the vertex list of level j + 1 beyond
               2^31 - 1 entries, with want_interp nnz of P_j beyond 2^31 - 1.  Nothing of a refused call is kept.
  info         [0] NV of the result, [1] its NE, [2] entries of its vertex list, [3] levels, [4] total nnz of the kept P, [5] the
               most edges one vertex owns over all lifted levels, [6] -1 or the lowest refused element, [7] vertices that no
               element lists.  A refusal leaves [0, 0, 0, 0, 0, 0, -1 or the element, 0].
  level_info   per level j in [0, levels]: [0] NV, [1] NE, [2] entries of the vertex list, [3] NEd, [4] NFq, [5] NC, [6] the most
               edges one vertex owns, [7] nnz of P_j (0: not kept); level `levels` was not lifted, its [3 .. 7] are -1.
"""
import numpy as np

from . import mesh_lift_model as lm
from .elmat_model import FACE_NODES, HEX_LOC, Q2_HEX_LOC, Q2_QUAD_LOC
from .mesh_lift_model import LiftError, MeshError

NC = {2: 4, 3: 8}
MAX_LEVELS = 15                  # 3 * 4^16 entries are beyond 32 bits already
LIMIT = 2 ** 31 - 1              # (tests lower it, with mesh_lift_model._MAX_INT, to reach the overflow refusals by counts only)
_QUAD_LOC = [(x // 2, y // 2) for x, y in Q2_QUAD_LOC[:4]]
CHILDREN = {
    (2, 3): ((0, 3, 5), (3, 1, 4), (5, 4, 2), (3, 4, 5)),
    (2, 4): tuple(tuple(Q2_QUAD_LOC.index((k[0] + j[0], k[1] + j[1])) for j in _QUAD_LOC) for k in _QUAD_LOC),
    (3, 4): ((0, 4, 5, 6), (4, 1, 7, 8), (5, 7, 2, 9), (6, 8, 9, 3), (4, 5, 6, 8), (7, 5, 4, 8), (5, 6, 8, 9), (8, 7, 5, 9)),
    (3, 8): tuple(tuple(Q2_HEX_LOC.index((k[0] + j[0], k[1] + j[1], k[2] + j[2])) for j in HEX_LOC) for k in HEX_LOC),
}
assert CHILDREN[(2, 4)] == ((0, 4, 8, 7), (4, 1, 5, 8), (8, 5, 2, 6), (7, 8, 6, 3))


class Interp(object):
    """P_j: nrows, ncols, nnz, rowptr (int32), col (int32), val (float64)"""

    def __init__(self, nrows, ncols, rowptr, col, val):
        self.nrows, self.ncols, self.nnz = int(nrows), int(ncols), int(len(col))
        self.rowptr, self.col, self.val = rowptr, col, val

    def arrays(self):
        return (self.rowptr, self.col, self.val)

    def dot(self, x):
        """P x for x of ncols rows (each row's products added in column order)"""
        x = np.asarray(x, np.float64)
        out = np.zeros((self.nrows,) + x.shape[1:])
        row = np.repeat(np.arange(self.nrows), np.diff(self.rowptr))
        np.add.at(out, row, (self.val.reshape((-1,) + (1,) * (x.ndim - 1))) * x[self.col])
        return out

    def dense(self):
        P = np.zeros((self.nrows, self.ncols))
        P[np.repeat(np.arange(self.nrows), np.diff(self.rowptr)), self.col] = self.val
        return P


def _interp(L, dim, ep, e2v, nd):
    """P of one step from the lift L of the mesh (ep, e2v, nd)"""
    NV, NE = L.NV, L.NE
    NEd, NFq = len(L.edge_hi), len(L.face_slot)
    cc = 4 if dim == 2 else 8
    cent = np.flatnonzero(nd == cc)
    rows = [np.arange(NV, dtype=np.int64)[:, None]]
    owner = np.repeat(np.arange(NV, dtype=np.int64), np.diff(L.edge_ptr))
    rows.append(np.stack([owner, L.edge_hi.astype(np.int64)], axis=1).reshape(NEd, 2))
    if NFq:
        nfaces = np.array([len(FACE_NODES[(dim, int(c))]) for c in nd], np.int64)
        slot_ptr = np.concatenate([[0], np.cumsum(nfaces)])
        fe = np.searchsorted(slot_ptr, L.face_slot, side="right") - 1
        fl = L.face_slot - slot_ptr[fe]
        local = np.array(FACE_NODES[(3, 8)], np.int64)[fl]                                # (NFq, 4)
        rows.append(np.sort(e2v[ep[fe][:, None] + local], axis=1))
    rows.append(np.sort(e2v[ep[cent][:, None] + np.arange(cc)[None, :]], axis=1).reshape(len(cent), cc))
    weight = [1.0, 0.5] + ([0.25] if NFq else []) + [0.25 if dim == 2 else 0.125]
    col = np.concatenate([r.ravel() for r in rows]).astype(np.int32)
    val = np.concatenate([np.full(r.size, w) for r, w in zip(rows, weight)])
    counts = np.concatenate([np.full(r.shape[0], r.shape[1], np.int64) for r in rows])
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    assert len(counts) == L.NV2
    return Interp(L.NV2, NV, rowptr, col, val)


class MeshRefine(object):
    """NV, NE, coords (or None), elem_ptr (int32), elem_to_vertex (int32, flat), info, level_info (levels + 1 lists), P (a list
    of Interp, empty without want_interp) of a mesh refined `levels` times (the module's docstring)."""

    def __init__(self, NV, dim, coords, elem_to_vertex, elem_ptr=None, levels=1, want_interp=False):
        NV, dim, levels = int(NV), int(dim), int(levels)
        self.info = [0, 0, 0, 0, 0, 0, -1, 0]
        if levels < 1:
            raise ValueError("levels must be at least 1")
        if levels > MAX_LEVELS:
            raise ValueError("levels above %d" % MAX_LEVELS)
        X = coords
        e2v, ep = elem_to_vertex, elem_ptr
        self.level_info, self.P = [], []
        owned, unlisted, total_nnz = 0, 0, 0
        for j in range(levels):
            try:
                L = lm.MeshLift(NV, dim, X, e2v, ep)
            except (LiftError, MeshError) as err:
                self.info[6] = int(err.element)
                raise
            tep, te2v, nd = lm._topology(NV, dim, e2v, ep)
            nc = NC[dim]
            NE, entries = len(nd), int(tep[-1])
            NEd, NFq, NCj = L.info[1], L.info[2], L.info[3]
            if nc * entries > LIMIT:
                raise ValueError("level %d: the element -> vertex lists are beyond 32 bits" % (j + 1))
            nnz = NV + 2 * NEd + 4 * NFq + (4 if dim == 2 else 8) * NCj
            if want_interp and nnz > LIMIT:
                raise ValueError("level %d: nnz = %d entries of the interpolation are beyond 32 bits" % (j, nnz))
            if want_interp:
                self.P.append(_interp(L, dim, tep, te2v, nd))
                total_nnz += nnz
            self.level_info.append([NV, NE, entries, NEd, NFq, NCj, L.info[5], nnz if want_interp else 0])
            owned = max(owned, L.info[5])
            if j == 0:
                unlisted = L.info[7]
            # ---- the children
            out = np.zeros(nc * entries, np.int64)
            ep2 = L.elem_ptr2.astype(np.int64)
            for c in [int(c) for c in np.unique(nd)]:
                ids = np.flatnonzero(nd == c)
                tab = np.array(CHILDREN[(dim, c)], np.int64)                              # (nc, c)
                src = L.elem_to_node[ep2[ids][:, None, None] + tab[None, :, :]]
                dst = nc * tep[ids][:, None, None] + (np.arange(nc) * c)[None, :, None] + np.arange(c)[None, None, :]
                out[dst] = src
            nep = np.concatenate([(nc * tep[:-1][:, None] + np.arange(nc)[None, :] * nd[:, None]).ravel(), [nc * entries]])
            NV, X, e2v, ep = L.NV2, L.coords2, out.astype(np.int32), nep.astype(np.int32)
        self.NV, self.NE, self.dim, self.levels = NV, len(ep) - 1, dim, levels
        self.coords, self.elem_ptr, self.elem_to_vertex = X, ep, e2v
        self.level_info.append([NV, self.NE, len(e2v), -1, -1, -1, -1, -1])
        self.info = [NV, self.NE, len(e2v), levels, total_nnz, owned, -1, unlisted]

    def arrays(self):
        return (self.coords, self.elem_ptr, self.elem_to_vertex)

    def lists(self):
        """elem_to_vertex as (NE, nodes) of a mesh of one type"""
        n = np.diff(self.elem_ptr)
        assert len(n) and (n == n[0]).all()
        return self.elem_to_vertex.reshape(self.NE, int(n[0]))


def refine(NV, dim, coords, elem_to_vertex, elem_ptr=None, levels=1, want_interp=False):
    return MeshRefine(NV, dim, coords, elem_to_vertex, elem_ptr, levels, want_interp)


__all__ = ["NC", "MAX_LEVELS", "CHILDREN", "Interp", "LiftError", "MeshError", "MeshRefine", "refine"]
