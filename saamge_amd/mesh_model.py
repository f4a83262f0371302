"""CPU model of the face table of a mesh (csrc/mesh_faces.hip) -- numpy only, test infrastructure like elmat_model.py.

This file is the DEFINITION of the result: every output is an integer the mesh fixes uniquely, and the device gives the same.

  types        those of elmat_model.FACE_NODES, all nine (dim, nodes): (2, 3), (2, 4), (2, 6), (2, 9), (3, 4), (3, 6), (3, 8),
               (3, 10), (3, 27); local face lf of an element is FACE_NODES[(dim, nodes)][lf].
  corners      of a face: in 2D the first and the last node of its entry (3-node segments are start, middle, end); a
               triangular face of 3 or 6 nodes: its first three nodes; a quadrilateral face of 4 or 9 nodes: its first four.
  slot         a pair (element, local face): s = slot_ptr[e] + lf, slot_ptr int64 of NE + 1 entries.
  matching     two slots match when their SORTED corner vertex ids are equal; midside and centre nodes take no part, so a
               hex8 face and a hex27 face on the same four vertices are an interior pair.  A corner set that one slot holds is a
               boundary face, one that two slots hold an interior pair (of two different elements: an element lists no vertex
               twice); three or more make the mesh non-manifold, which is refused (MeshError, .element the lowest element id
               that has such a face).
  outputs      nbr_elem[s], nbr_local[s]: the element and the local face across slot s, -1 and -1 on a boundary face;
               bdr_elem, bdr_local: the boundary faces, ascending by (element, local face) -- the order of
               problems.boundary_faces; xadj (int64) / adj (int32): row e the distinct elements across the faces of e,
               ascending, no self loop -- two elements that share two faces are in each other's row once.
  info         [0] slots, [1] interior pairs, [2] boundary faces ([0] = 2 [1] + [2]), [3] graph entries, [4] interior pairs whose
               two faces have different node counts, [5] the largest number of elements at one vertex (node), [6] -1 or the first
               element with a non-manifold face, [7] elements without a neighbour.
  face_nodes   the global node ids of each listed face in the face's own node order, midside nodes included.
  face_dofs    bdr_dofs[vdim * a + i] |= flag for every node a of every listed face and every component i with bit i of
               comp_mask set; info [0] faces, [1] distinct nodes touched, [2] bytes whose value changed, [3] -1 or the first
               refused face.
  refused      what elmat_model._mesh refuses that needs no coordinates (dim, malformed offsets, a vertex id outside [0, NV),
               a vertex listed twice, a node count that is no type of the dimension), then the non-manifold mesh.  The
               face-list calls refuse what boundary_mass refuses of a face list (FaceError, the lowest index) except the
               measure, and vdim not 1 or dim, comp_mask outside 1 .. 2^vdim - 1, flag outside 1 .. 127.
"""
import numpy as np

from .elmat_model import ALL_TYPE_INDEX, FACE_NODES, FaceError, _face_list


class MeshError(ValueError):
    """A non-manifold mesh; .element is the lowest element id that has a face three or more slots hold."""

    def __init__(self, element, info):
        ValueError.__init__(self, "element %d: a face is shared by more than two elements" % element)
        self.element = int(element)
        self.info = list(info)


def face_corners(dim, nodes):
    """the local node ids of the corners of a face, nodes = its entry of FACE_NODES"""
    if dim == 2:
        return (nodes[0], nodes[-1])
    return tuple(nodes[:3]) if len(nodes) in (3, 6) else tuple(nodes[:4])


def _topology(NV, dim, elem_to_vertex, elem_ptr):
    """elmat_model._mesh without the coordinates: (ep int64, e2v int64 flat, nd)"""
    if dim not in (2, 3):
        raise ValueError("dim must be 2 or 3")
    if NV < 0:
        raise ValueError("NV < 0")
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
    return ep, e2v, nd


class FaceTable(object):
    """slot_ptr, nbr_elem, nbr_local, bdr_elem, bdr_local, xadj, adj, info of a mesh (the module's docstring)."""

    def __init__(self, NV, dim, elem_to_vertex, elem_ptr=None):
        ep, e2v, nd = _topology(int(NV), int(dim), elem_to_vertex, elem_ptr)
        NE = len(nd)
        nfaces = np.array([len(FACE_NODES[(dim, int(c))]) for c in nd], np.int64)
        self.slot_ptr = np.concatenate([[0], np.cumsum(nfaces)]).astype(np.int64)
        S = int(self.slot_ptr[-1])
        key = np.full((S, 4), -1, np.int64)                          # sorted corners, -1 first for a triangle beside quads
        fn = np.zeros(S, np.int64)
        selem = np.repeat(np.arange(NE, dtype=np.int64), nfaces)
        slocal = np.arange(S, dtype=np.int64) - self.slot_ptr[selem]
        for c in np.unique(nd):
            ids = np.flatnonzero(nd == c)
            for lf, nodes in enumerate(FACE_NODES[(dim, int(c))]):
                v = np.sort(e2v[ep[ids][:, None] + np.array(face_corners(dim, nodes))], axis=1)
                s = self.slot_ptr[ids] + lf
                key[s, 4 - v.shape[1]:] = v
                fn[s] = len(nodes)
        self.nbr_elem = np.full(S, -1, np.int32)
        self.nbr_local = np.full(S, -1, np.int32)
        info = [S, 0, 0, 0, 0, 0, -1, 0]
        info[5] = int(np.bincount(e2v, minlength=1).max()) if len(e2v) else 0
        if S:
            order = np.lexsort((key[:, 3], key[:, 2], key[:, 1], key[:, 0]))
            k = key[order]
            start = np.concatenate([[True], (k[1:] != k[:-1]).any(axis=1)])
            run = np.cumsum(start) - 1
            count = np.bincount(run)
            many = count[run] > 2
            if many.any():
                info[6] = int(selem[order[many]].min())
                self.info = info
                raise MeshError(info[6], info)
            first = np.flatnonzero(start)
            a = order[first[count == 2]]
            b = order[first[count == 2] + 1]
            self.nbr_elem[a], self.nbr_local[a] = selem[b], slocal[b]
            self.nbr_elem[b], self.nbr_local[b] = selem[a], slocal[a]
            info[1] = len(a)
            info[4] = int((fn[a] != fn[b]).sum())
        bdr = np.flatnonzero(self.nbr_elem < 0)                      # (slot order is (element, local face) order)
        self.bdr_elem, self.bdr_local = selem[bdr].astype(np.int32), slocal[bdr].astype(np.int32)
        info[2] = len(bdr)
        inner = np.flatnonzero(self.nbr_elem >= 0)
        pairs = np.unique(selem[inner] * max(NE, 1) + self.nbr_elem[inner].astype(np.int64))
        rows = pairs // max(NE, 1)
        self.xadj = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=NE))]).astype(np.int64)
        self.adj = (pairs % max(NE, 1)).astype(np.int32)
        info[3] = len(pairs)
        info[7] = int((np.diff(self.xadj) == 0).sum())
        self.info = info
        self.NE, self.NB, self.nnz = NE, len(bdr), len(pairs)

    def arrays(self):
        return (self.slot_ptr, self.nbr_elem, self.nbr_local, self.bdr_elem, self.bdr_local, self.xadj, self.adj)


def face_table(NV, dim, elem_to_vertex, elem_ptr=None):
    return FaceTable(NV, dim, elem_to_vertex, elem_ptr)


def _checked_faces(NV, dim, elem_to_vertex, elem_ptr, face_elem, face_local):
    if NV is None:                                                   # (no upper bound is known: only a negative id is refused)
        flat = np.asarray(elem_to_vertex).ravel()
        NV = int(flat.max()) + 1 if len(flat) else 0
    ep, e2v, nd = _topology(int(NV), int(dim), elem_to_vertex, elem_ptr)
    fe, fl = _face_list(dim, nd, face_elem, face_local)
    return ep, e2v, nd, fe, fl


def face_nodes(dim, elem_to_vertex, elem_ptr, face_elem, face_local, NV=None):
    """(face_ptr int32 (NF + 1), nodes int32): the global node ids of each listed face in the face's own node order.  NV None:
    the largest vertex id + 1."""
    ep, e2v, nd, fe, fl = _checked_faces(NV, dim, elem_to_vertex, elem_ptr, face_elem, face_local)
    lists = [e2v[ep[e] + np.array(FACE_NODES[(dim, int(nd[e]))][l])] for e, l in zip(fe, fl)]
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32)
    nodes = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return ptr, nodes


def face_dofs(dim, elem_to_vertex, elem_ptr, face_elem, face_local, vdim, comp_mask, flag, bdr_dofs):
    """bdr_dofs (int8, vdim * NV, IN PLACE): flag ORed into the dofs of the listed faces' nodes; returns info (4 integers)."""
    if vdim not in (1, dim):
        raise ValueError("vdim: 1 or dim")
    if not 1 <= int(comp_mask) <= 2 ** vdim - 1:
        raise ValueError("comp_mask: 1 .. 2^vdim - 1")
    if not 1 <= int(flag) <= 127:
        raise ValueError("flag: 1 .. 127")
    if not (isinstance(bdr_dofs, np.ndarray) and bdr_dofs.dtype == np.int8 and bdr_dofs.size % vdim == 0):
        raise ValueError("bdr_dofs: int8 of vdim * NV entries is needed")
    _, nodes = face_nodes(dim, elem_to_vertex, elem_ptr, face_elem, face_local, NV=bdr_dofs.size // vdim)
    touched = np.unique(nodes.astype(np.int64))
    comps = np.array([i for i in range(vdim) if (int(comp_mask) >> i) & 1], np.int64)
    idx = (vdim * touched[:, None] + comps[None, :]).ravel()
    flat = bdr_dofs.reshape(-1)
    before = flat[idx].copy()
    flat[idx] = before | np.int8(flag)
    return [len(np.asarray(face_elem).ravel()), len(touched), int((flat[idx] != before).sum()), -1]


__all__ = ["MeshError", "FaceError", "FaceTable", "face_table", "face_corners", "face_nodes", "face_dofs"]
