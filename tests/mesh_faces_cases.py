"""Meshes shared by the face-table tests (test_mesh_faces_model.py, test_gpu_mesh_faces.py): the 22 meshes of
elmat_cases.MESHES, elmat_q2_cases.MESHES and elmat_p2_cases.MESHES (undeformed; the largest is hex_9x8x7 with 504 elements and
3 024 slots over several workgroups, the smallest partial wavefront has 12 elements), and cases built here, each the smallest mesh
that hits one way to go wrong:

  single_<dim>_<nodes>     one element of each of the nine types: every slot is a boundary face
  pair_rotated_hex / _tet  two elements glued on one face; the second element's vertex list is rotated / permuted, so the shared
  pair_wedge_hex / _tet    face is not its matching local face and its corners come in another cyclic order: nbr_local is the
                           thing to get right
  hex8_on_hex27            a hex8 on a hex27, on the same four corner vertices: a pair of faces with 4 and 9 nodes
  double_contact           quads (a, b, c, d) and (a, b, c, e): two pairs, one graph entry per row
  fan_70                   70 triangles around vertex 0, closed: the valence exceeds one wavefront
  renumbered_hex_5x4x3     hex_5x4x3 with elements and vertices permuted (seed 5)
  hole                     hex_5x4x3 without its interior elements: boundary faces inside
  two_blocks               two disjoint copies of hex_3x2x2: a disconnected graph
  empty, isolated          NE = 0; two tetrahedra that share one vertex only
  nonmanifold_2d / _3d     three triangles on one edge, three tetrahedra on one face: refused

A case is (NV, dim, elem_to_vertex, elem_ptr); coords(name) gives the undeformed coordinates of an existing mesh."""
import numpy as np

from saamge_amd import elmat_model as em
from saamge_amd import mesh_model as mm

import elmat_cases as ec
import elmat_p2_cases as pc
import elmat_q2_cases as qc

EXISTING = [("q1", n) for n in ec.MESHES] + [("q2", n) for n in qc.MESHES] + [("p2", n) for n in pc.MESHES]
TYPES = sorted(em.FACE_NODES)
# min_shared with which partition_model.build_element_graph gives the graph through faces, on the meshes of one element type
# (and mixed_4, whose triangular wedge faces never meet a hexahedron)
PURE_MIN_SHARED = {"hex_3x2x2": 4, "hex_5x4x3": 4, "hex_9x8x7": 4, "tets_3x2x2": 3, "quads_4x3": 2, "tris_4x3": 2, "mixed_4": 3,
                   "hex27_3x2x2": 9, "hex27_5x4x3": 9, "hex27_7x3x3": 9, "tet10_3x2x2": 6, "tet10_70": 6, "tet10_5x4x3": 6,
                   "tet10_7x3x3": 6, "quad9_4x3": 3, "quad9_9x8": 3, "tri6_4x3": 3, "tri6_5x3": 3, "tri6_9x8": 3}


def existing(family, name):
    """(coords, elem_to_vertex, elem_ptr) of an existing mesh, undeformed"""
    if family == "q1":
        return ec.mesh(name, False)
    return qc.mesh(name, "box") if family == "q2" else pc.mesh(name, "box")


def _hole():
    X, e2v, _ = ec.mesh("hex_5x4x3", False)
    nx, ny, nz = 5, 4, 3
    ez, ey, ex = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    inner = ((ex > 0) & (ex < nx - 1) & (ey > 0) & (ey < ny - 1) & (ez > 0) & (ez < nz - 1)).ravel()
    return X.shape[0], 3, np.ascontiguousarray(e2v[~inner]), None


def renumbering():
    """(element permutation, vertex permutation) of renumbered_hex_5x4x3: new element k is old element pe[k], old vertex v is
    new vertex pv[v]"""
    X, e2v, _ = ec.mesh("hex_5x4x3", False)
    rng = np.random.default_rng(5)
    return rng.permutation(e2v.shape[0]), rng.permutation(X.shape[0])


def _renumbered():
    X, e2v, _ = ec.mesh("hex_5x4x3", False)
    pe, pv = renumbering()
    return X.shape[0], 3, np.ascontiguousarray(pv[e2v[pe]].astype(np.int32)), None


def _two_blocks():
    X, e2v, _ = ec.mesh("hex_3x2x2", False)
    return 2 * X.shape[0], 3, np.ascontiguousarray(np.concatenate([e2v, e2v + X.shape[0]]).astype(np.int32)), None


def _flat(lists):
    ep = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32)
    return np.concatenate([np.asarray(v) for v in lists]).astype(np.int32), ep


def _wedge_hex():
    e2v, ep = _flat([[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 0, 3, 4, 1]])      # the wedge's face (0, 1, 4, 3) is the hex's top, reversed
    return 10, 3, e2v, ep


def _wedge_tet():
    e2v, ep = _flat([[0, 1, 2, 3, 4, 5], [6, 5, 3, 4]])                  # the wedge's face (3, 4, 5) is the tet's face (1, 2, 3)
    return 7, 3, e2v, ep


def _hex8_on_hex27():
    e2v, ep = _flat([[27, 28, 29, 30, 0, 2, 8, 6], list(range(27))])     # the hex8's top is the bottom of the lexicographic hex27
    return 31, 3, e2v, ep


def _fan():
    k = np.arange(70)
    return 71, 2, np.ascontiguousarray(np.stack([0 * k, 1 + k, 1 + (k + 1) % 70], axis=1).astype(np.int32)), None


def _i32(rows):
    return np.ascontiguousarray(np.array(rows, np.int32))


ADDED = {
    # the second hex is the natural (1, 8, 9, 2, 5, 10, 11, 6) turned a quarter about its z axis
    "pair_rotated_hex": lambda: (12, 3, _i32([[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 2, 1, 10, 11, 6, 5]]), None),
    "pair_rotated_tet": lambda: (5, 3, _i32([[0, 1, 2, 3], [2, 4, 3, 1]]), None),
    "pair_wedge_hex": _wedge_hex,
    "pair_wedge_tet": _wedge_tet,
    "hex8_on_hex27": _hex8_on_hex27,
    "double_contact": lambda: (5, 2, _i32([[0, 1, 2, 3], [0, 1, 2, 4]]), None),
    "fan_70": _fan,
    "renumbered_hex_5x4x3": _renumbered,
    "hole": _hole,
    "two_blocks": _two_blocks,
    "empty": lambda: (0, 3, np.zeros((0, 8), np.int32), None),
    "isolated": lambda: (7, 3, _i32([[0, 1, 2, 3], [3, 4, 5, 6]]), None),
}
for _d, _n in TYPES:
    ADDED["single_%d_%d" % (_d, _n)] = (lambda d, n: lambda: (n, d, np.arange(n, dtype=np.int32)[None, :].copy(), None))(_d, _n)
NONMANIFOLD = {
    "nonmanifold_2d": lambda: (5, 2, _i32([[0, 1, 2], [0, 1, 3], [0, 1, 4]]), None),
    "nonmanifold_3d": lambda: (6, 3, _i32([[0, 1, 2, 3], [4, 1, 2, 3], [5, 1, 2, 3]]), None),
}
NAMES = [n for _, n in EXISTING] + sorted(ADDED)
_family = {n: f for f, n in EXISTING}
_cases, _tables = {}, {}


def case(name):
    """(NV, dim, elem_to_vertex int32, elem_ptr int32 or None); computed once"""
    if name not in _cases:
        if name in _family:
            X, e2v, ep = existing(_family[name], name)
            c = (X.shape[0], X.shape[1], np.ascontiguousarray(e2v, np.int32), None if ep is None else np.ascontiguousarray(ep, np.int32))
        else:
            c = (ADDED[name] if name in ADDED else NONMANIFOLD[name])()
        _cases[name] = c
    return _cases[name]


def coords(name):
    return existing(_family[name], name)[0]


def table(name):
    """the model's face table of a case, computed once and left unchanged"""
    if name not in _tables:
        NV, dim, e2v, ep = case(name)
        _tables[name] = mm.FaceTable(NV, dim, e2v, ep)
        for a in _tables[name].arrays():
            a.setflags(write=False)
    return _tables[name]


def node_counts(e2v, ep):
    return np.diff(ep).astype(np.int64) if ep is not None else np.full(e2v.shape[0], e2v.shape[1], np.int64)


# ---- what the mesh checks refuse: name -> (NV, dim, elem_to_vertex, elem_ptr, a word of the message)
REFUSED_MESHES = {
    "dim_4": (4, 4, _i32([[0, 1, 2, 3]]), None, "dim"),
    "ptr_start": (8, 3, _i32([0, 1, 2, 3, 4, 5, 6, 7]), _i32([1, 4, 8]), "elem_ptr"),
    "ptr_descending": (8, 3, _i32([0, 1, 2, 3, 4, 5, 6, 7]), _i32([0, 4, 4]), "elem_ptr"),
    "vertex_high": (4, 3, _i32([[0, 1, 2, 4]]), None, "out of range"),
    "vertex_negative": (4, 3, _i32([[0, 1, 2, -1]]), None, "out of range"),
    "vertex_twice": (4, 3, _i32([[0, 1, 2, 1]]), None, "twice"),
    "nodes_5_uniform": (5, 3, _i32([[0, 1, 2, 3, 4]]), None, "no supported element type"),
    "nodes_5_second": (9, 3, _i32([0, 1, 2, 3, 4, 5, 6, 7, 8]), _i32([0, 4, 9]), "element 1"),
}


def face_variants(name):
    """{variant: (face_elem, face_local)} of an existing mesh: the four lists of bdr_forms_cases / elmat_p2_cases"""
    import bdr_forms_cases as bc
    f = _family[name]
    if f == "p2":
        return {v: pc.faces(name, v) for v in pc.VARIANTS}
    return {v: bc.faces(f, name, v) for v in bc.VARIANTS}
