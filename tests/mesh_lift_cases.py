"""Meshes shared by the order-2 lift tests (test_mesh_lift_model.py, test_gpu_mesh_lift.py): the order-1 liftable cases of
mesh_faces_cases, and three built here:

  tris_and_quads    quads_4x3 with its upper row split into triangles, through elem_ptr: two lifts in one list, in 2D
  tet_beside_hex    one hexahedron and one tetrahedron that share one edge only: two lifts in 3D, a face table whose slots are
                    not 6 per element, an edge node that two types list
  unused_vertex     tets_3x2x2 with NV + 2: vertices that no element lists keep their ids, and every new id moves up by 2

A case is (NV, dim, elem_to_vertex, elem_ptr) as in mesh_faces_cases; coords(name) gives coordinates for it: the mesh's own
where it has a geometry (GEOMETRIC), numbers drawn from a seed elsewhere -- the lift only adds and halves them."""
import numpy as np

from saamge_amd import mesh_lift_model as lm
from saamge_amd import problems as pr

import elmat_cases as ec
import mesh_faces_cases as mc

FROM_FACES = ["hex_3x2x2", "hex_5x4x3", "hex_9x8x7", "tets_3x2x2", "quads_4x3", "tris_4x3", "pair_rotated_hex", "pair_rotated_tet",
              "double_contact", "fan_70", "renumbered_hex_5x4x3", "hole", "two_blocks", "empty", "isolated", "single_2_3",
              "single_2_4", "single_3_4", "single_3_8"]


def _tris_and_quads():
    X, e2v, _ = ec.mesh("quads_4x3", False)
    top = X[e2v, 1].mean(axis=1)
    lists = []
    for q, y in zip(e2v.tolist(), top):
        lists += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]] if y == top.max() else [q]
    flat, ep = mc._flat(lists)
    return X.shape[0], 2, flat, ep


def _tet_beside_hex():
    flat, ep = mc._flat([[0, 1, 2, 3, 4, 5, 6, 7], [1, 2, 8, 9]])
    return 10, 3, flat, ep


def _unused_vertex():
    NV, dim, e2v, ep = mc.case("tets_3x2x2")
    return NV + 2, dim, e2v, ep


ADDED = {"tris_and_quads": _tris_and_quads, "tet_beside_hex": _tet_beside_hex, "unused_vertex": _unused_vertex}
NAMES = FROM_FACES + sorted(ADDED)
_TET_BESIDE_HEX_X = np.array(pr.grid_coords((1, 1, 1))[[0, 1, 3, 2, 4, 5, 7, 6]].tolist() + [[2.0, 0.5, 0.0], [1.5, 0.5, -1.0]])
_cases, _coords, _models = {}, {}, {}


def case(name):
    if name not in _cases:
        _cases[name] = ADDED[name]() if name in ADDED else mc.case(name)
    return _cases[name]


def _geometry(name):
    if name in ("hex_3x2x2", "hex_5x4x3", "hex_9x8x7", "tets_3x2x2", "quads_4x3", "tris_4x3"):
        return mc.coords(name)
    if name == "tris_and_quads":
        return mc.coords("quads_4x3")
    if name == "hole":
        return mc.coords("hex_5x4x3")
    if name == "renumbered_hex_5x4x3":
        X = mc.coords("hex_5x4x3")
        out = np.zeros_like(X)
        out[mc.renumbering()[1]] = X
        return out
    if name == "two_blocks":
        X = mc.coords("hex_3x2x2")
        return np.concatenate([X, X + np.array([2.0, 0.0, 0.0])])
    if name == "unused_vertex":
        return np.concatenate([mc.coords("tets_3x2x2"), [[3.0, 3.0, 3.0], [4.0, 4.0, 4.0]]])
    if name == "tet_beside_hex":
        return _TET_BESIDE_HEX_X
    return None


GEOMETRIC = [n for n in NAMES if _geometry(n) is not None]


def coords(name):
    """(NV, dim) float64, computed once and read-only"""
    if name not in _coords:
        NV, dim, _, _ = case(name)
        X = _geometry(name)
        if X is None:
            X = np.random.default_rng(23).uniform(-1.0, 1.0, (NV, dim))
        X = np.array(X, dtype=np.float64, order="C")             # (a copy: the other case files keep theirs writeable)
        assert X.shape == (NV, dim)
        X.setflags(write=False)
        _coords[name] = X
    return _coords[name]


def model(name):
    """the model's lift of a case (with coordinates), computed once and left unchanged"""
    if name not in _models:
        NV, dim, e2v, ep = case(name)
        L = lm.MeshLift(NV, dim, coords(name), e2v, ep)
        for a in L.arrays():
            a.setflags(write=False)
        _models[name] = L
    return _models[name]


def jittered_hex():
    """(coords, elem_to_vertex) of hex_5x4x3 with every vertex moved by up to 0.2 mesh widths"""
    X, e2v, _ = ec.mesh("hex_5x4x3", True)
    return X, np.ascontiguousarray(e2v, np.int32)
