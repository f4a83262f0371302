"""The definition of the order-2 lift (saamge_amd/mesh_lift_model.py) against independent host code and against its own
invariants: problems.p2_simplex_nodes on the simplex meshes (bit for bit), the structured Q2 grid of problems.q2_hex_nodes on
undeformed boxes (exactly), the face table of the lifted mesh against the face table of the original, the node sets across
interior faces, closed-form counts on a box, problems.q2_straight_sided on a jittered box (to 1e-14), the element layer's
Jacobians, and the refusals."""
import numpy as np
import pytest

from saamge_amd import elmat_model as em
from saamge_amd import mesh_lift_model as lm
from saamge_amd import mesh_model as mm
from saamge_amd import problems as pr

import mesh_faces_cases as mc
import mesh_lift_cases as lc


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("name", ["tets_3x2x2", "tris_4x3", "fan_70", "pair_rotated_tet"])
def test_simplex_lift_equals_p2_simplex_nodes(name):
    NV, dim, e2v, ep = lc.case(name)
    L = lc.model(name)
    X2, e2n = pr.p2_simplex_nodes(lc.coords(name), e2v)
    assert np.array_equal(L.lists(), e2n) and L.lists().dtype == e2n.dtype
    assert np.array_equal(_bits(L.coords2), _bits(X2))
    assert L.info[2] == 0 and L.info[3] == 0 and len(L.face_slot) == 0


@pytest.mark.parametrize("n", [(3, 2, 2), (5, 4, 3)])
def test_undeformed_hex_lift_sits_on_the_q2_grid(n):
    name = "hex_%dx%dx%d" % n
    L = lc.model(name)
    want = pr.grid_coords(tuple(2 * m for m in n))[pr.q2_hex_nodes(n)]
    assert np.array_equal(L.coords2[L.lists()], want)


@pytest.mark.parametrize("name", lc.NAMES)
def test_invariants(name):
    NV, dim, e2v, ep = lc.case(name)
    L = lc.model(name)
    NE = L.NE
    assert L.info[0] == L.NV2 == NV + L.info[1] + L.info[2] + L.info[3]
    assert L.info[4] == len(L.elem_to_node) == L.elem_ptr2[-1] and L.info[6] == -1
    assert (L.edge_ptr.dtype, L.edge_hi.dtype, L.face_slot.dtype) == (np.int64, np.int32, np.int64)
    assert (L.elem_ptr2.dtype, L.elem_to_node.dtype) == (np.int32, np.int32)
    assert len(L.edge_ptr) == NV + 1 and L.edge_ptr[-1] == len(L.edge_hi) == L.info[1] and len(L.face_slot) == L.info[2]
    assert L.info[7] == NV - len(np.unique(e2v))
    # edge_hi: strictly ascending within each owner and above its owner
    owner = np.repeat(np.arange(NV), np.diff(L.edge_ptr))
    assert (L.edge_hi > owner).all()
    inner = np.ones(len(owner), bool)
    inner[L.edge_ptr[:-1][np.diff(L.edge_ptr) > 0]] = False
    assert (np.diff(L.edge_hi.astype(np.int64))[inner[1:]] > 0).all()
    assert L.info[5] == (np.diff(L.edge_ptr).max() if NV else 0)
    # every new node is listed, the vertices keep their ids
    assert np.array_equal(np.unique(L.elem_to_node[L.elem_to_node >= NV]), np.arange(NV, L.NV2))
    assert np.array_equal(L.coords2[:NV], lc.coords(name))
    # the face table of the lifted mesh is the face table of the original
    T1 = mm.FaceTable(NV, dim, e2v, ep)
    T2 = mm.FaceTable(L.NV2, dim, L.elem_to_node, L.elem_ptr2)
    for a, b in zip(T1.arrays(), T2.arrays()):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert T1.info == T2.info
    # across every interior pair both elements list the same nodes
    s = np.flatnonzero(T2.nbr_elem >= 0)
    selem = np.repeat(np.arange(NE), np.diff(T2.slot_ptr))
    if len(s):
        ptr, a = mm.face_nodes(dim, L.elem_to_node, L.elem_ptr2, selem[s], s - T2.slot_ptr[selem[s]])
        ptr_b, b = mm.face_nodes(dim, L.elem_to_node, L.elem_ptr2, T2.nbr_elem[s], T2.nbr_local[s])
        assert np.array_equal(ptr, ptr_b)
        for k in range(len(s)):
            assert sorted(a[ptr[k]:ptr[k + 1]]) == sorted(b[ptr[k]:ptr[k + 1]])
    # the face nodes: one per representative slot, in slot order
    if len(L.face_slot):
        other = np.where(T1.nbr_elem >= 0, T1.slot_ptr[np.maximum(T1.nbr_elem, 0)] + T1.nbr_local, np.arange(len(T1.nbr_elem)))
        assert (np.diff(L.face_slot) > 0).all() and (other[L.face_slot] >= L.face_slot).all()


@pytest.mark.parametrize("name", ["hex_5x4x3", "pair_rotated_hex", "tet_beside_hex"])
def test_a_given_face_table_gives_the_same(name):
    NV, dim, e2v, ep = lc.case(name)
    L = lm.MeshLift(NV, dim, lc.coords(name), e2v, ep, faces=mm.FaceTable(NV, dim, e2v, ep))
    for a, b in zip(L.arrays(), lc.model(name).arrays()):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="does not fit"):
        lm.MeshLift(NV, dim, None, e2v, ep, faces=mc.table("hex_3x2x2"))
    assert lm.MeshLift(NV, dim, None, e2v, ep).coords2 is None


@pytest.mark.parametrize("n", [(3, 2, 2), (5, 4, 3), (9, 8, 7)])
def test_counts_on_a_box(n):
    nx, ny, nz = n
    info = lc.model("hex_%dx%dx%d" % n).info
    assert info[1] == nx * (ny + 1) * (nz + 1) + (nx + 1) * ny * (nz + 1) + (nx + 1) * (ny + 1) * nz
    assert info[2] == (nx + 1) * ny * nz + nx * (ny + 1) * nz + nx * ny * (nz + 1)
    assert info[3] == nx * ny * nz and info[4] == 27 * nx * ny * nz
    assert info[0] == (2 * nx + 1) * (2 * ny + 1) * (2 * nz + 1) and info[5] == 3 and info[7] == 0


def test_counts_on_a_rectangle():
    info = lc.model("quads_4x3").info
    assert info[:5] == [9 * 7, 4 * 4 + 5 * 3, 0, 12, 9 * 12]
    info = lc.model("tris_and_quads").info
    assert info[:5] == [20 + 31 + 4 + 8, 31 + 4, 0, 8, 9 * 8 + 6 * 8]
    assert lc.model("fan_70").info[5] == 70
    assert lc.model("unused_vertex").info[7] == 2


def test_q2_straight_sided_moves_a_jittered_lift_by_rounding_only():
    """q2_straight_sided sums the corners of a face or cell in another order: at most 8 additions of numbers below 1.3, 8 ulp"""
    X, e2v = lc.jittered_hex()
    assert np.abs(X).max() < 1.3
    L = lm.MeshLift(X.shape[0], 3, X, e2v)
    moved = np.abs(pr.q2_straight_sided(L.coords2, L.lists()) - L.coords2).max()
    print("largest move: %.3e" % moved)
    assert moved <= 1e-14


@pytest.mark.parametrize("name", lc.GEOMETRIC + ["jittered_hex"])
def test_the_element_layer_accepts_the_lift(name):
    if name == "jittered_hex":
        X, e2v = lc.jittered_hex()
        L = lm.MeshLift(X.shape[0], 3, X, e2v)
    else:
        L = lc.model(name)
    NE = L.NE
    em.element_matrices(L.coords2, L.elem_to_node, 0, np.ones(NE), elem_ptr=L.elem_ptr2)       # (raises ElementError otherwise)
    em.element_mass(L.coords2, L.elem_to_node, np.ones(NE), elem_ptr=L.elem_ptr2)


def test_refusals():
    NV, dim, e2v, ep = mc.case("mixed_4")
    wedge = int(np.flatnonzero(mc.node_counts(e2v, ep) == 6)[0])
    with pytest.raises(lm.LiftError, match="element %d: a wedge" % wedge) as r:
        lm.MeshLift(NV, dim, None, e2v, ep)
    assert r.value.element == wedge and r.value.info == [0, 0, 0, 0, 0, 0, wedge, 0]
    NV, dim, e2v, ep = mc.case("hex27_3x2x2")
    with pytest.raises(lm.LiftError, match="element 0: 27 nodes") as r:
        lm.MeshLift(NV, dim, None, e2v, ep)
    assert r.value.info[6] == 0
    for name in ("single_2_6", "single_2_9", "single_3_10", "single_3_6"):
        NV, dim, e2v, ep = mc.case(name)
        with pytest.raises(lm.LiftError, match="element 0"):
            lm.MeshLift(NV, dim, None, e2v, ep)
    flat = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 1, 2, 3, 4, 5], np.int32)                # tet, wedge, wedge
    with pytest.raises(lm.LiftError, match="element 1: a wedge"):
        lm.MeshLift(10, 3, None, np.array([0, 1, 2, 3] + flat[4:].tolist(), np.int32), np.array([0, 4, 10, 16], np.int32))
    for name, (NV, dim, e2v, ep, word) in sorted(mc.REFUSED_MESHES.items()):
        with pytest.raises(ValueError, match=word):
            lm.MeshLift(NV, dim, None, e2v, ep)
    NV, dim, e2v, ep = mc.case("nonmanifold_3d")                                               # (no hexahedron: no face table)
    assert lm.MeshLift(NV, dim, None, e2v, ep).info[1] == 12
    with pytest.raises(ValueError, match="coords"):
        lm.MeshLift(5, 3, np.zeros((4, 3)), *mc.case("pair_rotated_tet")[2:])
