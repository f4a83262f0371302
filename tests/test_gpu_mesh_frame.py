"""What the mesh entry points share (csrc/mesh.hip, capi._Handle): one refusal of an element of no type and one refusal of a
node count of no type, word for word from FaceTable, face_nodes, face_dofs, MeshLift, MeshRefine and element_matrices, with host
and with device pointers; and one life of a handle -- free() twice, the end of a `with` block, calls after free(), the device
memory given back, pointer(name) in the shape and type of get() -- for FaceTable, MeshLift and MeshRefine."""
import numpy as np
import pytest

from saamge_amd import capi

pytestmark = pytest.mark.gpu

# a tetrahedron and an element of 5 nodes: no type in 3D has 5
NV, DIM = 6, 3
COORDS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [2, 1, 1]], np.float64)
MIXED_PTR = np.array([0, 4, 9], np.int32)
MIXED_E2V = np.array([0, 1, 2, 3, 1, 2, 3, 4, 5], np.int32)
UNIFORM_E2V = np.array([[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]], np.int32)
FACE_ELEM, FACE_LOCAL = np.array([0], np.int32), np.array([0], np.int32)


def _cuda(a):
    import torch
    return torch.as_tensor(np.array(a)).cuda()


def _entry_points(X, e2v, ep, fe, fl):
    """(name, call, index of the refused element / face in .info or None: the call has no info) of the six entry points"""
    return [
        ("FaceTable", lambda: capi.FaceTable(NV, DIM, e2v, elem_ptr=ep), 6),
        ("face_nodes", lambda: capi.face_nodes(NV, DIM, e2v, fe, fl, elem_ptr=ep), None),
        ("face_dofs", lambda: capi.face_dofs(NV, DIM, e2v, fe, fl, np.zeros(NV, np.int8), elem_ptr=ep), 3),
        ("MeshLift", lambda: capi.MeshLift(X, e2v, elem_ptr=ep), 6),
        ("MeshRefine", lambda: capi.MeshRefine(X, e2v, elem_ptr=ep), 6),
        ("element_matrices", lambda: capi.element_matrices(X, e2v, 0, np.ones(2), elem_ptr=ep), 6),
    ]


def _all_refuse(message, e2v, ep, device):
    dev = _cuda if device else (lambda a: a)
    live = capi.memory_stats()[0]
    calls = _entry_points(dev(COORDS), dev(e2v), None if ep is None else dev(ep), dev(FACE_ELEM), dev(FACE_LOCAL))
    assert len(calls) == 6
    for name, call, where in calls:
        with pytest.raises(RuntimeError, match=message) as r:
            call()
        assert "saamge_amd_" in str(r.value), name
        if where is not None:      # no element and no face was named in info: -1, and every other word as a call without elements leaves it
            assert r.value.info == [0] * where + [-1] + [0] * (len(r.value.info) - where - 1), name
            assert len(r.value.info) == (4 if name == "face_dofs" else 8), name
    assert capi.memory_stats()[0] == live


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_an_element_of_no_type_is_refused_alike_by_every_entry_point(device):
    _all_refuse("element 1: 5 nodes are no supported element type in 3D", MIXED_E2V, MIXED_PTR, device)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_node_count_of_no_type_is_refused_alike_by_every_entry_point(device):
    _all_refuse("nde = 5 nodes are no supported element type in 3D", UNIFORM_E2V, None, device)


# ---- the life of a handle, on one hexahedron ----------------------------------------------------------------------------------
HEX_X = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64)
HEX_E2V = np.arange(8, dtype=np.int32).reshape(1, 8)
MAKERS = {
    "FaceTable": (lambda: capi.FaceTable(8, 3, HEX_E2V), ("slot_ptr", "nbr_elem", "nbr_local", "bdr_elem", "bdr_local", "xadj", "adj")),
    "MeshLift": (lambda: capi.MeshLift(HEX_X, HEX_E2V), ("coords2", "elem_ptr2", "elem_to_node", "edge_ptr", "edge_hi", "face_slot")),
    "MeshRefine": (lambda: capi.MeshRefine(HEX_X, HEX_E2V, levels=1, want_interp=True), ("coords", "elem_ptr", "elem_to_vertex")),
}


@pytest.mark.parametrize("kind", sorted(MAKERS))
def test_the_life_of_a_handle(kind):
    make, names = MAKERS[kind]
    live = capi.memory_stats()[0]
    h = make()
    assert capi.memory_stats()[0] > live and h.h is not None and h.h.value
    # pointer(name): the address of arrays(), in the shape and the type of the array get() gives
    got, addresses = h.get(), h.arrays()
    assert len(got) == len(names) and set(names) <= set(addresses)
    for name, g in zip(names, got):
        p = h.pointer(name)
        assert p.data_ptr() == addresses[name] and (p.data_ptr() != 0) == (g.size > 0), name      # (one hexahedron: no adj)
        assert tuple(p.shape) == tuple(g.shape) and np.dtype(p.dtype) == g.dtype, name
    for k, g in enumerate(h.get(device=True)):
        assert np.array_equal(g.cpu().numpy(), got[k]) and tuple(g.shape) == tuple(got[k].shape), names[k]
    h.free()
    assert h.h is None and capi.memory_stats()[0] == live
    h.free()                                                  # twice is harmless, and so is close()
    h.close()
    for call in (h.arrays, h.get) + ((lambda: h.interp(0), lambda: h.level_info(0)) if kind == "MeshRefine" else ()):
        with pytest.raises(RuntimeError, match="null argument"):
            call()
    assert capi.memory_stats()[0] == live
    with make() as w:
        assert capi.memory_stats()[0] > live and w.arrays()[names[0]]
    assert w.h is None and capi.memory_stats()[0] == live
    with type(h).build(*((8, 3, HEX_E2V) if kind == "FaceTable" else (HEX_X, HEX_E2V))) as b:      # build(): the constructor
        assert type(b) is type(h) and b.info[:3] == h.info[:3]
    assert capi.memory_stats()[0] == live
