"""The order-2 lift on the device (csrc/mesh_lift.hip) against its definition (saamge_amd/mesh_lift_model.py), integer for
integer and coordinate bit for coordinate bit: every array, NV2 and info of MeshLift on every case of mesh_lift_cases with host
and with device pointers, with and without coordinates, with the face table built inside and handed in; the memory statistics
after free; every refusal (which leaves the outputs unwritten); element_matrices and element_mass fed the handle's own device
arrays; and two chains on device pointers -- lift -> element matrices -> face table of the lifted mesh -> faces on x = 0 -> flags
-> operator -> partition -> hierarchy -> PCG -- against the same chain fed from the host: the model's arrays for the jittered
hexahedra, problems.p2_simplex_nodes (independent host code) for the tetrahedra."""
import ctypes as C

import numpy as np
import pytest

from saamge_amd import capi
from saamge_amd import mesh_lift_model as lm
from saamge_amd import mesh_model as mm
from saamge_amd import problems as pr

import elmat_cases as ec
import mesh_faces_cases as mc
import mesh_lift_cases as lc

pytestmark = pytest.mark.gpu

NAMES = ("coords2", "elem_ptr2", "elem_to_node", "edge_ptr", "edge_hi", "face_slot")


def _cuda(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()      # (a copy: the cases' arrays are read-only)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _same(got, want, what):
    g = _host(got)
    assert g.dtype == want.dtype and g.shape == want.shape, what
    assert np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, want.view(np.int64) if g.dtype == np.float64 else want), what


def _refused(message, call):
    with pytest.raises(RuntimeError, match=message) as r:
        call()
    return r.value.info


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_lift_equals_the_model(name, device):
    NV, dim, e2v, ep = lc.case(name)
    want = lc.model(name)
    dev = _cuda if device else (lambda a: a)
    X, de, dp = dev(lc.coords(name)), dev(e2v), dev(ep)
    live = capi.memory_stats()[0]
    with capi.FaceTable.build(NV, dim, de, elem_ptr=dp) as T:
        held = capi.memory_stats()[0]
        for with_coords in (True, False):
            for faces in (None, T):
                with capi.MeshLift.build(X if with_coords else None, de, elem_ptr=dp, faces=faces, NV=NV, dim=dim) as L:
                    what = (with_coords, faces is not None)
                    assert L.info == want.info and L.NV2 == want.NV2, what
                    a = L.arrays()
                    assert a["NV2"] == want.NV2 and a["elem_ptr2"] and a["edge_ptr"] and bool(a["coords2"]) == (with_coords and want.NV2 > 0)
                    got = L.get(device=device)
                    assert (got[0] is None) == (not with_coords)
                    for k, g, w in zip(NAMES, got, want.arrays()):
                        if g is not None:
                            _same(g, w, (k,) + what)
                    assert capi.memory_stats()[0] > held
                assert capi.memory_stats()[0] == held                 # the handle's arrays and every temporary are back
    assert capi.memory_stats()[0] == live


def test_a_repeated_lift_gives_the_same_bits():
    """the positions inside an owner's bucket depend on the order in which atomics land; the result must not"""
    NV, dim, e2v, ep = lc.case("hex_9x8x7")
    X = _cuda(lc.coords("hex_9x8x7"))
    de = _cuda(e2v)
    for _ in range(3):
        with capi.MeshLift(X, de) as L:
            for k, g, w in zip(NAMES, L.get(device=True), lc.model("hex_9x8x7").arrays()):
                _same(g, w, k)


def _raw_lift(NV, dim, X, e2v, ep, faces, out, info):
    NV, NE, nde = capi._mesh_sizes(NV, e2v, ep)
    return capi.load().saamge_amd_mesh_lift_order2(
        C.c_int(NV), C.c_int(dim), capi._ptr(X), C.c_int(NE), C.c_int(nde), capi._ptr(ep), capi._ptr(e2v),
        faces.h if faces is not None else None, C.c_void_p(0), C.byref(out) if out is not None else None, info)


def test_refusals_leave_the_outputs_unwritten():
    live = capi.memory_stats()[0]
    sentinel = 0x5a5a5a5a
    cases = []
    NV, dim, e2v, ep = mc.case("mixed_4")
    wedge = int(np.flatnonzero(mc.node_counts(e2v, ep) == 6)[0])
    cases.append((NV, dim, e2v, ep, "element %d: a wedge" % wedge, wedge))
    NV, dim, e2v, ep = mc.case("hex27_3x2x2")
    cases.append((NV, dim, e2v, ep, "element 0: 27 nodes", 0))
    for name in ("single_2_6", "single_2_9", "single_3_10", "single_3_6"):
        NV, dim, e2v, ep = mc.case(name)
        cases.append((NV, dim, e2v, ep, "element 0", 0))
    for name, (NV, dim, e2v, ep, word) in sorted(mc.REFUSED_MESHES.items()):
        cases.append((NV, dim, e2v, ep, word, -1))
    NV, dim, e2v, ep = mc.case("nonmanifold_3d")
    hexes = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 8, 9, 10, 11], [0, 1, 2, 3, 12, 13, 14, 15]], np.int32)
    cases.append((16, 3, hexes, None, "shared by more than two", 0))
    for NV, dim, e2v, ep, word, element in cases:
        for dev in (_cuda, lambda a: a):
            out = C.c_void_p(sentinel)
            info = (C.c_longlong * 8)()
            rc = _raw_lift(NV, dim, None, dev(e2v), dev(ep), None, out, info)
            assert rc != 0 and out.value == sentinel, word
            assert list(info) == [0, 0, 0, 0, 0, 0, element, 0], word
            _refused(word, lambda: capi.MeshLift(None, dev(e2v), elem_ptr=dev(ep), NV=NV, dim=dim))
    assert _raw_lift(4, 3, None, np.zeros((1, 4), np.int32), None, None, None, (C.c_longlong * 8)()) != 0      # out NULL
    # a face table built on another mesh: another number of elements, then other slots
    NV, dim, e2v, ep = lc.case("hex_5x4x3")
    tets = lc.case("tets_3x2x2")
    few = tets[2][:10]
    with capi.FaceTable(*lc.case("hex_3x2x2")[:3]) as T3, capi.FaceTable(tets[0], 3, few) as T10:
        held = capi.memory_stats()[0]
        for dev in (_cuda, lambda a: a):
            out = C.c_void_p(sentinel)
            assert _raw_lift(NV, dim, None, dev(e2v), None, T3, out, (C.c_longlong * 8)()) != 0 and out.value == sentinel
            _refused("does not fit the mesh", lambda: capi.MeshLift(None, dev(e2v), faces=T3, NV=NV, dim=dim))
            ten = np.ascontiguousarray(e2v[:10])
            out = C.c_void_p(sentinel)
            assert _raw_lift(NV, dim, None, dev(ten), None, T10, out, (C.c_longlong * 8)()) != 0 and out.value == sentinel
            _refused("the slots of element 0", lambda: capi.MeshLift(None, dev(ten), faces=T10, NV=NV, dim=dim))
        assert capi.memory_stats()[0] == held
    assert capi.memory_stats()[0] == live


@pytest.mark.parametrize("name", ["hex_5x4x3", "tets_3x2x2", "quads_4x3", "tris_4x3", "tris_and_quads", "tet_beside_hex"])
def test_the_element_layer_takes_the_handles_arrays(name):
    NV, dim, e2v, ep = lc.case(name)
    want = lc.model(name)
    NE = want.NE
    coef = np.random.default_rng(3).uniform(0.5, 2.0, NE)
    K = capi.element_matrices(want.coords2, want.elem_to_node, 0, coef, elem_ptr=want.elem_ptr2)
    Mm = capi.element_mass(want.coords2, want.elem_to_node, coef, elem_ptr=want.elem_ptr2)
    with capi.MeshLift(_cuda(lc.coords(name)), _cuda(e2v), elem_ptr=_cuda(ep)) as L:
        X2, e2n, ep2 = L.pointer("coords2"), L.pointer("elem_to_node"), L.get(device=True)[1]
        Kd = capi.element_matrices(X2, e2n, 0, _cuda(coef), elem_ptr=ep2, device=True)
        Md = capi.element_mass(X2, e2n, _cuda(coef), elem_ptr=ep2, device=True)
        if ep is None:                                                     # a mesh of one type: (NE, nodes) lists, no offsets
            rows = L.pointer("elem_to_node", shape=(NE, L.entries // NE))
            Ku = capi.element_matrices(X2, rows, 0, _cuda(coef), device=True)
            assert np.array_equal(_host(Ku).ravel().view(np.int64), K.view(np.int64))
    assert np.array_equal(_host(Kd).view(np.int64), K.view(np.int64))
    assert np.array_equal(_host(Md).view(np.int64), Mm.view(np.int64))


# ---- the chains on device pointers ----
def _solve(n, ep, e2n, elmat, elvec, bdr, part, device):
    """operator_assemble -> assemble_rhs -> eliminate_rhs -> ml_produce_data_mixed64 -> pcg, everything as host arrays"""
    import torch
    op = capi.Operator(n, e2n, elmat, bdr, elem_ptr=ep)
    h = None
    try:
        A = [_host(a) for a in op.get(device=device)]
        b = op.assemble_rhs(elvec, device=device)
        op.eliminate_rhs(elmat, torch.zeros(n, dtype=torch.float64, device="cuda") if device else np.zeros(n), b)
        prob = pr.Problem(elem_to_dof=e2n, elmat=elmat, bdr=bdr, partitions=[part], elem_ptr=ep)
        h = capi.Hierarchy.from_operator(prob, op, capi.default_params(num_coarsenings=1))
        x, it, conv, hist = h.pcg(b, x=torch.zeros_like(b), rel_tol=1e-8) if device else h.pcg(b, rel_tol=1e-8)
        return A, _host(x), it, conv, np.asarray(hist), _host(b)
    finally:
        if h is not None:
            h.close()
        op.close()


def _chain(dim, X2, X02, e2n, ep2, f, epa, device):
    """from the lifted mesh on: -Laplace u = f, u = 0 on the side x = 0 of the undeformed mesh (coordinates X02).  Device
    tensors with device=True, numpy arrays otherwise; returns (flags, part, the results of _solve), all on the host."""
    import torch
    NV2, NE = int(X2.shape[0]), int(ep2.shape[0]) - 1
    dev = _cuda if device else (lambda a: a)
    elmat = capi.element_matrices(X2, e2n, 0, dev(np.ones(NE)), elem_ptr=ep2, device=device)
    elvec = capi.element_loads(X2, e2n, dev(f), elem_ptr=ep2, device=device)
    with capi.FaceTable(NV2, dim, e2n, elem_ptr=ep2) as T:
        be, bl = T.get(device=device)[3:5]
        ptr, nodes = capi.face_nodes(NV2, dim, e2n, be, bl, elem_ptr=ep2, device=device)
        if device:
            off = (X02[nodes.long(), 0] != 0.0).to(torch.int32)
            csum = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(off, 0)])
            on_side = (csum[ptr[1:].long()] - csum[ptr[:-1].long()]) == 0
            se, sl = be[on_side].contiguous(), bl[on_side].contiguous()
            flags = torch.zeros(NV2, dtype=torch.int8, device="cuda")
            part = torch.zeros(NE, dtype=torch.int32, device="cuda")
            capi.partition_graph(NE, T.pointer("xadj"), T.pointer("adj"), epa, part=part)
        else:
            on_side = np.array([bool((X02[nodes[a:b], 0] == 0.0).all()) for a, b in zip(ptr[:-1], ptr[1:])])
            se, sl = np.ascontiguousarray(be[on_side]), np.ascontiguousarray(bl[on_side])
            flags = np.zeros(NV2, np.int8)
            xadj, adj = T.get()[5:7]
            part, _ = capi.partition_graph(NE, xadj, adj, epa)
        capi.face_dofs(NV2, dim, e2n, se, sl, flags, flag=0x02, elem_ptr=ep2)
    return _host(flags), _host(part), _solve(NV2, ep2, e2n, elmat, elvec, flags, part, device)


@pytest.mark.parametrize("name,epa", [("hex_5x4x3", 8), ("tets_3x2x2", 12)])
def test_chain_from_an_order_1_mesh(name, epa):
    X0, e2v, _ = ec.mesh(name, False)
    X = ec.mesh(name, True)[0]                                             # every vertex moved by up to 0.2 mesh widths
    NV, dim = X.shape
    e2v = np.ascontiguousarray(e2v, np.int32)
    # ---- on device pointers, end to end: the lift of the jittered mesh, and of the undeformed one to find the side x = 0
    de = _cuda(e2v)
    with capi.MeshLift(_cuda(X), de) as L, capi.MeshLift(_cuda(X0), de) as L0:
        dX2, dp2, dn = L.get(device=True)[:3]
        dX02 = L0.get(device=True)[0]
        NV2 = L.NV2
    f = np.random.default_rng(5).uniform(0.0, 1.0, NV2)
    d = _chain(dim, dX2, dX02, dn, dp2, f, epa, True)
    # ---- the same chain fed from the host
    if name == "hex_5x4x3":
        W, W0 = lm.MeshLift(NV, dim, X, e2v), lm.MeshLift(NV, dim, X0, e2v)
        X2, X02, e2n, ep2 = W.coords2, W0.coords2, W.elem_to_node, W.elem_ptr2
    else:
        X2, rows = pr.p2_simplex_nodes(X, e2v)
        X02 = pr.p2_simplex_nodes(X0, e2v)[0]
        e2n, ep2 = np.ascontiguousarray(rows.ravel()), (rows.shape[1] * np.arange(rows.shape[0] + 1)).astype(np.int32)
    assert np.array_equal(_host(dX2).view(np.int64), X2.view(np.int64)) and np.array_equal(_host(dn), e2n)
    g = _chain(dim, X2, X02, e2n, ep2, f, epa, False)
    assert np.array_equal(d[0], g[0]) and np.array_equal(d[0], np.where(X02[:, 0] == 0.0, 2, 0))
    assert d[0].any() and np.array_equal(d[1], g[1])
    (Ad, xd, itd, convd, histd, bd), (Ag, xg, itg, convg, histg, bg) = d[2], g[2]
    for a, b in zip(Ad, Ag):
        assert np.array_equal(a, b)                                        # the operator, bit for bit
    assert np.array_equal(bd, bg)
    assert convd and convg and itd == itg
    assert np.array_equal(histd, histg) and np.array_equal(xd, xg)
