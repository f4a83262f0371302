"""The face table on the device (csrc/mesh_faces.hip) against its definition (saamge_amd/mesh_model.py), integer for integer:
every array and info of FaceTable on every case of mesh_faces_cases with host and with device pointers, face_nodes and
face_dofs on the four face lists of the boundary-form cases, every refusal (which leaves the outputs unwritten), the memory
statistics after free, the partitioner's own element graph on the meshes of one type, boundary_mass fed the table's device
arrays, and the chain coordinates -> element matrices -> face table -> faces on x = 0 -> flags -> operator -> partition ->
hierarchy -> PCG on device pointers against the same chain fed the model's flags and graph from the host."""
import numpy as np
import pytest

from saamge_amd import capi
from saamge_amd import elmat_model as em
from saamge_amd import mesh_model as mm
from saamge_amd import problems as pr

import elmat_cases as ec
import elmat_p2_cases as pc
import mesh_faces_cases as mc

pytestmark = pytest.mark.gpu

EXISTING = [n for _, n in mc.EXISTING]
NAMES = ("slot_ptr", "nbr_elem", "nbr_local", "bdr_elem", "bdr_local", "xadj", "adj")


def _cuda(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()      # (a copy: the model's arrays are read-only)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _refused(message, call):
    with pytest.raises(RuntimeError, match=message) as r:
        call()
    return r.value.info


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", mc.NAMES)
def test_face_table_equals_the_model(name, device):
    NV, dim, e2v, ep = mc.case(name)
    want = mc.table(name)
    dev = _cuda if device else (lambda a: a)
    live = capi.memory_stats()[0]
    with capi.FaceTable.build(NV, dim, dev(e2v), elem_ptr=dev(ep)) as T:
        assert T.info == want.info
        assert (T.NB, T.nnz, T.slots) == (want.NB, want.nnz, want.info[0])
        got = T.get(device=device)
        for k, g, w in zip(NAMES, got, want.arrays()):
            assert _host(g).dtype == w.dtype and np.array_equal(_host(g), w), k
        a = T.arrays()
        assert (a["NB"], a["nnz"]) == (want.NB, want.nnz) and a["slot_ptr"] and a["xadj"]
        assert capi.memory_stats()[0] > live
    assert capi.memory_stats()[0] == live                     # the handle's arrays and every temporary are back


@pytest.mark.parametrize("name", sorted(mc.NONMANIFOLD))
def test_nonmanifold_is_refused(name):
    NV, dim, e2v, ep = mc.case(name)
    live = capi.memory_stats()[0]
    for dev in (_cuda, lambda a: a):
        info = _refused("element 0: a face is shared by more than two elements", lambda: capi.FaceTable(NV, dim, dev(e2v)))
        assert info[6] == 0 and info[0] == 3 * (dim + 1) and info[5] == 3
    assert capi.memory_stats()[0] == live


def test_nonmanifold_names_the_lowest_element():
    e2v = np.array([[6, 7, 8, 9], [0, 1, 2, 3], [4, 1, 2, 3], [5, 1, 2, 3]], np.int32)
    assert _refused("element 1: a face is shared", lambda: capi.FaceTable(10, 3, _cuda(e2v)))[6] == 1


@pytest.mark.parametrize("name", sorted(mc.REFUSED_MESHES))
def test_mesh_refusals(name):
    NV, dim, e2v, ep, word = mc.REFUSED_MESHES[name]
    live = capi.memory_stats()[0]
    for dev in (_cuda, lambda a: a):
        info = _refused(word, lambda: capi.FaceTable(NV, dim, dev(e2v), elem_ptr=dev(ep)))
        assert info == [0, 0, 0, 0, 0, 0, -1, 0]
        flags = dev(np.full(max(NV, 1) * 3, 4, np.int8))
        one = dev(np.zeros(1, np.int32))
        with pytest.raises(RuntimeError, match=word):
            capi.face_dofs(NV, dim, dev(e2v), one, one, flags[:NV], elem_ptr=dev(ep))
        assert (_host(flags) == 4).all()
    assert capi.memory_stats()[0] == live


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", EXISTING)
def test_face_nodes_and_face_dofs_equal_the_model(name, device):
    NV, dim, e2v, ep = mc.case(name)
    dev = _cuda if device else (lambda a: np.array(a))
    de, dp = dev(e2v), None if ep is None else dev(ep)
    for variant, (fe, fl) in mc.face_variants(name).items():
        ptr, nodes = capi.face_nodes(NV, dim, de, dev(fe), dev(fl), elem_ptr=dp, device=device)
        wptr, wnodes = mm.face_nodes(dim, e2v, ep, fe, fl)
        assert np.array_equal(_host(ptr), wptr) and np.array_equal(_host(nodes), wnodes), variant
        for vdim, mask, flag in [(1, 1, 0x02), (dim, 1, 0x02), (dim, 2, 0x05), (dim, 2 ** dim - 1, 0x02)]:
            before = np.random.default_rng(19).integers(0, 8, vdim * NV).astype(np.int8)      # bits set beforehand
            want = before.copy()
            winfo = mm.face_dofs(dim, e2v, ep, fe, fl, vdim, mask, flag, want)
            got = dev(before)
            info = capi.face_dofs(NV, dim, de, dev(fe), dev(fl), got, vdim=vdim, comp_mask=mask, flag=flag, elem_ptr=dp)
            assert info == winfo and np.array_equal(_host(got), want), (variant, vdim, mask, flag)


def test_face_dofs_keeps_the_bytes_around_an_unaligned_array():
    """20 bytes at an odd address inside a larger tensor: the words of the first and of the last byte reach outside the array"""
    NV, dim, e2v, ep = mc.case("tris_4x3")
    assert NV == 20
    T = mc.table("tris_4x3")
    whole = _cuda(np.full(NV + 16, 0x10, np.int8))
    view = whole[5:5 + NV]
    info = capi.face_dofs(NV, dim, _cuda(e2v), _cuda(T.bdr_elem), _cuda(T.bdr_local), view, flag=0x02)
    want = np.full(NV, 0x10, np.int8)
    winfo = mm.face_dofs(dim, e2v, ep, T.bdr_elem, T.bdr_local, 1, 1, 0x02, want)
    got = _host(whole)
    assert info == winfo and np.array_equal(got[5:5 + NV], want)
    assert (got[:5] == 0x10).all() and (got[5 + NV:] == 0x10).all()


def test_face_list_refusals_leave_the_outputs_unwritten():
    NV, dim, e2v, ep = mc.case("mixed_4")
    nd = mc.node_counts(e2v, ep)
    wedge = int(np.flatnonzero(nd == 6)[0])
    ok_l = np.zeros(4, np.int32)
    lists = [(np.array([0, 1, len(nd), -1], np.int32), ok_l, 2, r"face 2: face_elem is outside \[0, NE\)"),
             (np.array([0, wedge, wedge], np.int32), np.array([0, 5, 7], np.int32), 1, "face 1: face_local is outside"),
             (np.array([3, 0, 1, 0, 1], np.int32), np.array([0, 2, 1, 2, 1], np.int32), 1, "face 1: the same")]
    live = capi.memory_stats()[0]
    for dev in (_cuda, lambda a: np.array(a)):
        for fe, fl, index, message in lists:
            flags = dev(np.full(NV, 4, np.int8))
            info = _refused(message, lambda: capi.face_dofs(NV, dim, dev(e2v), dev(fe), dev(fl), flags, elem_ptr=dev(ep)))
            assert info == [0, 0, 0, index] and (_host(flags) == 4).all()
            with pytest.raises(RuntimeError, match=message):
                capi.face_nodes(NV, dim, dev(e2v), dev(fe), dev(fl), elem_ptr=dev(ep))
        fe = np.arange(4, dtype=np.int32)
        for vdim, mask, flag, word in [(2, 1, 2, "vdim"), (1, 0, 2, "comp_mask"), (1, 2, 2, "comp_mask"), (3, 8, 2, "comp_mask"),
                                       (1, 1, 0, "flag"), (1, 1, 128, "flag")]:
            flags = dev(np.full(3 * NV, 4, np.int8))
            _refused(word, lambda: capi.face_dofs(NV, dim, dev(e2v), dev(fe), dev(ok_l), flags[:NV * (vdim if vdim != 2 else 1)],
                                                  vdim=vdim, comp_mask=mask, flag=flag, elem_ptr=dev(ep)))
            assert (_host(flags) == 4).all()
    assert capi.memory_stats()[0] == live
    empty = np.zeros(0, np.int32)
    ptr, nodes = capi.face_nodes(NV, dim, e2v, empty, empty, elem_ptr=ep)      # NF = 0 is legal
    assert len(nodes) == 0 and ptr.tolist() == [0]
    flags = np.full(NV, 4, np.int8)
    assert capi.face_dofs(NV, dim, e2v, empty, empty, flags, elem_ptr=ep) == [0, 0, 0, -1] and (flags == 4).all()


@pytest.mark.parametrize("name", sorted(mc.PURE_MIN_SHARED))
def test_graph_equals_the_partitioners_own(name):
    """graph 0 of saamge_amd_partition_mesh with min_shared = the nodes of a face: independent device code"""
    NV, dim, e2v, ep = mc.case(name)
    P = capi.partition_mesh(_cuda(e2v.ravel() if ep is not None else e2v), NV, [4], elem_ptr=_cuda(ep),
                            min_shared=mc.PURE_MIN_SHARED[name])
    try:
        xadj, adj = P.graph(0)
    finally:
        P.close()
    with capi.FaceTable(NV, dim, _cuda(e2v), elem_ptr=_cuda(ep)) as T:
        got = T.get()
    assert np.array_equal(got[5], xadj) and np.array_equal(got[6], adj)


@pytest.mark.parametrize("name", ["hex_5x4x3", "mixed_4", "tet10_3x2x2", "mixed_hex8_hex27"])
def test_boundary_mass_takes_the_tables_own_boundary_list(name):
    X = mc.coords(name)
    NV, dim, e2v, ep = mc.case(name)
    fe, fl = pr.boundary_faces(dim, e2v, ep)
    coef = np.random.default_rng(13).uniform(0.5, 2.0, len(fe))
    dX, dv, dp = _cuda(X), _cuda(e2v), _cuda(ep)
    want = capi.boundary_mass(dX, dv, _cuda(fe), _cuda(fl), _cuda(coef), elem_ptr=dp, device=True)
    with capi.FaceTable(NV, dim, dv, elem_ptr=dp) as T:
        assert T.NB == len(fe)
        got = capi.boundary_mass(dX, dv, T.pointer("bdr_elem"), T.pointer("bdr_local"), _cuda(coef), elem_ptr=dp, device=True)
    assert np.array_equal(_host(got).view(np.int64), _host(want).view(np.int64))


# ---- the chain on device pointers ----
def _solve(NV, ep, e2v, elmat, elvec, bdr, part, device):
    """operator_assemble -> assemble_rhs -> eliminate_rhs -> ml_produce_data_mixed64 -> pcg: the operator and the solve as host
    arrays"""
    import torch
    op = capi.Operator(NV, e2v, elmat, bdr, elem_ptr=ep)
    h = None
    try:
        A = [_host(a) for a in op.get(device=device)]
        b = op.assemble_rhs(elvec, device=device)
        op.eliminate_rhs(elmat, torch.zeros(NV, dtype=torch.float64, device="cuda") if device else np.zeros(NV), b)
        prob = pr.Problem(elem_to_dof=e2v, elmat=elmat, bdr=bdr, partitions=[part], elem_ptr=ep)
        h = capi.Hierarchy.from_operator(prob, op, capi.default_params(num_coarsenings=1))
        x, it, conv, hist = h.pcg(b, x=torch.zeros_like(b), rel_tol=1e-8) if device else h.pcg(b, rel_tol=1e-8)
        return A, _host(x), it, conv, np.asarray(hist), _host(b)
    finally:
        if h is not None:
            h.close()
        op.close()


@pytest.mark.parametrize("name,epa", [("hex_5x4x3", 8), ("tet10_3x2x2", 12)])
def test_chain_from_a_mesh_alone(name, epa):
    """-Laplace u = f, u = 0 on the side x = 0, from coords and elem_to_vertex alone"""
    import torch
    if name == "hex_5x4x3":
        X0, e2v, _ = ec.mesh(name, False)
        X = ec.mesh(name, True)[0]
    else:
        X0, e2v, _ = pc.mesh(name, "box")
        X = pc.mesh(name, "straight")[0]
    NV, dim = X.shape
    NE, nde = e2v.shape
    ep = (nde * np.arange(NE + 1)).astype(np.int32)
    flat = np.ascontiguousarray(e2v.ravel(), np.int32)
    f = np.random.default_rng(5).uniform(0.0, 1.0, NV)
    # ---- everything on device pointers
    dX, dX0, dv, dp = _cuda(X), _cuda(X0), _cuda(flat), _cuda(ep)
    elmat_d = capi.element_matrices(dX, dv, 0, _cuda(np.ones(NE)), elem_ptr=dp, device=True)                      # 1
    elvec_d = capi.element_loads(dX, dv, _cuda(f), elem_ptr=dp, device=True)
    with capi.FaceTable(NV, dim, dv, elem_ptr=dp) as T:                                                           # 2
        be, bl = T.pointer("bdr_elem"), T.pointer("bdr_local")
        ptr, nodes = capi.face_nodes(NV, dim, dv, be, bl, elem_ptr=dp, device=True)                               # 3
        off = (dX0[nodes.long(), 0] != 0.0).to(torch.int32)                # per face node: off the side x = 0
        csum = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(off, 0)])
        on_side = (csum[ptr[1:].long()] - csum[ptr[:-1].long()]) == 0
        tbe, tbl = T.get(device=True)[3:5]
        se, sl = tbe[on_side].contiguous(), tbl[on_side].contiguous()
        flags_d = torch.zeros(NV, dtype=torch.int8, device="cuda")
        info = capi.face_dofs(NV, dim, dv, se, sl, flags_d, flag=0x02, elem_ptr=dp)                               # 4
        part_d = torch.zeros(NE, dtype=torch.int32, device="cuda")
        _, nparts_d = capi.partition_graph(NE, T.pointer("xadj"), T.pointer("adj"), epa, part=part_d)            # 6
        d = _solve(NV, dp, dv, elmat_d, elvec_d, flags_d, part_d, True)                                           # 5, 7, 8
    # the flags are the dofs whose undeformed x is 0
    assert np.array_equal(_host(flags_d), np.where(X0[:, 0] == 0.0, 2, 0))
    assert info[0] == int(on_side.sum()) and info[1] == info[2] == int((X0[:, 0] == 0.0).sum()) and info[3] == -1
    # ---- the same chain fed the model's flags and graph from the host
    W = mm.FaceTable(NV, dim, flat, ep)
    wptr, wnodes = mm.face_nodes(dim, flat, ep, W.bdr_elem, W.bdr_local)
    side = np.array([bool((X0[wnodes[a:b], 0] == 0.0).all()) for a, b in zip(wptr[:-1], wptr[1:])])
    flags = np.zeros(NV, np.int8)
    mm.face_dofs(dim, flat, ep, W.bdr_elem[side], W.bdr_local[side], 1, 1, 0x02, flags)
    part, nparts = capi.partition_graph(NE, W.xadj, W.adj, epa)
    assert nparts == nparts_d and np.array_equal(_host(part_d), part)
    elmat = np.ascontiguousarray(em.element_matrices(X, flat, 0, np.ones(NE), elem_ptr=ep))
    elvec = np.ascontiguousarray(em.element_loads(X, flat, f, elem_ptr=ep))
    assert np.array_equal(_host(elmat_d), elmat) and np.array_equal(_host(elvec_d), elvec)
    g = _solve(NV, ep, flat, elmat, elvec, flags, part, False)
    (Ad, xd, itd, convd, histd, bd), (Ag, xg, itg, convg, histg, bg) = d, g
    for a, b in zip(Ad, Ag):
        assert np.array_equal(a, b)                           # the operator, bit for bit
    assert np.array_equal(bd, bg)
    assert convd and convg and itd == itg
    assert np.array_equal(histd, histg) and np.array_equal(xd, xg)
