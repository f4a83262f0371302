"""The uniform refinement on the device (csrc/mesh_refine.hip) against its definition (saamge_amd/mesh_refine_model.py), integer
for integer and coordinate bit for coordinate bit: the arrays of the result, every P_j, info and every level's counts on every
case of mesh_refine_cases with host and with device pointers, with and without coordinates and interpolations; repeated calls;
the memory statistics after free; every refusal (which leaves the outputs unwritten); two levels in one call against one level
applied twice through the handle's own device arrays; saamge_amd_spmv with the device P; and two chains on device pointers --
refine -> element matrices -> face table -> essential flags -> operator (-> nested partitions by shifts -> hierarchy -> PCG) --
against the same chain fed the model's arrays from the host."""
import ctypes as C

import numpy as np
import pytest

from saamge_amd import capi
from saamge_amd import mesh_refine_model as rm
from saamge_amd import problems as pr

import elmat_cases as ec
import mesh_faces_cases as mc
import mesh_refine_cases as rc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


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
    return getattr(r.value, "info", None)


def _check(R, want, with_coords, interp, device, what):
    """every output of the handle R against the model `want` (which keeps its interpolations)"""
    info = list(want.info)
    info[4] = info[4] if interp else 0
    assert R.info == info and (R.NV, R.NE, R.levels) == (want.NV, want.NE, want.levels), what
    for j in range(want.levels + 1):
        li = list(want.level_info[j])
        li[7] = li[7] if interp or j == want.levels else 0
        assert R.level_info(j) == li, what + (j,)
    a = R.arrays()
    assert (a["NV"], a["NE"]) == (want.NV, want.NE) and a["elem_ptr"] and bool(a["coords"]) == (with_coords and want.NV > 0), what
    got = R.get(device=device)
    assert (got[0] is None) == (not with_coords)
    for k, g, w in zip(capi.MeshRefine.NAMES, got, want.arrays()):
        if g is not None:
            _same(g, w, (k,) + what)
    for j in range(want.levels if interp else 0):
        nrows, ncols, rowptr, col, val = R.interp(j, device=device)
        P = want.P[j]
        assert (nrows, ncols) == (P.nrows, P.ncols) and R.interp_arrays(j)["nnz"] == P.nnz, what + (j,)
        for k, g, w in zip(("rowptr", "col", "val"), (rowptr, col, val), P.arrays()):
            _same(g, w, (k, j) + what)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,levels", rc.CASES)
def test_refine_equals_the_model(name, levels, device):
    NV, dim, e2v, ep = rc.case(name)
    want = rc.model(name, levels)
    dev = _cuda if device else (lambda a: a)
    X, de, dp = dev(rc.coords(name)), dev(e2v), dev(ep)
    live = capi.memory_stats()[0]
    for with_coords in (True, False):
        for interp in (True, False):
            with capi.MeshRefine.build(X if with_coords else None, de, elem_ptr=dp, levels=levels, want_interp=interp, NV=NV,
                                       dim=dim) as R:
                _check(R, want, with_coords, interp, device, (with_coords, interp))
                assert capi.memory_stats()[0] > live
                if not interp:
                    _refused("without want_interp", lambda: R.interp(0))
            assert capi.memory_stats()[0] == live                 # the handle's arrays and every temporary are back


def test_a_repeated_call_gives_the_same_bits():
    NV, dim, e2v, ep = rc.case("hex_9x8x7")
    X, de = _cuda(rc.coords("hex_9x8x7")), _cuda(e2v)
    for _ in range(3):
        with capi.MeshRefine(X, de, levels=2, want_interp=True) as R:
            _check(R, rc.model("hex_9x8x7", 2), True, True, True, ("repeat",))


def _raw(NV, dim, X, e2v, ep, levels, out, info):
    NV, NE, nde = capi._mesh_sizes(NV, e2v, ep)
    return capi.load().saamge_amd_mesh_refine(
        C.c_int(NV), C.c_int(dim), capi._ptr(X), C.c_int(NE), C.c_int(nde), capi._ptr(ep), capi._ptr(e2v), C.c_int(levels), C.c_int(1),
        C.c_void_p(0), C.byref(out) if out is not None else None, info)


def test_refusals_leave_the_outputs_unwritten():
    live = capi.memory_stats()[0]
    sentinel = 0x5a5a5a5a
    cases = []
    NV, dim, e2v, ep = mc.case("mixed_4")
    wedge = int(np.flatnonzero(mc.node_counts(e2v, ep) == 6)[0])
    cases.append((NV, dim, e2v, ep, 2, "level 0: .*element %d: a wedge" % wedge, wedge))
    NV, dim, e2v, ep = mc.case("hex27_3x2x2")
    cases.append((NV, dim, e2v, ep, 1, "element 0: 27 nodes", 0))
    for name in ("single_2_6", "single_2_9", "single_3_10", "single_3_6"):
        NV, dim, e2v, ep = mc.case(name)
        cases.append((NV, dim, e2v, ep, 1, "element 0", 0))
    for name, (NV, dim, e2v, ep, word) in sorted(mc.REFUSED_MESHES.items()):
        cases.append((NV, dim, e2v, ep, 1, word, -1))
    hexes = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 8, 9, 10, 11], [0, 1, 2, 3, 12, 13, 14, 15]], np.int32)
    cases.append((16, 3, hexes, None, 1, "shared by more than two", 0))
    NV, dim, e2v, ep = rc.case("hex_3x2x2")
    cases.append((NV, dim, e2v, ep, 0, "levels must be at least 1", -1))
    cases.append((NV, dim, e2v, ep, -3, "levels must be at least 1", -1))
    cases.append((NV, dim, e2v, ep, rm.MAX_LEVELS + 1, "levels above %d" % rm.MAX_LEVELS, -1))
    for NV, dim, e2v, ep, levels, word, element in cases:
        for dev in (_cuda, lambda a: a):
            out = C.c_void_p(sentinel)
            info = (C.c_longlong * 8)()
            rc_ = _raw(NV, dim, None, dev(e2v), dev(ep), levels, out, info)
            assert rc_ != 0 and out.value == sentinel, word
            assert list(info) == [0, 0, 0, 0, 0, 0, element, 0], word
            got = _refused(word, lambda: capi.MeshRefine(None, dev(e2v), elem_ptr=dev(ep), levels=levels, NV=NV, dim=dim))
            assert got == [0, 0, 0, 0, 0, 0, element, 0]
    assert _raw(4, 3, None, np.zeros((1, 4), np.int32), None, 1, None, (C.c_longlong * 8)()) != 0      # out NULL
    # the level queries of a handle
    with capi.MeshRefine(None, rc.case("tris_4x3")[2], NV=rc.case("tris_4x3")[0], dim=2, levels=2, want_interp=True) as R:
        _refused("outside \\[0, levels\\]", lambda: R.level_info(3))
        _refused("outside \\[0, levels\\)", lambda: R.interp(2))
        _refused("outside \\[0, levels\\)", lambda: R.interp_arrays(-1))
    assert capi.memory_stats()[0] == live


@pytest.mark.parametrize("name", ["hex_5x4x3", "tets_3x2x2", "tris_and_quads", "tet_beside_hex", "quads_4x3"])
def test_two_levels_are_one_level_twice(name):
    NV, dim, e2v, ep = rc.case(name)
    want = rc.model(name, 2)
    with capi.MeshRefine(_cuda(rc.coords(name)), _cuda(e2v), elem_ptr=_cuda(ep), want_interp=True) as R1:
        ep1 = R1.get(device=True)[1]
        with capi.MeshRefine(R1.pointer("coords"), R1.pointer("elem_to_vertex"), elem_ptr=ep1, want_interp=True) as R2:
            for k, g, w in zip(capi.MeshRefine.NAMES, R2.get(device=True), want.arrays()):
                _same(g, w, k)
            for k, g, w in zip(("rowptr", "col", "val"), R2.interp(0)[2:], want.P[1].arrays()):
                _same(g, w, k)
            assert R2.level_info(0) == want.level_info[1]
        if ep is None:                                                     # a mesh of one type: (NE, nodes) lists, no offsets
            rows = R1.pointer("elem_to_vertex", shape=(R1.NE, R1.entries // R1.NE))
            with capi.MeshRefine(R1.pointer("coords"), rows) as R2:
                for k, g, w in zip(capi.MeshRefine.NAMES, R2.get(), want.arrays()):
                    _same(g, w, k)


@pytest.mark.parametrize("name", ["hex_5x4x3", "tets_3x2x2", "tris_and_quads", "tet_beside_hex"])
def test_spmv_takes_the_device_interpolation(name):
    import torch
    NV, dim, e2v, ep = rc.case(name)
    want = rc.model(name, 2)
    with capi.MeshRefine(None, _cuda(e2v), elem_ptr=_cuda(ep), levels=2, want_interp=True, NV=NV, dim=dim) as R:
        for j in range(2):
            a = R.interp_arrays(j)
            x = np.random.default_rng(11 + j).uniform(-1.0, 1.0, a["ncols"])
            y = torch.zeros(a["nrows"], dtype=torch.float64, device="cuda")
            capi.spmv_raw(a["nrows"], a["ncols"], capi._DevicePointer(a["rowptr"], np.int32), capi._DevicePointer(a["col"], np.int32),
                          capi._DevicePointer(a["val"], np.float64), _cuda(x), y)
            err = np.abs(_host(y) - want.P[j].dot(x)).max()
            print("%s P_%d: |spmv - numpy| = %.3e" % (name, j, err))
            assert err <= 8 * U * np.abs(x).max()


# ---- the chains on device pointers ----
def _operator(dim, X, e2v, ep, device):
    """element matrices -> face table -> essential flags on every boundary face -> operator; returns (elmat, flags, op)"""
    import torch
    NV, NE = int(X.shape[0]), int(ep.shape[0]) - 1
    dev = _cuda if device else (lambda a: a)
    elmat = capi.element_matrices(X, e2v, 0, dev(np.ones(NE)), elem_ptr=ep, device=device)
    with capi.FaceTable(NV, dim, e2v, elem_ptr=ep) as T:
        be, bl = T.get(device=device)[3:5]
        flags = torch.zeros(NV, dtype=torch.int8, device="cuda") if device else np.zeros(NV, np.int8)
        capi.face_dofs(NV, dim, e2v, be, bl, flags, flag=0x02, elem_ptr=ep)
    return elmat, flags, capi.Operator(NV, e2v, elmat, flags, elem_ptr=ep)


def test_chain_from_a_coarse_hexahedral_mesh():
    """jittered hex_5x4x3 -> two levels -> ... -> operator -> the nested partitions arange(NE) >> 3 and >> 6 -> hierarchy -> PCG"""
    import torch
    X = ec.mesh("hex_5x4x3", True)[0]
    e2v = np.ascontiguousarray(ec.mesh("hex_5x4x3", True)[1], np.int32)
    want = rm.MeshRefine(X.shape[0], 3, X, e2v, levels=2)
    NE = want.NE
    b = np.random.default_rng(5).uniform(0.0, 1.0, want.NV)
    results = []
    with capi.MeshRefine(_cuda(X), _cuda(e2v), levels=2) as R:
        for device in (True, False):
            if device:
                dX, dp, dv = R.pointer("coords"), R.get(device=True)[1], R.pointer("elem_to_vertex")
                parts = [torch.arange(NE, dtype=torch.int32, device="cuda") >> 3,
                         torch.arange(NE >> 3, dtype=torch.int32, device="cuda") >> 3]
            else:
                dX, dp, dv = want.arrays()
                parts = [(np.arange(NE) >> 3).astype(np.int32), (np.arange(NE >> 3) >> 3).astype(np.int32)]
            elmat, flags, op = _operator(3, dX, dv, dp, device)
            h = None
            try:
                A = [_host(a) for a in op.get(device=device)]
                rhs = _cuda(b) if device else b.copy()
                op.eliminate_rhs(elmat, torch.zeros(want.NV, dtype=torch.float64, device="cuda") if device else np.zeros(want.NV), rhs)
                prob = pr.Problem(elem_to_dof=dv, elmat=elmat, bdr=flags, partitions=parts, elem_ptr=dp)
                h = capi.Hierarchy.from_operator(prob, op, capi.default_params(num_coarsenings=2))
                x, it, conv, hist = h.pcg(rhs, x=torch.zeros_like(rhs), rel_tol=1e-8) if device else h.pcg(rhs, rel_tol=1e-8)
                results.append((A, _host(flags), _host(x), it, conv, np.asarray(hist)))
            finally:
                if h is not None:
                    h.close()
                op.close()
    (Ad, fd, xd, itd, convd, histd), (Ag, fg, xg, itg, convg, histg) = results
    for a, g in zip(Ad, Ag):
        assert np.array_equal(a, g)                                        # the operator, bit for bit
    assert fd.any() and np.array_equal(fd, fg)
    assert convd and convg and itd == itg
    assert np.array_equal(histd, histg) and np.array_equal(xd, xg)


def test_chain_from_a_tetrahedral_mesh():
    X = ec.mesh("tets_3x2x2", True)[0]
    e2v = np.ascontiguousarray(ec.mesh("tets_3x2x2", True)[1], np.int32)
    want = rm.MeshRefine(X.shape[0], 3, X, e2v)
    with capi.MeshRefine(_cuda(X), _cuda(e2v)) as R:
        _, flags, op = _operator(3, R.pointer("coords"), R.pointer("elem_to_vertex"), R.get(device=True)[1], True)
        try:
            Ad, fd = [_host(a) for a in op.get(device=True)], _host(flags)
        finally:
            op.close()
    _, flags, op = _operator(3, want.coords, want.elem_to_vertex, want.elem_ptr, False)
    try:
        Ag = [_host(a) for a in op.get()]
    finally:
        op.close()
    for a, g in zip(Ad, Ag):
        assert np.array_equal(a, g)
    assert fd.any() and np.array_equal(fd, flags)
