"""The element matrices with coefficients at the points on the device (emkq_kernel, mass_kq_kernel of csrc/elmat.hip) against
their definition (saamge_amd/elmat_model.py element_matrices_points / element_mass_points), bit for bit: every type undeformed
and moved, a jittered hex_5x4x3, tets_3x2x2, hex_9x8x7 (504 elements: a second, partly filled workgroup), the mixed lists, one
element and none; a coefficient that differs at every point, kinds 0 (all three ncoef) and 1, the mass with vdim 1 and dim and
accumulated onto the stiffness output; host and device pointers, the sizes-only call, the dof lists, info, a repeated call, the
memory pool; the refusals in their order; and the chain eval -> k(u_q), sigma(u_q) -> matrices -> mass (accumulate) -> operator
-> hierarchy -> PCG on device pointers against the same chain on the model."""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import capi
from saamge_amd import elmat_model as em
from saamge_amd import mesh_refine_model as rm
from saamge_amd import problems as pr

import elmat_cases as ec
import elmat_kq_cases as kq
import elmat_points_cases as cs

pytestmark = pytest.mark.gpu

CASES = [(kind, moved) for kind in sorted(cs.TYPES) for moved in (False, True)] + \
        [("hex_5x4x3", True), ("tets_3x2x2", True), ("hex_9x8x7", True), ("mixed:3d", True), ("mixed:2d", True)]
IDS = ["%s-%s" % (c[0], "moved" if c[1] else "box") for c in CASES]


def _cuda(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()      # (a copy: the model's arrays are read-only)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _same(got, want, what):
    got = _host(got)
    assert got.shape == want.shape and got.dtype == np.float64 and np.array_equal(got, want), what


def _info(X, e2v, ep, doubles):
    dim = X.shape[1]
    return em.type_counts(dim, e2v, ep) + [doubles, -1, em.order2_count(dim, e2v, ep)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,moved", CASES, ids=IDS)
def test_device_equals_model(name, moved, device):
    X, e2v, ep = kq.mesh(name, moved)
    w = kq.model(name, moved)
    dim = X.shape[1]
    sym = dim * (dim + 1) // 2
    dev = _cuda if device else (lambda a: a)
    dX, dv, dp, ds = dev(X), dev(e2v), dev(ep), dev(w["sigma"])
    live = capi.memory_stats()[0]
    for kind, ncoef in kq.forms(dim):
        c, want = w[(kind, ncoef)]
        dc = dev(c)
        got, dptr, dofs = capi.element_matrices_points(dX, dv, kind, dc, elem_ptr=dp, device=device, dofs=True)
        _same(got, want, (kind, ncoef))
        mptr, mdofs = em.dof_lists(dim, e2v, kind, ep)
        assert np.array_equal(_host(dptr), mptr) and np.array_equal(_host(dofs).ravel(), mdofs)
        assert capi.element_matrices_points_info(dX, dv, kind, dc, elem_ptr=dp) == _info(X, e2v, ep, want.size)      # elmat_out NULL
        again = capi.element_matrices_points(dX, dv, kind, dc, elem_ptr=dp, device=device)      # a repeated call: the same bits
        assert np.array_equal(_host(again), _host(got))
        if (kind, ncoef) in ((0, sym), (1, 2)):                     # K + sigma M: the mass accumulated onto the stiffness output
            vdim = dim if kind else 1
            total = capi.element_mass_points(dX, dv, ds, vdim=vdim, elem_ptr=dp, add_to=got)
            _same(total, w[("sum", kind)], ("sum", kind))
        del got, dptr, dofs, again, dc
    for vdim in (1, dim):
        want = w[("mass", vdim)]
        _same(capi.element_mass_points(dX, dv, ds, vdim=vdim, elem_ptr=dp, device=device), want, ("mass", vdim))
        assert capi.element_mass_points(dX, dv, ds, vdim=vdim, elem_ptr=dp, sizes_only=True) == _info(X, e2v, ep, want.size)
    total = None
    del dX, dv, dp, ds, total
    assert capi.memory_stats()[0] == live                           # every temporary is back in the pool


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_one_element_and_none(device):
    X, e2v, _ = cs.mesh("hex8", True)
    dev = _cuda if device else (lambda a: a)
    one = np.ascontiguousarray(e2v[5:6])
    c6, c2, s = kq.coefq(8, 3, 0, 6), kq.coefq(8, 3, 1, 2), kq.coefq(8, 3, 0, 1)
    _same(capi.element_matrices_points(dev(X), dev(one), 0, dev(c6), device=device), em.element_matrices_points(X, one, 0, c6), "one")
    got = capi.element_matrices_points(dev(X), dev(one), 1, dev(c2), device=device)
    _same(got, em.element_matrices_points(X, one, 1, c2), "one, elasticity")
    _same(capi.element_mass_points(dev(X), dev(one), dev(s), vdim=3, add_to=got),
          em.element_mass_points(X, one, s, vdim=3, add_to=em.element_matrices_points(X, one, 1, c2)), "one, sum")
    none = np.zeros((0, 8), np.int32)
    empty = np.zeros(1)
    assert _host(capi.element_matrices_points(dev(X), dev(none), 0, dev(empty), device=device)).size == 0
    assert capi.element_matrices_points_info(dev(X), dev(none), 0, dev(empty)) == [0, 0, 0, 0, 0, 0, -1, 0]
    assert _host(capi.element_mass_points(dev(X), dev(none), dev(empty), device=device)).size == 0
    assert capi.element_mass_points(dev(X), dev(none), dev(empty), sizes_only=True) == [0, 0, 0, 0, 0, 0, -1, 0]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals_in_their_order(device):
    """What needs no device (kind, ncoef, vdim, a NULL coefq) before the mesh, the mesh before the determinants; the first element
    with a non-positive determinant in info[6]."""
    X, e2v, _ = ec.mesh("hex_5x4x3", jittered=True)
    NE, NV, NQ = len(e2v), len(X), 8 * len(e2v)
    dev = _cuda if device else (lambda a: a)
    one = np.ones(NQ)
    out_of_range = np.where(e2v == 7, NV, e2v).astype(np.int32)
    flipped = e2v.copy()
    flipped[[17, 41], 0], flipped[[17, 41], 1] = e2v[[17, 41], 1], e2v[[17, 41], 0]               # two vertices swapped, twice
    live = capi.memory_stats()[0]

    def refused(match, call):
        with pytest.raises(RuntimeError, match=match) as err:
            call()
        return err.value.info
    stiff = lambda lists, kind, c, **kw: (lambda: capi.element_matrices_points(dev(X), dev(lists), kind, dev(c), device=device, **kw))
    mass = lambda lists, c, **kw: (lambda: capi.element_mass_points(dev(X), dev(lists), dev(c), device=device, **kw))
    refused("kind must be 0", stiff(out_of_range, 2, one))                                        # the arguments before the mesh
    refused("ncoef must be 1, dim or", stiff(out_of_range, 0, np.ones((NQ, 2))))
    refused("ncoef must be 2", stiff(out_of_range, 1, np.ones((NQ, 3))))
    refused("out of range", stiff(out_of_range, 0, one))
    refused("nde = 5 nodes are no supported element type in 3D", stiff(np.ascontiguousarray(e2v[:, :5]), 0, one))
    ep = np.array([0, 8, 13, 21], np.int32)                                                       # hex, 5-node pyramid, hex
    refused("element 1: 5 nodes are no supported element type in 3D",
            stiff(np.concatenate([e2v[0], e2v[1, :5], e2v[2]]), 0, np.ones(24), elem_ptr=dev(ep)))
    for kind, c in ((0, one), (0, np.ones((NQ, 6))), (1, np.ones((NQ, 2)))):                      # the mesh before the determinants
        info = refused("element 17: the Jacobian determinant is not positive", stiff(flipped, kind, c))
        assert info[6] == 17 and info[4] == NE
    with pytest.raises(RuntimeError, match="element 17") as err:                                  # the sizes-only call checks too
        capi.element_matrices_points_info(dev(X), dev(flipped), 0, dev(one))
    assert err.value.info[6] == 17
    refused("vdim must be 1 or dim", mass(out_of_range, one, vdim=2))
    refused("null argument: coefq", mass(out_of_range, None))
    refused("out of range", mass(out_of_range, one))
    for vdim in (1, 3):
        info = refused("element 17: the Jacobian determinant is not positive", mass(flipped, one, vdim=vdim))
        assert info[6] == 17 and info[4] == NE
    if device:
        import torch
        torch.cuda.synchronize()
    assert capi.memory_stats()[0] == live


def test_chain_on_device_pointers_equals_the_chain_on_the_model():
    """jittered hex_5x4x3 -> one level of refinement -> a nodal u -> element_eval -> k_q = 1 + u_q^2 and sigma_q = 1 + |u_q| with
    torch on the device -> element_matrices_points -> element_mass_points (accumulate) -> operator: the element matrices and the
    operator equal, bit for bit, those of the model fed the device's k_q and sigma_q copied back (so that how torch rounds does
    not enter); then hierarchy -> PCG on the device pointers and on the model's matrices from the host: the same iterations,
    history and solution."""
    import torch
    X0, e2v0, _ = ec.mesh("hex_5x4x3", True)
    e2v0 = np.ascontiguousarray(e2v0, np.int32)
    want = rm.MeshRefine(X0.shape[0], 3, X0, e2v0, levels=1)
    NE, NV = want.NE, want.NV
    u = np.sin(2.0 * want.coords[:, 0]) * np.cos(3.0 * want.coords[:, 1]) + want.coords[:, 2]
    rhs = np.random.default_rng(8).uniform(-1.0, 1.0, NV)

    def solve(dv, dp, elmat, device):
        dev = _cuda if device else (lambda a: a)
        with capi.FaceTable(NV, 3, dv, elem_ptr=dp) as T:
            be, bl = T.get(device=device)[3:5]
            flags = torch.zeros(NV, dtype=torch.int8, device="cuda") if device else np.zeros(NV, np.int8)
            capi.face_dofs(NV, 3, dv, be, bl, flags, flag=0x02, elem_ptr=dp)
        op = capi.Operator(NV, dv, elmat, flags, elem_ptr=dp)
        h = None
        try:
            A = tuple(_host(a).copy() for a in op.get(device=device))
            b = dev(rhs)
            op.eliminate_rhs(elmat, torch.zeros(NV, dtype=torch.float64, device="cuda") if device else np.zeros(NV), b)
            parts = [torch.arange(NE, dtype=torch.int32, device="cuda") >> 3] if device else [(np.arange(NE) >> 3).astype(np.int32)]
            prob = pr.Problem(elem_to_dof=dv, elmat=elmat, bdr=flags, partitions=parts, elem_ptr=dp)
            h = capi.Hierarchy.from_operator(prob, op, capi.default_params(num_coarsenings=1))
            x, it, conv, hist = h.pcg(b, x=torch.zeros_like(b), rel_tol=1e-8) if device else h.pcg(b, rel_tol=1e-8)
            return A, _host(flags).copy(), _host(x), it, conv, np.asarray(hist)
        finally:
            if h is not None:
                h.close()
            op.close()
    with capi.MeshRefine(_cuda(X0), _cuda(e2v0), levels=1) as R:
        dX, dp, dv = R.pointer("coords"), R.get(device=True)[1], R.pointer("elem_to_vertex")
        uq = capi.element_eval(dX, dv, _cuda(u), elem_ptr=dp, device=True, want=("uq",))[0]
        assert uq.is_cuda and np.array_equal(_host(uq), em.element_eval(want.coords, want.elem_to_vertex, u, elem_ptr=want.elem_ptr)[0])
        kq_d = 1.0 + uq[:, 0] * uq[:, 0]
        sq_d = 1.0 + torch.abs(uq[:, 0])
        elmat = capi.element_matrices_points(dX, dv, 0, kq_d, elem_ptr=dp, device=True)
        assert elmat.is_cuda
        capi.element_mass_points(dX, dv, sq_d, elem_ptr=dp, add_to=elmat)
        elmat_d = _host(elmat).copy()
        Ad, flags_d, xd, itd, convd, histd = solve(dv, dp, elmat, True)
    # the model, fed the device's coefficients
    k_h, s_h = _host(kq_d), _host(sq_d)
    assert (k_h >= 1.0).all() and (s_h >= 1.0).all() and len(np.unique(k_h)) > len(k_h) // 2      # it varies inside the elements
    K = em.element_matrices_points(want.coords, want.elem_to_vertex, 0, k_h, elem_ptr=want.elem_ptr)
    KM = em.element_mass_points(want.coords, want.elem_to_vertex, s_h, elem_ptr=want.elem_ptr, add_to=K)
    assert np.array_equal(elmat_d, KM)
    rowptr, col, val = am.assemble(NV, want.elem_ptr, want.elem_to_vertex, KM, flags_d)
    assert np.array_equal(Ad[0], rowptr) and np.array_equal(Ad[1], col) and np.array_equal(Ad[2], val)
    Ag, flags_g, xg, itg, convg, histg = solve(want.elem_to_vertex, want.elem_ptr, KM, False)
    assert all(np.array_equal(a, b) for a, b in zip(Ad, Ag)) and np.array_equal(flags_d, flags_g)
    assert convd and convg and itd == itg
    assert np.array_equal(histd, histg) and np.array_equal(xd, xg)
    print("PCG iterations %d" % itd)
