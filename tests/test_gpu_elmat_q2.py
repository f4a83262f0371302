"""The order-2 element matrices computed on the device (em2_kernel of csrc/elmat.hip) against their definition
(saamge_amd/elmat_model.py), bit for bit: the 9-node quadrilateral and the 27-node hexahedron, both kinds, every coefficient
form, boxes, straight-sided and curved elements, host and device inputs, one list of order-1 and order-2 hexes; the sizes-only
call, the refusals, the zero-copy chain element matrices -> operator -> hierarchy -> solve against the same chain on the
model's matrices and against the project's own Q2 generator, and a coefficient change without an upload."""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import capi
from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import elmat_cases as ec
import elmat_q2_cases as qc

pytestmark = pytest.mark.gpu


def _cuda(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


CASES = [(name, kind, ncoef) for name in qc.MESHES for (kind, ncoef) in qc.forms(name)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("jitter", qc.JITTERS)
@pytest.mark.parametrize("name,kind,ncoef", CASES, ids=["%s-k%d-c%d" % c for c in CASES])
def test_device_equals_model(name, kind, ncoef, jitter, device):
    X, e2n, ep = qc.mesh(name, jitter)
    want, coef = qc.model(name, jitter, kind, ncoef)
    dim = X.shape[1]
    NE = ec.num_elements(e2n, ep)
    if ncoef == 1:
        coef = coef[:, 0]
    args = [X, e2n, coef, ep]
    if device:
        args = [_cuda(a) for a in args]
    got, dptr, dofs = capi.element_matrices(args[0], args[1], kind, args[2], elem_ptr=args[3], device=device, dofs=True)
    if device:
        got, dptr, dofs = (t.cpu().numpy() for t in (got, dptr, dofs))
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got, want)
    mptr, mdofs = em.dof_lists(dim, e2n, kind, ep)
    assert np.array_equal(dptr, mptr) and np.array_equal(dofs.ravel(), mdofs)
    info = capi.element_matrices_info(args[0], args[1], kind, args[2], elem_ptr=args[3])
    assert info[:5] == em.type_counts(dim, e2n, ep) and info[5] == want.size and info[6] == -1
    assert info[7] == em.order2_count(dim, e2n, ep)
    if ep is None:
        assert info[:5] == [0] * 5 and info[7] == NE
    else:
        assert info[4] > 0 and info[7] > 0 and info[4] + info[7] == NE


def test_sizes_only_call_writes_nothing():
    """elmat_out = NULL: info[5] says how many doubles the matrices take; no output pointer is passed at all."""
    X, e2n, ep = qc.mesh("mixed_hex8_hex27")
    nd = np.diff(ep).astype(np.int64)
    info = capi.element_matrices_info(X, e2n, 1, np.ones((len(nd), 2)), elem_ptr=ep)
    assert info[5] == int(((3 * nd) ** 2).sum()) and info[:5] == [0, 0, 0, 0, int((nd == 8).sum())] and info[7] == int((nd == 27).sum())
    assert capi.element_matrices_info(X, e2n, 0, np.ones(len(nd)), elem_ptr=ep)[5] == int((nd ** 2).sum())
    X, e2n, _ = qc.mesh("quad9_9x8")
    assert capi.element_matrices_info(X, e2n, 1, np.ones((72, 2)))[5:] == [72 * 324, -1, 72]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals(device):
    X, e2n, _ = qc.mesh("hex27_5x4x3", "straight")
    X2, q2n, _ = qc.mesh("quad9_4x3")
    NE, NV = len(e2n), len(X)
    one = np.ones(NE)
    dev = _cuda if device else (lambda a: a)

    def refused(match, coords, lists, kind, coef, elem_ptr=None):
        with pytest.raises(RuntimeError, match=match) as err:
            capi.element_matrices(dev(coords), dev(lists), kind, dev(coef), elem_ptr=dev(elem_ptr), device=device)
        return err.value.info
    refused("out of range", X, np.where(e2n == 7, NV, e2n).astype(np.int32), 0, one)               # a node id equal to NV
    twice = e2n.copy()
    twice[23, 26] = twice[23, 4]
    refused("twice", X, twice, 0, one)                                                              # a node listed twice
    refused("nde = 9 nodes are no supported element type in 3D", X, np.ascontiguousarray(e2n[:, :9]), 0, one)
    refused("nde = 27 nodes are no supported element type in 2D", X2, np.arange(54, dtype=np.int32).reshape(2, 27), 0, np.ones(2))
    ep = np.array([0, 27, 36, 63], np.int32)                                                        # hex27, 9 nodes, hex27
    refused("element 1: 9 nodes are no supported element type in 3D", X, np.concatenate([e2n[0], e2n[1, :9], e2n[2]]), 0,
            np.ones(3), elem_ptr=ep)
    ep = np.array([0, 9, 36], np.int32)                                                             # quad9, 27 nodes
    refused("element 1: 27 nodes are no supported element type in 2D", X2, np.concatenate([q2n[0], np.arange(27, dtype=np.int32)]),
            0, np.ones(2), elem_ptr=ep)
    refused("ncoef", X, e2n, 0, np.ones((NE, 2)))
    bad = e2n.copy()
    bad[[17, 41], 0], bad[[17, 41], 2] = e2n[[17, 41], 2], e2n[[17, 41], 0]                         # two corners swapped, twice
    for kind, coef in ((0, one), (1, np.ones((NE, 2)))):
        info = refused("element 17: the Jacobian determinant is not positive", X, bad, kind, coef)
        assert info[6] == 17 and info[7] == NE and info[4] == 0
    with pytest.raises(RuntimeError, match="element 17") as err:                                    # the sizes-only call checks too
        capi.element_matrices_info(dev(X), dev(bad), 0, dev(one))
    assert err.value.info[6] == 17


# ---- the zero-copy chain ----
def _solve(h, b):
    return h.pcg(b, rel_tol=1e-8)


def _q2_hex_chain(jitter, coef):
    """(problem, node coordinates, node lists) of Q2 hex elasticity on 4 x 4 x 4 elements: 2 187 dofs, AEs of 2 x 2 x 2,
    clamped on x = 0"""
    pb = pr.elasticity3d_q2_problem(4, blk=(2, 2, 2))
    e2n = pr.q2_hex_nodes(4)
    X = qc._moved(pr.grid_coords(8), e2n, (4, 4, 4), jitter)
    return pb, X, e2n


def _same_hierarchy_and_solve(h, g, b):
    assert h.num_levels == g.num_levels == 2
    assert h.level_info(0) == g.level_info(0)
    for which in ("P", "Ac"):
        Ah, Ag = h.get_csr(0, which), g.get_csr(0, which)
        assert Ah.nnz > 0 and np.array_equal(Ah.indptr, Ag.indptr) and np.array_equal(Ah.indices, Ag.indices)
        assert np.array_equal(Ah.data, Ag.data)
    xh, ih, ch, hh = _solve(h, b)
    xg, ig, cg, hg = _solve(g, b)
    assert ch and cg and ih == ig
    assert np.array_equal(hh, hg) and np.array_equal(xh, xg)


def _chain(pb, X, e2n, kind, coef):
    """the chain on device pointers against the chain on the model's matrices from the host: bits in are bits out"""
    want = em.element_matrices(X, e2n, kind, coef)
    elmat, _, dofs = capi.element_matrices(_cuda(X), _cuda(e2n), kind, _cuda(coef), device=True, dofs=True)
    assert elmat.is_cuda and dofs.is_cuda and np.array_equal(elmat.cpu().numpy(), want)
    assert np.array_equal(dofs.cpu().numpy(), pb.elem_to_dof)
    dprob = pr.Problem(**dict(pb.__dict__, elmat=elmat, elem_to_dof=dofs))
    hprob = pr.Problem(**dict(pb.__dict__, elmat=np.ascontiguousarray(want)))
    op = capi.Operator(pb.ND, dofs, elmat, _cuda(pb.bdr))
    og = capi.Operator(pb.ND, pb.elem_to_dof, hprob.elmat, pb.bdr)
    h = g = None
    try:
        h = capi.Hierarchy.from_operator(dprob, op, capi.default_params(num_coarsenings=1))
        g = capi.Hierarchy.from_operator(hprob, og, capi.default_params(num_coarsenings=1))
        _same_hierarchy_and_solve(h, g, pb.b)
    finally:
        for x in (h, g):
            if x is not None:
                x.close()
        op.close()
        og.close()


def test_q2_hex_chain_on_device_pointers_equals_the_chain_on_the_model():
    pb, X, e2n = _q2_hex_chain("straight", None)
    _chain(pb, X, e2n, 1, ec.coefficients(len(e2n), 3, 1, 2))


def test_quad9_chain_on_device_pointers_equals_the_chain_on_the_model():
    """quad9 4 x 3 diffusion with the mltest agglomerates (MLTEST_PARTITION)"""
    pb = pr.mltest_problem(order=2)
    assert np.array_equal(pb.partitions[0], pr.MLTEST_PARTITION)
    X, e2n, _ = qc.mesh("quad9_4x3", "straight")
    assert np.array_equal(e2n, pb.elem_to_dof)
    _chain(pb, X, e2n, 0, ec.coefficients(12, 2, 0, 3))


def test_q2_hex_chain_against_the_q2_generator():
    """The unjittered grid with lambda = mu = 1: the device chain's operator and elasticity3d_q2_problem's differ by rounding
    only, so both solves converge in the same number of iterations and the device chain's solution solves the generator's
    system: true relative residual |b - A x| / |b| at most twice the PCG tolerance."""
    pb, X, e2n = _q2_hex_chain("box", None)
    elmat, _, dofs = capi.element_matrices(_cuda(X), _cuda(e2n), 1, _cuda(np.ones((len(e2n), 2))), device=True, dofs=True)
    dprob = pr.Problem(**dict(pb.__dict__, elmat=elmat, elem_to_dof=dofs))
    op = capi.Operator(pb.ND, dofs, elmat, _cuda(pb.bdr))
    h = g = None
    try:
        h = capi.Hierarchy.from_operator(dprob, op, capi.default_params(num_coarsenings=1))
        g = capi.Hierarchy.from_problem(pb, capi.default_params(num_coarsenings=1))
        xh, ih, ch, _ = _solve(h, pb.b)
        xg, ig, cg, _ = _solve(g, pb.b)
        res = np.linalg.norm(pb.b - pb.A @ xh) / np.linalg.norm(pb.b)
        print("iterations %d (device chain) %d (generator), true relative residual %.3e" % (ih, ig, res))
        assert ch and cg and ih == ig
        assert res <= 2e-8
    finally:
        for x in (h, g):
            if x is not None:
                x.close()
        op.close()


def test_coefficient_change_is_three_device_calls_without_an_upload():
    import torch
    name = "hex27_5x4x3"
    X, e2n, ep = qc.mesh(name, "curved")
    NE, NV = len(e2n), len(X)
    c1, c2 = ec.coefficients(NE, 3, 0, 6, seed=5), ec.coefficients(NE, 3, 0, 6, seed=6)
    dX, dv, dc = _cuda(X), _cuda(e2n), _cuda(c1)
    elmat = capi.element_matrices(dX, dv, 0, dc, device=True)
    op = capi.Operator(NV, dv, elmat, None)
    try:
        first = qc.model(name, "curved", 0, 6)[0]
        m1 = am.assemble(NV, ep, e2n, np.asarray(first).ravel(), None)
        assert np.array_equal(op.get()[2], m1[2])
        before, where = op.arrays(), elmat.data_ptr()
        dc.copy_(torch.as_tensor(c2))                      # the new physics: NE x 6 doubles, written where the old ones were
        torch.cuda.synchronize()
        capi.pool_counts(reset=True)
        again = capi.element_matrices(dX, dv, 0, dc, device=True, out=elmat.reshape(-1))
        op.update(elmat)
        assert capi.pool_counts()[0] == 0, "the second call went to the driver for memory"
        assert again.data_ptr() == where and op.arrays() == before
        want = em.element_matrices(X, e2n, 0, c2)
        assert not np.array_equal(want, first)
        assert np.array_equal(elmat.cpu().numpy().ravel(), want.ravel())
        m2 = am.assemble(NV, ep, e2n, want.ravel(), None)
        rowptr, col, val = op.get()
        assert np.array_equal(rowptr, m2[0]) and np.array_equal(col, m2[1]) and np.array_equal(val, m2[2])
    finally:
        op.close()
