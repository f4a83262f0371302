"""The element matrices computed on the device (csrc/elmat.hip) against their definition (saamge_amd/elmat_model.py), bit for
bit: every type and kind, every coefficient form, boxes and jittered meshes, host and device inputs; the sizes-only call, the
refusals, the zero-copy chain element matrices -> operator -> hierarchy -> solve, and a coefficient change without an upload."""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import capi
from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import elmat_cases as ec

pytestmark = pytest.mark.gpu


def _forms(name):
    """(kind, ncoef) of the mesh's dimension: every coefficient form of diffusion, and elasticity"""
    dim = 2 if name in ("quads_4x3", "tris_4x3") else 3
    return [(0, 1), (0, dim), (0, dim * (dim + 1) // 2), (1, 2)]


def _cuda(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


CASES = [(name, kind, ncoef) for name in sorted(ec.MESHES) for (kind, ncoef) in _forms(name)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("jittered", [False, True], ids=["box", "jitter"])
@pytest.mark.parametrize("name,kind,ncoef", CASES, ids=["%s-k%d-c%d" % c for c in CASES])
def test_device_equals_model(name, kind, ncoef, jittered, device):
    X, e2v, ep = ec.mesh(name, jittered)
    want, coef = ec.model(name, jittered, kind, ncoef)
    dim = X.shape[1]
    if ncoef == 1:
        coef = coef[:, 0]
    args = [X, e2v, coef, ep]
    if device:
        args = [_cuda(a) for a in args]
    got, dptr, dofs = capi.element_matrices(args[0], args[1], kind, args[2], elem_ptr=args[3], device=device, dofs=True)
    if device:
        got, dptr, dofs = (t.cpu().numpy() for t in (got, dptr, dofs))
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got, want)
    mptr, mdofs = em.dof_lists(dim, e2v, kind, ep)
    assert np.array_equal(dptr, mptr) and np.array_equal(dofs.ravel(), mdofs)
    if kind == 1:
        assert np.array_equal(dofs.ravel(), (dim * np.asarray(e2v, np.int64).ravel()[:, None] + np.arange(dim)).ravel())
    info = capi.element_matrices_info(args[0], args[1], kind, args[2], elem_ptr=args[3])
    assert info[:5] == em.type_counts(dim, e2v, ep) and info[5] == want.size and info[6] == -1 and info[7] == 0
    if name == "mixed_4":
        assert info[3] > 0 and info[4] > 0 and info[3] + info[4] == len(ep) - 1


def test_sizes_only_call_writes_nothing():
    """elmat_out = NULL: info[5] says how many doubles the matrices take; no output pointer is passed at all."""
    X, e2v, ep = ec.mesh("mixed_4")
    NE = len(ep) - 1
    info = capi.element_matrices_info(X, e2v, 1, np.ones((NE, 2)), elem_ptr=ep)
    nd = np.diff(ep).astype(np.int64)
    assert info[5] == int(((3 * nd) ** 2).sum()) and info[:5] == [0, 0, 0, int((nd == 6).sum()), int((nd == 8).sum())]
    assert capi.element_matrices_info(X, e2v, 0, np.ones(NE), elem_ptr=ep)[5] == int((nd ** 2).sum())


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals(device):
    X, e2v, _ = ec.mesh("hex_5x4x3", jittered=True)
    NE, NV = len(e2v), len(X)
    one = np.ones(NE)
    dev = _cuda if device else (lambda a: a)

    def refused(match, coords, lists, kind, coef, elem_ptr=None):
        with pytest.raises(RuntimeError, match=match) as err:
            capi.element_matrices(dev(coords), dev(lists), kind, dev(coef), elem_ptr=dev(elem_ptr), device=device)
        return err.value.info
    refused("out of range", X, np.where(e2v == 7, NV, e2v).astype(np.int32), 0, one)             # a vertex id equal to NV
    refused("nde = 5 nodes are no supported element type in 3D", X, np.ascontiguousarray(e2v[:, :5]), 0, one)
    ep = np.array([0, 8, 13, 21], np.int32)                                                       # hex, 5-node pyramid, hex
    refused("element 1: 5 nodes are no supported element type in 3D", X, np.concatenate([e2v[0], e2v[1, :5], e2v[2]]), 0,
            np.ones(3), elem_ptr=ep)
    refused("ncoef", X, e2v, 0, np.ones((NE, 2)))                                                 # 3D diffusion takes 1, 3 or 6
    refused("ncoef", X, e2v, 1, np.ones((NE, 3)))
    bad = e2v.copy()
    bad[[17, 41], 0], bad[[17, 41], 1] = e2v[[17, 41], 1], e2v[[17, 41], 0]                       # two vertices swapped, twice
    for kind, coef in ((0, one), (1, np.ones((NE, 2)))):
        info = refused("element 17: the Jacobian determinant is not positive", X, bad, kind, coef)
        assert info[6] == 17 and info[4] == NE
    with pytest.raises(RuntimeError, match="element 17") as err:                                  # the sizes-only call checks too
        capi.element_matrices_info(dev(X), dev(bad), 0, dev(one))
    assert err.value.info[6] == 17


# ---- the zero-copy chain ----
def _chain_problem():
    n = (8, 8, 8)
    pb = pr.poisson3d_problem(n, blk=(4, 4, 4), coef="skew", coarse_blk=[(2, 2, 2)])
    X = pr.jitter(pr.grid_coords(n), n, ec.JITTER, seed=7)
    return pb, X


def _solve(h, b):
    x, it, conv, hist = h.pcg(b, rel_tol=1e-8)
    return x, it, conv, hist


def test_chain_on_device_pointers_equals_the_chain_on_the_model():
    """Two coarsenings (8 agglomerates, then 1), so that levels 0 and 1 both have a level_info and get_csr(1, "A") is the first
    coarse operator; bits in are bits out, so every comparison is exact."""
    pb, X = _chain_problem()
    e2v = np.ascontiguousarray(pb.elem_to_dof, dtype=np.int32)
    want = em.element_matrices(X, e2v, 0, pb.coefs)
    elmat = capi.element_matrices(_cuda(X), _cuda(e2v), 0, _cuda(pb.coefs), device=True)
    assert elmat.is_cuda and np.array_equal(elmat.cpu().numpy(), want)
    dprob = pr.Problem(**dict(pb.__dict__, elmat=elmat, elem_to_dof=_cuda(e2v)))
    hprob = pr.Problem(**dict(pb.__dict__, elmat=np.ascontiguousarray(want)))
    op = capi.Operator(pb.ND, dprob.elem_to_dof, elmat, _cuda(pb.bdr))
    og = capi.Operator(pb.ND, e2v, hprob.elmat, pb.bdr)
    h = g = None
    try:
        h = capi.Hierarchy.from_operator(dprob, op, capi.default_params(num_coarsenings=2))
        g = capi.Hierarchy.from_operator(hprob, og, capi.default_params(num_coarsenings=2))
        assert h.num_levels == g.num_levels == 3
        for lev in range(2):
            assert h.level_info(lev) == g.level_info(lev)
        for lev, which in ((1, "A"), (1, "Ac")):
            Ah, Ag = h.get_csr(lev, which), g.get_csr(lev, which)
            assert Ah.nnz > 0 and np.array_equal(Ah.indptr, Ag.indptr) and np.array_equal(Ah.indices, Ag.indices)
            assert np.array_equal(Ah.data, Ag.data)
        xh, ih, ch, hh = _solve(h, pb.b)
        xg, ig, cg, hg = _solve(g, pb.b)
        assert ch and cg and ih == ig
        assert np.array_equal(hh, hg) and np.array_equal(xh, xg)
    finally:
        for x in (h, g):
            if x is not None:
                x.close()
        op.close()
        og.close()


@pytest.mark.parametrize("name", ["hex_5x4x3", "mixed_4"])
def test_coefficient_change_is_three_device_calls_without_an_upload(name):
    import torch
    X, e2v, ep = ec.mesh(name, jittered=True)
    NE, NV = ec.num_elements(e2v, ep), len(X)
    c1, c2 = ec.coefficients(NE, 3, 0, 6, seed=5), ec.coefficients(NE, 3, 0, 6, seed=6)
    dX, dv, dp, dc = _cuda(X), _cuda(e2v), _cuda(ep), _cuda(c1)
    elmat = capi.element_matrices(dX, dv, 0, dc, elem_ptr=dp, device=True)
    op = capi.Operator(NV, dv, elmat, None, elem_ptr=dp)
    try:
        m1 = am.assemble(NV, ep, e2v, np.asarray(ec.model(name, True, 0, 6)[0]).ravel(), None)
        assert np.array_equal(op.get()[2], m1[2])
        before, where = op.arrays(), elmat.data_ptr()
        dc.copy_(torch.as_tensor(c2))                      # the new physics: NE x 6 doubles, written where the old ones were
        torch.cuda.synchronize()
        capi.pool_counts(reset=True)
        again = capi.element_matrices(dX, dv, 0, dc, elem_ptr=dp, device=True, out=elmat.reshape(-1))
        op.update(elmat)
        assert capi.pool_counts()[0] == 0, "the second call went to the driver for memory"
        assert again.data_ptr() == where and op.arrays() == before
        want = em.element_matrices(X, e2v, 0, c2, elem_ptr=ep)
        assert not np.array_equal(want, ec.model(name, True, 0, 6)[0])
        assert np.array_equal(elmat.cpu().numpy().ravel(), want.ravel())
        m2 = am.assemble(NV, ep, e2v, want.ravel(), None)
        rowptr, col, val = op.get()
        assert np.array_equal(rowptr, m2[0]) and np.array_equal(col, m2[1]) and np.array_equal(val, m2[2])
    finally:
        op.close()
