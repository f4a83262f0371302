"""Mass matrices, load vectors and the right-hand side assembly on the device (mass_kernel, load_kernel of csrc/elmat.hip,
op_rhs_assemble_kernel of csrc/operator.hip) against their definition (saamge_amd/elmat_model.py element_mass / element_loads,
saamge_amd/assemble_model.py assemble_rhs), bit for bit: all seven types, vdim 1 and dim, the mass added to the device's
stiffness matrices, loads with and without a coefficient, every mesh and jitter of elmat_cases and elmat_q2_cases, host and
device inputs; the sizes-only call and the refusals; the zero-copy chain coordinates -> K + c M, loads -> operator ->
assemble_rhs -> eliminate_rhs -> hierarchy -> PCG against the same chain fed the model's arrays from the host; and a
manufactured solution of -Laplace u + 10 u = f on the box grids 8^3 and 16^3 against a direct solve of the model's system."""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import capi
from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import elmat_cases as ec
import elmat_q2_cases as qc

pytestmark = pytest.mark.gpu

CASES = [("q1", name, jit) for name in ec.MESHES for jit in (False, True)] + \
        [("q2", name, jit) for name in qc.MESHES for jit in qc.JITTERS]
IDS = ["%s-%s" % (c[1], c[2]) for c in CASES]


def _cuda(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()      # (a copy: the model's arrays are read-only)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _mesh(family, name, jitter):
    return ec.mesh(name, jitter) if family == "q1" else qc.mesh(name, jitter)


def _inputs(family, name, jitter):
    """(coords, lists, elem_ptr, mass coefficient, nodal sources (NV,) and (NV, dim))"""
    X, e2v, ep = _mesh(family, name, jitter)
    rng = np.random.default_rng(11)
    c = rng.uniform(0.5, 2.0, ec.num_elements(e2v, ep))
    f1 = rng.uniform(-1.0, 1.0, len(X))
    fd = rng.uniform(-1.0, 1.0, X.shape)
    return X, e2v, ep, c, f1, fd


_want = {}


def _model(family, name, jitter):
    """the model's arrays of a case, computed once and left unchanged"""
    key = (family, name, jitter)
    if key not in _want:
        X, e2v, ep, c, f1, fd = _inputs(family, name, jitter)
        dim = X.shape[1]
        stiff = ec.model if family == "q1" else qc.model
        w = {
            "mass1": em.element_mass(X, e2v, c, elem_ptr=ep),
            "massd": em.element_mass(X, e2v, c, vdim=dim, elem_ptr=ep),
            "k_plus_m": em.element_mass(X, e2v, c, elem_ptr=ep, add_to=stiff(name, jitter, 0, 1)[0]),
            "e_plus_m": em.element_mass(X, e2v, c, vdim=dim, elem_ptr=ep, add_to=stiff(name, jitter, 1, 2)[0]),
            "loads1": em.element_loads(X, e2v, f1, coef=c, elem_ptr=ep),
            "loadsd": em.element_loads(X, e2v, fd, vdim=dim, coef=c, elem_ptr=ep),
            "loads1_unit": em.element_loads(X, e2v, f1, elem_ptr=ep),
        }
        for v in w.values():
            v.setflags(write=False)
        _want[key] = w
    return _want[key]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("family,name,jitter", CASES, ids=IDS)
def test_device_equals_model(family, name, jitter, device):
    X, e2v, ep, c, f1, fd = _inputs(family, name, jitter)
    want = _model(family, name, jitter)
    dim = X.shape[1]
    stiff = ec.model if family == "q1" else qc.model
    dev = _cuda if device else (lambda a: a)
    dX, dv, dp, dc = dev(X), dev(e2v), dev(ep), dev(c)
    for tag, vdim in (("mass1", 1), ("massd", dim)):
        got = capi.element_mass(dX, dv, dc, vdim=vdim, elem_ptr=dp, device=device)
        assert _host(got).shape == want[tag].shape and np.array_equal(_host(got), want[tag]), tag
        info = capi.element_mass(dX, dv, dc, vdim=vdim, elem_ptr=dp, sizes_only=True)
        assert info[:5] == em.type_counts(dim, e2v, ep) and info[5] == want[tag].size and info[6] == -1
        assert info[7] == em.order2_count(dim, e2v, ep)
    # the mass added to the device's own stiffness matrices
    for tag, kind, vdim in (("k_plus_m", 0, 1), ("e_plus_m", 1, dim)):
        K, coef = stiff(name, jitter, kind, 2 if kind else 1)
        base = capi.element_matrices(dX, dv, kind, dev(coef[:, 0] if kind == 0 else coef), elem_ptr=dp, device=device)
        assert np.array_equal(_host(base), K)
        got = capi.element_mass(dX, dv, dc, vdim=vdim, elem_ptr=dp, add_to=base)
        assert got is base and np.array_equal(_host(got), want[tag]), tag
    for tag, vdim, src, coef in (("loads1", 1, f1, dc), ("loadsd", dim, fd, dc), ("loads1_unit", 1, f1, None)):
        got = capi.element_loads(dX, dv, dev(src), vdim=vdim, coef=coef, elem_ptr=dp, device=device)
        assert _host(got).shape == want[tag].shape and np.array_equal(_host(got), want[tag]), tag


def test_sizes_only_call_writes_nothing():
    X, e2n, ep = qc.mesh("mixed_hex8_hex27")
    nd = np.diff(ep).astype(np.int64)
    one = np.ones(len(nd))
    info = capi.element_mass(X, e2n, one, vdim=3, elem_ptr=ep, sizes_only=True)
    assert info[5] == int(((3 * nd) ** 2).sum()) and info[:5] == [0, 0, 0, 0, int((nd == 8).sum())] and info[7] == int((nd == 27).sum())
    assert capi.element_mass(X, e2n, one, elem_ptr=ep, sizes_only=True)[5] == int((nd ** 2).sum())
    X, e2n, _ = qc.mesh("quad9_9x8")
    assert capi.element_mass(_cuda(X), _cuda(e2n), _cuda(np.ones(72)), vdim=2, sizes_only=True)[5:] == [72 * 324, -1, 72]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals(device):
    X, e2v, _ = ec.mesh("hex_5x4x3")
    NE, NV = len(e2v), len(X)
    one = np.ones(NE)
    dev = _cuda if device else (lambda a: a)

    def refused(match, call):
        with pytest.raises(RuntimeError, match=match) as err:
            call()
        return err.value.info

    def both(match, coords, lists, elem_ptr=None, NEc=NE):
        """refused by the mass and by the loads"""
        c = np.ones(NEc)
        a = refused(match, lambda: capi.element_mass(dev(coords), dev(lists), dev(c), elem_ptr=dev(elem_ptr), device=device))
        b = refused(match, lambda: capi.element_loads(dev(coords), dev(lists), dev(np.ones(len(coords))), coef=dev(c),
                                                      elem_ptr=dev(elem_ptr), device=device))
        return a, b
    # the arguments alone
    refused("vdim must be 1 or dim", lambda: capi.element_mass(dev(X), dev(e2v), dev(one), vdim=2, device=device))
    refused("vdim must be 1 or dim", lambda: capi.element_loads(dev(X), dev(e2v), dev(np.ones((NV, 2))), vdim=2, device=device))
    refused("null argument: coef", lambda: capi.element_mass(dev(X), dev(e2v), None, device=device))
    refused("null argument: src", lambda: capi.element_loads(dev(X), dev(e2v), None, device=device))
    info = (capi.C.c_longlong * 8)()
    assert capi.load().saamge_amd_element_mass(NV, 3, capi._ptr(dev(X)), NE, 8, None, capi._ptr(dev(e2v)), 1, capi._ptr(dev(one)),
                                               None, 1, None, info) != 0
    assert b"accumulate" in capi.load().saamge_amd_last_error()
    # the mesh
    both("out of range", X, np.where(e2v == 7, NV, e2v).astype(np.int32))
    twice = e2v.copy()
    twice[23, 7] = twice[23, 4]
    both("twice", X, twice)
    both("nde = 5 nodes are no supported element type in 3D", X, np.ascontiguousarray(e2v[:, :5]))
    ep = np.array([0, 8, 13, 21], np.int32)
    both("element 1: 5 nodes are no supported element type in 3D", X, np.concatenate([e2v[0], e2v[1, :5], e2v[2]]), ep, 3)
    # a determinant that is not positive: the first such element in info[6]
    bad = e2v.copy()
    bad[[17, 41], 0], bad[[17, 41], 2] = e2v[[17, 41], 2], e2v[[17, 41], 0]
    for info in both("element 17: the Jacobian determinant is not positive", X, bad):
        assert info[6] == 17 and info[4] == NE
    with pytest.raises(RuntimeError, match="element 17") as err:                                    # the sizes-only call checks too
        capi.element_mass(dev(X), dev(bad), dev(one), sizes_only=True)
    assert err.value.info[6] == 17
    Xt, t2v, _ = ec.mesh("tets_3x2x2")                                                              # a simplex, all four points
    flipped = t2v.copy()
    flipped[[3, 50], 0], flipped[[3, 50], 1] = t2v[[3, 50], 1], t2v[[3, 50], 0]
    with pytest.raises(RuntimeError, match="element 3: the Jacobian determinant is not positive") as err:
        capi.element_mass(dev(Xt), dev(flipped), dev(np.ones(len(t2v))), device=device)
    assert err.value.info[6] == 3


# ---- the global right-hand side ----
RHS_MESHES = [("q1", "hex_5x4x3", True), ("q1", "mixed_4", True), ("q2", "hex27_3x2x2", "curved")]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("flags", [False, True], ids=["free", "essential"])
@pytest.mark.parametrize("family,name,jitter", RHS_MESHES, ids=[c[1] for c in RHS_MESHES])
def test_assemble_rhs_and_eliminate_equal_the_model(family, name, jitter, flags, device):
    X, e2v, ep, c, f1, _ = _inputs(family, name, jitter)
    NV = len(X)
    want = _model(family, name, jitter)
    elmat, elvec = np.asarray(want["k_plus_m"]).ravel(), np.asarray(want["loads1"]).ravel()
    rng = np.random.default_rng(2)
    bdr = np.where(rng.random(NV) < 0.3, am.ON_ESS_DOMAIN_BORDER, 0).astype(np.int8) if flags else None
    x_ess = rng.uniform(-1.0, 1.0, NV)
    b_model = am.assemble_rhs(NV, ep, e2v, elvec)
    dev = _cuda if device else (lambda a: a)
    op = capi.Operator(NV, dev(e2v), dev(elmat), dev(bdr), elem_ptr=dev(ep))
    try:
        b = op.assemble_rhs(dev(elvec), device=device)
        assert np.array_equal(_host(b), b_model)
        again = op.assemble_rhs(dev(elvec), b=dev(np.full(NV, 7.0)))                            # overwritten, not added to
        assert np.array_equal(_host(again), b_model)
        op.eliminate_rhs(dev(elmat), dev(x_ess), b)
        if flags:
            assert np.array_equal(_host(b), am.eliminate_rhs(NV, ep, e2v, elmat, bdr, x_ess, b_model))
        else:
            assert np.array_equal(_host(b), b_model)
    finally:
        op.close()


# ---- the whole chain on device pointers ----
REACTION = 10.0


def _device_chain(n, X, f, rel_tol):
    """-div grad u + REACTION u = f (nodal) with zero Dirichlet values on the n^3 hex grid with the vertices X, everything on
    device pointers: returns (x, iterations, converged, history) as host arrays and the device's element arrays."""
    import torch
    pb = pr.poisson3d_problem(n, blk=(4, 4, 4), with_elmat=False)
    e2v = pb.elem_to_dof
    NE, NV = len(e2v), len(X)
    dX, dv, dbdr = _cuda(X), _cuda(e2v), _cuda(pb.bdr)
    elmat = capi.element_matrices(dX, dv, 0, _cuda(np.ones(NE)), device=True)
    assert capi.element_mass(dX, dv, _cuda(np.full(NE, REACTION)), add_to=elmat) is elmat and elmat.is_cuda
    elvec = capi.element_loads(dX, dv, _cuda(f), device=True)
    op = capi.Operator(NV, dv, elmat, dbdr)
    h = None
    try:
        b = op.assemble_rhs(elvec, device=True)
        op.eliminate_rhs(elmat, torch.zeros(NV, dtype=torch.float64, device="cuda"), b)
        assert b.is_cuda and elvec.is_cuda
        dprob = pr.Problem(**dict(pb.__dict__, elmat=elmat, elem_to_dof=dv, bdr=dbdr))
        h = capi.Hierarchy.from_operator(dprob, op, capi.default_params(num_coarsenings=1))
        x, it, conv, hist = h.pcg(b, x=torch.zeros_like(b), rel_tol=rel_tol)
        return (x.cpu().numpy(), it, conv, hist), (elmat.cpu().numpy(), elvec.cpu().numpy(), b.cpu().numpy())
    finally:
        if h is not None:
            h.close()
        op.close()


def test_chain_on_device_pointers_equals_the_chain_on_the_model():
    n = 8
    X = pr.jitter(pr.grid_coords(n), (n, n, n), ec.JITTER, seed=7)
    f = np.random.default_rng(5).uniform(0.0, 1.0, len(X))
    pb = pr.poisson3d_problem(n, blk=(4, 4, 4), with_elmat=False)
    e2v, NE, NV = pb.elem_to_dof, len(pb.elem_to_dof), len(X)
    (xd, itd, convd, histd), (elmat_d, elvec_d, b_d) = _device_chain(n, X, f, 1e-8)
    # the model's arrays, fed from the host
    elmat = em.element_mass(X, e2v, np.full(NE, REACTION), add_to=em.element_matrices(X, e2v, 0, np.ones(NE)))
    elvec = em.element_loads(X, e2v, f)
    assert np.array_equal(elmat_d, elmat) and np.array_equal(elvec_d, elvec)
    b = am.eliminate_rhs(NV, None, e2v, elmat, pb.bdr, np.zeros(NV), am.assemble_rhs(NV, None, e2v, elvec))
    assert np.array_equal(b_d, b)
    hprob = pr.Problem(**dict(pb.__dict__, elmat=np.ascontiguousarray(elmat)))
    og = capi.Operator(NV, e2v, hprob.elmat, pb.bdr)
    g = None
    try:
        g = capi.Hierarchy.from_operator(hprob, og, capi.default_params(num_coarsenings=1))
        xg, itg, convg, histg = g.pcg(b, rel_tol=1e-8)
    finally:
        if g is not None:
            g.close()
        og.close()
    assert convd and convg and itd == itg
    assert np.array_equal(histd, histg) and np.array_equal(xd, xg)


_reference = {}


def _manufactured(n):
    """(X, f, u at the nodes, the model's global mass matrix, the relative M-norm error of a direct solve of the model's
    system) on the box grid n^3, computed once"""
    if n not in _reference:
        import scipy.sparse as sp
        from scipy.sparse.linalg import spsolve
        X = pr.grid_coords(n)
        pb = pr.poisson3d_problem(n, blk=(4, 4, 4), with_elmat=False)
        e2v, NE, NV = pb.elem_to_dof, len(pb.elem_to_dof), len(X)
        u = np.sin(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) * np.sin(np.pi * X[:, 2])
        f = (3.0 * np.pi ** 2 + REACTION) * u
        one = np.ones(NE)
        mass = em.element_mass(X, e2v, one)
        elmat = em.element_mass(X, e2v, np.full(NE, REACTION), add_to=em.element_matrices(X, e2v, 0, one))
        b = am.eliminate_rhs(NV, None, e2v, elmat, pb.bdr, np.zeros(NV), am.assemble_rhs(NV, None, e2v, em.element_loads(X, e2v, f)))
        rp, col, val = am.assemble(NV, None, e2v, elmat, pb.bdr)
        A = sp.csr_matrix((val, col, rp), shape=(NV, NV))
        rp, col, val = am.assemble(NV, None, e2v, mass)
        M = sp.csr_matrix((val, col, rp), shape=(NV, NV))
        _reference[n] = (X, f, u, M, _m_error(spsolve(A.tocsc(), b), u, M))
    return _reference[n]


def _m_error(x, u, M):
    e = x - u
    return float(np.sqrt(e @ (M @ e)) / np.sqrt(u @ (M @ u)))


def test_manufactured_solution_converges_at_second_order():
    """-Laplace u + 10 u = f, u = sin(pi x) sin(pi y) sin(pi z), f = (3 pi^2 + 10) u given at the nodes, zero Dirichlet
    values, PCG to 1e-10 through the device chain.  Each relative M-norm error is within 1e-3 (relative) of the error of a
    direct solve of the model's system (the algebraic error is orders below the discretisation error, so this bounds
    wiring mistakes), and the error falls by at least 3.5 from 8^3 to 16^3 (direct solves: 9.56e-3 and 2.40e-3, ratio 3.87)."""
    err = {}
    for n in (8, 16):
        X, f, u, M, ref = _manufactured(n)
        (x, it, conv, _), _ = _device_chain(n, X, f, 1e-10)
        err[n] = _m_error(x, u, M)
        print("n = %d: %d iterations, relative M-norm error %.6e (direct solve of the model's system: %.6e)" % (n, it, err[n], ref))
        assert conv
        assert abs(err[n] - ref) <= 1e-3 * ref
    print("ratio %.3f" % (err[8] / err[16]))
    assert err[8] / err[16] >= 3.5
