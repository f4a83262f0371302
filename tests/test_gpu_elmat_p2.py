"""The order-2 simplices on the device (csrc/elmat.hip: em2_kernel<2, 6, .> / <3, 10, .>, mass_kernel, load_kernel, the 6-node
triangular face of bdr_mass_kernel / bdr_load_kernel) against their definition (saamge_amd/elmat_model.py), bit for bit: stiffness
(the three coefficient forms of diffusion, elasticity), mass (vdim 1 and dim, written and accumulated onto the device's own
stiffness), loads (with and without coef), boundary mass and loads (the four face lists of elmat_p2_cases), on every mesh and
jitter of elmat_p2_cases with host and device pointers; the sizes-only calls, info on the mixed lists, the refusals; the chain
operator_assemble -> assemble_rhs -> eliminate_rhs -> ml_produce_data_mixed -> pcg on device pointers against the same chain fed
the model's arrays, twice; and a manufactured solution on tri6 and tet10 against a direct solve of the model's system.

Every case here fails on a library without the two types: 6 nodes in 2D and 10 in 3D are refused there."""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import capi
from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import elmat_cases as ec
import elmat_p2_cases as pc

pytestmark = pytest.mark.gpu


def _cuda(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()      # (a copy: the model's arrays are read-only)


def _numpy(a):
    return None if a is None else np.array(a)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _copy(a):
    return a.clone() if hasattr(a, "data_ptr") else np.array(a)


def _node_counts(e2n, ep):
    return np.diff(ep).astype(np.int64) if ep is not None else np.full(e2n.shape[0], e2n.shape[1], np.int64)


# ---- stiffness ----
CASES = [(name, kind, ncoef) for name in pc.MESHES for (kind, ncoef) in pc.forms(name)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("jitter", pc.JITTERS)
@pytest.mark.parametrize("name,kind,ncoef", CASES, ids=["%s-k%d-c%d" % c for c in CASES])
def test_stiffness_equals_model(name, kind, ncoef, jitter, device):
    X, e2n, ep = pc.mesh(name, jitter)
    want, coef = pc.model(name, jitter, kind, ncoef)
    dim = X.shape[1]
    if ncoef == 1:
        coef = coef[:, 0]
    dev = _cuda if device else _numpy
    args = [dev(a) for a in (X, e2n, coef, ep)]
    got, dptr, dofs = capi.element_matrices(args[0], args[1], kind, args[2], elem_ptr=args[3], device=device, dofs=True)
    got, dptr, dofs = _host(got), _host(dptr), _host(dofs)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got, want)
    mptr, mdofs = em.dof_lists(dim, e2n, kind, ep)
    assert np.array_equal(dptr, mptr) and np.array_equal(dofs.ravel(), mdofs)
    info = capi.element_matrices_info(args[0], args[1], kind, args[2], elem_ptr=args[3])
    assert info[:5] == em.type_counts(dim, e2n, ep) and info[5] == want.size and info[6] == -1
    assert info[7] == em.order2_count(dim, e2n, ep) and info[7] > 0
    if ep is None:
        assert info[:5] == [0] * 5 and info[7] == len(e2n)


# ---- mass and loads ----
_zeroth = {}


def _zeroth_model(name, jitter):
    """the model's mass matrices and load vectors of a case, computed once and left unchanged"""
    key = (name, jitter)
    if key not in _zeroth:
        X, e2n, ep = pc.mesh(name, jitter)
        dim, NE = X.shape[1], ec.num_elements(e2n, ep)
        c = ec.coefficients(NE, dim, 0, 1, seed=9)[:, 0]
        f1, fd = pc.nodal_data(len(X), dim)
        w = {
            "c": c, "f1": f1, "fd": fd,
            "mass1": em.element_mass(X, e2n, c, elem_ptr=ep),
            "massd": em.element_mass(X, e2n, c, vdim=dim, elem_ptr=ep),
            "k_plus_m": em.element_mass(X, e2n, c, elem_ptr=ep, add_to=pc.model(name, jitter, 0, 1)[0]),
            "e_plus_m": em.element_mass(X, e2n, c, vdim=dim, elem_ptr=ep, add_to=pc.model(name, jitter, 1, 2)[0]),
            "loads1": em.element_loads(X, e2n, f1, coef=c, elem_ptr=ep),
            "loadsd": em.element_loads(X, e2n, fd, vdim=dim, coef=c, elem_ptr=ep),
            "loads1_unit": em.element_loads(X, e2n, f1, elem_ptr=ep),
        }
        for v in w.values():
            v.setflags(write=False)
        _zeroth[key] = w
    return _zeroth[key]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("jitter", pc.JITTERS)
@pytest.mark.parametrize("name", pc.MESHES)
def test_mass_and_loads_equal_model(name, jitter, device):
    X, e2n, ep = pc.mesh(name, jitter)
    dim = X.shape[1]
    want = _zeroth_model(name, jitter)
    dev = _cuda if device else _numpy
    dX, dv, dp, dc = dev(X), dev(e2n), dev(ep), dev(want["c"])
    for tag, vdim in (("mass1", 1), ("massd", dim)):
        got = capi.element_mass(dX, dv, dc, vdim=vdim, elem_ptr=dp, device=device)
        assert hasattr(got, "data_ptr") == device and _host(got).tobytes() == want[tag].tobytes(), tag      # (+0.0 included)
    for tag, kind, vdim in (("k_plus_m", 0, 1), ("e_plus_m", 1, dim)):
        K, coef = pc.model(name, jitter, kind, 2 if kind else 1)
        own = capi.element_matrices(dX, dv, kind, dev(coef[:, 0] if kind == 0 else coef), elem_ptr=dp, device=device)
        got = capi.element_mass(dX, dv, dc, vdim=vdim, elem_ptr=dp, add_to=own)
        assert got is own and np.array_equal(_host(got).ravel(), want[tag].ravel()), tag
    for tag, vdim, src, coef in (("loads1", 1, "f1", dc), ("loadsd", dim, "fd", dc), ("loads1_unit", 1, "f1", None)):
        got = capi.element_loads(dX, dv, dev(want[src]), vdim=vdim, coef=coef, elem_ptr=dp, device=device)
        assert np.array_equal(_host(got), want[tag]), tag
    info = capi.element_mass(dX, dv, dc, vdim=dim, elem_ptr=dp, sizes_only=True)
    assert info[:5] == em.type_counts(dim, e2n, ep) and info[5] == want["massd"].size and info[6] == -1
    assert info[7] == em.order2_count(dim, e2n, ep)


# ---- boundary forms ----
_bdr = {}


def _bdr_model(name, jitter, variant):
    key = (name, jitter, variant)
    if key not in _bdr:
        X, e2n, ep = pc.mesh(name, jitter)
        dim, NE = X.shape[1], ec.num_elements(e2n, ep)
        fe, fl = pc.faces(name, variant)
        c = pc.face_coefficients(NE, fe, fl)
        g1, gd = pc.nodal_data(len(X), dim, seed=18)
        z = _zeroth_model(name, jitter)
        w = {
            "k_plus_r": em.boundary_mass(X, e2n, fe, fl, c, elem_ptr=ep, add_to=pc.model(name, jitter, 0, 1)[0]),
            "e_plus_r": em.boundary_mass(X, e2n, fe, fl, c, vdim=dim, elem_ptr=ep, add_to=pc.model(name, jitter, 1, 2)[0]),
            "loads1": em.boundary_loads(X, e2n, fe, fl, g1, coef=c, elem_ptr=ep, add_to=z["loads1"]),
            "loadsd": em.boundary_loads(X, e2n, fe, fl, gd, vdim=dim, coef=c, elem_ptr=ep, add_to=z["loadsd"]),
            "loads1_unit": em.boundary_loads(X, e2n, fe, fl, g1, elem_ptr=ep, add_to=z["loads1"]),
        }
        for v in w.values():
            v.setflags(write=False)
        _bdr[key] = w
    return _bdr[key]


def _bdr_info(dim, e2n, ep, fe, fl, vdim, mass):
    nd = _node_counts(e2n, ep)
    want = [0] * 8
    for e, l in zip(fe, fl):
        fn = len(em.FACE_NODES[(dim, int(nd[e]))][l])
        want[em.face_info_index(dim, fn)] += 1
        want[5] += fn * fn * vdim if mass else fn * vdim
    want[6], want[7] = -1, len(set(fe.tolist()))
    return want


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("jitter", pc.JITTERS)
@pytest.mark.parametrize("name", pc.MESHES)
def test_boundary_forms_equal_model(name, jitter, device):
    X, e2n, ep = pc.mesh(name, jitter)
    dim, NE = X.shape[1], ec.num_elements(e2n, ep)
    dev = _cuda if device else _numpy
    dX, dv, dp = dev(X), dev(e2n), dev(ep)
    g1, gd = pc.nodal_data(len(X), dim, seed=18)
    z = _zeroth_model(name, jitter)
    own = {kind: dev(pc.model(name, jitter, kind, 2 if kind else 1)[0]) for kind in (0, 1)}
    for variant in pc.VARIANTS:
        fe, fl = pc.faces(name, variant)
        c = pc.face_coefficients(NE, fe, fl)
        want = _bdr_model(name, jitter, variant)
        dfe, dfl, dc = dev(fe), dev(fl), dev(c)
        for tag, kind, vdim in (("k_plus_r", 0, 1), ("e_plus_r", 1, dim)):
            base = _copy(own[kind])
            got = capi.boundary_mass(dX, dv, dfe, dfl, dc, vdim=vdim, elem_ptr=dp, add_to=base)
            assert got is base and np.array_equal(_host(got), want[tag]), (variant, tag)
        for tag, vdim, g, coef, b in (("loads1", 1, g1, dc, z["loads1"]), ("loadsd", dim, gd, dc, z["loadsd"]),
                                      ("loads1_unit", 1, g1, None, z["loads1"])):
            base = dev(b)
            got = capi.boundary_loads(dX, dv, dfe, dfl, dev(g), vdim=vdim, coef=coef, elem_ptr=dp, add_to=base)
            assert got is base and np.array_equal(_host(got).ravel(), want[tag].ravel()), (variant, tag)
    assert np.array_equal(_bdr_model(name, jitter, "all")["k_plus_r"], _bdr_model(name, jitter, "shuffled")["k_plus_r"])
    fe, fl = pc.faces(name, "interior")
    for vdim in (1, dim):
        info = capi.boundary_mass(dX, dv, dev(fe), dev(fl), dev(np.ones(len(fe))), vdim=vdim, elem_ptr=dp, sizes_only=True)
        assert info == _bdr_info(dim, e2n, ep, fe, fl, vdim, True)
        info = capi.boundary_loads(dX, dv, dev(fe), dev(fl), dev(np.ones((len(X), vdim))), vdim=vdim, elem_ptr=dp, sizes_only=True)
        assert info == _bdr_info(dim, e2n, ep, fe, fl, vdim, False)


def test_untouched_entries_keep_their_bits():
    name = "tet10_5x4x3"
    X, e2n, _ = pc.mesh(name, "curved")
    NE = len(e2n)
    fe, fl = pc.faces(name, "all")
    rng = np.random.default_rng(29)
    K = rng.uniform(-1.0, 1.0, (NE, 30, 30))
    touched = np.zeros(K.shape, bool)
    for e, l in zip(fe, fl):
        dofs = (3 * np.array(em.FACE_NODES[(3, 10)][l])[:, None] + np.arange(3)[None, :])
        for i in range(3):
            touched[e][np.ix_(dofs[:, i], dofs[:, i])] = True
    K[~touched] = np.where(rng.random((~touched).sum()) < 0.5, -0.0, np.nan)
    c = pc.face_coefficients(NE, fe, fl)
    want = em.boundary_mass(X, e2n, fe, fl, c, vdim=3, add_to=K)
    got = capi.boundary_mass(_cuda(X), _cuda(e2n), _cuda(fe), _cuda(fl), _cuda(c), vdim=3, add_to=_cuda(K))
    assert _host(got).tobytes() == want.tobytes()
    assert _host(got)[~touched].tobytes() == K[~touched].tobytes()


# ---- sizes, info, refusals ----
def test_sizes_only_calls_and_info_on_the_mixed_lists():
    for name, order1, counts in (("mixed_tri3_tri6_quad9", 0, {3: 12, 6: 10, 9: 3}), ("mixed_tet4_tet10_hex27", 2, {4: 12, 10: 11, 27: 3})):
        X, lists, ep = pc.mesh(name)
        dim = X.shape[1]
        nd = np.diff(ep).astype(np.int64)
        assert {int(k): int((nd == k).sum()) for k in np.unique(nd)} == counts
        first = [0] * 5
        first[order1] = 12
        NE = len(nd)
        info = capi.element_matrices_info(X, lists, 1, np.ones((NE, 2)), elem_ptr=ep)
        assert info == first + [int(((dim * nd) ** 2).sum()), -1, NE - 12]
        assert capi.element_matrices_info(X, lists, 0, np.ones(NE), elem_ptr=ep)[5] == int((nd ** 2).sum())
        assert capi.element_mass(X, lists, np.ones(NE), elem_ptr=ep, sizes_only=True) == first + [int((nd ** 2).sum()), -1, NE - 12]
    X, e2n, _ = pc.mesh("tet10_70")
    assert capi.element_matrices_info(X, e2n, 1, np.ones((70, 2))) == [0] * 5 + [70 * 900, -1, 70]
    X, e2n, _ = pc.mesh("tri6_5x3")
    assert capi.element_matrices_info(X, e2n, 1, np.ones((30, 2))) == [0] * 5 + [30 * 144, -1, 30]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals(device):
    X, e2n, _ = pc.mesh("tet10_3x2x2")
    X2, t6, _ = pc.mesh("tri6_4x3")
    NE, NV = len(e2n), len(X)
    one = np.ones(NE)
    dev = _cuda if device else _numpy

    def refused(match, call):
        with pytest.raises(RuntimeError, match=match) as err:
            call()
        return err.value.info
    # a curved element whose determinant is not positive at a mass point only: the mass refuses it, the stiffness does not
    Y, moved = pc.mass_only_inversion()
    K = capi.element_matrices(dev(Y), dev(moved), 0, dev(one), device=device)
    assert np.array_equal(_host(K), em.element_matrices(Y, moved, 0, one))
    for call in (lambda: capi.element_mass(dev(Y), dev(moved), dev(one), device=device),
                 lambda: capi.element_mass(dev(Y), dev(moved), dev(one), sizes_only=True),
                 lambda: capi.element_loads(dev(Y), dev(moved), dev(np.ones(len(Y))), device=device)):
        info = refused("element 5: the Jacobian determinant is not positive", call)
        assert info[6] == 5 and info[7] == NE
    # mirrored elements: every form refuses them
    bad = e2n.copy()
    bad[[17, 41]] = e2n[[17, 41]][:, pc.INVERTED]
    for call in (lambda: capi.element_matrices(dev(X), dev(bad), 0, dev(one), device=device),
                 lambda: capi.element_matrices(dev(X), dev(bad), 1, dev(np.ones((NE, 2))), device=device),
                 lambda: capi.element_mass(dev(X), dev(bad), dev(one), vdim=3, device=device)):
        assert refused("element 17: the Jacobian determinant is not positive", call)[6] == 17
    # a repeated node, a node id out of range, node counts that are no type
    twice = e2n.copy()
    twice[23, 9] = twice[23, 4]
    refused("twice", lambda: capi.element_matrices(dev(X), dev(twice), 0, dev(one), device=device))
    refused("twice", lambda: capi.element_mass(dev(X), dev(twice), dev(one), device=device))
    refused("out of range", lambda: capi.element_loads(dev(X), dev(np.where(e2n == 7, NV, e2n).astype(np.int32)), dev(np.ones(NV))))
    refused("nde = 5 nodes are no supported element type in 3D",
            lambda: capi.element_matrices(dev(X), dev(np.ascontiguousarray(e2n[:, :5])), 0, dev(one), device=device))
    refused("nde = 10 nodes are no supported element type in 2D",
            lambda: capi.element_matrices(dev(X2), dev(np.arange(20, dtype=np.int32).reshape(2, 10)), 0, dev(np.ones(2)), device=device))
    ep = np.array([0, 10, 17, 27], np.int32)
    refused("element 1: 7 nodes are no supported element type in 3D",
            lambda: capi.element_mass(dev(X), dev(np.concatenate([e2n[0], e2n[1, :7], e2n[2]])), dev(np.ones(3)), elem_ptr=dev(ep)))
    # faces: local index 4 on a tet10, 3 on a tri6
    fe, fl = pc.faces("tet10_3x2x2", "all")
    wrong = fl.copy()
    wrong[7] = 4
    info = refused("face 7: face_local is outside the element type's range",
                   lambda: capi.boundary_mass(dev(X), dev(e2n), dev(fe), dev(wrong), dev(np.ones(len(fe))), add_to=dev(np.zeros((NE, 10, 10)))))
    assert info[6] == 7
    f2, l2 = pc.faces("tri6_4x3", "all")
    wrong = l2.copy()
    wrong[3] = 3
    info = refused("face 3: face_local is outside the element type's range",
                   lambda: capi.boundary_loads(dev(X2), dev(t6), dev(f2), dev(wrong), dev(np.ones(len(X2))), add_to=dev(np.zeros((len(t6), 6)))))
    assert info[6] == 3
    flat = np.array(X)
    nodes = e2n[fe[4], list(em.FACE_NODES[(3, 10)][fl[4]])]
    flat[nodes] = X[nodes[0]]
    info = refused("face 4: the measure is not positive",
                   lambda: capi.boundary_mass(dev(flat), dev(e2n), dev(fe), dev(fl), dev(np.ones(len(fe))), add_to=dev(np.zeros((NE, 10, 10)))))
    assert info[6] == 4


# ---- the chain on device pointers ----
REACTION = 10.0


def _simplex_grid(dim, n, blk, jitter="box"):
    """(X, e2n, X of the box, agglomerates): the P2 split of the n^dim grid, jittered or not; one agglomerate per block of
    blk^dim parent cells"""
    if dim == 3:
        V, cells = pr.grid_coords(n), pr.hex_to_tets(n)
        ez, ey, ex = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
        nb = n // blk
        part = np.repeat((((ez // blk) * nb + ey // blk) * nb + ex // blk).ravel(), 6)
    else:
        V, cells = pr.grid_coords((n, n)), pr.quads_to_tris(n, n)
        ex, ey = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
        part = np.repeat(((ey // blk) * (n // blk) + ex // blk).ravel(), 2)
    X0, e2n = pr.p2_simplex_nodes(V, cells)
    X = pc._moved(X0, e2n, (n,) * dim, jitter)
    return X, e2n, X0, np.ascontiguousarray(part.astype(np.int32))


def _solve(n_dofs, ep, dofs, elmat, elvec, bdr, part, rel_tol, device):
    """operator_assemble -> assemble_rhs -> eliminate_rhs -> ml_produce_data_mixed -> pcg, on device tensors or host arrays:
    (x, iterations, converged, history, b) as host arrays"""
    import torch
    dev = _cuda if device else (lambda a: a)
    dp, dbdr = dev(ep), dev(bdr)
    op = capi.Operator(n_dofs, dofs, elmat, dbdr, elem_ptr=dp)
    h = None
    try:
        b = op.assemble_rhs(elvec, device=device)
        op.eliminate_rhs(elmat, torch.zeros(n_dofs, dtype=torch.float64, device="cuda") if device else np.zeros(n_dofs), b)
        prob = pr.Problem(elem_to_dof=dofs, elmat=elmat, bdr=dbdr, partitions=[part], elem_ptr=dp)
        h = capi.Hierarchy.from_operator(prob, op, capi.default_params(num_coarsenings=1))
        x, it, conv, hist = h.pcg(b, x=torch.zeros_like(b), rel_tol=rel_tol) if device else h.pcg(b, rel_tol=rel_tol)
        return _host(x), it, conv, np.asarray(hist), _host(b)
    finally:
        if h is not None:
            h.close()
        op.close()


def _same(d, g):
    (xd, itd, convd, histd, bd), (xg, itg, convg, histg, bg) = d, g
    assert np.array_equal(bd, bg)
    assert convd and convg and itd == itg
    assert np.array_equal(histd, histg) and np.array_equal(xd, xg)


def test_reaction_diffusion_chain_on_device_pointers_equals_the_chain_on_the_model():
    """-Laplace u + 10 u = f without essential dofs on the jittered tet10 split of 4^3 (729 nodes, 384 elements)"""
    X, e2n, _, part = _simplex_grid(3, 4, 2, "straight")
    NE, NV = len(e2n), len(X)
    assert NV == 9 ** 3 and NE == 384
    f = np.random.default_rng(5).uniform(0.0, 1.0, NV)
    ep = (10 * np.arange(NE + 1)).astype(np.int32)
    bdr = np.zeros(NV, np.int8)
    dX, dv = _cuda(X), _cuda(e2n)
    elmat_d = capi.element_matrices(dX, dv, 0, _cuda(np.ones(NE)), device=True)
    assert capi.element_mass(dX, dv, _cuda(np.full(NE, REACTION)), add_to=elmat_d) is elmat_d and elmat_d.is_cuda
    elvec_d = capi.element_loads(dX, dv, _cuda(f), device=True)
    elmat = em.element_mass(X, e2n, np.full(NE, REACTION), add_to=em.element_matrices(X, e2n, 0, np.ones(NE)))
    elvec = em.element_loads(X, e2n, f)
    assert np.array_equal(_host(elmat_d), elmat) and np.array_equal(_host(elvec_d), elvec)
    d = _solve(NV, ep, dv.reshape(-1), elmat_d.reshape(-1), elvec_d.reshape(-1), bdr, part, 1e-8, True)
    g = _solve(NV, ep, np.ascontiguousarray(e2n.ravel()), np.ascontiguousarray(elmat.ravel()), np.ascontiguousarray(elvec.ravel()),
               bdr, part, 1e-8, False)
    assert np.array_equal(g[4], am.assemble_rhs(NV, ep, e2n.ravel(), elvec.ravel()))
    _same(d, g)


def test_elasticity_chain_with_a_traction_on_device_pointers_equals_the_chain_on_the_model():
    """elasticity on the same mesh, clamped on x = 0, a traction (boundary_loads, vdim 3) on the faces of x = 1"""
    X, e2n, X0, part = _simplex_grid(3, 4, 2, "straight")
    NE, NV = len(e2n), len(X)
    fe, fl = pr.boundary_faces(3, e2n)
    on = np.array([bool(np.all(X0[e2n[e, list(em.FACE_NODES[(3, 10)][l])], 0] == 1.0)) for e, l in zip(fe, fl)])
    fe, fl = np.ascontiguousarray(fe[on]), np.ascontiguousarray(fl[on])
    assert len(fe) == 2 * 4 * 4
    coef = ec.coefficients(NE, 3, 1, 2)
    t = np.random.default_rng(6).uniform(-1.0, 1.0, (NV, 3))
    bdr = np.repeat(np.where(X0[:, 0] == 0.0, am.ON_ESS_DOMAIN_BORDER, 0).astype(np.int8), 3)
    dX, dv = _cuda(X), _cuda(e2n)
    elmat_d, dptr_d, dofs_d = capi.element_matrices(dX, dv, 1, _cuda(coef), device=True, dofs=True)
    elvec_d = capi.boundary_loads(dX, dv, _cuda(fe), _cuda(fl), _cuda(t), vdim=3, device=True)
    assert elvec_d.is_cuda and dofs_d.is_cuda
    elmat = em.element_matrices(X, e2n, 1, coef)
    elvec = em.boundary_loads(X, e2n, fe, fl, t, vdim=3, add_to=np.zeros((NE, 30)))
    dptr, dofs = em.dof_lists(3, e2n, 1)
    assert np.array_equal(_host(elmat_d), elmat) and np.array_equal(_host(elvec_d).ravel(), elvec.ravel())
    assert np.array_equal(_host(dptr_d), dptr) and np.array_equal(_host(dofs_d).ravel(), dofs)
    d = _solve(3 * NV, dptr, dofs_d.reshape(-1), elmat_d.reshape(-1), elvec_d.reshape(-1), bdr, part, 1e-8, True)
    g = _solve(3 * NV, dptr, dofs, np.ascontiguousarray(elmat.ravel()), np.ascontiguousarray(elvec.ravel()), bdr, part, 1e-8, False)
    _same(d, g)


# ---- a manufactured solution ----
_reference = {}


def _manufactured(dim, n):
    """(X, e2n, agglomerates, bdr, f, u at the nodes, the model's global mass matrix, the relative M-norm error of a direct solve of
    the model's system) on the straight box split, computed once"""
    if (dim, n) not in _reference:
        import scipy.sparse as sp
        from scipy.sparse.linalg import spsolve
        X, e2n, _, part = _simplex_grid(dim, n, n // 2)
        NE, NV = len(e2n), len(X)
        u = np.prod(np.sin(np.pi * X), axis=1)
        f = (dim * np.pi ** 2 + REACTION) * u
        bdr = np.where(np.any((X == 0.0) | (X == 1.0), axis=1), am.ON_ESS_DOMAIN_BORDER, 0).astype(np.int8)
        one = np.ones(NE)
        mass = em.element_mass(X, e2n, one)
        elmat = em.element_mass(X, e2n, np.full(NE, REACTION), add_to=em.element_matrices(X, e2n, 0, one))
        b = am.eliminate_rhs(NV, None, e2n, elmat, bdr, np.zeros(NV), am.assemble_rhs(NV, None, e2n, em.element_loads(X, e2n, f)))
        rp, col, val = am.assemble(NV, None, e2n, elmat, bdr)
        A = sp.csr_matrix((val, col, rp), shape=(NV, NV))
        rp, col, val = am.assemble(NV, None, e2n, mass)
        M = sp.csr_matrix((val, col, rp), shape=(NV, NV))
        _reference[(dim, n)] = (X, e2n, part, bdr, f, u, M, _m_error(spsolve(A.tocsc(), b), u, M))
    return _reference[(dim, n)]


def _m_error(x, u, M):
    e = x - u
    return float(np.sqrt(e @ (M @ e)) / np.sqrt(u @ (M @ u)))


@pytest.mark.parametrize("dim", [2, 3], ids=["tri6", "tet10"])
def test_manufactured_solution_converges_at_third_order(dim):
    """-Laplace u + 10 u = f, u the product of sin(pi x_i), f = (dim pi^2 + 10) u given at the nodes, zero Dirichlet values, on
    the straight box split at n = 4 and n = 8, PCG to 1e-10 through the device chain.  Each relative M-norm error is within
    1e-3 (relative) of the error of a direct solve of the model's system, and the 4 / 8 error ratio is at least 0.9 times the
    ratio of the two direct solves (direct solves: tri6 2.928e-3 and 2.062e-4, ratio 14.2; tet10 7.797e-3 and 6.081e-4, ratio
    12.8 -- above the 8 of third order: the error is measured at the nodes, against the nodal values of u)."""
    err, ref = {}, {}
    for n in (4, 8):
        X, e2n, part, bdr, f, u, M, ref[n] = _manufactured(dim, n)
        NE, NV = len(e2n), len(X)
        nd = e2n.shape[1]
        dX, dv = _cuda(X), _cuda(e2n)
        elmat = capi.element_matrices(dX, dv, 0, _cuda(np.ones(NE)), device=True)
        capi.element_mass(dX, dv, _cuda(np.full(NE, REACTION)), add_to=elmat)
        elvec = capi.element_loads(dX, dv, _cuda(f), device=True)
        ep = (nd * np.arange(NE + 1)).astype(np.int32)
        x, it, conv, _, _ = _solve(NV, ep, dv.reshape(-1), elmat.reshape(-1), elvec.reshape(-1), bdr, part, 1e-10, True)
        err[n] = _m_error(x, u, M)
        print("%dD n = %d: %d iterations, relative M-norm error %.6e (direct solve of the model's system: %.6e)" % (dim, n, it, err[n], ref[n]))
        assert conv
        assert abs(err[n] - ref[n]) <= 1e-3 * ref[n]
    print("ratio %.3f (direct solves: %.3f)" % (err[4] / err[8], ref[4] / ref[8]))
    assert err[4] / err[8] >= 0.9 * (ref[4] / ref[8])
