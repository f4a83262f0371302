"""Boundary forms on the device (bdr_mass_kernel, bdr_load_kernel and the face checks of csrc/elmat.hip) against their
definition (saamge_amd/elmat_model.py boundary_mass / boundary_loads), bit for bit: the face mass for vdim 1 and dim added to the
device's own diffusion / elasticity matrices, the face loads with and without a coefficient, every mesh and jitter and the four
face lists of bdr_forms_cases, host and device pointers; the calls that write nothing or equal a union; every refusal; the chain
coordinates -> K + Robin term, loads + Neumann term -> operator -> assemble_rhs -> hierarchy -> PCG on device pointers against
the same chain fed the model's arrays from the host; and a manufactured Robin problem on the box grids 8^3 and 16^3 against a
direct solve of the model's system."""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import capi
from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import bdr_forms_cases as bc
import elmat_cases as ec
import elmat_q2_cases as qc

pytestmark = pytest.mark.gpu


def _cuda(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()      # (a copy: the model's arrays are read-only)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _numpy(a):
    return None if a is None else np.array(a)                               # (a copy: the calls write in place)


def _copy(a):
    return a.clone() if hasattr(a, "data_ptr") else np.array(a)


_want = {}


def _model(family, name, jitter, variant):
    """the model's arrays of a case and a face list, computed once and left unchanged"""
    key = (family, name, jitter, variant)
    if key not in _want:
        X, e2v, ep = bc.mesh(family, name, jitter)
        dim, NE = X.shape[1], ec.num_elements(e2v, ep)
        stiff = ec.model if family == "q1" else qc.model
        fe, fl = bc.faces(family, name, variant)
        c = bc.face_coefficients(NE, fe, fl)
        g1, gd = bc.nodal_data(len(X), dim)
        base1, based = _load_bases(e2v, ep, dim)
        w = {
            "k_plus_r": em.boundary_mass(X, e2v, fe, fl, c, elem_ptr=ep, add_to=stiff(name, jitter, 0, 1)[0]),
            "e_plus_r": em.boundary_mass(X, e2v, fe, fl, c, vdim=dim, elem_ptr=ep, add_to=stiff(name, jitter, 1, 2)[0]),
            "loads1": em.boundary_loads(X, e2v, fe, fl, g1, coef=c, elem_ptr=ep, add_to=base1),
            "loadsd": em.boundary_loads(X, e2v, fe, fl, gd, vdim=dim, coef=c, elem_ptr=ep, add_to=based),
            "loads1_unit": em.boundary_loads(X, e2v, fe, fl, g1, elem_ptr=ep, add_to=base1),
        }
        for v in w.values():
            v.setflags(write=False)
        _want[key] = w
    return _want[key]


def _load_bases(e2v, ep, dim):
    """the vectors the loads are added to: random, so that an addition to the wrong dof shows"""
    rng = np.random.default_rng(19)
    return rng.uniform(-1.0, 1.0, bc.zeros(e2v, ep, 1, False).shape), rng.uniform(-1.0, 1.0, bc.zeros(e2v, ep, dim, False).shape)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("family,name,jitter", bc.CASES, ids=bc.IDS)
def test_device_equals_model(family, name, jitter, device):
    X, e2v, ep = bc.mesh(family, name, jitter)
    dim, NE = X.shape[1], ec.num_elements(e2v, ep)
    stiff = ec.model if family == "q1" else qc.model
    dev = _cuda if device else _numpy
    dX, dv, dp = dev(X), dev(e2v), dev(ep)
    g1, gd = bc.nodal_data(len(X), dim)
    base1, based = _load_bases(e2v, ep, dim)
    # the device's own stiffness matrices, once
    own = {}
    for kind in (0, 1):
        K, coef = stiff(name, jitter, kind, 2 if kind else 1)
        own[kind] = capi.element_matrices(dX, dv, kind, dev(coef[:, 0] if kind == 0 else coef), elem_ptr=dp, device=device)
        assert np.array_equal(_host(own[kind]), K)
    for variant in bc.VARIANTS:
        fe, fl = bc.faces(family, name, variant)
        c = bc.face_coefficients(NE, fe, fl)
        want = _model(family, name, jitter, variant)
        dfe, dfl, dc = dev(fe), dev(fl), dev(c)
        for tag, kind, vdim in (("k_plus_r", 0, 1), ("e_plus_r", 1, dim)):
            base = _copy(own[kind])
            got = capi.boundary_mass(dX, dv, dfe, dfl, dc, vdim=vdim, elem_ptr=dp, add_to=base)
            assert got is base and np.array_equal(_host(got), want[tag]), (variant, tag)
        for tag, vdim, g, coef, b in (("loads1", 1, g1, dc, base1), ("loadsd", dim, gd, dc, based), ("loads1_unit", 1, g1, None, base1)):
            base = dev(np.array(b))
            got = capi.boundary_loads(dX, dv, dfe, dfl, dev(g), vdim=vdim, coef=coef, elem_ptr=dp, add_to=base)
            assert got is base and np.array_equal(_host(got).ravel(), want[tag].ravel()), (variant, tag)
    # a permuted list gives the same bits (the model says so; here for the record of the device)
    assert np.array_equal(_model(family, name, jitter, "all")["k_plus_r"], _model(family, name, jitter, "shuffled")["k_plus_r"])


def _info(dim, e2v, ep, fe, fl, vdim, mass):
    """what info must hold"""
    nd = bc.node_counts(e2v, ep)
    want = [0] * 8
    for e, l in zip(fe, fl):
        fn = len(em.FACE_NODES[(dim, int(nd[e]))][l])
        want[em.FACE_TYPE_INDEX[(dim, fn)]] += 1
        want[5] += fn * fn * vdim if mass else fn * vdim
    want[6], want[7] = -1, len(set(fe.tolist()))
    return want


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_sizes_only_and_empty_list_write_nothing(device):
    dev = _cuda if device else _numpy
    for family, name in (("q1", "mixed_4"), ("q2", "mixed_hex8_hex27"), ("q2", "quad9_9x8"), ("q1", "tris_4x3")):
        X, e2v, ep = bc.box_mesh(family, name)
        dim, NE = X.shape[1], ec.num_elements(e2v, ep)
        fe, fl = bc.faces(family, name, "interior")
        c = bc.face_coefficients(NE, fe, fl)
        dX, dv, dp = dev(X), dev(e2v), dev(ep)
        for vdim in (1, dim):
            info = capi.boundary_mass(dX, dv, dev(fe), dev(fl), dev(c), vdim=vdim, elem_ptr=dp, sizes_only=True)
            assert info == _info(dim, e2v, ep, fe, fl, vdim, True)
            info = capi.boundary_loads(dX, dv, dev(fe), dev(fl), dev(np.ones((len(X), vdim))), vdim=vdim, elem_ptr=dp, sizes_only=True)
            assert info == _info(dim, e2v, ep, fe, fl, vdim, False)
        # without a target: the face terms alone, in new zeros, on the device when asked for
        alone = capi.boundary_loads(dX, dv, dev(fe), dev(fl), dev(np.ones(len(X))), coef=dev(c), elem_ptr=dp, device=device)
        assert hasattr(alone, "data_ptr") == device
        assert np.array_equal(_host(alone), np.ravel(em.boundary_loads(X, e2v, fe, fl, np.ones(len(X)), coef=c, elem_ptr=ep,
                                                                         add_to=bc.zeros(e2v, ep, 1, False))))
        alone = capi.boundary_mass(dX, dv, dev(fe), dev(fl), dev(c), vdim=dim, elem_ptr=dp, device=device)
        assert hasattr(alone, "data_ptr") == device
        assert np.array_equal(_host(alone), np.ravel(em.boundary_mass(X, e2v, fe, fl, c, vdim=dim, elem_ptr=ep,
                                                                        add_to=bc.zeros(e2v, ep, dim, True))))
        # NF = 0: the target keeps its bits
        rng = np.random.default_rng(23)
        K, b = rng.uniform(-1, 1, bc.zeros(e2v, ep, 1, True).shape), rng.uniform(-1, 1, bc.zeros(e2v, ep, 1, False).shape)
        K[:3], b[:3] = [-0.0, np.nan, 0.0], [-0.0, np.nan, 0.0]
        none = np.zeros(0, np.int32)
        gotK = capi.boundary_mass(dX, dv, dev(none), dev(none), dev(np.zeros(0)), elem_ptr=dp, add_to=dev(K))
        gotb = capi.boundary_loads(dX, dv, dev(none), dev(none), dev(np.ones(len(X))), elem_ptr=dp, add_to=dev(b))
        assert _host(gotK).tobytes() == K.tobytes() and _host(gotb).tobytes() == b.tobytes()
        assert capi.boundary_mass(dX, dv, dev(none), dev(none), dev(np.zeros(0)), elem_ptr=dp, sizes_only=True) == [0] * 6 + [-1, 0]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_untouched_entries_keep_their_bits_and_six_sides_equal_the_model(device):
    """A target seeded with -0.0 and NaN where no face reaches; the six sides of the box one call each, each with its own g."""
    dev = _cuda if device else _numpy
    family, name = "q1", "hex_5x4x3"
    X, e2v, ep = bc.mesh(family, name, True)
    NE, NV = len(e2v), len(X)
    fe, fl = bc.faces(family, name, "all")
    rng = np.random.default_rng(29)
    K = rng.uniform(-1.0, 1.0, (NE, 24, 24))
    touched = em.boundary_mass(X, e2v, fe, fl, np.ones(len(fe)), vdim=3, add_to=np.zeros_like(K)) != 0.0
    K[~touched] = np.where(rng.random((~touched).sum()) < 0.5, -0.0, np.nan)
    c = bc.face_coefficients(NE, fe, fl)
    want = em.boundary_mass(X, e2v, fe, fl, c, vdim=3, add_to=K)
    got = capi.boundary_mass(dev(X), dev(e2v), dev(fe), dev(fl), dev(c), vdim=3, add_to=dev(K))
    assert _host(got).tobytes() == want.tobytes()
    assert _host(got)[~touched].tobytes() == K[~touched].tobytes()
    # six one-side calls, each with its own nodal g
    b = rng.uniform(-1.0, 1.0, (NE, 8))
    want_b, got_b = b, dev(b)
    for axis in range(3):
        for value in (0.0, 1.0):
            sel = bc.on_side(family, name, fe, fl, axis, value)
            g = rng.uniform(-1.0, 1.0, NV)
            want_b = em.boundary_loads(X, e2v, fe[sel], fl[sel], g, coef=c[sel], add_to=want_b)
            got_b = capi.boundary_loads(dev(X), dev(e2v), dev(fe[sel]), dev(fl[sel]), dev(g), coef=dev(c[sel]), add_to=got_b)
    assert np.array_equal(_host(got_b), want_b)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals(device):
    X, e2v, _ = ec.mesh("hex_5x4x3")
    NE, NV = len(e2v), len(X)
    fe, fl = bc.faces("q1", "hex_5x4x3", "shuffled")
    NF = len(fe)
    one = np.ones(NF)
    dev = _cuda if device else _numpy

    def refused(match, call):
        with pytest.raises(RuntimeError, match=match) as err:
            call()
        return err.value.info

    def both(match, coords=X, lists=e2v, face_elem=fe, face_local=fl, face=None):
        """refused by the mass and by the loads, from the writing call and from the sizes-only call"""
        for sizes_only in (False, True):
            a = refused(match, lambda: capi.boundary_mass(dev(coords), dev(lists), dev(face_elem), dev(face_local), dev(one[:len(face_elem)]),
                                                          add_to=dev(np.zeros((NE, 8, 8))), sizes_only=sizes_only))
            b = refused(match, lambda: capi.boundary_loads(dev(coords), dev(lists), dev(face_elem), dev(face_local), dev(np.ones(NV)),
                                                           add_to=dev(np.zeros((NE, 8))), sizes_only=sizes_only))
            if face is not None:
                assert a[6] == face and b[6] == face
    # the arguments alone
    K, b = np.zeros((NE, 8, 8)), np.zeros((NE, 8))
    refused("vdim must be 1 or dim", lambda: capi.boundary_mass(dev(X), dev(e2v), dev(fe), dev(fl), dev(one), vdim=2, add_to=dev(K)))
    refused("vdim must be 1 or dim", lambda: capi.boundary_loads(dev(X), dev(e2v), dev(fe), dev(fl), dev(np.ones((NV, 2))), vdim=2,
                                                                 add_to=dev(b)))
    refused("null argument: coef", lambda: capi.boundary_mass(dev(X), dev(e2v), dev(fe), dev(fl), None, add_to=dev(K)))
    refused("null argument: g", lambda: capi.boundary_loads(dev(X), dev(e2v), dev(fe), dev(fl), None, add_to=dev(b)))
    refused("null argument: face_elem or face_local", lambda: capi.boundary_mass(dev(X), dev(e2v), dev(fe), None, dev(one), add_to=dev(K)))
    info = (capi.C.c_longlong * 8)()
    assert capi.load().saamge_amd_boundary_mass(NV, 3, capi._ptr(dev(X)), NE, 8, None, capi._ptr(dev(e2v)), -1, None, None, 1, None,
                                                None, None, info) != 0
    assert b"NF < 0" in capi.load().saamge_amd_last_error()
    # the mesh: what element_mass refuses
    both("out of range", lists=np.where(e2v == 7, NV, e2v).astype(np.int32))
    twice = e2v.copy()
    twice[23, 7] = twice[23, 4]
    both("twice", lists=twice)
    both("nde = 5 nodes are no supported element type in 3D", lists=np.ascontiguousarray(e2v[:, :5]))
    # the face list: the lowest offending index of the list
    wrong = fe.copy()
    wrong[[40, 11, 77]] = [NE, -1, NE + 5]
    both(r"face 11: face_elem is outside \[0, NE\)", face_elem=wrong, face=11)
    wrong = fl.copy()
    wrong[[60, 9]] = [6, -1]
    both("face 9: face_local is outside the element type's range", face_local=wrong, face=9)
    wrong_e, wrong_l = fe.copy(), fl.copy()
    wrong_e[5], wrong_l[30] = NE, 7                                                                  # both kinds: the lower index
    both(r"face 5: face_elem is outside \[0, NE\)", face_elem=wrong_e, face_local=wrong_l, face=5)
    twice_e, twice_l = fe.copy(), fl.copy()
    twice_e[[50, 81]], twice_l[[50, 81]] = [fe[20], fe[33]], [fl[20], fl[33]]                        # pairs (20, 50) and (33, 81)
    both("face 20: the same \\(element, local face\\) is listed twice", face_elem=twice_e, face_local=twice_l, face=20)
    # a measure that is not positive: the lowest such face of the list.  Faces 31 and 12 shrink to a point each (their elements
    # become pyramids, whose determinants the boundary calls do not look at); the model names the faces it refuses one by one
    flat = X.copy()
    for f in (31, 12):
        v = bc.face_vertices(3, e2v, None, fe[f:f + 1], fl[f:f + 1])[0]
        flat[v] = flat[v[0]]
    measured = []
    for f in range(NF):
        try:
            em.boundary_mass(flat, e2v, fe[f:f + 1], fl[f:f + 1], one[:1], add_to=K)
        except em.FaceError:
            measured.append(f)
    assert measured == [12, 31]
    both("face 12: the measure is not positive", coords=flat, face=12)


# ---- the whole chain on device pointers ----
def _sides(n):
    """the boundary faces of the n^3 hex grid and, per side (axis, value), which of them lie on it"""
    e2v = ec.hex_vertices((n, n, n))
    X = pr.grid_coords(n)
    fe, fl = pr.boundary_faces(3, e2v)
    verts = bc.face_vertices(3, e2v, None, fe, fl)
    sides = {(axis, value): np.array([bool(np.all(X[v, axis] == value)) for v in verts]) for axis in range(3) for value in (0.0, 1.0)}
    return e2v, fe, fl, sides


def _solve(pb, NV, e2v, elmat, elvec, rel_tol, device):
    """Operator -> assemble_rhs -> Hierarchy.from_operator -> PCG without essential dofs, on device tensors or host arrays"""
    import torch
    bdr = np.zeros(NV, np.int8)
    dv, dbdr = (_cuda(e2v), _cuda(bdr)) if device else (e2v, bdr)
    op = capi.Operator(NV, dv, elmat, dbdr)
    h = None
    try:
        b = op.assemble_rhs(elvec, device=device)
        prob = pr.Problem(**dict(pb.__dict__, elmat=elmat, elem_to_dof=dv, bdr=dbdr))
        h = capi.Hierarchy.from_operator(prob, op, capi.default_params(num_coarsenings=1))
        x, it, conv, hist = h.pcg(b, x=torch.zeros_like(b), rel_tol=rel_tol) if device else h.pcg(b, rel_tol=rel_tol)
        return _host(x), it, conv, np.asarray(hist), _host(b)
    finally:
        if h is not None:
            h.close()
        op.close()


def test_chain_on_device_pointers_equals_the_chain_on_the_model():
    """-div grad u = f with the Robin condition du/dn + alpha u = g, alpha per face in [0.5, 2), on the jittered 8^3 grid."""
    n = 8
    X = pr.jitter(pr.grid_coords(n), (n, n, n), ec.JITTER, seed=7)
    pb = pr.poisson3d_problem(n, blk=(4, 4, 4), with_elmat=False)
    e2v, fe, fl, _ = _sides(n)
    assert np.array_equal(e2v, pb.elem_to_dof)
    NE, NV = len(e2v), len(X)
    rng = np.random.default_rng(5)
    f, g, alpha = rng.uniform(0.0, 1.0, NV), rng.uniform(0.0, 1.0, NV), rng.uniform(0.5, 2.0, len(fe))
    dX, dv, dfe, dfl = _cuda(X), _cuda(e2v), _cuda(fe), _cuda(fl)
    elmat_d = capi.element_matrices(dX, dv, 0, _cuda(np.ones(NE)), device=True)
    assert capi.boundary_mass(dX, dv, dfe, dfl, _cuda(alpha), add_to=elmat_d) is elmat_d and elmat_d.is_cuda
    elvec_d = capi.element_loads(dX, dv, _cuda(f), device=True)
    assert capi.boundary_loads(dX, dv, dfe, dfl, _cuda(g), add_to=elvec_d) is elvec_d and elvec_d.is_cuda
    xd, itd, convd, histd, bd = _solve(pb, NV, e2v, elmat_d, elvec_d, 1e-8, True)
    # the model's arrays, fed from the host
    elmat = em.boundary_mass(X, e2v, fe, fl, alpha, add_to=em.element_matrices(X, e2v, 0, np.ones(NE)))
    elvec = em.boundary_loads(X, e2v, fe, fl, g, add_to=em.element_loads(X, e2v, f))
    assert np.array_equal(_host(elmat_d), elmat) and np.array_equal(_host(elvec_d), elvec)
    xg, itg, convg, histg, bg = _solve(pb, NV, e2v, np.ascontiguousarray(elmat), np.ascontiguousarray(elvec), 1e-8, False)
    assert np.array_equal(bd, bg) and np.array_equal(bg, am.assemble_rhs(NV, None, e2v, elvec))
    assert convd and convg and itd == itg
    assert np.array_equal(histd, histg) and np.array_equal(xd, xg)


# ---- a manufactured Robin problem ----
def _exact(X):
    """u = sin(x + 2y + 3z) and its gradient at the points X"""
    t = X[:, 0] + 2.0 * X[:, 1] + 3.0 * X[:, 2]
    return np.sin(t), np.cos(t)[:, None] * np.array([1.0, 2.0, 3.0])[None, :]


_reference = {}


def _manufactured(n):
    """(X, f, the six (faces, g), u at the nodes, the model's global mass matrix, the relative M-norm error of a direct solve of
    the model's system) on the box grid n^3, computed once"""
    if n not in _reference:
        import scipy.sparse as sp
        from scipy.sparse.linalg import spsolve
        X = pr.grid_coords(n)
        e2v, fe, fl, sides = _sides(n)
        NE, NV = len(e2v), len(X)
        u, grad = _exact(X)
        f = 14.0 * u
        data = []
        for (axis, value), sel in sorted(sides.items()):
            data.append((fe[sel], fl[sel], (1.0 if value else -1.0) * grad[:, axis] + u))      # du/dn + u on this side
        one = np.ones(NE)
        mass = em.element_mass(X, e2v, one)
        elmat = em.boundary_mass(X, e2v, fe, fl, np.ones(len(fe)), add_to=em.element_matrices(X, e2v, 0, one))
        elvec = em.element_loads(X, e2v, f)
        for sfe, sfl, g in data:
            elvec = em.boundary_loads(X, e2v, sfe, sfl, g, add_to=elvec)
        rp, col, val = am.assemble(NV, None, e2v, elmat, np.zeros(NV, np.int8))
        A = sp.csr_matrix((val, col, rp), shape=(NV, NV))
        rp, col, val = am.assemble(NV, None, e2v, mass)
        M = sp.csr_matrix((val, col, rp), shape=(NV, NV))
        ref = _m_error(spsolve(A.tocsc(), am.assemble_rhs(NV, None, e2v, elvec)), u, M)
        _reference[n] = (X, e2v, fe, fl, f, data, u, M, ref)
    return _reference[n]


def _m_error(x, u, M):
    e = x - u
    return float(np.sqrt(e @ (M @ e)) / np.sqrt(u @ (M @ u)))


def test_manufactured_robin_problem_converges_at_second_order():
    """-Laplace u = 14 u on the unit cube, u = sin(x + 2y + 3z), du/dn + u = g on all six sides with g given at the nodes of
    each side (six boundary_loads calls: g jumps across the edges), PCG to 1e-10 through the device chain.  Each relative
    M-norm error is within 1e-3 (relative) of the error of a direct solve of the model's system, and the 8^3 / 16^3 error
    ratio is at least 0.9 times the ratio of the two direct solves (direct solves: 7.698e-3 and 1.934e-3, ratio 3.98)."""
    err, ref = {}, {}
    for n in (8, 16):
        X, e2v, fe, fl, f, data, u, M, ref[n] = _manufactured(n)
        pb = pr.poisson3d_problem(n, blk=(4, 4, 4), with_elmat=False)
        NE, NV = len(e2v), len(X)
        dX, dv = _cuda(X), _cuda(e2v)
        elmat = capi.element_matrices(dX, dv, 0, _cuda(np.ones(NE)), device=True)
        capi.boundary_mass(dX, dv, _cuda(fe), _cuda(fl), _cuda(np.ones(len(fe))), add_to=elmat)
        elvec = capi.element_loads(dX, dv, _cuda(f), device=True)
        for sfe, sfl, g in data:
            capi.boundary_loads(dX, dv, _cuda(sfe), _cuda(sfl), _cuda(g), add_to=elvec)
        x, it, conv, _, _ = _solve(pb, NV, e2v, elmat, elvec, 1e-10, True)
        err[n] = _m_error(x, u, M)
        print("n = %d: %d iterations, relative M-norm error %.6e (direct solve of the model's system: %.6e)" % (n, it, err[n], ref[n]))
        assert conv
        assert abs(err[n] - ref[n]) <= 1e-3 * ref[n]
    print("ratio %.3f (direct solves: %.3f)" % (err[8] / err[16], ref[8] / ref[16]))
    assert err[8] / err[16] >= 0.9 * (ref[8] / ref[16])
