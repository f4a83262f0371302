"""Boundary data at the face points on the device (bdr_points_kernel, bdr_eval_kernel, bdr_mass_q_kernel, bdr_load_q_kernel and the
offsets of the face points of csrc/elmat.hip) against its definition (saamge_amd/elmat_model.py boundary_points / boundary_eval /
boundary_mass_points / boundary_loads_points), bit for bit: all four calls on every mesh, jitter and face list of bdr_points_cases,
host and device pointers, vdim 1 and dim; the empty list, one face, the calls that only check, targets that keep their bits; the
reductions to the calls per face; every refusal, from the writing and from the checking call, with the outputs untouched; the
chain coordinates -> K + Robin term with alpha at the points, loads + flux data formed on the device from the call's own points and
normals -> operator -> assemble_rhs -> hierarchy -> PCG on device pointers against the same chain fed the model's arrays from the
host; and the manufactured Robin problem of test_gpu_bdr_forms.py with g given at the face points in one call."""
import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import capi
from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import bdr_forms_cases as bc
import bdr_points_cases as bp
import elmat_cases as ec

pytestmark = pytest.mark.gpu


def _cuda(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).cuda()      # (a copy: the model's arrays are read-only)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _numpy(a):
    return None if a is None else np.array(a)                               # (a copy: the calls write in place)


def _same(got, want):
    return _host(got).tobytes() == np.ascontiguousarray(want).tobytes()


_want = {}


def _forms(family, name, jitter, variant):
    """the model's matrices and vectors of a case and a face list with data at the points, computed once and left unchanged"""
    key = (family, name, jitter, variant)
    if key not in _want:
        X, e2v, ep = bp.mesh(family, name, jitter)
        dim, NE = X.shape[1], ec.num_elements(e2v, ep)
        fe, fl = bp.faces(family, name, variant)
        m = bp.model(family, name, jitter, variant)
        c = bc.face_coefficients(NE, fe, fl)
        K1, Kd, b1, bd = _bases(e2v, ep, dim)
        w = {"mass1": em.boundary_mass_points(X, e2v, fe, fl, m["cq"], elem_ptr=ep, add_to=K1),
             "massd": em.boundary_mass_points(X, e2v, fe, fl, m["cq"], vdim=dim, elem_ptr=ep, add_to=Kd),
             "loads1": em.boundary_loads_points(X, e2v, fe, fl, m["gq1"], coef=c, elem_ptr=ep, add_to=b1),
             "loadsd": em.boundary_loads_points(X, e2v, fe, fl, m["gqd"], vdim=dim, coef=c, elem_ptr=ep, add_to=bd),
             "loads1_unit": em.boundary_loads_points(X, e2v, fe, fl, m["gq1"], elem_ptr=ep, add_to=b1)}
        for v in w.values():
            v.setflags(write=False)
        _want[key] = w
    return _want[key]


def _bases(e2v, ep, dim):
    """the matrices and vectors the faces are added to: random, so that an addition to the wrong entry shows"""
    rng = np.random.default_rng(19)
    return [rng.uniform(-1.0, 1.0, bc.zeros(e2v, ep, vdim, square).shape) for square in (True, False) for vdim in (1, dim)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("family,name,jitter", bp.CASES, ids=bp.IDS)
def test_device_equals_model(family, name, jitter, device):
    X, e2v, ep = bp.mesh(family, name, jitter)
    dim, NE = X.shape[1], ec.num_elements(e2v, ep)
    dev = _cuda if device else _numpy
    dX, dv, dp = dev(X), dev(e2v), dev(ep)
    u1, ud = bc.nodal_data(len(X), dim)
    du1, dud = dev(u1), dev(ud)
    K1, Kd, b1, bd = _bases(e2v, ep, dim)
    for variant in bp.VARIANTS:
        fe, fl = bp.faces(family, name, variant)
        m, want = bp.model(family, name, jitter, variant), _forms(family, name, jitter, variant)
        dfe, dfl, dc = dev(fe), dev(fl), dev(bc.face_coefficients(NE, fe, fl))
        fp, xq, wmeas, normal = capi.boundary_points(dX, dv, dfe, dfl, elem_ptr=dp, device=device)
        assert hasattr(xq, "data_ptr") == device and _host(fp).dtype == np.int64
        assert _same(fp, m["fp"]) and _same(xq, m["xq"]) and _same(wmeas, m["wmeas"]) and _same(normal, m["normal"]), variant
        for vdim, u, tag in ((1, du1, "1"), (dim, dud, "d")):
            uq, gq = capi.boundary_eval(dX, dv, dfe, dfl, u, vdim=vdim, elem_ptr=dp, device=device)
            assert _same(uq, m["uq" + tag]) and _same(gq, m["gradq" + tag]), (variant, vdim)
        for tag, vdim, base in (("mass1", 1, K1), ("massd", dim, Kd)):
            target = dev(base)
            got = capi.boundary_mass_points(dX, dv, dfe, dfl, dev(m["cq"]), vdim=vdim, elem_ptr=dp, add_to=target)
            assert got is target and _same(got, want[tag]), (variant, tag)
        for tag, vdim, coef, base in (("loads1", 1, dc, b1), ("loadsd", dim, dc, bd), ("loads1_unit", 1, None, b1)):
            target = dev(base)
            got = capi.boundary_loads_points(dX, dv, dfe, dfl, dev(m["gq1" if vdim == 1 else "gqd"]), vdim=vdim, coef=coef, elem_ptr=dp,
                                             add_to=target)
            assert got is target and _same(got, want[tag]), (variant, tag)


def _info(dim, e2v, ep, fe, fl, fifth):
    """what info must hold"""
    nd = bc.node_counts(e2v, ep)
    want = [0] * 8
    for e, l in zip(fe, fl):
        want[em.face_info_index(dim, len(em.FACE_NODES[(dim, int(nd[e]))][l]))] += 1
    want[5], want[6], want[7] = fifth, -1, len(set(np.asarray(fe).tolist()))
    return want


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_empty_list_one_face_and_the_calls_that_only_check(device):
    dev = _cuda if device else _numpy
    for family, name, jitter in (("q1", "mixed_4", True), ("q2", "mixed_hex8_hex27", "curved"), ("p2", "tet10_3x2x2", "curved"),
                                 ("q1", "tris_4x3", False)):
        X, e2v, ep = bp.mesh(family, name, jitter)
        dim, NV = X.shape[1], len(X)
        fe, fl = bp.faces(family, name, "interior")
        m = bp.model(family, name, jitter, "interior")
        NFQ = int(m["fp"][-1])
        nd = bc.node_counts(e2v, ep)
        fns = [len(em.FACE_NODES[(dim, int(nd[e]))][l]) for e, l in zip(fe, fl)]
        dX, dv, dp, dfe, dfl = dev(X), dev(e2v), dev(ep), dev(fe), dev(fl)
        u1, ud = bc.nodal_data(NV, dim)
        # the calls that only check: info, nothing written
        assert capi.boundary_points(dX, dv, dfe, dfl, elem_ptr=dp, sizes_only=True) == _info(dim, e2v, ep, fe, fl, NFQ)
        assert capi.boundary_eval(dX, dv, dfe, dfl, dev(u1), elem_ptr=dp, want=()) == (None, None)
        for vdim in (1, dim):
            info = capi.boundary_mass_points(dX, dv, dfe, dfl, dev(m["cq"]), vdim=vdim, elem_ptr=dp, sizes_only=True)
            assert info == _info(dim, e2v, ep, fe, fl, sum(f * f * vdim for f in fns))
            info = capi.boundary_loads_points(dX, dv, dfe, dfl, dev(m["gqd" if vdim > 1 else "gq1"]), vdim=vdim, elem_ptr=dp, sizes_only=True)
            assert info == _info(dim, e2v, ep, fe, fl, sum(f * vdim for f in fns))
        # one output at a time
        only = capi.boundary_points(dX, dv, dfe, dfl, elem_ptr=dp, device=device, want=("normal",))
        assert only[0] is None and only[1] is None and only[2] is None and _same(only[3], m["normal"])
        only = capi.boundary_eval(dX, dv, dfe, dfl, dev(ud), vdim=dim, elem_ptr=dp, device=device, want=("gradq",))
        assert only[0] is None and _same(only[1], m["gradqd"])
        # an output the caller brings must have the call's size: refused by the wrapper, before the library writes through it
        with pytest.raises(ValueError, match="xq"):
            capi.boundary_points(dX, dv, dfe, dfl, elem_ptr=dp, out={"xq": dev(np.zeros(NFQ * dim - 1))})
        with pytest.raises(ValueError, match="gradq"):
            capi.boundary_eval(dX, dv, dfe, dfl, dev(u1), elem_ptr=dp, out={"gradq": dev(np.zeros(NFQ * dim + 1))})
        # without a target: the face terms alone, in new zeros, on the device when asked for
        alone = capi.boundary_mass_points(dX, dv, dfe, dfl, dev(m["cq"]), vdim=dim, elem_ptr=dp, device=device)
        assert hasattr(alone, "data_ptr") == device
        assert _same(alone, em.boundary_mass_points(X, e2v, fe, fl, m["cq"], vdim=dim, elem_ptr=ep, add_to=bc.zeros(e2v, ep, dim, True)))
        # NF = 0: the targets keep their bits, fp_ptr is the one offset 0
        rng = np.random.default_rng(23)
        K, b = rng.uniform(-1, 1, bc.zeros(e2v, ep, 1, True).shape), rng.uniform(-1, 1, bc.zeros(e2v, ep, 1, False).shape)
        K[:3], b[:3] = [-0.0, np.nan, 0.0], [-0.0, np.nan, 0.0]
        none = np.zeros(0, np.int32)
        gotK = capi.boundary_mass_points(dX, dv, dev(none), dev(none), dev(np.zeros(0)), elem_ptr=dp, add_to=dev(K))
        gotb = capi.boundary_loads_points(dX, dv, dev(none), dev(none), dev(np.zeros(0)), elem_ptr=dp, add_to=dev(b))
        assert _same(gotK, K) and _same(gotb, b)
        fp, xq, wmeas, normal = capi.boundary_points(dX, dv, dev(none), dev(none), elem_ptr=dp, device=device)
        assert _host(fp).tolist() == [0] and xq.shape == (0, dim) and wmeas.shape == (0,) and normal.shape == (0, dim)
        uq, gq = capi.boundary_eval(dX, dv, dev(none), dev(none), dev(u1), elem_ptr=dp, device=device)
        assert uq.shape == (0, 1) and gq.shape == (0, 1, dim)
        assert capi.boundary_points(dX, dv, dev(none), dev(none), elem_ptr=dp, sizes_only=True) == [0] * 6 + [-1, 0]
        # NF = 1: the last face of the list alone
        one = (fe[-1:], fl[-1:])
        fp1, xq1, wm1, n1 = em.boundary_points(X, e2v, *one, elem_ptr=ep)
        got = capi.boundary_points(dX, dv, dev(one[0]), dev(one[1]), elem_ptr=dp, device=device)
        assert all(_same(g, w) for g, w in zip(got, (fp1, xq1, wm1, n1))) and _same(xq1, m["xq"][m["fp"][-2]:])
        uq, gq = capi.boundary_eval(dX, dv, dev(one[0]), dev(one[1]), dev(ud), vdim=dim, elem_ptr=dp, device=device)
        assert _same(uq, m["uqd"][m["fp"][-2]:]) and _same(gq, m["gradqd"][m["fp"][-2]:])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_untouched_entries_keep_their_bits_and_the_calls_reduce_to_the_calls_per_face(device):
    """Targets seeded with -0.0 and NaN where no face reaches; equal coefficients at the points of each face give the bits of
    boundary_mass; the trace of a nodal g as point data gives the bits of boundary_loads; a permuted list permutes the point
    arrays by whole faces and leaves the matrices and vectors bit-identical -- all on the device's own outputs."""
    dev = _cuda if device else _numpy
    family, name = "q1", "hex_5x4x3"
    X, e2v, ep = bp.mesh(family, name, True)
    NE, NV = len(e2v), len(X)
    fe, fl = bp.faces(family, name, "all")
    se, sl = bp.faces(family, name, "shuffled")
    m, ms = bp.model(family, name, True, "all"), bp.model(family, name, True, "shuffled")
    rng = np.random.default_rng(29)
    K, b = rng.uniform(-1.0, 1.0, (NE, 24, 24)), rng.uniform(-1.0, 1.0, (NE, 24))
    touchedK = em.boundary_mass(X, e2v, fe, fl, np.ones(len(fe)), vdim=3, add_to=np.zeros_like(K)) != 0.0
    touchedb = em.boundary_loads(X, e2v, fe, fl, np.ones((NV, 3)), vdim=3, add_to=np.zeros_like(b)) != 0.0
    K[~touchedK] = np.where(rng.random((~touchedK).sum()) < 0.5, -0.0, np.nan)
    b[~touchedb] = np.where(rng.random((~touchedb).sum()) < 0.5, -0.0, np.nan)
    c = bc.face_coefficients(NE, fe, fl)
    dX, dv = dev(X), dev(e2v)
    gotK = capi.boundary_mass_points(dX, dv, dev(fe), dev(fl), dev(m["cq"]), vdim=3, add_to=dev(K))
    assert _same(gotK, em.boundary_mass_points(X, e2v, fe, fl, m["cq"], vdim=3, add_to=K))
    assert _host(gotK)[~touchedK].tobytes() == K[~touchedK].tobytes() and touchedK.any() and not touchedK.all()
    gotb = capi.boundary_loads_points(dX, dv, dev(fe), dev(fl), dev(m["gqd"]), vdim=3, coef=dev(c), add_to=dev(b))
    assert _same(gotb, em.boundary_loads_points(X, e2v, fe, fl, m["gqd"], vdim=3, coef=c, add_to=b))
    assert _host(gotb)[~touchedb].tobytes() == b[~touchedb].tobytes()
    # a permuted list
    gotKs = capi.boundary_mass_points(dX, dv, dev(se), dev(sl), dev(ms["cq"]), vdim=3, add_to=dev(K))
    gotbs = capi.boundary_loads_points(dX, dv, dev(se), dev(sl), dev(ms["gqd"]), vdim=3, coef=dev(bc.face_coefficients(NE, se, sl)), add_to=dev(b))
    assert _same(gotKs, _host(gotK)) and _same(gotbs, _host(gotb))
    pts, ptss = capi.boundary_points(dX, dv, dev(fe), dev(fl), device=device), capi.boundary_points(dX, dv, dev(se), dev(sl), device=device)
    at = bp.whole_faces(fe, fl, _host(pts[0]), se, sl, _host(ptss[0]))
    assert not np.array_equal(at, np.arange(len(at)))
    for a, s in zip(pts[1:], ptss[1:]):
        assert _host(a)[at].tobytes() == _host(s).tobytes()
    # the reductions, on what the device itself returns
    g = bc.nodal_data(NV, 3)[1]
    uq, _ = capi.boundary_eval(dX, dv, dev(fe), dev(fl), dev(g), vdim=3, device=device)
    got = capi.boundary_loads_points(dX, dv, dev(fe), dev(fl), uq, vdim=3, coef=dev(c), add_to=dev(b))
    assert _same(got, _host(capi.boundary_loads(dX, dv, dev(fe), dev(fl), dev(g), vdim=3, coef=dev(c), add_to=dev(b))))
    got = capi.boundary_mass_points(dX, dv, dev(fe), dev(fl), dev(np.repeat(c, np.diff(m["fp"]))), vdim=3, add_to=dev(K))
    assert _same(got, _host(capi.boundary_mass(dX, dv, dev(fe), dev(fl), dev(c), vdim=3, add_to=dev(K))))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals(device):
    X, e2v, _ = ec.mesh("hex_5x4x3")
    NE, NV = len(e2v), len(X)
    fe, fl = bc.faces("q1", "hex_5x4x3", "shuffled")
    NF = len(fe)
    NFQ = 4 * NF
    dev = _cuda if device else _numpy
    u = np.ones(NV)
    seed = np.random.default_rng(43).uniform(1.0, 2.0, NE * 64)      # no call below writes these bits by itself

    def refused(match, call):
        with pytest.raises(RuntimeError, match=match) as err:
            call()
        return err.value.info

    def every(match, coords=X, lists=e2v, face_elem=fe, face_local=fl, face=None, only_eval=False):
        """refused by all four calls, from the writing call and from the call that only checks; the outputs keep their bits"""
        dX, dv, de, dl = dev(coords), dev(lists), dev(face_elem), dev(face_local)
        n = 4 * len(face_elem)
        for checks in (False, True):
            outs = {k: dev(seed[:s]) for k, s in (("fp_ptr", 0), ("xq", 3 * n), ("wmeas", n), ("normal", 3 * n), ("uq", n),
                                                  ("gradq", 3 * n), ("K", NE * 64), ("b", NE * 8))}
            outs["fp_ptr"] = dev(np.full(len(face_elem) + 1, -7, np.int64))
            calls = [lambda: capi.boundary_eval(dX, dv, de, dl, dev(u), want=() if checks else ("uq", "gradq"),
                                                out={} if checks else {"uq": outs["uq"], "gradq": outs["gradq"]})]
            if not only_eval:
                calls += [lambda: capi.boundary_points(dX, dv, de, dl, sizes_only=checks,
                                                       out={} if checks else {k: outs[k] for k in ("fp_ptr", "xq", "wmeas", "normal")}),
                          lambda: capi.boundary_mass_points(dX, dv, de, dl, dev(np.ones(n)), add_to=outs["K"], sizes_only=checks),
                          lambda: capi.boundary_loads_points(dX, dv, de, dl, dev(np.ones(n)), add_to=outs["b"], sizes_only=checks)]
            for call in calls:
                info = refused(match, call)
                assert face is None or info[6] == face
            for k, o in outs.items():
                assert _same(o, np.full(len(face_elem) + 1, -7, np.int64) if k == "fp_ptr" else seed[:_host(o).size]), k
    # the arguments alone
    dX, dv, de, dl = dev(X), dev(e2v), dev(fe), dev(fl)
    refused("vdim must be 1 or dim", lambda: capi.boundary_eval(dX, dv, de, dl, dev(np.ones((NV, 2))), vdim=2))
    refused("vdim must be 1 or dim", lambda: capi.boundary_mass_points(dX, dv, de, dl, dev(np.ones(NFQ)), vdim=2, add_to=dev(np.zeros((NE, 16, 16)))))
    refused("vdim must be 1 or dim", lambda: capi.boundary_loads_points(dX, dv, de, dl, dev(np.ones((NFQ, 2))), vdim=2, add_to=dev(np.zeros((NE, 16)))))
    refused("null argument: u", lambda: capi.boundary_eval(dX, dv, de, dl, None))
    refused("null argument: coefq", lambda: capi.boundary_mass_points(dX, dv, de, dl, None, add_to=dev(np.zeros((NE, 8, 8)))))
    refused("null argument: gq", lambda: capi.boundary_loads_points(dX, dv, de, dl, None, add_to=dev(np.zeros((NE, 8)))))
    refused("null argument: face_elem or face_local", lambda: capi.boundary_points(dX, dv, de, None))
    info = (capi.C.c_longlong * 8)()
    assert capi.load().saamge_amd_boundary_points(NV, 3, capi._ptr(dX), NE, 8, None, capi._ptr(dv), -1, None, None, None, None, None, None,
                                                  None, info) != 0
    assert b"NF < 0" in capi.load().saamge_amd_last_error()
    # the mesh: what element_mass refuses
    every("out of range", lists=np.where(e2v == 7, NV, e2v).astype(np.int32))
    twice = e2v.copy()
    twice[23, 7] = twice[23, 4]
    every("twice", lists=twice)
    # the face list: the lowest offending index of the list
    wrong = fe.copy()
    wrong[[40, 11, 77]] = [NE, -1, NE + 5]
    every(r"face 11: face_elem is outside \[0, NE\)", face_elem=wrong, face=11)
    wrong = fl.copy()
    wrong[[60, 9]] = [6, -1]
    every("face 9: face_local is outside the element type's range", face_local=wrong, face=9)
    twice_e, twice_l = fe.copy(), fl.copy()
    twice_e[[50, 81]], twice_l[[50, 81]] = [fe[20], fe[33]], [fl[20], fl[33]]                        # pairs (20, 50) and (33, 81)
    every("face 20: the same \\(element, local face\\) is listed twice", face_elem=twice_e, face_local=twice_l, face=20)
    # a measure that is not positive: faces 31 and 12 shrink to a point each, the lower index is named
    flat = X.copy()
    for f in (31, 12):
        v = bc.face_vertices(3, e2v, None, fe[f:f + 1], fl[f:f + 1])[0]
        flat[v] = flat[v[0]]
    every("face 12: the measure is not positive", coords=flat, face=12)
    # an element turned inside out keeps the measures of its faces: eval alone refuses, with or without outputs, and names the
    # lowest face of the list the element owns; the measure comes first
    turned = e2v.copy()
    e = int(fe[25])
    turned[e] = e2v[e][[4, 5, 6, 7, 0, 1, 2, 3]]
    owned = int(np.flatnonzero(fe == e)[0])
    with pytest.raises(em.FaceError) as err:
        em.boundary_eval(X, turned, fe, fl, u, grad=False)
    assert err.value.face == owned
    every("face %d: the Jacobian determinant of the element is not positive" % owned, lists=turned, face=owned, only_eval=True)
    every("face 12: the measure is not positive", coords=flat, lists=turned, face=12, only_eval=True)
    want = em.boundary_points(X, turned, fe, fl)
    assert all(_same(g, w) for g, w in zip(capi.boundary_points(dX, dev(turned), de, dl), want))


# ---- the whole chain on device pointers ----
def _sides(n):
    e2v = ec.hex_vertices((n, n, n))
    fe, fl = pr.boundary_faces(3, e2v)
    return e2v, fe, fl


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
    """-div grad u = f with du/dn + alpha u = g on the jittered 8^3 grid: alpha in [0.5, 2) per face POINT, g formed on the device
    as grad u_ex(x_q) . n_q + alpha_q u_ex(x_q), u_ex = sin(x + 2y + 3z), from boundary_points' own xq and normal; all six sides in
    one call.  The host chain is fed the model's arrays and the same g (the model's points and normals have the device's bits)."""
    import torch
    n = 8
    X = pr.jitter(pr.grid_coords(n), (n, n, n), ec.JITTER, seed=7)
    pb = pr.poisson3d_problem(n, blk=(4, 4, 4), with_elmat=False)
    e2v, fe, fl = _sides(n)
    assert np.array_equal(e2v, pb.elem_to_dof)
    NE, NV = len(e2v), len(X)
    rng = np.random.default_rng(5)
    f = rng.uniform(0.0, 1.0, NV)
    dX, dv, dfe, dfl = _cuda(X), _cuda(e2v), _cuda(fe), _cuda(fl)
    fp, xq, wmeas, normal = capi.boundary_points(dX, dv, dfe, dfl, device=True)
    alpha = _cuda(rng.uniform(0.5, 2.0, xq.shape[0]))
    t = xq[:, 0] + 2.0 * xq[:, 1] + 3.0 * xq[:, 2]
    g = torch.cos(t) * (normal @ torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device="cuda")) + alpha * torch.sin(t)
    assert g.is_cuda and g.shape == (6 * n * n * 4,)
    elmat_d = capi.element_matrices(dX, dv, 0, _cuda(np.ones(NE)), device=True)
    assert capi.boundary_mass_points(dX, dv, dfe, dfl, alpha, add_to=elmat_d) is elmat_d and elmat_d.is_cuda
    elvec_d = capi.element_loads(dX, dv, _cuda(f), device=True)
    assert capi.boundary_loads_points(dX, dv, dfe, dfl, g, add_to=elvec_d) is elvec_d and elvec_d.is_cuda
    xd, itd, convd, histd, bd = _solve(pb, NV, e2v, elmat_d, elvec_d, 1e-8, True)
    # the model's arrays, fed from the host
    mfp, mxq, _, mnormal = em.boundary_points(X, e2v, fe, fl)
    assert _same(fp, mfp) and _same(xq, mxq) and _same(normal, mnormal)
    elmat = em.boundary_mass_points(X, e2v, fe, fl, _host(alpha), add_to=em.element_matrices(X, e2v, 0, np.ones(NE)))
    elvec = em.boundary_loads_points(X, e2v, fe, fl, _host(g), add_to=em.element_loads(X, e2v, f))
    assert np.array_equal(_host(elmat_d), elmat) and np.array_equal(_host(elvec_d), elvec)
    xg, itg, convg, histg, bg = _solve(pb, NV, e2v, np.ascontiguousarray(elmat), np.ascontiguousarray(elvec), 1e-8, False)
    assert np.array_equal(bd, bg) and np.array_equal(bg, am.assemble_rhs(NV, None, e2v, elvec))
    assert convd and convg and itd == itg
    assert np.array_equal(histd, histg) and np.array_equal(xd, xg)


# ---- the manufactured Robin problem, g at the face points ----
_reference = {}


def _manufactured(n):
    """(X, e2v, faces, f, g at the face points of all six sides, u at the nodes, the model's global mass matrix, the relative
    M-norm error of a direct solve of the model's system) on the box grid n^3, computed once"""
    if n not in _reference:
        import scipy.sparse as sp
        from scipy.sparse.linalg import spsolve
        X = pr.grid_coords(n)
        e2v, fe, fl = _sides(n)
        NE, NV = len(e2v), len(X)
        t = X[:, 0] + 2.0 * X[:, 1] + 3.0 * X[:, 2]
        u = np.sin(t)
        f = 14.0 * u
        _, xq, _, normal = em.boundary_points(X, e2v, fe, fl)
        tq = xq[:, 0] + 2.0 * xq[:, 1] + 3.0 * xq[:, 2]
        g = np.cos(tq) * (normal @ np.array([1.0, 2.0, 3.0])) + np.sin(tq)      # du/dn + u at the face points
        one = np.ones(NE)
        mass = em.element_mass(X, e2v, one)
        elmat = em.boundary_mass(X, e2v, fe, fl, np.ones(len(fe)), add_to=em.element_matrices(X, e2v, 0, one))
        elvec = em.boundary_loads_points(X, e2v, fe, fl, g, add_to=em.element_loads(X, e2v, f))
        rp, col, val = am.assemble(NV, None, e2v, elmat, np.zeros(NV, np.int8))
        A = sp.csr_matrix((val, col, rp), shape=(NV, NV))
        rp, col, val = am.assemble(NV, None, e2v, mass)
        M = sp.csr_matrix((val, col, rp), shape=(NV, NV))
        ref = _m_error(spsolve(A.tocsc(), am.assemble_rhs(NV, None, e2v, elvec)), u, M)
        _reference[n] = (X, e2v, fe, fl, f, g, u, M, ref)
    return _reference[n]


def _m_error(x, u, M):
    e = x - u
    return float(np.sqrt(e @ (M @ e)) / np.sqrt(u @ (M @ u)))


def test_manufactured_robin_problem_with_data_at_the_face_points():
    """-Laplace u = 14 u on the unit cube, u = sin(x + 2y + 3z), du/dn + u = g on all six sides with g given AT THE FACE POINTS
    in a single boundary_loads_points call (the normal jumps across the edges, the data at the points does not care), PCG to
    1e-10 through the device chain.  Each relative M-norm error is within 1e-3 (relative) of the error of a direct solve of the
    model's system, and the 8^3 / 16^3 error ratio is at least 0.9 times the ratio of the two direct solves (direct solves:
    7.137e-3 and 1.792e-3, ratio 3.98)."""
    err, ref = {}, {}
    for n in (8, 16):
        X, e2v, fe, fl, f, g, u, M, ref[n] = _manufactured(n)
        pb = pr.poisson3d_problem(n, blk=(4, 4, 4), with_elmat=False)
        NE, NV = len(e2v), len(X)
        dX, dv, dfe, dfl = _cuda(X), _cuda(e2v), _cuda(fe), _cuda(fl)
        elmat = capi.element_matrices(dX, dv, 0, _cuda(np.ones(NE)), device=True)
        capi.boundary_mass_points(dX, dv, dfe, dfl, _cuda(np.ones(len(g))), add_to=elmat)
        elvec = capi.element_loads(dX, dv, _cuda(f), device=True)
        capi.boundary_loads_points(dX, dv, dfe, dfl, _cuda(g), add_to=elvec)
        x, it, conv, _, _ = _solve(pb, NV, e2v, elmat, elvec, 1e-10, True)
        err[n] = _m_error(x, u, M)
        print("n = %d: %d iterations, relative M-norm error %.6e (direct solve of the model's system: %.6e)" % (n, it, err[n], ref[n]))
        assert conv
        assert abs(err[n] - ref[n]) <= 1e-3 * ref[n]
    print("ratio %.3f (direct solves: %.3f)" % (err[8] / err[16], ref[8] / ref[16]))
    assert err[8] / err[16] >= 0.9 * (ref[8] / ref[16])
