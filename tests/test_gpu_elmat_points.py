"""Data at quadrature points on the device (qp_points_kernel, qp_eval_kernel, qp_load_kernel, qp_error_kernel of
csrc/elmat.hip) against its definition (saamge_amd/elmat_model.py element_points / element_eval / element_loads_points /
element_errors), bit for bit: every type undeformed and moved, a jittered hex_5x4x3, tets_3x2x2, hex_9x8x7 (504 elements: more
than one workgroup, the last partly filled), the mixed lists, one element and none; host and device pointers, every combination
of NULL optional outputs, vdim 1 and dim, with and without coef; info, repeated calls, the memory pool; the refusals, which
write nothing; and the chain refine -> points -> f(xq) -> loads_points -> assemble_rhs -> hierarchy -> PCG -> errors on device
pointers against the same chain fed the model's arrays."""
import itertools

import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import capi
from saamge_amd import elmat_model as em
from saamge_amd import mesh_refine_model as rm
from saamge_amd import problems as pr

import elmat_cases as ec
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


def _mesh(name, moved):
    if name.startswith("mixed:"):
        return cs.mixed(name[6:])
    if name in cs.TYPES:
        return cs.mesh(name, moved)
    return ec.mesh(name, moved)


_want = {}


def _model(name, moved):
    """the inputs and the model's arrays of a case, computed once and left unchanged"""
    key = (name, moved)
    if key not in _want:
        X, e2v, ep = _mesh(name, moved)
        dim = X.shape[1]
        NE = ec.num_elements(e2v, ep)
        rng = np.random.default_rng(21)
        w = {"coef": rng.uniform(0.5, 2.0, NE)}
        w["qp_ptr"], w["xq"], w["wdet"] = em.element_points(X, e2v, ep)
        NQ = int(w["qp_ptr"][-1])
        for vdim in (1, dim):
            u = rng.uniform(-1.0, 1.0, (len(X), vdim))
            fq, ex, exg = rng.uniform(-1.0, 1.0, (NQ, vdim)), rng.uniform(-1.0, 1.0, (NQ, vdim)), rng.uniform(-1.0, 1.0, (NQ, vdim, dim))
            uq, gq = em.element_eval(X, e2v, u, vdim=vdim, elem_ptr=ep)
            w[vdim] = {
                "u": u, "fq": fq, "exq": ex, "exgradq": exg, "uq": uq, "gradq": gq,
                "loads": em.element_loads_points(X, e2v, fq, vdim=vdim, elem_ptr=ep),
                "loads_coef": em.element_loads_points(X, e2v, fq, vdim=vdim, coef=w["coef"], elem_ptr=ep),
                "errors": em.element_errors(X, e2v, u, ex, exg, vdim=vdim, elem_ptr=ep),
                "errors_l2": em.element_errors(X, e2v, u, ex, None, vdim=vdim, elem_ptr=ep),
                "errors_h1": em.element_errors(X, e2v, u, None, exg, vdim=vdim, elem_ptr=ep),
            }
        for v in list(w.values()) + [a for vdim in (1, dim) for a in w[vdim].values()]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[key] = w
    return _want[key]


def _same(got, want, what):
    got = _host(got)
    assert got.shape == want.shape and np.array_equal(got, want), what


def _info(X, e2v, ep, NQ):
    dim = X.shape[1]
    return em.type_counts(dim, e2v, ep) + [NQ, -1, em.order2_count(dim, e2v, ep)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,moved", CASES, ids=IDS)
def test_device_equals_model(name, moved, device):
    X, e2v, ep = _mesh(name, moved)
    w = _model(name, moved)
    dim = X.shape[1]
    dev = _cuda if device else (lambda a: a)
    dX, dv, dp = dev(X), dev(e2v), dev(ep)
    live = capi.memory_stats()[0]
    qp, xq, wdet = capi.element_points(dX, dv, elem_ptr=dp, device=device)
    assert str(qp.dtype).endswith("int64")
    _same(qp, w["qp_ptr"], "qp_ptr")
    _same(xq, w["xq"], "xq")
    _same(wdet, w["wdet"], "wdet")
    NQ = int(w["qp_ptr"][-1])
    assert capi.element_points(dX, dv, elem_ptr=dp, sizes_only=True) == _info(X, e2v, ep, NQ)
    for vdim in (1, dim):
        m = w[vdim]
        du = dev(m["u"])
        uq, gq = capi.element_eval(dX, dv, du, vdim=vdim, elem_ptr=dp, device=device)
        _same(uq, m["uq"], "uq")
        _same(gq, m["gradq"], "gradq")
        want = m["loads"] if ep is not None else m["loads"].reshape(len(e2v), -1)
        _same(capi.element_loads_points(dX, dv, dev(m["fq"]), vdim=vdim, elem_ptr=dp, device=device), want, "loads")
        got = capi.element_loads_points(dX, dv, dev(m["fq"]), vdim=vdim, coef=dev(w["coef"]), elem_ptr=dp, device=device)
        _same(got, m["loads_coef"].reshape(want.shape), "loads with coef")
        for tag, ex, exg in (("errors", m["exq"], m["exgradq"]), ("errors_l2", m["exq"], None), ("errors_h1", None, m["exgradq"])):
            got = capi.element_errors(dX, dv, du, dev(ex), dev(exg), vdim=vdim, elem_ptr=dp, device=device)
            _same(got, m[tag], tag)
            assert (_host(got) >= 0.0).all()
        again = capi.element_eval(dX, dv, du, vdim=vdim, elem_ptr=dp, device=device)      # a repeated call: the same bits
        assert np.array_equal(_host(again[0]), _host(uq)) and np.array_equal(_host(again[1]), _host(gq))
    del qp, xq, wdet, uq, gq, got, again, du, dX, dv, dp
    assert capi.memory_stats()[0] == live                           # every temporary is back in the pool


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,moved", [("hex8", True), ("mixed:2d", True)], ids=["hex8", "mixed2d"])
def test_every_combination_of_null_outputs(name, moved, device):
    X, e2v, ep = _mesh(name, moved)
    w = _model(name, moved)
    dim = X.shape[1]
    dev = _cuda if device else (lambda a: a)
    dX, dv, dp = dev(X), dev(e2v), dev(ep)
    NQ = int(w["qp_ptr"][-1])
    names = ("qp_ptr", "xq", "wdet")
    for r in range(4):
        for want in itertools.combinations(names, r):
            got = capi.element_points(dX, dv, elem_ptr=dp, device=device, want=want)
            for k, g in zip(names, got):
                if k in want:
                    _same(g, w[k], (want, k))
                else:
                    assert g is None
    m = w[dim]
    for want in ((), ("uq",), ("gradq",), ("uq", "gradq")):
        got = capi.element_eval(dX, dv, dev(m["u"]), vdim=dim, elem_ptr=dp, device=device, want=want)
        for k, g in zip(("uq", "gradq"), got):
            if k in want:
                _same(g, m[k], (want, k))
            else:
                assert g is None
    # all outputs NULL: the mesh is checked and info is filled
    info = (capi.C.c_longlong * 8)()
    NE = ec.num_elements(e2v, ep)
    nde = 0 if ep is not None else e2v.shape[1]
    assert capi.load().saamge_amd_element_eval(len(X), dim, capi._ptr(dX), NE, nde, capi._ptr(dp), capi._ptr(dv), dim,
                                               capi._ptr(dev(m["u"])), None, None, None, info) == 0
    assert [int(v) for v in info] == _info(X, e2v, ep, NQ)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_one_element_and_none(device):
    X, e2v, _ = cs.mesh("hex8", True)
    dev = _cuda if device else (lambda a: a)
    u = cs.nodal(X, 3)
    one = np.ascontiguousarray(e2v[5:6])
    qp, xq, wdet = capi.element_points(dev(X), dev(one), device=device)
    mq, mx, mw = em.element_points(X, one)
    _same(qp, mq, "qp_ptr")
    _same(xq, mx, "xq")
    _same(wdet, mw, "wdet")
    uq, gq = capi.element_eval(dev(X), dev(one), dev(u), vdim=3, device=device)
    _same(uq, em.element_eval(X, one, u, vdim=3)[0], "uq")
    _same(gq, em.element_eval(X, one, u, vdim=3)[1], "gradq")
    _same(capi.element_loads_points(dev(X), dev(one), dev(mx), vdim=3, device=device), em.element_loads_points(X, one, mx, vdim=3), "loads")
    _same(capi.element_errors(dev(X), dev(one), dev(u), dev(mx), None, vdim=3, device=device), em.element_errors(X, one, u, mx, None, vdim=3),
          "errors")
    none = np.zeros((0, 8), np.int32)
    qp, xq, wdet = capi.element_points(dev(X), dev(none), device=device)
    assert _host(qp).tolist() == [0] and _host(xq).shape == (0, 3) and _host(wdet).shape == (0,)
    assert capi.element_points(dev(X), dev(none), sizes_only=True) == [0, 0, 0, 0, 0, 0, -1, 0]
    uq, gq = capi.element_eval(dev(X), dev(none), dev(u), vdim=3, device=device)
    assert _host(uq).shape == (0, 3) and _host(gq).shape == (0, 3, 3)
    assert _host(capi.element_loads_points(dev(X), dev(none), dev(np.zeros(1)), device=device)).size == 0
    assert _host(capi.element_errors(dev(X), dev(none), dev(u[:, 0].copy()), device=device)).shape == (0, 2)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals_write_nothing(device):
    import torch
    X, t2v, _ = ec.mesh("tets_3x2x2", True)
    NE, NV = len(t2v), len(X)
    flipped = t2v.copy()
    flipped[[3, 50], 0], flipped[[3, 50], 1] = t2v[[3, 50], 1], t2v[[3, 50], 0]          # two vertices exchanged
    dev = _cuda if device else (lambda a: a)
    NQ = 4 * NE
    u, fq = np.ones(NV), np.ones(NQ)
    live = capi.memory_stats()[0]

    def sentinel(n, dt=np.float64):
        a = np.full(n, 7, dt)
        return _cuda(a) if device else a

    def refused(match, call):
        with pytest.raises(RuntimeError, match=match) as err:
            call()
        return err.value.info

    def calls(lists, vdim, with_data):
        """the four calls with sentinel outputs: (name, call, outputs)"""
        dX, dv = dev(X), dev(lists)
        du, df = (dev(u), dev(fq)) if with_data else (None, None)
        o = {k: sentinel(n) for k, n in (("xq", NQ * 3), ("wdet", NQ), ("uq", NQ * vdim), ("gradq", NQ * vdim * 3),
                                         ("elvec", NE * 4 * vdim), ("err", NE * 2))}
        o["qp_ptr"] = sentinel(NE + 1, np.int64)
        return [
            ("points", lambda: capi.element_points(dX, dv, device=device, out=o), [o["qp_ptr"], o["xq"], o["wdet"]]),
            ("eval", lambda: capi.element_eval(dX, dv, du, vdim=vdim, device=device, out=o), [o["uq"], o["gradq"]]),
            ("loads_points", lambda: capi.element_loads_points(dX, dv, df, vdim=vdim, device=device, out=o["elvec"]), [o["elvec"]]),
            ("errors", lambda: capi.element_errors(dX, dv, du, dev(fq), None, vdim=vdim, device=device, out=o["err"]), [o["err"]]),
        ]
    out_of_range = np.where(t2v == 7, NV, t2v).astype(np.int32)
    for name, call, outs in calls(out_of_range, 2, False):
        refused("out of range" if name == "points" else "vdim must be 1 or dim", call)      # vdim before the mesh and the data
        assert all((_host(a) == 7).all() for a in outs)
    for name, call, outs in calls(out_of_range, 1, False):
        refused("out of range", call)                                                       # the mesh before the data
        assert all((_host(a) == 7).all() for a in outs)
    for name, call, outs in calls(flipped, 1, False):
        if name == "points":
            continue
        refused("null argument: %s" % ("fq" if name == "loads_points" else "u"), call)      # the data before the determinants
        assert all((_host(a) == 7).all() for a in outs)
    for name, call, outs in calls(flipped, 1, True):
        info = refused("element 3: the Jacobian determinant is not positive", call)
        assert info[6] == 3 and info[2] == NE and info[5] == NQ, name
        assert all((_host(a) == 7).all() for a in outs), name
    del outs, call
    if device:
        torch.cuda.synchronize()
    assert capi.memory_stats()[0] == live


def test_chain_on_device_pointers_equals_the_chain_on_the_model():
    """jittered hex_5x4x3 -> one level of refinement -> points -> fq = f(xq) with torch on the device -> loads_points ->
    assemble_rhs: the right-hand side equals, bit for bit, that of the same chain fed the model's arrays from the host; then
    operator -> hierarchy -> PCG as in the refinement's chain test, and element_errors of the solution equal the model's on the
    same solution vector."""
    import torch
    X0, e2v0, _ = ec.mesh("hex_5x4x3", True)
    e2v0 = np.ascontiguousarray(e2v0, np.int32)
    want = rm.MeshRefine(X0.shape[0], 3, X0, e2v0, levels=1)
    NE, NV = want.NE, want.NV

    def source(x):          # single IEEE operations in a fixed order: the same bits from torch on the device and from numpy
        t = x[:, 0] * x[:, 1]
        return (t + x[:, 2]) + 1.0

    def solve(dX, dp, dv, fq, device):
        dev = _cuda if device else (lambda a: a)
        elvec = capi.element_loads_points(dX, dv, fq, elem_ptr=dp, device=device)
        elmat = capi.element_matrices(dX, dv, 0, dev(np.ones(NE)), elem_ptr=dp, device=device)
        with capi.FaceTable(NV, 3, dv, elem_ptr=dp) as T:
            be, bl = T.get(device=device)[3:5]
            flags = torch.zeros(NV, dtype=torch.int8, device="cuda") if device else np.zeros(NV, np.int8)
            capi.face_dofs(NV, 3, dv, be, bl, flags, flag=0x02, elem_ptr=dp)
        op = capi.Operator(NV, dv, elmat, flags, elem_ptr=dp)
        h = None
        try:
            b = op.assemble_rhs(elvec, device=device)
            rhs = _host(b).copy()
            op.eliminate_rhs(elmat, torch.zeros(NV, dtype=torch.float64, device="cuda") if device else np.zeros(NV), b)
            parts = [torch.arange(NE, dtype=torch.int32, device="cuda") >> 3] if device else [(np.arange(NE) >> 3).astype(np.int32)]
            prob = pr.Problem(elem_to_dof=dv, elmat=elmat, bdr=flags, partitions=parts, elem_ptr=dp)
            h = capi.Hierarchy.from_operator(prob, op, capi.default_params(num_coarsenings=1))
            x, it, conv, hist = h.pcg(b, x=torch.zeros_like(b), rel_tol=1e-8) if device else h.pcg(b, rel_tol=1e-8)
            return _host(elvec), rhs, x, it, conv, np.asarray(hist)
        finally:
            if h is not None:
                h.close()
            op.close()
    mq, mx, mw = em.element_points(want.coords, want.elem_to_vertex, want.elem_ptr)
    with capi.MeshRefine(_cuda(X0), _cuda(e2v0), levels=1) as R:
        dX, dp, dv = R.pointer("coords"), R.get(device=True)[1], R.pointer("elem_to_vertex")
        qp, xq, wdet = capi.element_points(dX, dv, elem_ptr=dp, device=True)
        assert xq.is_cuda and np.array_equal(_host(xq), mx) and np.array_equal(_host(wdet), mw) and np.array_equal(_host(qp), mq)
        fq = source(xq)
        assert fq.is_cuda and np.array_equal(_host(fq), source(mx))
        elvec_d, rhs_d, xd, itd, convd, histd = solve(dX, dp, dv, fq, True)
        exact = torch.sin(xq[:, 0])                                    # any data at the points: the same array goes to the model
        err_d = capi.element_errors(dX, dv, xd, exact, None, elem_ptr=dp, device=True)
        assert err_d.is_cuda
    # the model's arrays, fed from the host
    elvec = em.element_loads_points(want.coords, want.elem_to_vertex, source(mx), elem_ptr=want.elem_ptr)
    assert np.array_equal(elvec_d, elvec)
    assert np.array_equal(rhs_d, am.assemble_rhs(NV, want.elem_ptr, want.elem_to_vertex, elvec))
    elvec_g, rhs_g, xg, itg, convg, histg = solve(want.coords, want.elem_ptr, want.elem_to_vertex, source(mx), False)
    assert np.array_equal(elvec_g, elvec) and np.array_equal(rhs_g, rhs_d)
    assert convd and convg and itd == itg
    assert np.array_equal(histd, histg) and np.array_equal(_host(xd), xg)
    err = em.element_errors(want.coords, want.elem_to_vertex, xg, _host(exact), None, elem_ptr=want.elem_ptr)
    assert np.array_equal(_host(err_d), err)
    print("PCG iterations %d, sum of column 0: %.6e" % (itd, err[:, 0].sum()))
