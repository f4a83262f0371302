"""The operator assembled on the device (csrc/operator.hip) against its definition (saamge_amd/assemble_model.py), bit for
bit: pattern and values on four meshes with host and device inputs, every row path, the numeric-only update, the
right-hand-side elimination, hierarchies built on the operator in place, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from saamge_amd import assemble_model as am
from saamge_amd import capi
from saamge_amd import problems as pr

import partition_cases as pc

pytestmark = pytest.mark.gpu

CASES = {
    "hex_5x4x3": lambda: pr.poisson3d_problem((5, 4, 3), blk=(2, 2, 2)),
    "mixed_4": lambda: pr.poisson3d_mixed_problem(4, (2, 2, 2), wedges="half"),
    "q2_elasticity_2": lambda: pr.elasticity3d_q2_problem(2, blk=(2, 2, 2)),
    "mltest": lambda: pr.mltest_problem(),
}
_probs, _models = {}, {}


def scaled(prob, seed):
    """prob with every element matrix scaled by its own factor in [0.5, 2): a term from the wrong element or the wrong local
    index changes the value"""
    f = np.random.default_rng(seed).uniform(0.5, 2.0, prob.NE)
    ep = getattr(prob, "elem_ptr", None)
    if ep is None:
        elmat = prob.elmat * f[:, None, None]
    else:
        elmat = prob.elmat * np.repeat(f, np.diff(ep).astype(np.int64) ** 2)
    return pr.Problem(**dict(prob.__dict__, elmat=np.ascontiguousarray(elmat)))


def case(name, seed=11):
    if (name, seed) not in _probs:
        if (name, None) not in _probs:
            _probs[(name, None)] = CASES[name]()
        _probs[(name, seed)] = scaled(_probs[(name, None)], seed)
    return _probs[(name, seed)]


def model_of(prob, key=None):
    if key is None or key not in _models:
        m = am.assemble(prob.ND, getattr(prob, "elem_ptr", None), prob.elem_to_dof, prob.elmat, prob.bdr)
        if key is None:
            return m
        _models[key] = m
    return _models[key]


def assert_equal_to_model(op, model):
    rowptr, col, val = op.get()
    assert rowptr.dtype == np.int64 and np.array_equal(rowptr, model[0])
    assert np.array_equal(col, model[1])
    assert np.array_equal(val, model[2])
    assert op.nnz == len(model[1])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_model(name, device):
    prob = case(name)
    op = capi.Operator.assemble(prob, device=device)
    try:
        assert_equal_to_model(op, model_of(prob, (name, 11)))
        if device:
            d = op.get(device=True)
            assert all(np.array_equal(t.cpu().numpy(), m) for t, m in zip(d, model_of(prob, (name, 11))))
        paths, n = op.path_counts(), prob.ND
        assert sum(paths["symbolic"]) == n and sum(paths["numeric"]) == n
        if name == "q2_elasticity_2":          # 81 .. 648 candidates per row: one workgroup per row, in LDS
            assert paths["symbolic"] == (0, n, 0) and paths["numeric"] == (0, n, 0)
        if name in ("hex_5x4x3", "mltest"):    # at most 64 candidates: several rows per wavefront
            assert paths["symbolic"] == (n, 0, 0) and paths["numeric"] == (n, 0, 0)
        if name == "mixed_4":                  # inner vertices of split columns lie in up to 12 elements: up to 80 candidates
            assert paths["symbolic"][0] > 0 and paths["symbolic"][1] > 0 and paths["symbolic"][2] == 0
    finally:
        op.close()


def test_element_order_is_ascending_element_id():
    """The mixed mesh with its elements permuted: the terms of an entry are added in the NEW order of the elements."""
    prob = case("mixed_4")
    seed = 3
    ep, e2d, ND = pc.permuted((prob.elem_ptr.astype(np.int32), prob.elem_to_dof.astype(np.int32), prob.ND), seed)
    perm = np.random.default_rng(seed).permutation(prob.NE)
    nd2 = np.diff(prob.elem_ptr).astype(np.int64) ** 2
    moff = np.concatenate([[0], np.cumsum(nd2)])
    elmat = np.concatenate([prob.elmat[moff[e]:moff[e + 1]] for e in perm])
    part = prob.partitions[0][perm]             # (what a hierarchy on the permuted mesh would take; not an input here)
    assert len(part) == prob.NE
    model = am.assemble(ND, ep, e2d, elmat, prob.bdr)
    base = model_of(prob, ("mixed_4", 11))
    assert np.array_equal(model[0], base[0]) and np.array_equal(model[1], base[1])
    assert not np.array_equal(model[2], base[2]), "the permutation changes no rounding: the case shows nothing"
    op = capi.Operator(ND, e2d, elmat, prob.bdr, elem_ptr=ep)
    try:
        assert_equal_to_model(op, model)
    finally:
        op.close()


@pytest.mark.parametrize("limits,sym,num", [((0, -1), 1, 1), ((0, 0), 2, 2), ((-1, 0), None, None)],
                         ids=["all_lds", "all_global", "short_or_global"])
@pytest.mark.parametrize("name", ["mixed_4", "q2_elasticity_2"])
def test_every_row_path_gives_the_model(name, limits, sym, num):
    prob = case(name)
    capi.operator_path_limits(*limits)
    try:
        op = capi.Operator.assemble(prob)
    finally:
        capi.operator_path_limits()
    try:
        paths, n = op.path_counts(), prob.ND
        if sym is not None:
            assert paths["symbolic"][sym] == n and paths["numeric"][num] == n
        else:
            assert paths["symbolic"][1] == 0 and paths["symbolic"][2] > 0 and paths["numeric"][2] > 0
        assert_equal_to_model(op, model_of(prob, (name, 11)))
        x = np.random.default_rng(5).standard_normal(n)
        b = np.random.default_rng(6).standard_normal(n)
        want = am.eliminate_rhs(n, getattr(prob, "elem_ptr", None), prob.elem_to_dof, prob.elmat, prob.bdr, x, b)
        assert np.array_equal(op.eliminate_rhs(prob.elmat, x, b.copy()), want)
    finally:
        op.close()


def test_path_limits_are_bounded():
    with pytest.raises(RuntimeError, match="path limits"):
        capi.operator_path_limits(65, -1)
    with pytest.raises(RuntimeError, match="path limits"):
        capi.operator_path_limits(-1, 4097)


@pytest.mark.parametrize("name", sorted(CASES))
def test_update_runs_the_numeric_pass_only(name):
    import torch
    prob, prob2 = case(name), case(name, seed=12)
    op = capi.Operator.assemble(prob)
    try:
        before = op.arrays()
        pattern = op.get()[:2]
        want = model_of(prob2, (name, 12))
        assert not np.array_equal(want[2], model_of(prob, (name, 11))[2])
        dev = torch.as_tensor(np.ascontiguousarray(prob2.elmat)).cuda()
        torch.cuda.synchronize()
        capi.pool_counts(reset=True)
        op.update(dev)
        assert capi.pool_counts()[0] == 0, "the numeric pass went to the driver for memory"
        assert op.arrays() == before
        assert_equal_to_model(op, want)
        op.update(prob.elmat)                  # back, from host memory
        assert op.arrays() == before
        assert_equal_to_model(op, model_of(prob, (name, 11)))
        got = op.get()
        assert np.array_equal(got[0], pattern[0]) and np.array_equal(got[1], pattern[1])
    finally:
        op.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_eliminate_rhs_equals_model(name):
    import torch
    prob = case(name)
    n = prob.ND
    rng = np.random.default_rng(21)
    x, b = rng.standard_normal(n), rng.standard_normal(n)
    want = am.eliminate_rhs(n, getattr(prob, "elem_ptr", None), prob.elem_to_dof, prob.elmat, prob.bdr, x, b)
    assert not np.array_equal(want, b)
    op = capi.Operator.assemble(prob)
    try:
        host = b.copy()
        op.eliminate_rhs(prob.elmat, x, host)
        assert np.array_equal(host, want)
        db = torch.as_tensor(b.copy()).cuda()
        op.eliminate_rhs(torch.as_tensor(np.ascontiguousarray(prob.elmat)).cuda(), torch.as_tensor(x).cuda(), db)
        assert np.array_equal(db.cpu().numpy(), want)
    finally:
        op.close()


def test_no_flags_means_no_elimination():
    prob = case("hex_5x4x3")
    op = capi.Operator(prob.ND, np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32), prob.elmat, None)
    try:
        assert_equal_to_model(op, am.assemble(prob.ND, None, prob.elem_to_dof, prob.elmat, None))
        b = np.arange(prob.ND, dtype=np.float64)
        assert np.array_equal(op.eliminate_rhs(prob.elmat, np.ones(prob.ND), b.copy()), b)
    finally:
        op.close()


# ---- hierarchies on the operator in place ----
def _hier_cases():
    return {
        "mltest_3_levels": (lambda: pr.mltest_problem(levels=3), dict(num_coarsenings=2, testmesh=True)),
        "poisson_8_2_levels": (lambda: pr.poisson3d_problem(8, blk=(4, 4, 4)), dict(num_coarsenings=1)),
    }


def _from_model(prob, model, params):
    """the existing constructor given the model's matrix (64-bit offsets, host arrays)"""
    e2d = np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32)
    parts = [np.ascontiguousarray(p, dtype=np.int32) for p in prob.partitions[:params.num_coarsenings]]
    return capi.Hierarchy(model[0], model[1], model[2].copy(), prob.ND, e2d, np.ascontiguousarray(prob.elmat),
                          np.ascontiguousarray(prob.bdr, dtype=np.int8), parts, [int(p.max()) + 1 for p in parts], params,
                          e2d.shape[0], e2d.shape[1])


def _assert_same_hierarchy(h, g, b):
    assert h.num_levels == g.num_levels
    for lev in range(h.num_levels - 1):
        assert h.level_info(lev) == g.level_info(lev)
        Ah, Ag = h.get_csr(lev, "Ac"), g.get_csr(lev, "Ac")
        assert np.array_equal(Ah.indptr, Ag.indptr) and np.array_equal(Ah.indices, Ag.indices)
        assert np.array_equal(Ah.data, Ag.data)
    xh, ih, ch, hh = h.pcg(b, rel_tol=1e-8)
    xg, ig, cg, hg = g.pcg(b, rel_tol=1e-8)
    assert ch and cg and ih == ig
    assert np.array_equal(hh, hg) and np.array_equal(xh, xg)


@pytest.mark.parametrize("name", sorted(_hier_cases()))
def test_hierarchy_on_the_operator_in_place(name):
    make, pk = _hier_cases()[name]
    prob = scaled(make(), 31)
    prob2 = scaled(prob, 32)
    op = capi.Operator.assemble(prob)
    h = g = None
    try:
        model = model_of(prob)
        assert_equal_to_model(op, model)
        h = capi.Hierarchy.from_operator(prob, op, capi.default_params(**pk))
        g = _from_model(prob, model, capi.default_params(**pk))
        assert h.num_levels == pk["num_coarsenings"] + 1
        _assert_same_hierarchy(h, g, prob.b)
        # a coefficient change: the numeric pass rewrites the values the hierarchy already points at
        model2 = model_of(prob2)
        op.update(prob2.elmat)
        h.update_operators(None)
        g.update_operators(model2[2])
        _assert_same_hierarchy(h, g, prob.b)
        A0 = h.get_csr(0, "A")
        assert np.array_equal(A0.data, model2[2])
    finally:
        for x in (h, g):
            if x is not None:
                x.close()
        op.close()


# ---- refusals: all from the bounded checks that run before the kernels ----
def _assemble_raw(n, ep, e2d, elmat, nde=0):
    lib = capi.load()
    h = C.c_void_p()
    rc = lib.saamge_amd_operator_assemble(C.c_int(n), C.c_int(len(ep) - 1), C.c_int(nde), capi._ptr(ep), capi._ptr(e2d),
                                          capi._ptr(elmat), None, None, C.byref(h))
    err = lib.saamge_amd_last_error().decode()
    if rc == 0:
        free = lib.saamge_amd_operator_free
        free.restype = None
        free(h)
    return rc, err


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("what,match", [("twice", "lists a dof twice"), ("range", "out of range"), ("start", "must start at 0"),
                                        ("empty", "every element needs a dof"), ("orphan", "dof 3 lies in no element")])
def test_refusals(what, match, device):
    ep = np.array([0, 3, 6], np.int32)
    e2d = np.array([0, 1, 2, 2, 1, 4], np.int32)          # dof 3 of n = 5 is in no element
    if what == "twice":
        e2d[4] = 2
    elif what == "range":
        e2d[5] = 5
    elif what == "start":
        ep = np.array([1, 3, 6], np.int32)
    elif what == "empty":
        ep = np.array([0, 3, 3], np.int32)
    elmat = np.ones(18)
    if device:
        import torch
        ep, e2d, elmat = (torch.as_tensor(a).cuda() for a in (ep, e2d, elmat))
    rc, err = _assemble_raw(5, ep, e2d, elmat)
    assert rc != 0 and match in err, (rc, err)
    if what == "orphan":                                   # the same mesh with the dof in an element is taken
        ok = np.array([0, 1, 2, 2, 1, 4, 3], np.int32)
        rc, err = _assemble_raw(5, np.array([0, 3, 7], np.int32), ok, np.ones(9 + 16))
        assert rc == 0, err
