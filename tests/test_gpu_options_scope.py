"""saamge_amd_options belong to the hierarchy they were given to (saamge_amd_params.options), not to the process:
a hierarchy keeps the options it was built with for its whole life, building one does not alter the default that
saamge_amd_get_options returns, and out-of-range values are refused before anything is built.  Through the C ABI."""
import ctypes as C

import numpy as np
import pytest

from saamge_amd import capi


def _problem():
    from saamge_amd import problems as pr
    return pr.poisson3d_device((64, 64, 32), blk=(8, 8, 4), coarse_blk=[(8, 8, 4)], device="cuda:0")


def _build(prob, params):
    return capi.Hierarchy(prob.rowptr, prob.col, prob.val, prob.n, prob.elem_to_dof, prob.elmat, prob.bdr,
                          prob.partitions, prob.nparts, params, prob.NE_, 8)


def _options_dict(o):
    return {f: getattr(o, f) for f, _ in capi.Options._fields_}


@pytest.mark.gpu
def test_a_hierarchy_keeps_its_options():
    """h1 is built with the default SELL formats (sell = 31).  Then the default is changed to sell = 0, overlap = 0 and a
    second hierarchy h2 is built with it (plain slices only).  update_operators on h1 rebuilds h1's SELL copies: with h1's
    OWN options, so its operator format and its V-cycle (bitwise) are what they were."""
    import torch
    prob = _problem()
    old = capi.get_options()
    assert old.sell == 31
    h1 = h2 = None
    try:
        h1 = _build(prob, capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3))
        assert h1.num_levels == 3
        fmt1 = h1.level_format(0)
        assert fmt1["slices"]["pair_coded"] + fmt1["slices"]["offset_coded"] > 0
        torch.manual_seed(20260)
        b = torch.randn(prob.n, dtype=torch.float64, device="cuda:0")
        y1 = h1.vcycle(b, torch.zeros_like(b)).clone()

        capi.set_options(sell=0, overlap=0)
        h2 = _build(prob, capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3))
        fmt2 = h2.level_format(0)
        assert fmt2["slices"]["pair_coded"] == 0 and fmt2["slices"]["offset_coded"] == 0 and fmt2["slices"]["plain"] > 0

        h1.update_operators()          # (the values unchanged)
        assert h1.level_format(0) == fmt1
        y = h1.vcycle(b, torch.zeros_like(b))
        assert torch.equal(y, y1)
    finally:
        capi.load().saamge_amd_set_options(C.byref(old))
        for h in (h1, h2):
            if h is not None:
                h.close()


def _format(h):
    return {k: v for k, v in h.level_format(0).items() if k != "eigenproblems_solved"}


@pytest.mark.gpu
def test_rebuild_inherits_nothing():
    """update_operators rebuilds the SELL copy of every level operator in place.  Here the rebuild CHANGES the format:
    from the constant-coefficient stencil (pair-coded slices, staged tiles, row patterns) to A' = diag(d) A diag(d) with
    all d different (no two entries of a slice share an (offset, value) pair: no pair codes, no staging plan) and back.
    After each rebuild the format census and the level-0 smoother (bitwise) are those of a hierarchy built on that
    operator directly: nothing of the previous copy is left.

    32 x 32 x 16 nodes: 16 384 dofs, 64 tiles of 256 rows and no partial last slice -- a slice of fewer than 64 rows
    could still fit its distinct pairs into a table of 64, and every full one has 64 different diagonal entries alone."""
    import torch
    from saamge_amd import problems as pr
    prob = pr.poisson3d_device((31, 31, 15), blk=(8, 8, 4), device="cuda:0")
    assert prob.n % 256 == 0
    params = capi.default_params(num_coarsenings=1, theta=0.003, nu_relax=3)
    torch.manual_seed(20261)
    b = torch.randn(prob.n, dtype=torch.float64, device="cuda:0")
    h = h2 = None
    try:
        h = _build(prob, params)
        fmt_rich = _format(h)
        print("rich:", fmt_rich)
        assert fmt_rich["slices"]["pair_coded"] > 0 and fmt_rich["staged_tiles"] > 0
        y_rich = h.smoother(0, b, torch.zeros_like(b)).clone()

        A = h.get_csr(0, "A")
        d = 1.0 + np.arange(prob.n) / prob.n
        rows = np.repeat(np.arange(prob.n), np.diff(A.indptr))
        val2 = A.data * d[rows] * d[A.indices]
        h.update_operators(val2)
        fmt_poor = _format(h)
        print("poor:", fmt_poor)
        assert fmt_poor["slices"]["pair_coded"] == 0 and fmt_poor["staged_tiles"] == 0
        assert np.array_equal(A.indices, prob.col.cpu().numpy())      # (get_csr returns the operator in the order it was given)
        prob2 = pr.Problem(**dict(prob.__dict__, val=torch.from_numpy(val2).to("cuda:0")))
        h2 = _build(prob2, params)
        assert _format(h2) == fmt_poor
        assert torch.equal(h.smoother(0, b, torch.zeros_like(b)), h2.smoother(0, b, torch.zeros_like(b)))

        h.update_operators(A.data)
        assert _format(h) == fmt_rich
        assert torch.equal(h.smoother(0, b, torch.zeros_like(b)), y_rich)
    finally:
        for hh in (h, h2):
            if hh is not None:
                hh.close()


@pytest.mark.gpu
def test_building_does_not_leak_into_the_default():
    prob = _problem()
    before = _options_dict(capi.get_options())
    params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3)
    params.options.eig_dedupe = 1 - before["eig_dedupe"]
    params.options.sell = before["sell"] ^ 2
    h = _build(prob, params)
    try:
        assert _options_dict(capi.get_options()) == before
    finally:
        h.close()


@pytest.mark.parametrize("field,value", [
    ("eig_outer_panels", 1), ("sell", 1 << 7), ("overlap", 16), ("debug", 8), ("eig_min_n", -1),
    ("host_heap_pad_mb", -1), ("eig_strict", 2)])
def test_bad_option_values_are_refused(field, value):
    """Validation comes before the first use of the device or of the inputs: no GPU needed, a 2 x 2 identity is enough."""
    lib = capi.load()
    before = _options_dict(capi.get_options())
    params = capi.default_params()
    setattr(params.options, field, value)
    rowptr = np.array([0, 1, 2], dtype=np.int32)
    col = np.array([0, 1], dtype=np.int32)
    val = np.ones(2)
    e2d = np.array([0, 1], dtype=np.int32)
    elmat = np.eye(2).ravel()
    part = np.zeros(1, dtype=np.int32)
    parts = (C.c_void_p * 1)(part.ctypes.data)
    nparts = (C.c_int * 1)(1)
    h = C.c_void_p()
    rc = lib.saamge_amd_ml_produce_data(C.c_int(2), capi._ptr(rowptr), capi._ptr(col), capi._ptr(val), C.c_int(1), C.c_int(2),
                                        capi._ptr(e2d), capi._ptr(elmat), capi._ptr(None), parts, nparts, C.byref(params),
                                        C.c_void_p(0), C.byref(h))
    assert rc != 0
    assert not h.value
    assert field in lib.saamge_amd_last_error().decode()
    assert _options_dict(capi.get_options()) == before
