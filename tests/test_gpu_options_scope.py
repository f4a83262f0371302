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
