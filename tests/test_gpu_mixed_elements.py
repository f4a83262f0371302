"""GPU tests of the mixed-element entries (saamge_amd_ml_produce_data_mixed): elements of different numbers of dofs.
Uniform input through them is the existing entry bit for bit; hex / wedge meshes match the oracle (whose building blocks
all take a variable Table) at the parity tolerances of test_gpu_parity.py, take the sparse-row assembly and the device
topology, and keep the bitwise invariants of the uniform path (device inputs, duplicate agglomerates, operator updates).
Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import saamge_oracle as o
from saamge_amd import problems as pr

from test_gpu_parity import EIG_TOL, PROJ_TOL, VCYCLE_TOL, _compare_level  # noqa: F401

pytestmark = pytest.mark.gpu

TABLES = ("AE_to_dof", "dof_to_AE", "mis_to_dof", "mis_to_AE", "AE_to_mis", "elem_to_dof")


def _capi():
    from saamge_amd import capi
    return capi


def _same(a, b):
    """Bitwise equality of nested results (arrays, sparse matrices, lists, tuples, scalars)."""
    if sp.issparse(a):
        return (a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
                and np.array_equal(a.data.view(np.uint64), b.data.view(np.uint64)))
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64 and b.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return a.shape == b.shape and np.array_equal(a, b)


def _snapshot(h, nco, eigens=True):
    out = {}
    for lev in range(nco):
        for t in TABLES:
            out[(lev, t)] = h.get_table(lev, t)
        out[(lev, "mis")] = h.get_mis(lev)
        if eigens:
            out[(lev, "eig")] = h.get_ae_eigens(lev)
        for w in ("P", "R", "Ac"):
            out[(lev, w)] = h.get_csr(lev, w)
    return out


def _assert_same_hierarchy(h1, h2, nco, eigens=True):
    s1, s2 = _snapshot(h1, nco, eigens), _snapshot(h2, nco, eigens)
    for k in s1:
        assert _same(s1[k], s2[k]), k


def _as_mixed(prob):
    """The same problem with flat elem_to_dof, elem_ptr and packed element matrices."""
    NE, nde = prob.elem_to_dof.shape
    return pr.Problem(**dict(prob.__dict__, elem_to_dof=np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32).ravel(),
                             elem_ptr=(np.arange(NE + 1) * nde).astype(np.int32),
                             elmat=np.ascontiguousarray(prob.elmat, dtype=np.float64).ravel()))


def _mixed_oracle(monkeypatch, prob, ncoars, **kw):
    """The oracle on elements of different sizes: only ml_produce_data calls Table.from_fixed; it passes a Table through."""
    orig = o.Table.from_fixed
    monkeypatch.setattr(o.Table, "from_fixed",
                        staticmethod(lambda arr, ncols: arr if isinstance(arr, o.Table) else orig(arr, ncols)))
    e2d = o.Table(prob.elem_ptr, prob.elem_to_dof, prob.ND)
    elmats, off = [], 0
    for e in range(prob.NE):
        nd = int(prob.elem_ptr[e + 1] - prob.elem_ptr[e])
        elmats.append(prob.elmat[off:off + nd * nd].reshape(nd, nd))
        off += nd * nd
    return o.ml_produce_data(prob.A, e2d, elmats, prob.bdr, prob.partitions[:ncoars], **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. uniform elements through the mixed entry: the existing entry's hierarchy, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["poisson", "poisson3", "q2elast", "mltest"])
def test_uniform_input_through_mixed_entry_is_bitwise_the_uniform_path(case):
    capi = _capi()
    testmesh = False
    if case == "poisson":
        prob, nco = pr.poisson3d_problem((12, 8, 4), blk=(4, 4, 2)), 1
    elif case == "poisson3":
        prob, nco = pr.poisson3d_problem((16, 16, 8), blk=(4, 4, 2), coarse_blk=[(2, 2, 2)]), 2
    elif case == "q2elast":
        prob, nco = pr.elasticity3d_q2_problem(8), 1
    else:
        prob, nco, testmesh = pr.mltest_problem(order=1, levels=3), 2, True
    mk = lambda: capi.default_params(num_coarsenings=nco, keep_debug=True, testmesh=testmesh, coarse_rtol=1e-28)
    h1 = capi.Hierarchy.from_problem(prob, mk())
    h2 = capi.Hierarchy.from_problem(_as_mixed(prob), mk())
    _assert_same_hierarchy(h1, h2, nco)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    assert _same(h1.vcycle(b), h2.vcycle(b))
    r1, r2 = h1.pcg(prob.b, rel_tol=1e-8), h2.pcg(prob.b, rel_tol=1e-8)
    assert r1[1] == r2[1] and _same(r1[0], r2[0]) and _same(r1[3], r2[3])
    h1.close()
    h2.close()


def _copied(prob, weights):
    """The same problem with every element listed len(weights) times, copy i carrying weights[i] of its matrix (powers
    of two that sum to 1: the copies of an entry add up to the entry): a dof lies in len(weights) times as many
    elements, every agglomerate keeps its dofs."""
    k = len(weights)
    assert sum(weights) == 1.0 and all(np.frexp(w)[0] == 0.5 for w in weights)
    e2d = np.ascontiguousarray(np.tile(prob.elem_to_dof, (k, 1)))
    elmat = np.ascontiguousarray(np.concatenate([w * prob.elmat for w in weights]))
    A, b = pr._eliminate(pr._assemble(prob.ND, e2d, elmat), prob.b, prob.ess)
    return pr.Problem(**dict(prob.__dict__, A=A, b=b, elem_to_dof=e2d, elmat=elmat,
                             partitions=[np.tile(prob.partitions[0], k)] + list(prob.partitions[1:])))


def _copied_mixed(prob, weights):
    """_copied for a mesh with elements of different sizes (flat elem_to_dof, elem_ptr, packed element matrices)."""
    k = len(weights)
    assert sum(weights) == 1.0 and all(np.frexp(w)[0] == 0.5 for w in weights)
    nd = np.tile(np.diff(prob.elem_ptr).astype(np.int64), k)
    eptr = np.concatenate([[0], np.cumsum(nd)])
    e2d = np.ascontiguousarray(np.tile(prob.elem_to_dof, k))
    elmat = np.ascontiguousarray(np.concatenate([w * prob.elmat for w in weights]))
    moff = np.concatenate([[0], np.cumsum(nd * nd)])
    eid = np.repeat(np.arange(nd.size), nd * nd)        # element of every packed matrix entry, ascending
    loc = np.arange(elmat.size) - moff[eid]
    rows, cols = e2d[eptr[eid] + loc // nd[eid]], e2d[eptr[eid] + loc % nd[eid]]
    A0 = sp.coo_matrix((elmat, (rows, cols)), shape=(prob.ND, prob.ND)).tocsr()
    A0.sort_indices()
    A, b = pr._eliminate(A0, prob.b, prob.ess)
    return pr.Problem(**dict(prob.__dict__, A=A, b=b, elem_to_dof=e2d, elem_ptr=eptr.astype(np.int32), elmat=elmat,
                             partitions=[np.tile(prob.partitions[0], k)] + list(prob.partitions[1:])))


def _max_valence(prob):
    return int(np.bincount(prob.elem_to_dof.ravel(), minlength=prob.ND).max())


def _profiled_hierarchy(capi, prob, params):
    capi.profile(True)
    try:
        capi.profile_reset()
        h = capi.Hierarchy.from_problem(prob, params)
        names = [r["name"] for r in capi.profile_stats() if r["launches"] > 0]
    finally:
        capi.profile(False)
    return h, names


# ---------------------------------------------------------------------------------------------------------------------
# 1b. a dof in more elements than the per-dof element lists of the 8-dof sparse-row kernel hold (8): the agglomerate
#     takes the walk through the dof -> element list instead
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights,valence", [((0.5, 0.5), 16), ((0.5, 0.25, 0.25), 24)])
def test_dof_in_more_elements_than_the_row_lists_hold(weights, valence):
    """Every hex listed two / three times: an interior vertex lies in 16 / 24 elements and the 8-dof kernel walks.  The
    hierarchy is the oracle's on the same copied mesh, and the mixed entry gives it bit for bit -- through the SAME
    kernel: elements of one size continue as the uniform entry (hierarchy_create), so this compares the entries, not
    two kernels.  The walk of the kernel for elements of different sizes is pinned by the next test."""
    capi = _capi()
    prob = _copied(pr.poisson3d_problem((8, 8, 4), blk=(4, 4, 2), coef="skew"), weights)
    assert prob.ND == 405 and _max_valence(prob) == valence
    mk = lambda: capi.default_params(num_coarsenings=1, theta=0.003, nu_relax=3, keep_debug=True, coarse_rtol=1e-28)
    h1 = capi.Hierarchy.from_problem(prob, mk())
    h2 = capi.Hierarchy.from_problem(_as_mixed(prob), mk())
    _assert_same_hierarchy(h1, h2, 1)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    assert _same(h1.vcycle(b), h2.vcycle(b))
    r1, r2 = h1.pcg(prob.b, rel_tol=1e-8), h2.pcg(prob.b, rel_tol=1e-8)
    assert r1[1] == r2[1] and _same(r1[0], r2[0]) and _same(r1[3], r2[3])
    H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:1], theta=0.003, nu_relax=3)
    _compare_level(h1, H, 0, 0.003)
    h1.close()
    h2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1b'. the same for elements of different sizes: hexes and wedges, every element listed twice -- a vertex of the split
#      columns lies in up to 24 elements, more than the 16 the lists of that kernel hold
# ---------------------------------------------------------------------------------------------------------------------
def test_dof_in_more_elements_than_the_mixed_row_lists_hold(monkeypatch):
    capi = _capi()
    prob = _copied_mixed(pr.poisson3d_mixed_problem((8, 8, 4), (4, 4, 2), wedges="half", coef="skew", seed=7), (0.5, 0.5))
    assert set(np.diff(prob.elem_ptr)) == {6, 8}        # (sizes differ: the call stays with the mixed kernels)
    assert prob.ND == 405 and _max_valence(prob) > 16
    params = capi.default_params(num_coarsenings=1, theta=0.003, nu_relax=3, keep_debug=True, coarse_rtol=1e-28)
    h, names = _profiled_hierarchy(capi, prob, params)
    assert "ae_rows" in names, names
    H = _mixed_oracle(monkeypatch, prob, 1, theta=0.003, nu_relax=3)
    _compare_level(h, H, 0, 0.003)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= VCYCLE_TOL * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and it == itr
    assert np.allclose(hist, histr, rtol=1e-7, atol=1e-10 * histr[0])
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1c. agglomerates whose tables do not fit the LDS of the sparse-row kernel: 4 agglomerates of 11 x 11 x 10 = 1 210
#     dofs (93 570 bytes against 64 KB).  The eigenproblem pass takes the generic assembly; the pass that builds the
#     coarse element matrices takes the sparse rows from the kernel with one thread per (row, entry).  That pass runs
#     only where a further level needs element matrices: a second coarsening (the four agglomerates into one).
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(1.0,), (0.5, 0.5)])
def test_agglomerates_too_large_for_the_lds_rows_kernel(weights):
    """(0.5, 0.5): every element twice, an interior vertex in 16 elements -- the kernel's loop over the elements past
    the eighth."""
    capi = _capi()
    prob = pr.poisson3d_problem((20, 20, 9), blk=(10, 10, 9), coarse_blk=[(2, 2, 1)], coef="skew")
    if len(weights) > 1:
        prob = _copied(prob, weights)
    assert _max_valence(prob) == 8 * len(weights)
    assert np.bincount(prob.partitions[0]).size == 4
    params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3, keep_debug=True, coarse_rtol=1e-28)
    h, names = _profiled_hierarchy(capi, prob, params)
    assert "ae_rows" in names and "ae_assemble" in names and "coarse_elmats" in names, names
    H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:2], theta=0.003, nu_relax=3)
    _compare_level(h, H, 0, 0.003)
    _compare_level(h, H, 1, 0.003)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and it == itr, (it, itr)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. hex / wedge meshes against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,blk,wedges", [((8, 8, 4), (4, 4, 2), "half"), ((8, 8, 6), (4, 4, 3), "random"),
                                          ((6, 6, 4), (3, 3, 2), "all")])
def test_hex_wedge_two_level_matches_oracle(monkeypatch, n, blk, wedges):
    """'skew' coefficient: simple local eigenvalues, so the tight tolerances are meaningful."""
    capi = _capi()
    prob = pr.poisson3d_mixed_problem(n, blk, wedges=wedges, coef="skew", seed=7)
    params = capi.default_params(num_coarsenings=1, theta=0.003, nu_relax=3, keep_debug=True, coarse_rtol=1e-28)
    h = capi.Hierarchy.from_problem(prob, params)
    H = _mixed_oracle(monkeypatch, prob, 1, theta=0.003, nu_relax=3)
    _compare_level(h, H, 0, 0.003)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= VCYCLE_TOL * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and it == itr
    assert np.allclose(hist, histr, rtol=1e-7, atol=1e-10 * histr[0])
    h.close()


@pytest.mark.parametrize("wedges", ["half", "random"])
def test_hex_wedge_three_level_matches_oracle(monkeypatch, wedges):
    """Constant coefficient: symmetric agglomerates, a coarse basis that is not unique -- the allowance of
    test_poisson3d_matches_oracle for three levels (5e-2 on the V-cycle, +-1 PCG iteration)."""
    capi = _capi()
    prob = pr.poisson3d_mixed_problem((16, 16, 8), (4, 4, 2), coarse_blk=[(2, 2, 2)], wedges=wedges, seed=3)
    params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3, keep_debug=True, coarse_rtol=1e-28)
    h = capi.Hierarchy.from_problem(prob, params)
    H = _mixed_oracle(monkeypatch, prob, 2, theta=0.003, nu_relax=3)
    for lev in range(2):
        _compare_level(h, H, lev, 0.003, strict=False)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= 5e-2 * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and abs(it - itr) <= 1
    assert np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the sparse-row assembly runs for a hex / wedge mesh
# ---------------------------------------------------------------------------------------------------------------------
def test_hex_wedge_mesh_takes_the_sparse_rows():
    capi = _capi()
    prob = pr.poisson3d_mixed_problem((16, 16, 8), (4, 4, 4), wedges="half")
    params = capi.default_params(num_coarsenings=1, theta=0.003, nu_relax=3)
    capi.profile(True)
    try:
        capi.profile_reset()
        h = capi.Hierarchy.from_problem(prob, params)
        names = [r["name"] for r in capi.profile_stats() if r["launches"] > 0]
    finally:
        capi.profile(False)
    assert "ae_rows" in names, names
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    assert conv and np.linalg.norm(prob.A @ x - prob.b) <= 1e-6 * np.linalg.norm(prob.b)
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. device-resident inputs (CSR device topology) = host inputs, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wedges,nco", [("random", 1), ("half", 2)])
def test_device_inputs_give_the_host_hierarchy(wedges, nco):
    import torch
    capi = _capi()
    prob = pr.poisson3d_mixed_problem((16, 12, 8), (4, 4, 2), coarse_blk=[(2, 2, 2)], wedges=wedges, coef="skew", seed=4)
    mk = lambda: capi.default_params(num_coarsenings=nco, theta=0.003, nu_relax=3, keep_debug=True)
    h_host = capi.Hierarchy.from_problem(prob, mk())
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).cuda()
    dprob = pr.Problem(**dict(prob.__dict__, elem_to_dof=dev(prob.elem_to_dof, np.int32),
                              elem_ptr=dev(prob.elem_ptr, np.int32), elmat=dev(prob.elmat, np.float64),
                              bdr=dev(prob.bdr, np.int8),
                              partitions=[dev(prob.partitions[0], np.int32)] + list(prob.partitions[1:])))
    h_dev = capi.Hierarchy.from_problem(dprob, mk())
    _assert_same_hierarchy(h_host, h_dev, nco)
    h_host.close()
    h_dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. identical agglomerates solved once: the same hierarchy, fewer eigenproblems
# ---------------------------------------------------------------------------------------------------------------------
def test_eig_dedupe_on_a_mixed_mesh_is_bitwise_and_solves_fewer():
    capi = _capi()
    prob = pr.poisson3d_mixed_problem(16, (4, 4, 4), coarse_blk=[(2, 2, 2)], wedges="half")
    nparts = int(prob.partitions[0].max()) + 1
    hs = {}
    for dedupe in (0, 1):
        capi.set_options(eig_dedupe=dedupe)
        try:
            params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3)
            hs[dedupe] = capi.Hierarchy.from_problem(prob, params)
        finally:
            capi.reset_options()
    _assert_same_hierarchy(hs[0], hs[1], 2, eigens=False)
    assert hs[0].level_format(0)["eigenproblems_solved"] == nparts
    assert hs[1].level_format(0)["eigenproblems_solved"] < nparts
    for h in hs.values():
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. update_operators on a mixed hierarchy
# ---------------------------------------------------------------------------------------------------------------------
def test_update_operators_keeps_p_and_rebuilds_ac():
    capi = _capi()
    prob = pr.poisson3d_mixed_problem((12, 12, 8), (4, 4, 2), wedges="random", coef="skew", seed=9)
    params = capi.default_params(num_coarsenings=1, theta=0.003, nu_relax=3)
    h = capi.Hierarchy.from_problem(prob, params)
    P0 = h.get_csr(0, "P")
    A = prob.A.tocsr()
    d = 1.0 + 0.25 * np.sin(np.arange(prob.ND) * 0.71)
    rows = np.repeat(np.arange(prob.ND), np.diff(A.indptr))
    A2 = sp.csr_matrix((A.data * d[rows] * d[A.indices], A.indices, A.indptr), shape=A.shape)    # D A D: same pattern
    h.update_operators(np.ascontiguousarray(A2.data))
    assert _same(h.get_csr(0, "P"), P0)
    Ac = h.get_csr(0, "Ac").toarray()
    Ac_ref = (P0.T @ A2 @ P0).toarray()
    assert np.allclose(Ac, Ac_ref, rtol=0, atol=1e-12 * np.abs(Ac_ref).max())
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. malformed offsets are refused before any launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["first", "decreasing", "empty", "dof_negative", "dof_too_large"])
def test_malformed_elem_ptr_is_an_error(bad):
    capi = _capi()
    prob = pr.poisson3d_mixed_problem((4, 4, 2), (2, 2, 2), wedges="half")
    eptr = prob.elem_ptr.copy()
    e2d = prob.elem_to_dof.copy()
    if bad == "first":
        eptr[0] = 1
    elif bad == "decreasing":
        eptr[3] = eptr[5] + 1
    elif bad == "empty":
        eptr[2] = eptr[1]
    elif bad == "dof_negative":
        e2d[7] = -1
    else:
        e2d[-1] = prob.ND
    badprob = pr.Problem(**dict(prob.__dict__, elem_ptr=eptr, elem_to_dof=e2d))
    params = capi.default_params(num_coarsenings=1)
    with pytest.raises(RuntimeError, match="elem_ptr|elem_to_dof"):
        capi.Hierarchy.from_problem(badprob, params)
    h = capi.Hierarchy.from_problem(prob, params)       # the library is still usable
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    assert conv
    h.close()
