"""GPU tests of the sparse-row kernel's per-dof element lists (ae_rows_lds_kernel, csrc/assemble.hip): the lists are made for the
dofs shared between agglomerates only, several items of the chain of dependent loads per thread and trip.

The model.  get_ae_eigens returns per agglomerate the weights D of its rows.  D is not the matrix diagonal itself: the
fused build kernel makes it from the agglomerate's sparse rows as D[r] = sum over the row's slots k, in slot order, of
|a_rk| sqrt(d_r / d_c(k)) (each term added by one fused multiply-add; d = the diagonal entries).  So the model below restates
the ENTRY RULE for every entry of every row -- for two shared dofs (bit 0 of both flags, and no essential dof unless on the
diagonal) the sum over the row dof's elements inside the agglomerate that also hold the column dof, in ascending position of
its dof -> element list, of elmat_e[slot of row, slot of column], starting from 0.0; any other entry is A's -- and then the
weights from those entries with exactly rounded operations.  D must equal it bit for bit: a wrong element, slot, order or a
list missing for a shared dof changes an assembled diagonal or off-diagonal entry and with it the bits of D.

Which instantiation a case takes: the all-hex cases (hex_ess, hex_free, one_part, part_per_element, valence_*) take
ae_rows_lds_kernel<true>, also through the mixed entry -- elements of one size continue as the uniform entry, so
test_uniform_hexes_through_the_mixed_entry_... compares the two entries, not two kernels.  hex_wedge (lists of at most 12) and
hex_wedge_walk (every element twice: a shared dof in up to 24 elements, more than the 16 a list holds, so the walk) take <false>.

"bdr=None" of the all-hex case is spelled as flags without the essential bit (hex_free): the uniform entry of the Python layer
wants an array, and to the kernel the two are the same -- the dofs' flags then carry bit 0 only.  A multiple of the identity is
added to the element matrices there, so that the operator without essential dofs stays definite for the solve.

Random element-matrix factors as in tests/test_gpu_assemble.py::scaled.  Run with `pytest -m gpu` on an MI355X."""
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import saamge_oracle as o
from saamge_amd import problems as pr

from test_gpu_assemble import scaled
from test_gpu_mixed_elements import _as_mixed, _assert_same_hierarchy, _copied_mixed, _mixed_oracle, _same
from test_gpu_parity import VCYCLE_TOL, _compare_level

pytestmark = pytest.mark.gpu

THETA = 0.003


def _capi():
    from saamge_amd import capi
    return capi


def _params(capi):
    return capi.default_params(num_coarsenings=1, theta=THETA, nu_relax=3, keep_debug=True, coarse_rtol=1e-28)


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
def _elements(prob):
    """(offsets into the flat dof list, flat dof list, offsets into the packed element matrices)"""
    ep = getattr(prob, "elem_ptr", None)
    if ep is None:
        NE, nde = prob.elem_to_dof.shape
        ep = np.arange(NE + 1, dtype=np.int64) * nde
    ep = np.asarray(ep, dtype=np.int64)
    nd = np.diff(ep)
    return ep, np.asarray(prob.elem_to_dof).ravel(), np.concatenate([[0], np.cumsum(nd * nd)])


def _reassembled(prob, ess):
    """prob with A and b rebuilt from its own element matrices (ascending element order) and the essential dofs `ess`
    eliminated: the operator the element matrices define, as the oracle and the entry rule assume."""
    ep, e2d, moff = _elements(prob)
    nd = np.diff(ep)
    elmat = np.asarray(prob.elmat).ravel()
    eid = np.repeat(np.arange(nd.size), nd * nd)
    loc = np.arange(elmat.size) - moff[eid]
    rows, cols = e2d[ep[eid] + loc // nd[eid]], e2d[ep[eid] + loc % nd[eid]]
    A0 = sp.coo_matrix((elmat, (rows, cols)), shape=(prob.ND, prob.ND)).tocsr()
    A0.sort_indices()
    b0 = np.ones(prob.ND)
    A, b = pr._eliminate(A0, b0, ess)
    bdr = np.where(ess, prob.bdr, prob.bdr & ~pr.AGG_ON_ESS_DOMAIN_BORDER_FLAG).astype(np.int8)
    return pr.Problem(**dict(prob.__dict__, A=A, b=b, ess=ess, bdr=bdr))


def _randomised(prob, seed, free=False):
    """Every element matrix scaled by its own factor.  free: no essential dof at all (the flags carry bit 0 only); each
    element matrix then gets a multiple of the identity added, so that the operator stays definite."""
    prob = scaled(prob, seed)
    ess = np.asarray(prob.ess, dtype=bool)
    if free:
        ep, e2d, moff = _elements(prob)
        elmat = np.array(prob.elmat, dtype=np.float64).ravel()
        for e in range(ep.size - 1):
            nd = int(ep[e + 1] - ep[e])
            elmat[moff[e]:moff[e + 1]:nd + 1] += 0.03125
        prob = pr.Problem(**dict(prob.__dict__, elmat=elmat.reshape(np.shape(prob.elmat))))
        ess = np.zeros(prob.ND, dtype=bool)
    return _reassembled(prob, ess)


def _with_copies(prob, sel):
    """The elements `sel` listed twice, each copy with half of the matrix: the dofs of those elements lie in more elements,
    the operator and the agglomerates' dofs stay."""
    e2d = np.concatenate([prob.elem_to_dof, prob.elem_to_dof[sel]])
    elmat = np.array(prob.elmat, dtype=np.float64)
    elmat[sel] *= 0.5
    elmat = np.concatenate([elmat, elmat[sel]])
    return pr.Problem(**dict(prob.__dict__, elem_to_dof=np.ascontiguousarray(e2d), elmat=np.ascontiguousarray(elmat),
                             partitions=[np.concatenate([prob.partitions[0], prob.partitions[0][sel]])]
                             + list(prob.partitions[1:])))


def _around_vertex(n, v):
    """the (up to 8) elements of the n-grid that hold vertex v = (i, j, k)"""
    return np.array([(ez * n[1] + ey) * n[0] + ex for ez in (v[2] - 1, v[2]) for ey in (v[1] - 1, v[1]) for ex in (v[0] - 1, v[0])
                     if 0 <= ex < n[0] and 0 <= ey < n[1] and 0 <= ez < n[2]])


def _valence(vertex):
    """The 8 x 8 x 4 grid in four agglomerates of 4 x 4 x 4 elements, the eight elements around `vertex` listed twice: that
    vertex lies in 16 elements -- more than the lists of the 8-dof kernel hold --, its neighbours in at most 12."""
    n = (8, 8, 4)
    prob = _with_copies(pr.poisson3d_problem(n, blk=(4, 4, 4), coef="skew"), _around_vertex(n, vertex))
    g = (vertex[2] * 9 + vertex[1]) * 9 + vertex[0]
    val = np.bincount(prob.elem_to_dof.ravel(), minlength=prob.ND)
    assert val[g] == 16 and val.max() == 16
    return _randomised(prob, 19), g


def _make(name):
    if name in ("hex_ess", "hex_free"):
        return _randomised(pr.poisson3d_problem((12, 12, 6), blk=(4, 4, 2), coef="skew"), 11, free=name == "hex_free")
    if name == "one_part":
        prob = pr.poisson3d_problem((4, 4, 2), blk=(4, 4, 2), coef="skew")
        assert int(prob.partitions[0].max()) == 0
        return _randomised(prob, 13)
    if name == "part_per_element":
        # (no essential dofs: with them an 8-row agglomerate is diagonal but for one or two rows, its lowest eigenvalue is
        # multiple and the one vector kept is an arbitrary member of that eigenspace -- nothing to compare with the oracle)
        return _randomised(pr.poisson3d_problem((4, 4, 2), blk=(1, 1, 1), coef="skew"), 15, free=True)
    if name == "hex_wedge":
        return _randomised(pr.poisson3d_mixed_problem((8, 8, 4), (4, 4, 2), wedges="half", coef="skew", seed=7), 17)
    if name == "hex_wedge_walk":
        prob = _copied_mixed(pr.poisson3d_mixed_problem((8, 8, 4), (4, 4, 2), wedges="half", coef="skew", seed=7), (0.5, 0.5))
        eid = np.repeat(np.arange(prob.NE), np.diff(prob.elem_ptr))
        high = np.flatnonzero(np.bincount(prob.elem_to_dof, minlength=prob.ND) > 16)
        assert any(np.unique(prob.partitions[0][eid[prob.elem_to_dof == g]]).size > 1 for g in high)      # (a SHARED one)
        return _randomised(prob, 21)
    if name == "valence_shared":        # the vertex on the face between two agglomerates: they take the walk
        return _valence((4, 2, 2))[0]
    if name == "valence_inside":        # the vertex and all its neighbours inside one agglomerate: no walk any more
        return _valence((2, 2, 2))[0]
    raise KeyError(name)


CASES = ["hex_ess", "hex_free", "one_part", "part_per_element", "hex_wedge", "hex_wedge_walk", "valence_shared", "valence_inside"]
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _close_hierarchies():
    """the cases' hierarchies are shared by the tests of this module and released after the last of them"""
    yield
    for _, h in _cache.values():
        h.close()
    _cache.clear()


def _case(name):
    """(problem, hierarchy with the default options), built once per case and left unchanged"""
    if name not in _cache:
        capi = _capi()
        prob = _make(name)
        _cache[name] = (prob, capi.Hierarchy.from_problem(prob, _params(capi)))
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c rounded once"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def model_D(prob, ae_I, ae_J, flags):
    """Per agglomerate the weights of its rows in the order of its dof list (ae_I, ae_J), from the entry rule."""
    ep, e2d, moff = _elements(prob)
    elmat = np.asarray(prob.elmat, dtype=np.float64).ravel()
    part = np.asarray(prob.partitions[0])
    d2e = [[] for _ in range(prob.ND)]          # per dof: (element, first slot of the dof in it), ascending element
    for e in range(ep.size - 1):
        seen = set()
        for t, d in enumerate(e2d[ep[e]:ep[e + 1]]):
            if d not in seen:
                seen.add(d)
                d2e[d].append((e, t))
    nparts = {d: len({int(part[e]) for e, _ in d2e[d]}) for d in range(prob.ND)}
    A = prob.A.tocsr()
    out = []
    for p in range(ae_I.size - 1):
        dofs = ae_J[ae_I[p]:ae_I[p + 1]]
        loc = {int(g): i for i, g in enumerate(dofs)}
        rows = []
        for g in dofs:
            g = int(g)
            fg = int(flags[g])
            assert bool(fg & 1) == (nparts[g] > 1)
            row = []
            for k in range(A.indptr[g], A.indptr[g + 1]):
                c = int(A.indices[k])
                if c not in loc:
                    continue
                fc = int(flags[c])
                if (fg & 1) and (fc & 1) and (not ((fg | fc) & 2) or c == g):
                    v = 0.0
                    for e, kk in d2e[g]:
                        if part[e] != p:
                            continue
                        ed = e2d[ep[e]:ep[e + 1]]
                        jj = np.flatnonzero(ed == c)
                        if jj.size:
                            v = v + float(elmat[moff[e] + kk * ed.size + jj[0]])
                else:
                    v = float(A.data[k])
                row.append((loc[c], v))
            rows.append(row)
        diag = [next((v for lc, v in row if lc == i), 0.0) for i, row in enumerate(rows)]
        D = np.zeros(len(rows))
        for i, row in enumerate(rows):
            s = 0.0
            for lc, v in row:
                if v != 0.0:
                    s = _fma(abs(v), math.sqrt(diag[i] / diag[lc]), s)
            D[i] = s
        out.append(D)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_row_weights_equal_the_entry_rule_model_bit_for_bit(name):
    prob, h = _case(name)
    I, J = h.get_table(0, "AE_to_dof")
    flags = h.get_mis(0)[3]
    shared = (flags[J] & 1) != 0
    per_ae = np.add.reduceat(shared.astype(np.int64), I[:-1])
    print(name, "agglomerates", I.size - 1, "rows", np.diff(I).min(), "..", np.diff(I).max(), "shared rows per agglomerate",
          per_ae.min(), "..", per_ae.max())
    if name == "one_part":
        assert not shared.any()                                  # (the compact list is empty)
    elif name == "part_per_element":
        assert np.all(np.diff(I) == 8) and shared.sum() == shared.size - 8       # (all but the domain's 8 corners)
    elif name.startswith("hex_"):
        assert 0 < per_ae.min() and np.all(per_ae < np.diff(I))  # (neither none nor all)
    Ds = h.get_ae_eigens(0)[3]
    model = model_D(prob, I, J, flags)
    bad = [(p, int(np.sum(Ds[p].view(np.uint64) != model[p].view(np.uint64)))) for p in range(len(model))
           if not _same(Ds[p], model[p])]
    print(name, "agglomerates whose weights differ from the model:", bad[:8])
    assert not bad


@pytest.mark.parametrize("name", CASES)
def test_hierarchy_matches_the_oracle(monkeypatch, name):
    """The comparison and the tolerances of test_hex_wedge_two_level_matches_oracle."""
    prob, h = _case(name)
    if getattr(prob, "elem_ptr", None) is not None:
        H = _mixed_oracle(monkeypatch, prob, 1, theta=THETA, nu_relax=3)
    else:
        H = o.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, prob.partitions[:1], theta=THETA, nu_relax=3)
    _compare_level(h, H, 0, THETA)
    b = np.cos(np.arange(prob.ND) * 0.13) * (~prob.ess)
    x_gpu, x_ref = h.vcycle(b), o.vcycle(H, b)
    assert np.linalg.norm(x_gpu - x_ref) <= VCYCLE_TOL * np.linalg.norm(x_ref)
    x, it, conv, hist = h.pcg(prob.b, rel_tol=1e-8)
    xr, itr, convr, histr = o.solve(H, prob.b, rel_tol=1e-8)
    assert conv and convr and it == itr, (it, itr)
    assert np.allclose(hist, histr, rtol=1e-7, atol=1e-10 * histr[0])


@pytest.mark.parametrize("name", CASES)
def test_without_the_class_search_the_hierarchy_is_bitwise_the_same(name):
    capi = _capi()
    prob, h = _case(name)
    capi.set_options(eig_dedupe=0)
    try:
        h0 = capi.Hierarchy.from_problem(prob, _params(capi))
    finally:
        capi.reset_options()
    _assert_same_hierarchy(h, h0, 1)
    h0.close()


@pytest.mark.parametrize("name", ["hex_ess", "hex_free"])
def test_uniform_hexes_through_the_mixed_entry_are_bitwise_the_uniform_path(name):
    """P, Ac, D and the eigenvalues of all levels (and the tables)."""
    capi = _capi()
    prob, h = _case(name)
    h2 = capi.Hierarchy.from_problem(_as_mixed(prob), _params(capi))
    _assert_same_hierarchy(h, h2, 1)
    h2.close()
