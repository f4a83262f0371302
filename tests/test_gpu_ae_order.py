"""The optional level order of the agglomerate matrices (saamge_amd_options.ae_order) on the GPU: the stand-alone entry
saamge_amd_ae_order against the integers of saamge_amd/ae_order_model.py on the cases of tests/ae_order_cases.py, and
hierarchies built with the option on a mesh whose dofs are renumbered by a fixed random permutation (the band of today's order
is then as wide as the matrix) and on the lexicographic one (nothing may change)."""
import numpy as np
import pytest
import scipy.sparse as sp

import ae_order_cases as ac
from saamge_amd import ae_order_model as om
from saamge_amd import problems as pr
from test_gpu_parity import EIG_TOL

pytestmark = pytest.mark.gpu

LDS_BAND = 112      # 128 - SB (csrc/eig2.hip): the widest band factored in one launch with the band in LDS
THETA = 0.003


def _capi():
    from saamge_amd import capi
    return capi


def _oracle():
    from oracle import saamge_oracle as o
    return o


_model = {}


def model_of_cases():
    """the mesh of all cases and the model's answer per agglomerate and mode: computed once"""
    if not _model:
        cases = ac.all_cases()
        ND, ep, e2d, part, names = ac.mesh_of_cases(cases)
        _model.update(ND=ND, ep=ep, e2d=e2d, part=part, names=names)
    return _model


def elems_of(m, p):
    return [m["e2d"][m["ep"][e]:m["ep"][e + 1]].tolist() for e in np.flatnonzero(m["part"] == p)]


@pytest.mark.parametrize("mode", [1, 0])
def test_stand_alone_entry_gives_the_models_integers(mode):
    capi = _capi()
    m = model_of_cases()
    nparts = len(m["names"])
    I, J, pos, bw0, bw, choice = capi.ae_order(m["ND"], m["e2d"], m["part"], nparts, mode, elem_ptr=m["ep"])
    assert I[0] == 0 and I[-1] == len(J) == len(pos)
    taken = 0
    for p, name in enumerate(m["names"]):
        dofs = J[I[p]:I[p + 1]]
        want = om.ae_order(dofs, elems_of(m, p), mode)
        got = (pos[I[p]:I[p + 1]], int(bw0[p]), int(bw[p]), int(choice[p]))
        print(name, "rows", len(dofs), "bw0", got[1], "bw", got[2], "choice", got[3], "model", want[1:])
        assert got[1:] == want[1:], name
        assert np.array_equal(got[0], want[0]), name
        taken += got[3]
    if mode == 0:
        assert taken == 0
    else:
        assert taken >= 12      # every branch of the kernel ran: see tests/test_ae_order_model.py for which cases take it


def test_stand_alone_entry_with_the_adjacency_in_the_pool_buffer():
    # (an agglomerate of 1352 rows: its bit matrix, 1352 x 43 words, does not fit beside the 16-bit arrays in LDS; the whole
    # batch then keeps its bit matrices in the pool buffer)
    capi = _capi()
    cases = {"big_box": ac.big_box(), "path": ac.path(), "two_components_and_isolated": ac.two_components_and_isolated()}
    ND, ep, e2d, part, names = ac.mesh_of_cases(cases)
    m = dict(ep=ep, e2d=e2d, part=part)
    I, J, pos, bw0, bw, choice = capi.ae_order(ND, e2d, part, len(names), 1, elem_ptr=ep)
    for p, name in enumerate(names):
        dofs = J[I[p]:I[p + 1]]
        want = om.ae_order(dofs, elems_of(m, p), 1)
        print(name, "rows", len(dofs), "bw0", int(bw0[p]), "bw", int(bw[p]), "choice", int(choice[p]))
        assert (int(bw0[p]), int(bw[p]), int(choice[p])) == want[1:] and want[3] == 1, name
        assert np.array_equal(pos[I[p]:I[p + 1]], want[0]), name
    assert I[1] - I[0] == 1352


def test_stand_alone_entry_with_equal_sized_elements_and_refusals():
    capi = _capi()
    prob = pr.poisson3d_problem((16, 16, 4), blk=(8, 8, 4))      # four boxes of 9 x 9 x 5 vertices inside 17 x 17 x 5
    part = prob.partitions[0]
    I, J, pos, bw0, bw, choice = capi.ae_order(prob.ND, prob.elem_to_dof, part, 4, 1)
    for p in range(4):
        want = om.ae_order(J[I[p]:I[p + 1]], prob.elem_to_dof[part == p].tolist(), 1)
        assert (int(bw0[p]), int(bw[p]), int(choice[p])) == want[1:] == (51, 51, 0)      # the box rule, left alone
        assert np.array_equal(pos[I[p]:I[p + 1]], want[0])
    for bad in (2, -1):
        with pytest.raises(RuntimeError, match="ae_order"):
            capi.ae_order(prob.ND, prob.elem_to_dof, part, 4, bad)


# ---- hierarchies ----
def renumbered(prob, seed=11):
    """prob with dof i renamed perm[i] (a fixed random permutation): A, elem_to_dof, flags and b"""
    perm = np.random.RandomState(seed).permutation(prob.ND)
    A = prob.A.tocoo()
    Ap = sp.csr_matrix((A.data, (perm[A.row], perm[A.col])), shape=A.shape)
    Ap.sort_indices()
    inv = np.empty_like(perm)
    inv[perm] = np.arange(prob.ND)
    return pr.Problem(A=Ap, b=prob.b[inv], elem_to_dof=perm[prob.elem_to_dof].astype(np.int32), elmat=prob.elmat,
                      bdr=prob.bdr[inv], ess=prob.ess[inv], partitions=prob.partitions, dims=prob.dims, order=1)


_shared = {}


def shared():
    """the 16 x 16 x 8 problem (8 agglomerates of 405 rows), its renumbered copy and the oracle's hierarchy of that copy"""
    if not _shared:
        o = _oracle()
        prob = pr.poisson3d_problem((16, 16, 8), blk=(8, 8, 4))
        rp = renumbered(prob)
        H = o.ml_produce_data(rp.A, rp.elem_to_dof, rp.elmat, rp.bdr, rp.partitions[:1], theta=THETA, nu_relax=3, testmesh=False)
        xr, itr, convr, histr = o.solve(H, rp.b, rel_tol=1e-8)
        assert convr
        _shared.update(prob=prob, rp=rp, H=H, itr=itr)
    return _shared


def build(prob, ae_order, keep_debug, eig_strict=1):
    capi = _capi()
    params = capi.default_params(num_coarsenings=1, theta=THETA, keep_debug=keep_debug, coarse_rtol=1e-28)
    params.options.ae_order = ae_order
    params.options.eig_strict = eig_strict
    return capi.Hierarchy.from_problem(prob, params)


def test_renumbered_mesh_comes_back_under_the_lds_band_and_matches_the_oracle():
    sh = shared()
    rp, H = sh["rp"], sh["H"]
    olv = H.levels[0]
    dims = []
    for ae_order in (0, 1):
        h = build(rp, ae_order, keep_debug=True)
        info = h.level_order_info(0)
        print("ae_order", ae_order, "level_order_info", info)
        assert info[0] == 8
        if ae_order == 0:
            assert info[1] == 0 and info[3] >= 300 and info[3] == info[2]
        else:
            assert info[1] == 8 and info[3] <= LDS_BAND and info[2] >= 300
        m, ev, X, Ds = h.get_ae_eigens(0)
        for i in range(olv.rel.nparts):
            assert m[i] == olv.evects[i].shape[1]
            assert np.allclose(ev[i], olv.evals[i][:len(ev[i])], rtol=0, atol=EIG_TOL)
        li = h.level_info(0)
        assert li["ncoarse"] == olv.P.shape[1]
        dims.append([(h.level_info(l)["n"], h.level_info(l)["ncoarse"]) for l in range(h.num_levels - 1)])
        x, it, conv, hist = h.pcg(rp.b, rel_tol=1e-8)
        assert conv and it == sh["itr"]
        h.close()
    assert dims[0] == dims[1]


def test_lexicographic_mesh_is_left_alone():
    prob = shared()["prob"]
    got = []
    for ae_order in (0, 1):
        h = build(prob, ae_order, keep_debug=False)
        info = h.level_order_info(0)
        print("ae_order", ae_order, "level_order_info", info)
        assert info[0] == 8 and info[1] == 0 and info[2] == info[3] == 51
        P = h.get_csr(0, "P")
        got.append((h.level_format(0)["eigenproblems_solved"], P.indptr.copy(), P.indices.copy(), P.data.copy()))
        h.close()
    assert got[0][0] == got[1][0]      # the classes of identical agglomerates survive
    for a, b in zip(got[0][1:], got[1][1:]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()      # the prolongator, bitwise


def test_bad_ae_order_is_refused():
    capi = _capi()
    prob = shared()["prob"]
    for bad in (2, -1):
        with pytest.raises(RuntimeError, match="ae_order"):
            build(prob, bad, keep_debug=False)
    old = capi.get_options()
    assert old.ae_order == 0
