"""GPU tests of the Galerkin product through the MIS blocks (rap_mis): the stored Ac against a host emulation that adds
every product in the order DESIGN.md section 4 specifies (rap_cases.py, exactly rounded fma, compared with ==), an
entrywise a-priori bound against scipy's P^T A P for larger cases with the rows of 12 chosen MISes held to the emulation,
and the row pointers that the device scan makes.  Everything goes through the C ABI (get_csr, get_mis, get_table).
Run with `pytest -m gpu` on an MI355X.

The KC < k1 path of rap_numeric_kernel (a block too wide for its k rows of LDS at once) is reached by the theta = 0.5 case of
test_every_mis_in_the_specified_order: 12 of its 27 MISes (k = 49 and 147) need more than the 20 480 doubles a workgroup
may take (rap_cases.lds_need restates rap_size_kernel's count), and every one of them is held to the emulation bit for bit;
the test asserts that some MIS takes that path there and that none does at theta = 0.003."""
import numpy as np
import pytest

from saamge_amd import problems as pr

import rap_cases as rc

pytestmark = pytest.mark.gpu


def _capi():
    from saamge_amd import capi
    return capi


def _level(h, lev):
    """A, P, Ac and the MIS tables of level `lev`, as the library stores them."""
    A, P, Ac = (h.get_csr(lev, w) for w in ("A", "P", "Ac"))
    mises, k, _, _ = h.get_mis(lev)
    I, J = h.get_table(lev, "mis_to_dof")
    return A, P, Ac, mises, k, I, J


def _check_structure(h, lev, A, Ac, mises, k):
    """Ac.indptr from the device scan == the row lengths that the neighbour lists imply; nnzAc == indptr[-1]."""
    adj = rc.mis_adjacency(A, mises, k)
    adj.eliminate_zeros()
    ncol = np.asarray(adj @ k.astype(np.float64)).astype(np.int64)
    lens = np.repeat(ncol, k)
    assert np.array_equal(np.diff(Ac.indptr), lens)
    assert h.level_info(lev)["nnzAc"] == Ac.indptr[-1] == lens.sum()
    return adj


def _build(prob, nco, theta):
    capi = _capi()
    return capi.Hierarchy.from_problem(prob, capi.default_params(num_coarsenings=nco, theta=theta, nu_relax=3, keep_debug=True))


# ---------------------------------------------------------------------------------------------------------------------
# 1. every MIS of a small hierarchy, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef,theta", [(None, 0.003), ("skew", 0.003), (None, 0.5)])
def test_every_mis_in_the_specified_order(coef, theta):
    """Poisson (16,16,8), blk (8,8,4), two levels: MISes from the vertex of 1 dof over edges and faces to interiors of
    more dofs than one wavefront has lanes; theta = 0.5: many vectors per agglomerate, wide
    blocks."""
    prob = pr.poisson3d_problem((16, 16, 8), blk=(8, 8, 4), coef=coef)
    h = _build(prob, 1, theta)
    A, P, Ac, mises, k, I, J = _level(h, 0)
    sizes = np.diff(I)
    on = sizes[k > 0]
    assert on.min() == 1 and on.max() > 64 and len(set(on.tolist())) >= 5
    adj = _check_structure(h, 0, A, Ac, mises, k)
    # which path of rap_numeric_kernel the blocks take: all k rows of a block in LDS at once, or several passes (KC < k1)
    need, floor = rc.lds_need(adj, k)
    multipass = np.nonzero(need > rc.LDS_BUDGET)[0]
    print("theta %g: largest block needs %d doubles of LDS in one pass (budget %d); multi-pass MISes %s with k = %s" % (
        theta, need.max(), rc.LDS_BUDGET, multipass.tolist(), sorted(set(k[multipass].tolist()))))
    assert floor.max() <= rc.LDS_BUDGET
    assert len(multipass) >= 1 if theta == 0.5 else len(multipass) == 0
    fmas = sum(rc.check_mis_exact(Ac, A, P, mises, k, I, J, m1) for m1 in range(len(k)))
    assert fmas > 0
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. larger cases: entrywise bound against scipy, and the rows of 12 MISes bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _chosen_mises(A, k, I, J, adj):
    sizes = np.diff(I)
    on = np.nonzero(k > 0)[0]
    rowlen = np.diff(A.indptr)
    longest = np.array([rowlen[J[I[m]:I[m + 1]]].max() for m in on])
    nnbr = np.diff(adj.indptr)[on]
    pick = [on[np.argmax(sizes[on])], on[np.argmin(sizes[on])], on[np.argmax(nnbr)], on[np.argmax(longest)]]
    pick += list(np.random.default_rng(0).choice(on, size=min(8, len(on)), replace=False))
    return [int(m) for m in pick]


def _check_level(h, lev):
    A, P, Ac, mises, k, I, J = _level(h, lev)
    adj = _check_structure(h, lev, A, Ac, mises, k)
    # the a-priori bound of the two chains of fmas: (largest MIS + longest row + 2) u (|P|^T |A| |P|)_ij
    n = int(np.diff(I).max() + np.diff(A.indptr).max() + 2)
    ref = (P.T @ A @ P).toarray()
    bound = n * 2.0 ** -52 * (abs(P).T @ abs(A) @ abs(P)).toarray()
    err = np.abs(Ac.toarray() - ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print("level %d: n = %d, max |Ac - P^T A P| = %.3e, largest error / bound = %.3e" %
          (lev, n, err.max(), (err[bound > 0] / bound[bound > 0]).max()))
    assert (err <= bound).all(), (worst, err[worst], bound[worst])
    for m1 in _chosen_mises(A, k, I, J, adj):
        rc.check_mis_exact(Ac, A, P, mises, k, I, J, m1)


def test_three_level_poisson_both_levels():
    """Poisson (32,32,16), three levels: level 1's operator has rows of uneven length."""
    h = _build(pr.poisson3d_problem((32, 32, 16), coarse_blk=[(2, 2, 2)]), 2, 0.003)
    for lev in range(2):
        _check_level(h, lev)
    h.close()


def test_q2_elasticity_long_rows():
    """Q2 elasticity 8^3, blk (4,4,4): rows of 375 entries, several vectors per agglomerate."""
    h = _build(pr.elasticity3d_q2_problem(8, blk=(4, 4, 4)), 1, 0.003)
    assert np.diff(h.get_csr(0, "A").indptr).max() == 375
    _check_level(h, 0)
    h.close()


def test_hex_wedge_mesh():
    """The hex / wedge mesh of test_gpu_mixed_elements.py (its three-level case, random columns of wedges)."""
    from test_gpu_mixed_elements import pr as mixed_pr
    prob = mixed_pr.poisson3d_mixed_problem((16, 16, 8), (4, 4, 2), coarse_blk=[(2, 2, 2)], wedges="random", seed=3)
    h = _build(prob, 2, 0.003)
    for lev in range(2):
        _check_level(h, lev)
    h.close()
