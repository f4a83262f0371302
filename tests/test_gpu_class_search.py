"""The searches for classes of identical agglomerates (csrc/assemble.hip: ce_walk, ai_row_walk; csrc/dedupe.hip) and the row
order of the agglomerate matrices (ae_perm_kernel) visit their words lane-parallel and sort where they used to rank.  The class
hash is a sum over (word, position) pairs, so none of that may show in a result: the hierarchies below are, bit for bit, those
of the per-agglomerate computation (eig_dedupe = 0) AND those recorded from the commit before the walks were rewritten (GOLDEN:
sha256 of the sorted P and Ac of both levels, PCG iterations, eigenproblems solved per level), and the stand-alone row order is
numpy's argsort -- or the shortest-extent-first order of a lexicographic box."""
import hashlib

import numpy as np
import pytest

from saamge_amd import problems as pr

pytestmark = pytest.mark.gpu

AE_SORT_MIN = 1024      # csrc/assemble.hip: batches whose largest agglomerate has that many rows are sorted, smaller ones ranked

# recorded from the parent commit (python tests/test_gpu_class_search.py prints this dictionary)
GOLDEN = {
    "const": {"digests": ["52496b3613b8af27301e99df976d9e7656ec6365463777e66f39cd657148bca3",
                          "a42936f30815a0f3dcc5d4f2596dd1c505149c1896e50ce9d64ce7fc508c14ba",
                          "a50b1c13a8df685264da7b81730c804d4120bd974dc87da55414a895758ab99c",
                          "17ea63b75cc5971e8946c5b5dfbc0de16d45e3d13faa16a6802f1f5861d4d8ba"],
              "iterations": 9, "nparts": [512, 2], "solved": [27, 2]},
    "skew": {"digests": ["b5c64db253498eb955881bfd1c9497303963d014084347b67d3de4b399ed704d",
                         "65bd2482beaf9ab44c1bd8ec1063014d5e7615e6721b0879152d9d637f8b5bdb",
                         "42e66f273d6c1cc49449196fd896fa559b1c61845f31402b1493789349150741",
                         "a02e76e5b57ef9777462cda1defb57c76d94f250025ec540def3ae1b70ed9230"],
             "iterations": 10, "nparts": [512, 2], "solved": [512, 2]},
    "q2": {"digests": ["9a273a5bc1882ffdc1963e7bb782ad104928f6ea03ca2adc324f2038b8970df8",
                       "35676a3f2f22cbe2fc08389166c9017ba4b7312824da8f9263c0126aaab34e65",
                       "f535354d81c2283ec0d12de98209006a5a618a581dd92b810965920cf84a42a6",
                       "7e73b57ec56ed52617d47018fdd5aadb9c5f1f8103db9a8a8bd72e1cab90e2bb"],
           "iterations": 24, "nparts": [64, 8], "solved": [2, 8]},
    "wide": {"digests": ["3c546efc18016daac23ddb2411d1f3634b5c3c675e0afd463c33340a11c07767",
                         "b75e33afb93f5f14e8815c227986cc637a436bdc80bec3bec5ff535d57c49971",
                         "51baa28ba33cf95796b938d72921b37495b1e994e20bdd6ec03bedb50f3ceb3c",
                         "bb95c76701540f351af419b8f9cd0a5c892f6c9cad21a180b81fd9ecf3a7d800"],
             "iterations": 13, "nparts": [2048, 16], "solved": [27, 12]},
    "near": {"digests": ["7850d086f9dec32e3bd358c466c3013cb88715a2385fd51e7892f80ae145d4a9",
                         "9f3ffc20468e5d16422e73b1445590d28d8432b9d4580d63ef387d34fb9e2d56",
                         "8e97f4040a90d1905f435a589664f3d90fdcdf471a896f09256c974e8147272e",
                         "012a0dfae44154812f2dad0d0bcd3b43d90aad7976ed4000d29b1c0a1c23d991"],
             "iterations": 10, "nparts": [512, 2], "solved": [28, 2]},
}


def _problem(case):
    import torch
    if case == "q2":          # 64 agglomerates of 2 187 rows: the generic assembly, classes found on its inputs (ai_row_walk)
        prob = pr.elasticity3d_q2_device(16, blk=(4, 4, 4), coarse_blk=[(2, 2, 2)], device="cuda:0")
        return prob, 81, dict(workspace_bytes=2 << 30)
    if case == "wide":        # 16 level-1 agglomerates of 17 x 9 x 9 = 1 377 rows: the banded path and its input search on level 1
        prob = pr.poisson3d_device((128, 64, 64), blk=(8, 8, 4), coarse_blk=[(8, 4, 4)], device="cuda:0")
        return prob, 8, {}
    # 512 fine agglomerates in several chunks
    prob = pr.poisson3d_device((64, 64, 32), blk=(8, 8, 4), coarse_blk=[(8, 8, 4)], device="cuda:0",
                               coef="skew" if case == "skew" else None)
    if case == "near":        # the matrix of one element inside the mesh x 1.5: its agglomerate is nobody's duplicate.  (Element
        # (16, 16, 8), in the corner of agglomerate (2, 2, 2): the rows of dofs shared with the neighbours are summed from the
        # element matrices, the others are copied from the global matrix, which stays as it is.)
        e = (8 * 64 + 16) * 64 + 16
        prob.elmat[e] = prob.elmat[e] * 1.5
        torch.cuda.synchronize()
    return prob, 8, dict(workspace_bytes=1 << 28)


_built = {}


def build(case, dedupe):
    """(digests of P, Ac of levels 0 and 1; eigenproblems solved; nparts; PCG iterations; converged): computed once"""
    if (case, dedupe) in _built:
        return _built[(case, dedupe)]
    import torch
    from saamge_amd import capi
    capi.set_options(eig_dedupe=dedupe)
    try:
        prob, nde, kw = _problem(case)
        params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3, **kw)
        h = capi.Hierarchy(prob.rowptr, prob.col, prob.val, prob.n, prob.elem_to_dof, prob.elmat, prob.bdr,
                           prob.partitions, prob.nparts, params, prob.NE_, nde)
        dig = []
        for l in range(2):
            for which in ("P", "Ac"):
                M = h.get_csr(l, which).tocsr()
                M.sort_indices()
                dig.append(hashlib.sha256(M.indptr.tobytes() + M.indices.tobytes() + M.data.tobytes()).hexdigest())
        solved = [h.level_format(l)["eigenproblems_solved"] for l in range(2)]
        nparts = [h.level_info(l)["nparts"] for l in range(2)]
        x = torch.zeros_like(prob.b)
        _, it, conv, _ = h.pcg(prob.b, x, rel_tol=1e-8, max_iter=100)
        h.close()
    finally:
        capi.reset_options()
    _built[(case, dedupe)] = (dig, solved, nparts, int(it), bool(conv))
    return _built[(case, dedupe)]


def _check(case):
    on, off = build(case, 1), build(case, 0)
    print(case, "solved", on[1], "of", on[2], "iterations", on[3], "digests", on[0])
    assert on[0] == off[0] and on[3] == off[3] and on[4] == off[4]
    assert off[1] == off[2]                                     # without the search every agglomerate on its own
    g = GOLDEN[case]
    assert on[0] == g["digests"] and on[3] == g["iterations"]
    assert on[1] == g["solved"] and on[2] == g["nparts"]
    return on


def test_poisson_constant_coefficient():
    on = _check("const")
    assert on[4] and on[2][0] == 512 and on[1][0] * 4 < on[2][0]


def test_poisson_general_coefficient_merges_nothing():
    on = _check("skew")
    assert on[1] == on[2]


def test_q2_elasticity_generic_assembly():
    on = _check("q2")
    assert on[4] and on[2][0] == 64 and on[1][0] <= 4


def test_wide_level_1_agglomerates_are_searched():
    on = _check("wide")
    assert on[4] and on[2][1] == 16 and on[1][1] < on[2][1]    # the level-1 search ran and merged


def test_near_duplicate_is_not_merged():
    on = _check("near")
    assert on[1][0] > build("const", 1)[1][0]


# ---- the row order through the stand-alone entry ----
def _one_agglomerate(dofs, ND):
    """a mesh of 2-dof elements chaining the given dofs: agglomerate 0 has exactly `dofs`; every other dof of the mesh lies in
    further, smaller agglomerates (a dof needs an element; the largest agglomerate of the batch decides between ranking
    and sorting)"""
    dofs = np.asarray(dofs, np.int64)
    rest = np.setdiff1d(np.arange(ND), dofs)
    step = min(len(dofs) - 1, 1000)
    chains = [dofs] + [rest[i:i + step] for i in range(0, len(rest), step)]
    if len(chains[-1]) < 2:
        chains[-2] = chains[-2][:-1]      # (the last chain gets a second dof)
        chains[-1] = rest[-2:]
    e2d = np.concatenate([np.stack([c[:-1], c[1:]], axis=1).reshape(-1) for c in chains]).astype(np.int32)
    part = np.concatenate([np.full(len(c) - 1, p) for p, c in enumerate(chains)]).astype(np.int32)
    ep = np.arange(0, len(e2d) + 1, 2, dtype=np.int32)
    return ND, ep, np.ascontiguousarray(e2d), part, len(chains)


def _pos(ND, ep, e2d, part, nparts):
    """the dofs of agglomerate 0 in table order and the positions of its rows (mode 0: ae_perm_kernel alone)"""
    from saamge_amd import capi
    I, J, pos, bw0, bw, choice = capi.ae_order(ND, e2d, part, nparts, 0, elem_ptr=ep)
    assert I[0] == 0 and I[-1] == len(J) == len(pos)
    return np.asarray(J[:I[1]]), np.asarray(pos[:I[1]])


@pytest.mark.parametrize("n", [405, AE_SORT_MIN - 1, AE_SORT_MIN, AE_SORT_MIN + 1, 2601, 4001])
def test_row_order_of_random_dofs_is_the_argsort(n):
    rs = np.random.RandomState(n)
    ND = 3 * n + 7
    dofs = rs.permutation(ND)[:n]
    J, pos = _pos(*_one_agglomerate(dofs, ND))
    assert sorted(J.tolist()) == sorted(dofs.tolist())
    want = np.empty(n, np.int64)
    want[np.argsort(J, kind="stable")] = np.arange(n)          # the rank of every dof
    assert np.array_equal(pos, want)


@pytest.mark.parametrize("box", [(9, 9, 5), (17, 17, 9)])
def test_row_order_of_a_lexicographic_box_runs_its_shortest_extent_first(box):
    a, b, c = box                                               # a = b > c: extents of the box inside a 40 x 30 x 20 grid
    NX, NY, NZ = 40, 30, 20
    k, j, i = np.meshgrid(np.arange(c), np.arange(b), np.arange(a), indexing="ij")
    dofs = (5 + i + NX * (3 + j) + NX * NY * (2 + k)).ravel()
    dofs = dofs[np.random.RandomState(7).permutation(len(dofs))]
    J, pos = _pos(*_one_agglomerate(dofs, NX * NY * NZ))
    rank = np.empty(len(J), np.int64)
    rank[np.argsort(J)] = np.arange(len(J))
    ci, cj, ck = rank % a, (rank // a) % b, rank // (a * b)
    # extents ascending, stable: (c, a, b) -- c runs fastest, then a, then b
    assert np.array_equal(pos, ck + c * (ci + a * cj))


if __name__ == "__main__":
    import pprint
    import sys
    out = {}
    for case in sys.argv[1:] or ("const", "skew", "q2", "wide", "near"):
        dig, solved, nparts, it, conv = build(case, 1)
        out[case] = {"digests": dig, "iterations": it, "solved": solved, "nparts": nparts}
    pprint.pprint(out, width=120)
