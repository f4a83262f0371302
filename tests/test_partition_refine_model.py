"""CPU tests of the partitioner's boundary refinement as the model defines it (saamge_amd/partition_model.py, "refine"): the
invariants after every round, fixed points, the edge cut on the 24^3 graphs and the hierarchy the oracle builds from refined
partitions."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from saamge_amd import partition_model as pm
from saamge_amd import problems as pr

import partition_cases as pc
import partition_growth_cases as gc
import partition_refine_cases as rc


def _components_of_parts(n, xadj, adj, label):
    src = np.repeat(np.arange(n), np.diff(xadj))
    same = label[src] == label[adj]
    G = sp.csr_matrix((np.ones(int(same.sum())), (src[same], adj[same])), shape=(n, n))
    return connected_components(G, directed=False)[0]


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_reaches_its_branch(name):
    rc.verify(name)


@pytest.mark.parametrize("name", rc.NAMES)
def test_invariants_after_every_round(name):
    c = rc.get(name)
    floor = max(c.min_size, 1)
    size0 = np.bincount(c.part, minlength=c.nparts)
    ncomp0 = _components_of_parts(c.n, c.xadj, c.adj, c.part)
    state = dict(cut=pm.edge_cut(c.n, c.xadj, c.adj, c.part), rounds=0, gain=0)

    def hook(label, st):
        size = np.bincount(label, minlength=c.nparts)
        assert len(size) == c.nparts and size.min() >= 1                       # the part count stays, none is emptied
        assert _components_of_parts(c.n, c.xadj, c.adj, label) == ncomp0       # connected parts stay connected
        if c.max_size > 0:
            assert (size <= np.maximum(size0, c.max_size)).all()
        assert (size >= np.minimum(size0, floor)).all()
        cut = pm.edge_cut(c.n, c.xadj, c.adj, label)
        assert state["cut"] - st["gain"] == cut                                # each move counts alone
        assert st["movers"] >= 1 or st["candidates"] == 0                      # a round with a candidate moves a node
        assert st["movers"] <= st["admitted"] <= st["winners"] <= st["candidates"]
        state.update(cut=cut, rounds=state["rounds"] + (st["movers"] > 0), gain=state["gain"] + st["gain"])

    info = [0, 0, 0, 0]
    lab = pm.refine_graph(c.n, c.xadj, c.adj, c.part, c.nparts, c.rounds, c.max_size, c.min_size, c.seed, info, hook)
    assert info[0] == state["rounds"] <= c.rounds and info[2] == state["gain"]
    assert info[1] >= int((lab != c.part).sum())      # (a node may move again in a later round)
    assert np.array_equal(lab, rc.model(name)[0])
    if name in rc.MESH_NAMES:
        assert ncomp0 == c.nparts


def test_refusals():
    c = rc.get("leaf")
    args = (c.n, c.xadj, c.adj)
    for bad in (dict(rounds=-1), dict(max_size=-1), dict(min_size=-1)):
        kw = dict(rounds=4, max_size=0, min_size=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            pm.refine_graph(*args, c.part, c.nparts, kw["rounds"], kw["max_size"], kw["min_size"])
    with pytest.raises(ValueError, match="empty"):
        pm.refine_graph(*args, c.part, 3, 4, 0, 0)
    with pytest.raises(ValueError, match="labels"):
        pm.refine_graph(*args, c.part - 1, 2, 4, 0, 0)


@pytest.mark.parametrize("min_shared", [1, 4])
def test_box_partitions_are_fixed_points(min_shared):
    prob = pr.poisson3d_problem(16, blk=(8, 8, 4), with_elmat=False)
    e2d = np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32)
    ep = np.arange(0, e2d.size + 1, 8, dtype=np.int32)
    xadj, adj = pm.build_element_graph(ep, e2d.ravel(), prob.ND, min_shared)
    part = np.asarray(prob.partitions[0], np.int32)
    nparts = int(part.max()) + 1
    info = []
    lab = pm.refine_graph(len(part), xadj, adj, part, nparts, 16, 2 * 256, 64, info=info)
    assert info == [0, 0, 0, 1] and np.array_equal(lab, part)


@pytest.mark.parametrize("name", ["hex12_face", "mixed4_perm"])
def test_zero_rounds_is_the_model_without_the_argument(name):
    n, xadj, adj, epa, opts = gc.cases()[name]
    a = pm.partition_graph(n, xadj, adj, epa, **opts)
    info = [7, 7, 7, 7]
    b = pm.partition_graph(n, xadj, adj, epa, refine_rounds=0, refine_info=info, **opts)
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and info == [0, 0, 0, 0]


def test_partition_graph_applies_the_pass_before_the_renumbering():
    n, xadj, adj, epa, _ = gc.cases()["hex12_face"]
    part, nparts = pm.partition_graph(n, xadj, adj, epa)
    want = []
    lab = pm.refine_graph(n, xadj, adj, part, nparts, 4, *pm.resolve_sizes(epa), info=want)
    got = []
    ref, nref = pm.partition_graph(n, xadj, adj, epa, refine_rounds=4, refine_info=got)
    assert nref == nparts and got == want and got[0] == 4
    assert np.array_equal(ref, pm.renumber(lab.astype(np.int64), nparts)[0])
    pc.check_partition(n, xadj, adj, ref, nref, 2 * epa)


@pytest.mark.parametrize("min_shared,bound", [(1, 0.88), (4, 0.95)])
def test_cut_on_the_24_cubed_graphs(min_shared, bound):
    """growth = 0, elems_per_agg 64, 64 rounds.  The bounds leave room under what the rule gives (0.84 and 0.91): a condition,
    not a pin."""
    n, xadj, adj = gc.hex_graph(24, min_shared)
    p0, n0 = pm.partition_graph(n, xadj, adj, 64)
    info = []
    p1, n1 = pm.partition_graph(n, xadj, adj, 64, refine_rounds=64, refine_info=info)
    c0, c1 = pm.edge_cut(n, xadj, adj, p0), pm.edge_cut(n, xadj, adj, p1)
    print("min_shared %d: cut %d -> %d (%.3f), info %s" % (min_shared, c0, c1, c1 / c0, info))
    assert n1 == n0 and c0 - c1 == info[2]
    assert c1 <= bound * c0
    pc.check_partition(n, xadj, adj, p1, n1, 128)


def test_hierarchy_from_refined_partitions():
    """poisson3d 16^3, vertex graph, elems_per_agg (64, 8), theta 0.003: 64 rounds against none, through the oracle."""
    from oracle import saamge_oracle as oracle
    prob = pr.poisson3d_problem(16, blk=(8, 8, 4))
    e2d = np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32)
    ep = np.arange(0, e2d.size + 1, 8, dtype=np.int32)
    fig = {}
    for rounds in (0, 64):
        parts, nparts, _ = pm.partition_mesh(ep, e2d.ravel(), prob.ND, [64, 8], refine_rounds=[rounds, rounds])
        H = oracle.ml_produce_data(prob.A, prob.elem_to_dof, prob.elmat, prob.bdr, [p.astype(np.int64) for p in parts], theta=0.003)
        _, it, conv, _ = oracle.solve(H, prob.b, rel_tol=1e-8)
        assert conv
        fig[rounds] = dict(mises=[lv.rel.num_mises for lv in H.levels], dims=[lv.Ac.shape[0] for lv in H.levels],
                           nnz=[H.levels[0].A.nnz] + [lv.Ac.nnz for lv in H.levels], it=it, nparts=nparts)
        print(rounds, fig[rounds])
    a, b = fig[0], fig[64]
    assert all(x <= y for x, y in zip(b["mises"], a["mises"]))
    assert all(x <= y for x, y in zip(b["dims"], a["dims"]))
    assert sum(b["nnz"]) < sum(a["nnz"])
    assert b["it"] <= a["it"] + 1
