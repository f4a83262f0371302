"""Balanced growth (`growth = 1`) of the partitioner's model (saamge_amd/partition_model.py): the properties of the
partitions and of the balanced phase, the spread of the part sizes on the 24^3 grid graphs, the clip of the hit count, pinned
digests, and `growth = 0` equal to a call without the argument."""
import hashlib

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from saamge_amd import partition_model as pm

import partition_cases as pc
import partition_growth_cases as gc

_CASES = None


def _cases():
    global _CASES
    if _CASES is None:
        _CASES = gc.cases()
    return _CASES


def _components_of_labelled(n, xadj, adj, label):
    """Connected components of the graph of same-label edges among the labelled nodes."""
    src = np.repeat(np.arange(n), np.diff(xadj))
    keep = (label[src] >= 0) & (label[src] == label[adj])
    G = sp.csr_matrix((np.ones(int(keep.sum())), (src[keep], adj[keep])), shape=(n, n))
    ncomp, comp = connected_components(G, directed=False)
    return len(np.unique(comp[label >= 0]))


def _digest(part, nparts):
    return hashlib.sha256(np.int64(nparts).tobytes() + np.ascontiguousarray(part, np.int32).tobytes()).hexdigest()[:16]


# the case list of the balanced growth as it was specified: name -> (nodes, elems_per_agg, options)
CASE_LIST = {
    "path9": (9, 3, {}),
    "star40": (41, 4, {}),
    "hex6_vertex_epa2": (216, 2, {}),
    "hex12_face": (1728, 27, {}),
    "hex12_vertex": (1728, 27, {}),
    "seedless_component": (30, 5, {}),
    "hex6_vertex_epa1": (216, 1, {}),
    "path9_one_part": (9, 9, {}),
    "hex6_face_one_part": (216, 1000, {}),
    "mixed4_perm": (None, 8, {}),
    "hex12_face_spaced": (1728, 27, dict(seeding=1)),
    "hex12_vertex_spaced": (1728, 27, dict(seeding=1)),
    "hex12_face_lloyd": (1728, 27, dict(lloyd_iters=1)),
    "hex12_vertex_seed3": (1728, 27, dict(seed=3)),
}


def test_the_cases_are_those_of_the_list():
    """The parametrised tests take their names from gc.NAMES: every name is a case, and every case carries the graph size,
    the target, the degrees and the options that the list gives it."""
    c = _cases()
    assert sorted(c) == sorted(gc.NAMES) == sorted(CASE_LIST)
    for name, (n, epa, opts) in CASE_LIST.items():
        assert c[name][3] == epa and c[name][4] == opts, name
        assert n is None or c[name][0] == n, name
        assert len(c[name][1]) == c[name][0] + 1 and c[name][1][-1] == len(c[name][2]), name
    deg = {name: np.diff(c[name][1]) for name in c}
    assert deg["star40"].max() == 40 and deg["hex12_vertex"].max() == 26 and deg["hex12_face"].max() == 6
    assert deg["hex6_vertex_epa2"].max() == 26 and deg["hex6_face_one_part"].max() == 6
    assert c["hex12_vertex_spaced"][2] is c["hex12_vertex"][2] and c["hex12_face_lloyd"][2] is c["hex12_face"][2]
    assert c["mixed4_perm"][0] == len(pc.mesh_cases(4)["mixed_perm"][0][0]) - 1
    assert connected_components(sp.csr_matrix((np.ones(len(c["seedless_component"][2])), c["seedless_component"][2],
                                               c["seedless_component"][1]), shape=(30, 30)), directed=False)[0] == 2


@pytest.mark.parametrize("name", gc.NAMES)
def test_growth_0_equals_a_call_without_the_argument(name):
    n, xadj, adj, epa, opts = _cases()[name]
    info = [7, 7, 7, 7]
    a = pm.partition_graph(n, xadj, adj, epa, **opts)
    b = pm.partition_graph(n, xadj, adj, epa, growth=0, growth_info=info, **opts)
    assert a[1] == b[1] and np.array_equal(a[0], b[0])
    assert info == [0, 0, 0, 0]


@pytest.mark.parametrize("name", gc.NAMES)
def test_invariants(name):
    n, xadj, adj, epa, opts = _cases()[name]
    seen, info = [], []
    part, nparts = pm.partition_graph(n, xadj, adj, epa, growth=1, growth_info=info,
                                      balanced_hook=lambda label, nlabels: seen.append((label, nlabels)), **opts)
    assert part.dtype == np.int32
    # covered, none empty, connected, numbered by smallest member; the cap of the size repair where no hub defeats it
    pc.check_partition(n, xadj, adj, part, nparts, 0 if name == "star40" else 2 * epa)
    again = pm.partition_graph(n, xadj, adj, epa, growth=1, **opts)
    assert again[1] == nparts and np.array_equal(again[0], part)
    # directly after every balanced phase: no part above the cap, none empty, every part connected
    assert len(seen) == 1 + opts.get("lloyd_iters", 0)
    for label, nlabels in seen:
        sizes = np.bincount(label[label >= 0], minlength=nlabels)
        assert sizes.max() <= epa and sizes.min() >= 1, (sizes.max(), epa)
        assert _components_of_labelled(n, xadj, adj, label) == nlabels
    # the counts: what the last balanced phase labelled and what it left to the release
    rounds, quota_nodes, open_parts, released = info
    label, nlabels = seen[-1]
    assert released == int((label < 0).sum())
    assert quota_nodes == n - released - nlabels            # every part starts from one seed
    assert (rounds == 0) == (quota_nodes == 0)
    assert (released == 0) <= (open_parts == 0)
    if released:
        assert open_parts == int((np.bincount(label[label >= 0], minlength=nlabels) < epa).sum())


def test_branches_are_reached():
    c = _cases()
    info = []
    n, xadj, adj, epa, opts = c["seedless_component"]
    part, nparts = pm.partition_graph(n, xadj, adj, epa, growth=1, growth_info=info)
    assert info[3] >= 6 and info[2] >= 1        # the second path is labelled after the release, from a stalled seed
    n, xadj, adj, epa, opts = c["hex6_vertex_epa1"]
    part, nparts = pm.partition_graph(n, xadj, adj, epa, growth=1, growth_info=info)
    assert nparts == n and info == [0, 0, 0, 0]
    for name in ("path9_one_part", "hex6_face_one_part"):     # a single part that never closes: no release
        n, xadj, adj, epa, opts = c[name]
        part, nparts = pm.partition_graph(n, xadj, adj, epa, growth=1, growth_info=info)
        assert nparts == 1 and info[1] == n - 1 and info[2:] == [0, 0]
    n, xadj, adj, epa, opts = c["star40"]
    part, nparts = pm.partition_graph(n, xadj, adj, epa, growth=1, growth_info=info)
    assert info[3] > 0                          # the parts around the hub close and leave leaves to the release


def test_first_round_of_the_smallest_quota():
    """6^3 vertex graph, elems_per_agg 2: many claimants for a quota of 1.  Each has one neighbour in the part, so the
    claimant of lowest priority is taken, and that closes the part."""
    n, xadj, adj, epa, _ = _cases()["hex6_vertex_epa2"]
    g, prio = pm._Graph(n, xadj, adj), pm.priority(n)
    isseed = np.zeros(n, bool)
    label, nlabels = pm._reseed(g, np.zeros(n, np.int64), isseed, prio, 1, np.array([-(-n // epa)], np.int64))
    assert nlabels == n // 2
    seen = []
    pm._grow_balanced(g, label.copy(), isseed.copy(), prio, nlabels, epa, [0] * 4, lambda l, k: seen.append(l))
    after = seen[0]
    most = 0
    for s in np.flatnonzero(label >= 0):
        # the claimants of this seed: free neighbours that touch no seed of a smaller label
        mine = [u for u in adj[xadj[s]:xadj[s + 1]]
                if label[u] < 0 and min(l for l in label[adj[xadj[u]:xadj[u + 1]]] if l >= 0) == label[s]]
        most = max(most, len(mine))
        got = np.flatnonzero(after == label[s])
        assert len(got) <= 2     # (without a claimant in the first round, a later one may still fill the part)
        if mine:
            assert got[got != s].tolist() == [mine[int(np.argmin(prio[mine]))]]
    assert most > 1          # the case is one where claimants exceed the quota (half the nodes are seeds: 17 at most here)


def test_hits_are_clipped():
    prio = pm.priority(6)
    claim = np.array([0, 0, 0, 1, 1, -1])
    quota = np.array([1, 1])
    # part 0: 70 000 and 65 535 tie after the clip, so the priority decides; 65 534 is below both
    hits = np.array([70000, 65535, 65534, 3, 5, 9])
    chosen = pm.select_claimants(claim, hits, prio, quota)
    want0 = 0 if prio[0] < prio[1] else 1
    assert np.flatnonzero(chosen).tolist() == [want0, 4]
    swapped = pm.select_claimants(claim, hits[[1, 0, 2, 3, 4, 5]], prio, quota)
    assert np.array_equal(swapped, chosen)
    # without a tie the larger count wins whatever the priorities; a quota beyond the claimants takes them all
    assert np.flatnonzero(pm.select_claimants(claim, np.array([1, 2, 3, 1, 1, 0]), prio, quota)).tolist()[0] == 2
    assert pm.select_claimants(claim, hits, prio, np.array([5, 0])).tolist() == [True, True, True, False, False, False]
    assert pm.HITS_MAX == 65535


@pytest.mark.parametrize("min_shared", [1, 4])
def test_spread_on_the_24_cubed_graphs(min_shared):
    """elems_per_agg 64, defaults.  Figures of this model, size / 64:
    vertex  growth 0: 228 parts, median 0.82, p95 1.82, max 2.00   growth 1: 212 parts, median 1.02, p95 1.38, max 1.91
    face    growth 0: 230 parts, median 0.91, p95 1.68, max 1.97   growth 1: 213 parts, median 1.03, p95 1.34, max 1.72"""
    n, xadj, adj = gc.hex_graph(24, min_shared)
    s0 = pm.size_stats(*pm.partition_graph(n, xadj, adj, 64, growth=0), 64)
    s1 = pm.size_stats(*pm.partition_graph(n, xadj, adj, 64, growth=1), 64)
    print("min_shared %d growth 0 %s growth 1 %s" % (min_shared, s0, s1))
    assert s1["p95"] <= 1.5 and 0.95 <= s1["median"] <= 1.10
    assert s0["p95"] > 1.6


# sha256 of nparts and the part array with growth = 1: first 16 hex digits
DIGESTS = {
    "path9": "4d5c340b61c78138",
    "star40": "9658b089dd485264",
    "hex6_vertex_epa2": "0bc96ecefa108dee",
    "hex12_face": "c81e61d78ac90d45",
    "hex12_vertex": "e1f394edb2d7d8e2",
    "seedless_component": "9ae9b467ae84cb0e",
    "mixed4_perm": "e04517c82395da6b",
    "hex12_face_spaced": "2753bfdb894fc7b3",
    "hex12_vertex_spaced": "e87f771313fbb2af",
    "hex12_face_lloyd": "072a2de70c6bdf97",
    "hex12_vertex_seed3": "17b33270a74ec97d",
}


@pytest.mark.parametrize("name", sorted(DIGESTS))
def test_digests(name):
    n, xadj, adj, epa, opts = _cases()[name]
    part, nparts = pm.partition_graph(n, xadj, adj, epa, growth=1, **opts)
    assert _digest(part, nparts) == DIGESTS[name], (name, _digest(part, nparts))


def test_growth_changes_the_partition():
    """The digests above are not those of growth = 0."""
    n, xadj, adj, epa, opts = _cases()["hex12_vertex"]
    a = pm.partition_graph(n, xadj, adj, epa, growth=0)
    b = pm.partition_graph(n, xadj, adj, epa, growth=1)
    assert a[1] != b[1] or not np.array_equal(a[0], b[0])


def test_bad_growth_is_refused():
    n, xadj, adj, epa, _ = _cases()["path9"]
    for bad in (2, -1):
        with pytest.raises(ValueError, match="growth"):
            pm.partition_graph(n, xadj, adj, epa, growth=bad)
