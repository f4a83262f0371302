"""Spaced seeding (`seeding = 1`) of the partitioner's model (saamge_amd/partition_model.py): the model's greedy and
fixed-point forms against a brute-force greedy over BFS distances written here, the spacing property, the properties of the
resulting partitions, and `seeding = 0` pinned to what the function gave before the option existed."""
import hashlib

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from saamge_amd import partition_model as pm

import partition_cases as pc
import partition_seeding_cases as sc

EPAS = (4, 8, 27)
_GRAPHS = None
_REF = {}


def _graphs():
    global _GRAPHS
    if _GRAPHS is None:
        _GRAPHS = sc.graphs()
    return _GRAPHS


NAMES = ["grid_vertex", "grid_face", "path50", "star40", "three_components", "random120"]
NAMES += [x + "_perm" for x in NAMES]


def _reference(name, epa):
    """(D, prio, target, (radius, first, ext, seeds)) by brute force, computed once."""
    if (name, epa) not in _REF:
        graph = _graphs()[name]
        n = graph[0]
        if name not in _REF:
            _REF[name] = sc.distances(graph)
        D, prio, target = _REF[name], pm.priority(n), -(-n // epa)
        _REF[(name, epa)] = (D, prio, target, sc.brute_force_seeds(D, prio, target, pm.RADIUS_MAX))
    return _REF[(name, epa)]


def _components(graph):
    n, xadj, adj = graph
    G = sp.csr_matrix((np.ones(len(adj)), adj, xadj), shape=(n, n))
    return connected_components(G, directed=False)


@pytest.mark.parametrize("epa", EPAS)
@pytest.mark.parametrize("name", NAMES)
def test_both_forms_equal_the_brute_force_greedy(name, epa):
    n, xadj, adj = _graphs()[name]
    D, prio, target, (r, first, ext, seeds) = _reference(name, epa)
    g = pm._Graph(n, xadj, adj)
    for greedy in (True, False):
        got = pm.spaced_seeds(g, prio, target, greedy=greedy)
        assert got["radius"] == r, (greedy, got["radius"], r)
        assert np.array_equal(got["first"], first), greedy
        assert np.array_equal(got["ext"], ext), greedy
        assert np.array_equal(got["seeds"], seeds), greedy
    # the two forms of one set, with and without a fixed set, at radii the search above may not have visited
    for rr in (0, 1, 2, 3):
        a = pm.independent_set_greedy(g, prio, rr)
        b, _ = pm.independent_set_fixed_point(g, prio, rr)
        assert np.array_equal(a, b), rr
        if rr == 0:
            assert len(a) == n
        a2 = pm.independent_set_greedy(g, prio, rr, fixed=first)
        b2, _ = pm.independent_set_fixed_point(g, prio, rr, fixed=first)
        assert np.array_equal(a2, b2), rr
        assert not np.intersect1d(a2, first).size


@pytest.mark.parametrize("epa", EPAS)
@pytest.mark.parametrize("name", NAMES)
def test_spacing(name, epa):
    n, xadj, adj = _graphs()[name]
    D, prio, target, _ = _reference(name, epa)
    got = pm.spaced_seeds(pm._Graph(n, xadj, adj), prio, target)
    r, first, ext, seeds = got["radius"], got["first"], got["ext"], got["seeds"]
    off = ~np.eye(len(first), dtype=bool)
    assert (D[np.ix_(first, first)][off] > r).all()
    off = ~np.eye(len(seeds), dtype=bool)
    assert (D[np.ix_(seeds, seeds)][off] > r - 1).all()
    if len(first) <= target:
        assert len(seeds) == min(target, len(first) + len(ext))
    else:       # more components (or longer ones) than RADIUS_MAX can thin out: S_32 is kept whole
        assert r == pm.RADIUS_MAX and len(ext) == 0 and np.array_equal(seeds, first)
    # no smaller radius would do
    assert r == 1 or len(pm.independent_set_fixed_point(pm._Graph(n, xadj, adj), prio, r - 1)[0]) > target


@pytest.mark.parametrize("epa", EPAS)
@pytest.mark.parametrize("name", NAMES)
def test_partition_properties(name, epa):
    n, xadj, adj = _graphs()[name]
    part, nparts = pm.partition_graph(n, xadj, adj, epa, seeding=1)
    grid = name.startswith("grid")
    # covered, none empty, connected, numbered by smallest member; the cap on the grids (a hub may keep a part above it)
    pc.check_partition(n, xadj, adj, part, nparts, 2 * epa if grid else 0)
    assert part.dtype == np.int32


@pytest.mark.parametrize("name", NAMES)
def test_degenerate_sizes(name):
    graph = _graphs()[name]
    n, xadj, adj = graph
    part, nparts = pm.partition_graph(n, xadj, adj, 1, seeding=1)
    assert nparts == n and np.array_equal(part, np.arange(n))
    ncomp, comp = _components(graph)
    D = _reference(name, 4)[0]
    diameter = max(int(D[np.ix_(comp == c, comp == c)].max()) for c in range(ncomp))
    for epa in (n, 3 * n + 1):
        part, nparts = pm.partition_graph(n, xadj, adj, epa, seeding=1)
        pc.check_partition(n, xadj, adj, part, nparts, 0)
        if diameter <= pm.RADIUS_MAX:
            assert nparts == ncomp and np.array_equal(part, pm.renumber(comp.astype(np.int64), ncomp)[0])
        else:
            # the 50-node path: its ends are further apart than RADIUS_MAX, so S_32 may keep two nodes of it (the definition
            # gives up there); each seeds one connected part
            assert name.startswith("path50") and ncomp <= nparts <= 2


def test_radius_max_is_reached_on_isolated_nodes():
    n = 40
    xadj, adj = np.zeros(n + 1, np.int64), np.zeros(0, np.int32)
    g = pm._Graph(n, xadj, adj)
    for greedy in (True, False):
        got = pm.spaced_seeds(g, pm.priority(n), 5, greedy=greedy)
        assert got["radius"] == pm.RADIUS_MAX == 32
        assert np.array_equal(got["seeds"], np.arange(n)) and len(got["ext"]) == 0
    assert pm.spaced_seeds(g, pm.priority(n), 5)["rounds"] == pm.RADIUS_MAX      # one round per radius: no loop
    part, nparts = pm.partition_graph(n, xadj, adj, 8, seeding=1)
    assert nparts == n and np.array_equal(part, np.arange(n))


def test_bad_seeding_is_refused():
    n, xadj, adj = _graphs()["path50"]
    for bad in (2, -1):
        with pytest.raises(ValueError, match="seeding"):
            pm.partition_graph(n, xadj, adj, 4, seeding=bad)


# sha256 of nparts and the part array of partition_graph on the 6 x 6 x 4 grid graphs, from the commit before `seeding`
# existed: (graph, elems_per_agg, seed, lloyd_iters) -> first 16 hex digits
DIGESTS = {
    ("grid_vertex", 4, 0, 0): "46888e869bb6ea26",
    ("grid_vertex", 4, 0, 1): "46888e869bb6ea26",
    ("grid_vertex", 4, 3, 0): "0fe25d1c4d4b57f1",
    ("grid_vertex", 4, 3, 2): "0fe25d1c4d4b57f1",
    ("grid_vertex", 8, 0, 0): "3a429ea64a065b87",
    ("grid_vertex", 8, 0, 1): "3a429ea64a065b87",
    ("grid_vertex", 8, 3, 0): "539d68995c1985bf",
    ("grid_vertex", 8, 3, 2): "620c893298087deb",
    ("grid_vertex", 27, 0, 0): "972213b769d2af4d",
    ("grid_vertex", 27, 0, 1): "ca0e62e61e2fb5a5",
    ("grid_vertex", 27, 3, 0): "3f946caef77aeb0e",
    ("grid_vertex", 27, 3, 2): "810d82b0dfae8893",
    ("grid_face", 4, 0, 0): "5b3ec44303f5314b",
    ("grid_face", 4, 0, 1): "5b3ec44303f5314b",
    ("grid_face", 4, 3, 0): "472adb876fc5e7ab",
    ("grid_face", 4, 3, 2): "f92c2412ea1fca40",
    ("grid_face", 8, 0, 0): "ee23b25fed2f484e",
    ("grid_face", 8, 0, 1): "ee23b25fed2f484e",
    ("grid_face", 8, 3, 0): "be705a5f3e2ef8cc",
    ("grid_face", 8, 3, 2): "be705a5f3e2ef8cc",
    ("grid_face", 27, 0, 0): "7a8f059b54bd0a43",
    ("grid_face", 27, 0, 1): "7a8f059b54bd0a43",
    ("grid_face", 27, 3, 0): "fade22de138f5356",
    ("grid_face", 27, 3, 2): "396739a0d0d99754",
    ("grid_vertex_perm", 4, 0, 0): "168ed404b24f53ae",
    ("grid_vertex_perm", 4, 0, 1): "551dddfd3b419ee5",
    ("grid_vertex_perm", 4, 3, 0): "f95e4c2e69b79cda",
    ("grid_vertex_perm", 4, 3, 2): "f95e4c2e69b79cda",
    ("grid_vertex_perm", 8, 0, 0): "f6b126f4ec0f3c19",
    ("grid_vertex_perm", 8, 0, 1): "a9b4718acf36eff3",
    ("grid_vertex_perm", 8, 3, 0): "ab1f2cc5bd6ef956",
    ("grid_vertex_perm", 8, 3, 2): "ab1f2cc5bd6ef956",
    ("grid_vertex_perm", 27, 0, 0): "baf0b0e9dede2ff0",
    ("grid_vertex_perm", 27, 0, 1): "1193b131fdb0a24d",
    ("grid_vertex_perm", 27, 3, 0): "0726eaa4ac1a8689",
    ("grid_vertex_perm", 27, 3, 2): "629a575c73c56e47",
    ("grid_face_perm", 4, 0, 0): "bf3e97ce9b3d609d",
    ("grid_face_perm", 4, 0, 1): "bf3e97ce9b3d609d",
    ("grid_face_perm", 4, 3, 0): "43048b64db71a3fc",
    ("grid_face_perm", 4, 3, 2): "df8f67fc0711735c",
    ("grid_face_perm", 8, 0, 0): "dc201c815d5c7d7b",
    ("grid_face_perm", 8, 0, 1): "dc201c815d5c7d7b",
    ("grid_face_perm", 8, 3, 0): "11b7468478d0ebf7",
    ("grid_face_perm", 8, 3, 2): "11b7468478d0ebf7",
    ("grid_face_perm", 27, 0, 0): "13a05f8504121e5c",
    ("grid_face_perm", 27, 0, 1): "816c1d29ef66099e",
    ("grid_face_perm", 27, 3, 0): "1cea8fd4ca9fcc13",
    ("grid_face_perm", 27, 3, 2): "799bf41093a0f0e5",
}


def _digest(part, nparts):
    return hashlib.sha256(np.int64(nparts).tobytes() + np.ascontiguousarray(part, np.int32).tobytes()).hexdigest()[:16]


def _check_digests(**kw):
    assert len(DIGESTS) == 48
    for (name, epa, seed, lloyd), want in DIGESTS.items():
        n, xadj, adj = _graphs()[name]
        part, nparts = pm.partition_graph(n, xadj, adj, epa, seed=seed, lloyd_iters=lloyd, **kw)
        assert _digest(part, nparts) == want, (name, epa, seed, lloyd)


def test_the_default_is_what_it_was():
    _check_digests()


def test_seeding_0_is_what_the_default_was():
    _check_digests(seeding=0)
