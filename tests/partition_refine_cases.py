"""Graphs and partitions shared by the tests of the partitioner's boundary refinement (`refine_graph`; not a test module):
the smallest that reach each branch of a round.  `verify(name)` runs the model with its hook and asserts that the branch the
case was built for is really reached."""
import collections

import numpy as np

from saamge_amd import partition_model as pm

import partition_cases as pc
import partition_growth_cases as gc
import partition_seeding_cases as sc

Case = collections.namedtuple("Case", "n xadj adj part nparts rounds max_size min_size seed info expect")


def _case(n, edges, part, rounds=8, max_size=0, min_size=0, seed=0, info=None, expect=None):
    n, xadj, adj = sc.from_edges(n, edges)
    part = np.asarray(part, np.int32)
    return Case(n, xadj, adj, part, int(part.max()) + 1, rounds, max_size, min_size, seed, info, expect or [])


def _path(nodes):
    return [(nodes[i], nodes[i + 1]) for i in range(len(nodes) - 1)]


# A = part 0, B = part 1, C = part 2.  The leaf gadget: v with one neighbour in its own part and two adjacent ones in B.
LEAF = [(0, 1), (1, 2), (2, 3), (2, 4), (3, 4), (4, 5), (5, 6)]
# v = 2 has the path neighbours 1 and 3 in A (not linked: no common neighbour but v) and 5, 6, 7 in B
ARTICULATION = _path([0, 1, 2, 3, 4]) + [(2, 5), (2, 6), (2, 7), (5, 6), (6, 7), (5, 7)]
# v = 0 on the cycle 0-1-2-3 of A; its neighbours 1 and 3 are linked only through 2
CYCLE4 = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (0, 5), (0, 6), (4, 5), (5, 6)]
# u = 1 (A) and v = 2 (B) adjacent, each with gain 1: a1 = 0, b1 = 3, b2 = 4, a2 = 5
ADJACENT = [(0, 1), (1, 2), (1, 3), (2, 4), (2, 5), (3, 4), (5, 0)]
# v1 = 1 (A, with 0) and v2 = 3 (C, with 2) both next to b1 = 4: 2 hops apart.  B = 4, 5, 6
TWO_HOPS = [(0, 1), (2, 3), (1, 4), (1, 5), (3, 4), (3, 6), (4, 5), (4, 6)]
# v1 = 1 next to b1 = 4, b2 = 5; v2 = 3 next to b3 = 6, b4 = 7; B the path 4-5-6-7: v1 - 5 - 6 - v2 is 3 hops
THREE_HOPS = [(0, 1), (2, 3), (1, 4), (1, 5), (3, 6), (3, 7), (4, 5), (5, 6), (6, 7)]


def _hub(nown, nfor):
    """v = 0 with `nown` neighbours of its part A (a path among themselves) and `nfor` of B (a path too)."""
    a = list(range(1, 1 + nown))
    b = list(range(1 + nown, 1 + nown + nfor))
    edges = [(0, x) for x in a + b] + _path(a) + _path(b)
    return 1 + nown + nfor, edges, [0] * (1 + nown) + [1] * nfor


def _messy_cycle4():
    """CYCLE4 with a fourth neighbour in B, self-loops, the edge 0-1 listed twice and every row descending."""
    n, xadj, adj = sc.from_edges(8, CYCLE4 + [(0, 7), (6, 7)])
    rows = []
    for v in range(n):
        r = list(adj[xadj[v]:xadj[v + 1]]) + [v]
        if v in (0, 1):
            r.append(1 - v)
        rows.append(sorted(r, reverse=True))
    xadj = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return n, xadj, np.concatenate(rows).astype(np.int32)


def _from_model(graph, epa, **opts):
    n, xadj, adj = graph
    part, nparts = pm.partition_graph(n, xadj, adj, epa, **opts)
    max_size, min_size = pm.resolve_sizes(epa)
    return Case(n, xadj, adj, part, nparts, 64, max_size, min_size, opts.get("seed", 0), None, [])


def cases():
    out = collections.OrderedDict()
    out["leaf"] = _case(7, LEAF, [0, 0, 0, 1, 1, 1, 1], info=[1, 1, 1, 1],
                        expect=[dict(candidates=1, movers=1, gain=1), dict(candidates=0)])
    out["articulation"] = _case(8, ARTICULATION, [0, 0, 0, 0, 0, 1, 1, 1], info=[0, 0, 0, 1],
                                expect=[dict(gainers=1, not_free=1, candidates=0)])
    out["cycle4_two_hop_link"] = _case(7, CYCLE4, [0, 0, 0, 0, 1, 1, 1], info=[1, 1, 1, 1],
                                       expect=[dict(gainers=1, not_free=0, movers=1), dict(candidates=0)])
    # (entries count as often as they are listed: after 0 has moved, the doubled edge 0-1 gives node 1 a gain of 1)
    n, xadj, adj = _messy_cycle4()
    out["cycle4_messy_rows"] = Case(n, xadj, adj, np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32), 2, 8, 0, 0, 0, [2, 2, 2, 1],
                                    [dict(gainers=1, not_free=0, movers=1), dict(candidates=1, movers=1), dict(candidates=0)])
    out["adjacent_candidates"] = _case(6, ADJACENT, [0, 0, 1, 1, 1, 0], info=[1, 1, 1, 1],
                                       expect=[dict(candidates=2, winners=1, movers=1), dict(candidates=0)])
    out["two_hops"] = _case(7, TWO_HOPS, [0, 0, 2, 2, 1, 1, 1], info=[2, 2, 2, 1],
                            expect=[dict(candidates=2, winners=1, movers=1), dict(candidates=1, winners=1, movers=1),
                                    dict(candidates=0)])
    three = dict(n=8, edges=THREE_HOPS, part=[0, 0, 2, 2, 1, 1, 1, 1])
    out["three_hops"] = _case(info=[1, 2, 2, 1], expect=[dict(candidates=2, winners=2, movers=2), dict(candidates=0)], **three)
    # B holds 4 of at most 5: both win, one is admitted, and the full part then refuses the other
    out["in_quota"] = _case(max_size=5, info=[1, 1, 1, 1],
                            expect=[dict(winners=2, admitted=1, movers=1), dict(gainers=1, size_refused=1, candidates=0)], **three)
    # A = {0, 1, 2, 3} (0 - 2 joined) holds 4 with a floor of 3: both win and are admitted, one may leave
    out["out_quota"] = _case(8, THREE_HOPS + [(0, 2)], [0, 0, 0, 0, 1, 1, 1, 1], min_size=3, info=[1, 1, 1, 1],
                             expect=[dict(winners=2, admitted=2, movers=1), dict(gainers=1, size_refused=1, candidates=0)])
    n, edges, part = _hub(64, 65)
    out["hub_64_in_part"] = _case(n, edges, part, info=[1, 1, 1, 1], expect=[dict(candidates=1, movers=1, gain=1), dict(candidates=0)])
    n, edges, part = _hub(65, 66)
    out["hub_65_in_part"] = _case(n, edges, part, info=[0, 0, 0, 1], expect=[dict(gainers=1, local_refused=1, candidates=0)])
    n, edges, part = _hub(1, 1023)
    out["row_1024"] = _case(n, edges, part, info=[1, 1, 1022, 1], expect=[dict(candidates=1, movers=1, gain=1022), dict(candidates=0)])
    n, edges, part = _hub(1, 1024)
    out["row_1025"] = _case(n, edges, part, info=[0, 0, 0, 1], expect=[dict(gainers=1, deg_refused=1, candidates=0)])
    out["rounds_0"] = _case(7, LEAF, [0, 0, 0, 1, 1, 1, 1], rounds=0, info=[0, 0, 0, 0])
    out["rounds_1_of_2"] = _case(7, TWO_HOPS, [0, 0, 2, 2, 1, 1, 1], rounds=1, info=[1, 1, 1, 0])
    out["one_part"] = _case(7, LEAF, [0] * 7, info=[0, 0, 0, 1], expect=[dict(gainers=0, candidates=0)])
    out["nparts_n"] = _case(7, LEAF, list(range(7)), info=[0, 0, 0, 1], expect=[dict(gainers=0, candidates=0)])
    out["leaf_seed3"] = _case(7, TWO_HOPS, [0, 0, 2, 2, 1, 1, 1], seed=3, info=[2, 2, 2, 1])
    v12, f12 = gc.hex_graph(12, 1), gc.hex_graph(12, 4)
    out["hex12_vertex"] = _from_model(v12, 27)
    out["hex12_face"] = _from_model(f12, 27)
    out["hex12_vertex_growth1"] = _from_model(v12, 27, growth=1)
    mesh, ms = pc.mesh_cases(4)["mixed_perm"]
    out["mixed4_perm"] = _from_model((len(mesh[0]) - 1,) + pm.build_element_graph(mesh[0], mesh[1], mesh[2], ms), 8)
    return out


NAMES = ["leaf", "articulation", "cycle4_two_hop_link", "cycle4_messy_rows", "adjacent_candidates", "two_hops", "three_hops",
         "in_quota", "out_quota", "hub_64_in_part", "hub_65_in_part", "row_1024", "row_1025", "rounds_0", "rounds_1_of_2",
         "one_part", "nparts_n", "leaf_seed3", "hex12_vertex", "hex12_face", "hex12_vertex_growth1", "mixed4_perm"]
# the meshes must move nodes for many rounds and press against both caps (verify checks it)
MESH_NAMES = ["hex12_vertex", "hex12_face", "hex12_vertex_growth1", "mixed4_perm"]

_cache = {}


def get(name):
    if not _cache:
        _cache.update(cases())
    return _cache[name]


_model = {}


def model(name):
    """(labels, info, the stats of every round) of the model on the case; computed once."""
    if name not in _model:
        c = get(name)
        info, stats = [0, 0, 0, 0], []
        lab = pm.refine_graph(c.n, c.xadj, c.adj, c.part, c.nparts, c.rounds, c.max_size, c.min_size, c.seed, info,
                              lambda label, st: stats.append(st))
        _model[name] = (lab, info, stats)
    return _model[name]


def verify(name):
    """The branch the case stands for is reached."""
    c = get(name)
    lab, info, stats = model(name)
    if c.info is not None:
        assert info == c.info, (name, info, c.info)
    if c.expect:
        assert len(stats) == len(c.expect), (name, stats)
    for st, want in zip(stats, c.expect):
        for k, v in want.items():
            assert st[k] == v, (name, k, st, want)
    if name == "cycle4_two_hop_link":      # the mover's two neighbours of its part are not adjacent
        assert 3 not in c.adj[c.xadj[1]:c.xadj[2]] and lab[0] == 1
    if name in ("adjacent_candidates", "two_hops") and c.seed == 0:
        prio = pm.priority(c.n, c.seed)
        a, b = (1, 2) if name == "adjacent_candidates" else (1, 3)
        first, other = (a, b) if prio[a] < prio[b] else (b, a)
        assert stats[0]["movers"] == 1 and lab[first] != c.part[first]
        assert name == "two_hops" or lab[other] == c.part[other]
    if name in MESH_NAMES:
        assert info[0] >= 5 and info[1] >= info[0], (name, info)
        assert sum(st["size_refused"] for st in stats) > 0, (name, "no cap was pressed")
        assert any(st["winners"] > st["movers"] for st in stats) or any(st["not_free"] for st in stats), name
