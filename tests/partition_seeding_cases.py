"""Graphs and a brute-force greedy shared by the tests of the partitioner's spaced seeding (not a test module)."""
import collections

import numpy as np
import scipy.sparse as sp

from saamge_amd import problems as pr

import partition_cases as pc


def grid_mesh(n=(6, 6, 4)):
    """(elem_ptr, flat elem_to_dof, ND) of a grid of Q1 hexes."""
    p = pr.poisson3d_problem(n, blk=(2, 2, 2), with_elmat=False)
    e2d = np.ascontiguousarray(p.elem_to_dof, dtype=np.int32)
    return np.arange(0, e2d.size + 1, 8, dtype=np.int32), e2d.ravel(), p.ND


def from_edges(n, edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    A = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    A = ((A + A.T) > 0).astype(np.int8).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    return n, A.indptr.astype(np.int64), A.indices.astype(np.int32)


def permute(graph, seed=7):
    n, xadj, adj = graph
    perm = np.random.default_rng(seed).permutation(n)
    src = np.repeat(np.arange(n), np.diff(xadj))
    return from_edges(n, np.stack([perm[src], perm[adj]], axis=1))


def three_components():
    """A 5 x 6 grid graph (30 nodes), a path of 7 and one isolated node, interleaved by a fixed permutation."""
    edges = []
    for j in range(6):
        for i in range(5):
            v = 5 * j + i
            if i < 4:
                edges.append((v, v + 1))
            if j < 5:
                edges.append((v, v + 5))
    edges += [(30 + i, 31 + i) for i in range(6)]
    return permute(from_edges(38, edges), seed=5)


def random_graph(n=120, seed=11):
    rng = np.random.default_rng(seed)
    return from_edges(n, np.stack([rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)], axis=1))


def graphs():
    """name -> (n, xadj, adj) and, for the grids, True"""
    mesh = grid_mesh()
    n = len(mesh[0]) - 1
    out = collections.OrderedDict()
    out["grid_vertex"] = (n,) + pc.brute_force_graph(mesh, 1)
    out["grid_face"] = (n,) + pc.brute_force_graph(mesh, 4)
    out["path50"] = from_edges(50, [(i, i + 1) for i in range(49)])
    out["star40"] = from_edges(41, [(0, i + 1) for i in range(40)])
    out["three_components"] = three_components()
    out["random120"] = random_graph()
    for name in list(out):
        out[name + "_perm"] = permute(out[name])
    return out


def distances(graph):
    """All-pairs hop distances by one BFS per node; unreachable = a number beyond every radius."""
    n, xadj, adj = graph
    D = np.full((n, n), 10 ** 6, np.int64)
    for s in range(n):
        D[s, s] = 0
        front, d = [s], 0
        while front:
            d += 1
            nxt = []
            for v in front:
                for u in adj[xadj[v]:xadj[v + 1]]:
                    if D[s, u] > d:
                        D[s, u] = d
                        nxt.append(int(u))
            front = nxt
    return D


def brute_force_seeds(D, prio, target, radius_max):
    """The definition, from the distance matrix alone: (radius, S_r, E, seeds), node arrays ascending."""
    n = len(D)
    order = np.argsort(prio[:n], kind="stable")

    def greedy(r, fixed):
        members, new = list(fixed), []
        for v in order:
            if v not in fixed and all(D[v, m] > r for m in members):
                members.append(int(v))
                new.append(int(v))
        return np.sort(np.array(new, np.int64))

    for r in range(1, radius_max + 1):
        first = greedy(r, [])
        if len(first) <= target:
            break
    ext = np.zeros(0, np.int64)
    seeds = first
    if len(first) < target:
        ext = greedy(r - 1, list(first))
        by_prio = ext[np.argsort(prio[ext], kind="stable")]
        seeds = np.sort(np.concatenate([first, by_prio[:target - len(first)]]))
    return r, first, ext, seeds
