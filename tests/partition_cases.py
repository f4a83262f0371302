"""Meshes, graphs and model-independent checks shared by the partition tests (not a test module)."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from saamge_amd import problems as pr


def hex_mesh(n):
    """(elem_ptr, flat elem_to_dof, ND) of an n^3 grid of Q1 hexes."""
    p = pr.poisson3d_problem(n, blk=(2, 2, 2))
    e2d = np.ascontiguousarray(p.elem_to_dof, dtype=np.int32)
    return np.arange(0, e2d.size + 1, 8, dtype=np.int32), e2d.ravel(), p.ND


def mixed_mesh(n):
    """Half of the columns split into prisms."""
    p = pr.poisson3d_mixed_problem(n, (2, 2, 2), wedges="half")
    return (np.ascontiguousarray(p.elem_ptr, dtype=np.int32), np.ascontiguousarray(p.elem_to_dof, dtype=np.int32).ravel(),
            p.ND)


def permuted(mesh, seed=1):
    ep, e2d, ND = mesh
    perm = np.random.default_rng(seed).permutation(len(ep) - 1)
    nd = np.diff(ep)[perm]
    nep = np.concatenate([[0], np.cumsum(nd)]).astype(np.int32)
    out = np.concatenate([e2d[ep[e]:ep[e + 1]] for e in perm]).astype(np.int32)
    return nep, out, ND


def mesh_cases(n):
    """name -> (mesh, min_shared)"""
    hx, mx = hex_mesh(n), mixed_mesh(n)
    return {
        "hex_vertex": (hx, 1), "hex_face": (hx, 4), "mixed": (mx, 1),
        "hex_vertex_perm": (permuted(hx), 1), "hex_face_perm": (permuted(hx), 4), "mixed_perm": (permuted(mx), 1),
    }


def three_components():
    """A 5 x 5 grid graph, a path of 7 nodes and one isolated node, interleaved by a fixed permutation."""
    edges = []
    for j in range(5):
        for i in range(5):
            v = 5 * j + i
            if i < 4:
                edges.append((v, v + 1))
            if j < 4:
                edges.append((v, v + 5))
    edges += [(25 + i, 26 + i) for i in range(6)]
    n = 33
    perm = np.random.default_rng(5).permutation(n)
    e = perm[np.array(edges)]
    A = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    A = (A + A.T).tocsr()
    A.sort_indices()
    return n, A.indptr.astype(np.int64), A.indices.astype(np.int32)


def brute_force_graph(mesh, min_shared):
    ep, e2d, ND = mesh
    NE = len(ep) - 1
    E = sp.csr_matrix((np.ones(len(e2d)), e2d, ep), shape=(NE, ND))
    G = (E @ E.T).tocsr()
    G.setdiag(0)
    G.data[G.data < min_shared] = 0
    G.eliminate_zeros()
    G.sort_indices()
    return G.indptr.astype(np.int64), G.indices.astype(np.int32)


def check_partition(n, xadj, adj, part, nparts, max_size):
    """The properties the reference enforces on a partition, checked without the model."""
    part = np.asarray(part)
    assert part.shape == (n,)
    if n == 0:
        assert nparts == 0
        return
    assert part.min() >= 0 and part.max() == nparts - 1
    sizes = np.bincount(part, minlength=nparts)
    assert sizes.min() > 0, "empty part"
    src = np.repeat(np.arange(n), np.diff(xadj))
    same = part[src] == part[adj]
    G = sp.csr_matrix((np.ones(int(same.sum())), (src[same], adj[same])), shape=(n, n))
    ncomp, _ = connected_components(G, directed=False)
    assert ncomp == nparts, "disconnected parts: %d components of %d parts" % (ncomp, nparts)
    if max_size > 0:
        assert sizes.max() <= max_size, (sizes.max(), max_size)
    first = np.full(nparts, n)
    np.minimum.at(first, part, np.arange(n))
    assert (np.diff(first) > 0).all(), "parts are not numbered by their smallest member"
