"""CPU tests of the partitioner's model (saamge_amd/partition_model.py) and of the new exports: the properties are checked
with scipy, independently of the model."""
import os
import re

import numpy as np
import pytest

from saamge_amd import partition_model as pm

import partition_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = pc.mesh_cases(12)


@pytest.mark.parametrize("name", sorted(CASES))
def test_element_graph_matches_brute_force(name):
    mesh, ms = CASES[name]
    xadj, adj = pm.build_element_graph(mesh[0], mesh[1], mesh[2], ms)
    xr, ar = pc.brute_force_graph(mesh, ms)
    assert np.array_equal(xadj, xr) and np.array_equal(adj, ar)
    assert len(adj) > 0


@pytest.mark.parametrize("lloyd", [0, 2])
@pytest.mark.parametrize("epa", [1, 27, 10 ** 6])
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_partitions_have_the_enforced_properties(name, epa, lloyd):
    mesh, ms = CASES[name]
    n = len(mesh[0]) - 1
    xadj, adj = pm.build_element_graph(mesh[0], mesh[1], mesh[2], ms)
    part, nparts = pm.partition_graph(n, xadj, adj, epa, lloyd_iters=lloyd)
    pc.check_partition(n, xadj, adj, part, nparts, 2 * epa)
    part2, nparts2 = pm.partition_graph(n, xadj, adj, epa, lloyd_iters=lloyd)
    assert nparts2 == nparts and np.array_equal(part, part2)
    if epa == 1:
        assert nparts == n
    if epa >= n:
        assert nparts == 1


@pytest.mark.parametrize("epa", [1, 4, 100])
def test_model_on_three_components_one_isolated(epa):
    n, xadj, adj = pc.three_components()
    for seed in (0, 1):
        part, nparts = pm.partition_graph(n, xadj, adj, epa, seed=seed)
        pc.check_partition(n, xadj, adj, part, nparts, 2 * epa)
        assert nparts >= 3
        if epa == 100:
            assert nparts == 3
        again = pm.partition_graph(n, xadj, adj, epa, seed=seed)
        assert again[1] == nparts and np.array_equal(again[0], part)


def test_model_all_levels_and_quotient_graph():
    mesh, ms = CASES["mixed_perm"]
    parts, nparts, graphs = pm.partition_mesh(mesh[0], mesh[1], mesh[2], [32, 6], min_shared=ms)
    n = len(mesh[0]) - 1
    for k in range(2):
        xadj, adj = graphs[k]
        pc.check_partition(n, xadj, adj, parts[k], nparts[k], 2 * [32, 6][k])
        xq, aq = graphs[k + 1]
        # the quotient graph against a sparse product
        import scipy.sparse as sp
        P = sp.csr_matrix((np.ones(n), (np.arange(n), parts[k])), shape=(n, nparts[k]))
        A = sp.csr_matrix((np.ones(len(adj)), adj, xadj), shape=(n, n))
        Q = (P.T @ A @ P).tocsr()
        Q.setdiag(0)
        Q.eliminate_zeros()
        Q.sort_indices()
        assert np.array_equal(xq, Q.indptr) and np.array_equal(aq, Q.indices)
        n = nparts[k]


def test_priorities_never_tie():
    for seed in (0, 7):
        assert len(np.unique(pm.priority(1 << 16, seed))) == 1 << 16


def test_partition_symbols_are_declared_exported_and_bound():
    from saamge_amd import capi
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "saamge_amd.h")).read()
    declared = set(re.findall(r"\b(saamge_amd_[a-z_0-9]+)\s*\(", hdr))
    want = {"saamge_amd_partition_options_default", "saamge_amd_partition_graph", "saamge_amd_partition_mesh",
            "saamge_amd_partitioning_arrays", "saamge_amd_partitioning_get", "saamge_amd_partitioning_graph",
            "saamge_amd_partitioning_free"}
    assert want <= declared and want <= set(capi.SYMBOLS)
    for sym in want:
        assert hasattr(lib, sym), sym
    body = hdr[hdr.index("typedef struct saamge_amd_partition_options {"):hdr.index("} saamge_amd_partition_options;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(?:int|unsigned)\s+([a-z_0-9]+)\s*;", body) == [f for f, _ in capi.PartitionOptions._fields_]
    o = capi.partition_options()
    assert (o.min_shared, o.lloyd_iters, o.max_size, o.min_size, o.seed) == (1, pm.DEFAULT_LLOYD_ITERS, -1, -1, 0)
