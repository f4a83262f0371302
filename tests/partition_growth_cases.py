"""Graphs shared by the tests of the partitioner's balanced growth (`growth = 1`; not a test module): the smallest that
reach each branch of a round, of the release and of the stalled-seed rule."""
import collections

import numpy as np

from saamge_amd import partition_model as pm

import partition_cases as pc
import partition_seeding_cases as sc


def hex_graph(n, min_shared):
    mesh = pc.hex_mesh(n)
    return (len(mesh[0]) - 1,) + pm.build_element_graph(mesh[0], mesh[1], mesh[2], min_shared)


def seedless_component(n=30, epa=5, nb=6):
    """Two paths; every seed of `seeding = 0` (the ceil(n / epa) nodes of lowest priority, seed 0) lies on the first, the nb
    nodes of highest priority form the second: it is reached only by the release and its stalled-seed rule."""
    order = np.argsort(pm.priority(n), kind="stable")
    a, b = np.sort(order[:n - nb]), np.sort(order[n - nb:])
    assert -(-n // epa) <= len(a)
    edges = [(a[i], a[i + 1]) for i in range(len(a) - 1)] + [(b[i], b[i + 1]) for i in range(nb - 1)]
    return sc.from_edges(n, edges)


def cases():
    """name -> (n, xadj, adj, elems_per_agg, options)"""
    out = collections.OrderedDict()
    out["path9"] = sc.from_edges(9, [(i, i + 1) for i in range(8)]) + (3, {})
    # the quota is far below the claimants of one round and all hits are equal
    out["star40"] = sc.from_edges(41, [(0, i + 1) for i in range(40)]) + (4, {})
    # 26 neighbours, a quota of 1: many claimants for one place in the first round
    out["hex6_vertex_epa2"] = hex_graph(6, 1) + (2, {})
    v12, f12 = hex_graph(12, 1), hex_graph(12, 4)
    out["hex12_face"] = f12 + (27, {})
    out["hex12_vertex"] = v12 + (27, {})
    out["seedless_component"] = seedless_component() + (5, {})
    out["hex6_vertex_epa1"] = hex_graph(6, 1) + (1, {})
    out["path9_one_part"] = out["path9"][:3] + (9, {})
    out["hex6_face_one_part"] = hex_graph(6, 4) + (1000, {})
    mesh, ms = pc.mesh_cases(4)["mixed_perm"]
    out["mixed4_perm"] = (len(mesh[0]) - 1,) + pm.build_element_graph(mesh[0], mesh[1], mesh[2], ms) + (8, {})
    out["hex12_face_spaced"] = f12 + (27, dict(seeding=1))
    out["hex12_vertex_spaced"] = v12 + (27, dict(seeding=1))
    out["hex12_face_lloyd"] = f12 + (27, dict(lloyd_iters=1))
    out["hex12_vertex_seed3"] = v12 + (27, dict(seed=3))
    return out


NAMES = ["path9", "star40", "hex6_vertex_epa2", "hex12_face", "hex12_vertex", "seedless_component", "hex6_vertex_epa1",
         "path9_one_part", "hex6_face_one_part", "mixed4_perm", "hex12_face_spaced", "hex12_vertex_spaced", "hex12_face_lloyd",
         "hex12_vertex_seed3"]
