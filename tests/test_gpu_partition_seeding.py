"""GPU tests of the partitioner's spaced seeding (`seeding = 1`, csrc/partition.hip): exact integer agreement with the CPU
model (saamge_amd/partition_model.py), refusal of other values, device memory, and hierarchies built from its partitions."""
import ctypes as C
import math

import numpy as np
import pytest

from saamge_amd import partition_model as pm
from saamge_amd import problems as pr

import partition_cases as pc

pytestmark = pytest.mark.gpu

CASES24 = None


def _capi():
    from saamge_amd import capi
    capi.load()
    return capi


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cases24():
    global CASES24
    if CASES24 is None:
        CASES24 = pc.mesh_cases(24)
    return CASES24


@pytest.mark.parametrize("name", ["hex_vertex", "hex_face", "mixed", "hex_vertex_perm", "hex_face_perm", "mixed_perm"])
def test_partition_mesh_equals_the_model(name):
    capi = _capi()
    mesh, ms = _cases24()[name]
    ep, e2d, ND = mesh
    epa = [48, 6]
    for seed in (0, 3):
        parts, nparts, graphs = pm.partition_mesh(ep, e2d, ND, epa, min_shared=ms, seed=seed, seeding=1)
        got = []
        for device_in in (False, True):
            a, b = (_dev(e2d), _dev(ep)) if device_in else (e2d, ep)
            P = capi.partition_mesh(a, ND, epa, elem_ptr=b, min_shared=ms, seed=seed, seeding=1)
            assert P.nparts == nparts, (P.nparts, nparts)
            for k in range(3):
                xadj, adj = P.graph(k)
                assert np.array_equal(xadj, graphs[k][0]) and np.array_equal(adj, graphs[k][1]), "graph %d" % k
            for k in range(2):
                assert np.array_equal(P.part(k), parts[k]), "partition %d" % k
            got.append([P.part(k) for k in range(2)])
            P.close()
        assert all(np.array_equal(x, y) for x, y in zip(*got))       # host and device pointers: the same arrays
        # the spaced seeding of the last level, as the library reports it, against the model's
        xq, aq = graphs[1]
        want = pm.spaced_seeds(pm._Graph(nparts[0], xq, aq), pm.priority(nparts[0], seed), -(-nparts[0] // epa[1]))
        info = capi.partition_seeding_info()
        assert (info["radius"], info["seeds_first"], info["seeds"]) == (want["radius"], len(want["first"]), len(want["seeds"]))


@pytest.mark.parametrize("epa", [1, 4, 100])
def test_three_components_equal_the_model(epa):
    import torch
    capi = _capi()
    n, xadj, adj = pc.three_components()
    for seed in (0, 3):
        for lloyd in (0, 1):
            ref, nref = pm.partition_graph(n, xadj, adj, epa, seed=seed, lloyd_iters=lloyd, seeding=1)
            part, npt = capi.partition_graph(n, xadj, adj, epa, seed=seed, lloyd_iters=lloyd, seeding=1)
            assert npt == nref and np.array_equal(part, ref)
            pc.check_partition(n, xadj, adj, part, npt, 2 * epa)
            dpart = torch.empty(n, dtype=torch.int32, device="cuda")
            _, npt = capi.partition_graph(n, _dev(xadj), _dev(adj), epa, part=dpart, seed=seed, lloyd_iters=lloyd, seeding=1)
            assert npt == nref and np.array_equal(dpart.cpu().numpy(), ref)
    if epa == 100:      # three components and one target: no radius thins them out, the search ends at RADIUS_MAX
        info = capi.partition_seeding_info()
        assert (info["radius"], info["seeds_first"], info["seeds"]) == (pm.RADIUS_MAX, 3, 3)


def test_small_caps_equal_the_model():
    """A tight cap and a large minimum: many repair and merge rounds after the spaced seeds."""
    capi = _capi()
    mesh, ms = pc.mesh_cases(12)["mixed_perm"]
    xadj, adj = pm.build_element_graph(mesh[0], mesh[1], mesh[2], ms)
    n = len(mesh[0]) - 1
    for kw in (dict(max_size=40, min_size=20), dict(max_size=0, min_size=30), dict(max_size=33, min_size=0)):
        ref, nref = pm.partition_graph(n, xadj, adj, 32, seeding=1, **kw)
        part, npt = capi.partition_graph(n, xadj, adj, 32, seeding=1, **kw)
        assert npt == nref and np.array_equal(part, ref), kw
        pc.check_partition(n, xadj, adj, part, npt, kw["max_size"])


def test_isolated_nodes_reach_radius_max():
    capi = _capi()
    n = 40
    xadj, adj = np.zeros(n + 1, np.int64), np.zeros(1, np.int32)[:0]
    part, npt = capi.partition_graph(n, xadj, adj, 8, seeding=1)
    assert npt == n and np.array_equal(part, np.arange(n))
    assert capi.partition_seeding_info() == dict(radius=pm.RADIUS_MAX, rounds=pm.RADIUS_MAX, seeds_first=n, seeds=n)


@pytest.mark.parametrize("bad", [2, -1])
def test_other_values_are_refused(bad):
    capi = _capi()
    lib = capi.load()
    n, xadj, adj = pc.three_components()
    part = np.full(n, -7, np.int32)
    with pytest.raises(RuntimeError, match="seeding"):
        capi.partition_graph(n, xadj, adj, 4, part=part, seeding=bad)
    assert (part == -7).all()
    o = capi.partition_options(seeding=bad)
    npt = C.c_int(-7)
    rc = lib.saamge_amd_partition_graph(C.c_int(n), xadj.ctypes.data_as(C.c_void_p), adj.ctypes.data_as(C.c_void_p), C.c_int(4),
                                        C.byref(o), None, part.ctypes.data_as(C.c_void_p), C.byref(npt))
    assert rc != 0 and npt.value == -7 and (part == -7).all()
    mesh, _ = pc.mesh_cases(4)["mixed"]
    h = C.c_void_p(7)
    epa = (C.c_int * 1)(8)
    rc = lib.saamge_amd_partition_mesh(C.c_int(len(mesh[0]) - 1), C.c_int(0), mesh[0].ctypes.data_as(C.c_void_p),
                                       mesh[1].ctypes.data_as(C.c_void_p), C.c_int(mesh[2]), C.c_int(1), epa, C.byref(o), None,
                                       C.byref(h))
    assert rc != 0 and h.value == 7
    with pytest.raises(RuntimeError, match="seeding"):
        capi.partition_mesh(mesh[1], mesh[2], [8], elem_ptr=mesh[0], seeding=bad)
    # a zero-filled struct is today's seeding
    z = capi.PartitionOptions()
    d = capi.partition_options()
    assert z.seeding == d.seeding == 0


def test_nothing_outlives_the_calls():
    capi = _capi()
    mesh, ms = pc.mesh_cases(12)["mixed"]
    ep, e2d, ND = mesh
    xadj, adj = pm.build_element_graph(ep, e2d, ND, ms)
    n = len(ep) - 1
    live0, _ = capi.memory_stats(reset_peak=True)
    capi.partition_graph(n, xadj, adj, 32, lloyd_iters=1, seeding=1)
    live1, peak1 = capi.memory_stats()
    assert live1 == live0 and peak1 > live0
    capi.partition_graph(n, xadj, adj, 1, seeding=1)            # the top-up at radius 1
    capi.partition_graph(n, xadj, adj, 10 ** 6, seeding=1)      # one seed
    assert capi.memory_stats()[0] == live0
    P = capi.partition_mesh(e2d, ND, [32, 4], elem_ptr=ep, seeding=1)
    assert capi.memory_stats()[0] > live0
    P.close()
    assert capi.memory_stats()[0] == live0


def _true_rel_res(prob, x):
    return np.linalg.norm(prob.A @ x - prob.b) / np.linalg.norm(prob.b)


def test_poisson32_three_levels_from_spaced_seeds():
    """The bounds of test_gpu_partition.py::test_poisson32_three_levels_from_device_partitions, against the same box
    hierarchy.  The printed line holds the figures recorded in DESIGN.md section 4.5."""
    capi = _capi()
    prob = pr.poisson3d_problem(32, blk=(8, 8, 4), coarse_blk=[(2, 2, 2)])
    params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3, coarse_rtol=1e-28)
    hb = capi.Hierarchy.from_problem(prob, params)
    xb, itb, convb, _ = hb.pcg(prob.b, rel_tol=1e-8)
    hb.close()
    P = capi.partition_mesh(np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32), prob.ND, [256, 8], seeding=1)
    h = capi.Hierarchy.from_partitioning(prob, params, P)
    x, it, conv, _ = h.pcg(prob.b, rel_tol=1e-8)
    info = [h.level_info(l) for l in range(h.num_levels - 1)]
    h.close()
    rb, r = _true_rel_res(prob, xb), _true_rel_res(prob, x)
    print("box: it %d res %.2e | spaced seeds %s: it %d res %.2e levels %s" % (itb, rb, P.nparts, it, r, info))
    assert convb and conv
    assert r <= 1e-6 and r <= 10.0 * max(rb, 1e-16)
    assert it <= math.ceil(1.5 * itb), (it, itb)
    P.close()


def test_mixed_mesh_three_levels_from_spaced_seeds():
    """The bounds of test_gpu_partition.py::test_mixed_mesh_three_levels_from_device_partitions."""
    capi = _capi()
    prob = pr.poisson3d_mixed_problem((16, 16, 8), (4, 4, 2), coarse_blk=[(2, 2, 2)], wedges="half")
    params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3, coarse_rtol=1e-28)
    epa0 = int(round(prob.NE / (int(np.max(prob.partitions[0])) + 1)))
    P = capi.partition_mesh(np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32), prob.ND, [epa0, 8],
                            elem_ptr=np.ascontiguousarray(prob.elem_ptr, dtype=np.int32), seeding=1)
    h = capi.Hierarchy.from_partitioning(prob, params, P)
    x, it, conv, _ = h.pcg(prob.b, rel_tol=1e-8)
    print("mixed, spaced seeds: parts %s, it %d, res %.2e" % (P.nparts, it, _true_rel_res(prob, x)))
    assert conv and _true_rel_res(prob, x) <= 1e-6
    h.close()
    P.close()
