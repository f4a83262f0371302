"""GPU tests of the partitioner's balanced growth (`growth = 1`, csrc/partition.hip) through the C ABI: exact integer agreement
with the CPU model (saamge_amd/partition_model.py) in partitions and counts, refusal of other values, device memory, and a
hierarchy built from its partitions."""
import ctypes as C
import math

import numpy as np
import pytest

from saamge_amd import partition_model as pm
from saamge_amd import problems as pr

import partition_cases as pc
import partition_growth_cases as gc

pytestmark = pytest.mark.gpu

_CASES = None
_KEYS = ("rounds", "quota_nodes", "open_parts", "released_nodes")


def _capi():
    from saamge_amd import capi
    capi.load()
    return capi


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cases():
    global _CASES
    if _CASES is None:
        _CASES = gc.cases()
    return _CASES


@pytest.mark.parametrize("name", gc.NAMES)
def test_partition_graph_equals_the_model(name):
    import torch
    capi = _capi()
    n, xadj, adj, epa, opts = _cases()[name]
    want = []
    ref, nref = pm.partition_graph(n, xadj, adj, epa, growth=1, growth_info=want, **opts)
    live0 = capi.memory_stats()[0]
    part, npt = capi.partition_graph(n, xadj, adj, epa, growth=1, **opts)
    info = capi.partition_growth_info()
    assert capi.memory_stats()[0] == live0
    assert npt == nref and np.array_equal(part, ref)
    assert [info[k] for k in _KEYS] == want, (info, want)
    dpart = torch.empty(n, dtype=torch.int32, device="cuda")
    _, npt = capi.partition_graph(n, _dev(xadj), _dev(adj), epa, part=dpart, growth=1, **opts)
    assert npt == nref and np.array_equal(dpart.cpu().numpy(), ref)         # device pointers: the same result
    assert [capi.partition_growth_info()[k] for k in _KEYS] == want
    # growth = 0 afterwards: the default's partition, and the counts are cleared
    ref0, nref0 = pm.partition_graph(n, xadj, adj, epa, **opts)
    part0, npt0 = capi.partition_graph(n, xadj, adj, epa, growth=0, **opts)
    assert npt0 == nref0 and np.array_equal(part0, ref0)
    assert [capi.partition_growth_info()[k] for k in _KEYS] == [0, 0, 0, 0]


def test_partition_mesh_equals_the_model_on_all_levels():
    capi = _capi()
    ep, e2d, ND = pc.hex_mesh(12)
    epa = [27, 4]
    for ms in (1, 4):
        want = []
        parts, nparts, graphs = pm.partition_mesh(ep, e2d, ND, epa, min_shared=ms, growth=1, growth_info=want)
        got = []
        for device_in in (False, True):
            a, b = (_dev(e2d), _dev(ep)) if device_in else (e2d, ep)
            live0 = capi.memory_stats()[0]
            P = capi.partition_mesh(a, ND, epa, elem_ptr=b, min_shared=ms, growth=1)
            info = capi.partition_growth_info()
            assert P.nparts == nparts, (P.nparts, nparts)
            for k in range(3):
                xadj, adj = P.graph(k)
                assert np.array_equal(xadj, graphs[k][0]) and np.array_equal(adj, graphs[k][1]), "graph %d" % k
            for k in range(2):
                assert np.array_equal(P.part(k), parts[k]), "partition %d" % k
            got.append([P.part(k) for k in range(2)])
            assert [info[k] for k in _KEYS] == want        # the last level's growth
            P.close()
            assert capi.memory_stats()[0] == live0
        assert all(np.array_equal(x, y) for x, y in zip(*got))


@pytest.mark.parametrize("bad", [2, -1])
def test_other_values_are_refused(bad):
    capi = _capi()
    lib = capi.load()
    n, xadj, adj = pc.three_components()
    part = np.full(n, -7, np.int32)
    with pytest.raises(RuntimeError, match="growth"):
        capi.partition_graph(n, xadj, adj, 4, part=part, growth=bad)
    assert (part == -7).all()
    o = capi.partition_options(growth=bad)
    npt = C.c_int(-7)
    rc = lib.saamge_amd_partition_graph_v2(C.c_int(n), xadj.ctypes.data_as(C.c_void_p), adj.ctypes.data_as(C.c_void_p), C.c_int(4),
                                        C.byref(o), None, part.ctypes.data_as(C.c_void_p), C.byref(npt))
    assert rc != 0 and npt.value == -7 and (part == -7).all()
    mesh, _ = pc.mesh_cases(4)["mixed"]
    h = C.c_void_p(7)
    epa = (C.c_int * 1)(8)
    rc = lib.saamge_amd_partition_mesh_v2(C.c_int(len(mesh[0]) - 1), C.c_int(0), mesh[0].ctypes.data_as(C.c_void_p),
                                       mesh[1].ctypes.data_as(C.c_void_p), C.c_int(mesh[2]), C.c_int(1), epa, C.byref(o), None,
                                       C.byref(h))
    assert rc != 0 and h.value == 7
    with pytest.raises(RuntimeError, match="growth"):
        capi.partition_mesh(mesh[1], mesh[2], [8], elem_ptr=mesh[0], growth=bad)
    # a zero-filled struct is today's growth
    z = capi.PartitionOptionsV2()
    d = capi.partition_options(growth=0)
    assert isinstance(d, capi.PartitionOptionsV2) and z.growth == d.growth == 0
    assert not hasattr(capi.partition_options(), "growth")        # the struct without the field keeps its six


def test_nothing_outlives_the_calls():
    capi = _capi()
    n, xadj, adj, epa, _ = _cases()["hex12_vertex"]
    live0, _ = capi.memory_stats(reset_peak=True)
    capi.partition_graph(n, xadj, adj, epa, lloyd_iters=1, growth=1)
    live1, peak1 = capi.memory_stats()
    assert live1 == live0 and peak1 > live0
    capi.partition_graph(n, xadj, adj, 1, growth=1)             # nothing to grow
    capi.partition_graph(n, xadj, adj, 10 ** 6, growth=1)       # one part that never closes
    assert capi.memory_stats()[0] == live0


def _true_rel_res(prob, x):
    return np.linalg.norm(prob.A @ x - prob.b) / np.linalg.norm(prob.b)


def test_poisson32_three_levels_from_balanced_growth():
    """The bounds of test_gpu_partition.py::test_poisson32_three_levels_from_device_partitions, against the same box
    hierarchy.  The printed lines hold the figures recorded in DESIGN.md section 4.5; which growth gives the better ones is
    a measurement and not asserted."""
    capi = _capi()
    prob = pr.poisson3d_problem(32, blk=(8, 8, 4), coarse_blk=[(2, 2, 2)])
    params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3, coarse_rtol=1e-28)

    def figures(h):
        info = [h.level_info(l) for l in range(h.num_levels - 1)]
        nnz = [info[0]["nnz"]] + [i["nnzAc"] for i in info]
        return dict(dims=[info[0]["n"]] + [i["ncoarse"] for i in info], mises=[i["num_mises"] for i in info], nnz=nnz,
                    opc=round(sum(nnz) / float(nnz[0]), 4))

    hb = capi.Hierarchy.from_problem(prob, params)
    xb, itb, convb, _ = hb.pcg(prob.b, rel_tol=1e-8)
    rb = _true_rel_res(prob, xb)
    print("box: it %d res %.2e %s" % (itb, rb, figures(hb)))
    hb.close()
    assert convb
    e2d = np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32)
    for growth in (0, 1):
        P = capi.partition_mesh(e2d, prob.ND, [256, 8], growth=growth)
        h = capi.Hierarchy.from_partitioning(prob, params, P)
        x, it, conv, _ = h.pcg(prob.b, rel_tol=1e-8)
        r = _true_rel_res(prob, x)
        print("growth %d: parts %s it %d res %.2e %s" % (growth, P.nparts, it, r, figures(h)))
        h.close()
        P.close()
        if growth == 1:
            assert conv
            assert r <= 1e-6 and r <= 10.0 * max(rb, 1e-16)
            assert it <= math.ceil(1.5 * itb), (it, itb)
