"""GPU tests of the partitioner's boundary refinement (csrc/partition.hip) through the C ABI: exact integer agreement with the
CPU model (saamge_amd/partition_model.py, "refine") in labels and counts, on graphs and on meshes; refusals; device memory;
and a hierarchy built from refined partitions."""
import ctypes as C
import math

import numpy as np
import pytest

from saamge_amd import partition_model as pm
from saamge_amd import problems as pr

import partition_cases as pc
import partition_growth_cases as gc
import partition_refine_cases as rc

pytestmark = pytest.mark.gpu

_KEYS = ("rounds", "moved", "gain", "converged")


def _capi():
    from saamge_amd import capi
    capi.load()
    return capi


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", rc.NAMES)
def test_partition_refine_equals_the_model(name):
    capi = _capi()
    c = rc.get(name)
    ref, want, _ = rc.model(name)
    ref_numbered = pm.renumber(ref.astype(np.int64), c.nparts)[0]
    args = (c.rounds, c.max_size, c.min_size, c.seed)
    for renumber, expect in ((0, ref), (1, ref_numbered)):
        live0 = capi.memory_stats()[0]
        part, info = capi.partition_refine(c.n, c.xadj, c.adj, c.nparts, c.part.copy(), *args, renumber=renumber)
        assert capi.memory_stats()[0] == live0
        assert [info[k] for k in _KEYS] == want, (info, want)
        assert [capi.partition_refine_info()[k] for k in _KEYS] == want
        assert np.array_equal(part, expect), "host pointers, renumber %d" % renumber
        dpart = _dev(c.part)
        _, info = capi.partition_refine(c.n, _dev(c.xadj), _dev(c.adj), c.nparts, dpart, *args, renumber=renumber)
        assert [info[k] for k in _KEYS] == want
        assert np.array_equal(dpart.cpu().numpy(), expect), "device pointers, renumber %d" % renumber


@pytest.mark.parametrize("name", ["hex12_face", "hex12_vertex", "mixed4_perm"])
@pytest.mark.parametrize("growth", [0, 1])
def test_partition_graph_then_refine_equals_the_model(name, growth):
    capi = _capi()
    n, xadj, adj, epa, opts = gc.cases()[name]
    want = []
    ref, nref = pm.partition_graph(n, xadj, adj, epa, growth=growth, refine_rounds=16, refine_info=want, **opts)
    part, npt = capi.partition_graph(n, xadj, adj, epa, growth=growth, **opts)
    max_size, min_size = pm.resolve_sizes(epa)
    part, info = capi.partition_refine(n, xadj, adj, npt, part, 16, max_size, min_size, opts.get("seed", 0), renumber=True)
    assert npt == nref and [info[k] for k in _KEYS] == want and want[1] > 0
    assert np.array_equal(part, ref)
    pc.check_partition(n, xadj, adj, part, npt, max_size)


@pytest.mark.parametrize("min_shared", [1, 4])
@pytest.mark.parametrize("growth", [0, 1])
def test_partition_mesh_refined_equals_the_model_on_all_levels(min_shared, growth):
    capi = _capi()
    ep, e2d, ND = pc.hex_mesh(12)
    epa, rounds = [27, 4], [16, 16]
    want = []
    parts, nparts, graphs = pm.partition_mesh(ep, e2d, ND, epa, min_shared=min_shared, growth=growth, refine_rounds=rounds,
                                              refine_info=want)
    plain = pm.partition_mesh(ep, e2d, ND, epa, min_shared=min_shared, growth=growth)
    assert not np.array_equal(parts[0], plain[0][0])          # the pass does something here
    for device_in in (False, True):
        a, b = (_dev(e2d), _dev(ep)) if device_in else (e2d, ep)
        live0 = capi.memory_stats()[0]
        P = capi.partition_mesh(a, ND, epa, elem_ptr=b, min_shared=min_shared, growth=growth, refine_rounds=rounds)
        info = capi.partition_refine_info()
        assert P.nparts == nparts, (P.nparts, nparts)
        for k in range(3):
            xadj, adj = P.graph(k)
            assert np.array_equal(xadj, graphs[k][0]) and np.array_equal(adj, graphs[k][1]), "graph %d" % k
        for k in range(2):
            assert np.array_equal(P.part(k), parts[k]), "partition %d" % k
        assert [info[k] for k in _KEYS] == want        # the last level's pass
        P.close()
        assert capi.memory_stats()[0] == live0
    # no rounds, as NULL and as zeros: the entry point without the pass
    Q = capi.partition_mesh(e2d, ND, epa, elem_ptr=ep, min_shared=min_shared, growth=growth)
    for rr in (None, [0, 0]):
        lib = capi.load()
        o = capi.partition_options(min_shared=min_shared, growth=growth)
        h = C.c_void_p()
        cepa = (C.c_int * 2)(*epa)
        crr = None if rr is None else (C.c_int * 2)(*rr)
        rc_ = lib.saamge_amd_partition_mesh_refined(C.c_int(len(ep) - 1), C.c_int(0), ep.ctypes.data_as(C.c_void_p),
                                                    e2d.ctypes.data_as(C.c_void_p), C.c_int(ND), C.c_int(2), cepa, C.byref(o), crr,
                                                    None, C.byref(h))
        assert rc_ == 0
        for k in range(2):
            got = np.zeros(Q.n_elem[k], np.int32)
            assert lib.saamge_amd_partitioning_get(h, C.c_int(k), got.ctypes.data_as(C.c_void_p), None, None) == 0
            assert np.array_equal(got, Q.part(k)) and np.array_equal(got, plain[0][k])
        free = lib.saamge_amd_partitioning_free
        free.restype = None
        free(h)
    Q.close()


def test_partition_mesh_refine_record_without_a_pass():
    """What saamge_amd_partition_refine_info reports after the mesh entry when the last level has no pass: zeros when
    refine_rounds is given with 0 rounds there (not the counts of level 0, which moves nodes), and the counts of the earlier
    call, untouched, when refine_rounds is NULL."""
    capi = _capi()
    lib = capi.load()
    ep, e2d, ND = pc.hex_mesh(12)
    epa, rounds = [27, 4], [16, 0]
    want = []
    parts, nparts, _ = pm.partition_mesh(ep, e2d, ND, epa, refine_rounds=rounds, refine_info=want)
    plain = pm.partition_mesh(ep, e2d, ND, epa)
    assert want == [0, 0, 0, 0]
    assert not np.array_equal(parts[0], plain[0][0])          # level 0 moved nodes: the zeros are not what it left
    P = capi.partition_mesh(e2d, ND, epa, elem_ptr=ep, refine_rounds=rounds)
    info = capi.partition_refine_info()
    assert P.nparts == nparts, (P.nparts, nparts)
    for k in range(2):
        assert np.array_equal(P.part(k), parts[k]), "partition %d" % k
    assert [info[k] for k in _KEYS] == want
    P.close()
    # a pass with counts, then the mesh entry without refine_rounds
    c = rc.get("hex12_vertex")
    _, left, _ = rc.model("hex12_vertex")
    assert left[1] > 0
    capi.partition_refine(c.n, c.xadj, c.adj, c.nparts, c.part.copy(), c.rounds, c.max_size, c.min_size, c.seed)
    assert [capi.partition_refine_info()[k] for k in _KEYS] == left
    o = capi.partition_options(growth=0)      # (the _v2 struct, which this entry reads)
    h = C.c_void_p()
    rc_ = lib.saamge_amd_partition_mesh_refined(C.c_int(len(ep) - 1), C.c_int(0), ep.ctypes.data_as(C.c_void_p),
                                                e2d.ctypes.data_as(C.c_void_p), C.c_int(ND), C.c_int(2), (C.c_int * 2)(*epa),
                                                C.byref(o), None, None, C.byref(h))
    assert rc_ == 0
    assert [capi.partition_refine_info()[k] for k in _KEYS] == left
    free = lib.saamge_amd_partitioning_free
    free.restype = None
    free(h)


def test_refusals_leave_the_outputs_untouched():
    capi = _capi()
    lib = capi.load()
    c = rc.get("two_hops")
    good = dict(n=c.n, xadj=c.xadj, adj=c.adj, nparts=c.nparts, part=c.part, rounds=4, max_size=0, min_size=0, renumber=0)
    asym = c.adj.copy()
    asym[0] = 6 if asym[0] != 6 else 5          # an entry without its transpose
    bad_label = c.part.copy()
    bad_label[0] = c.nparts
    neg_label = c.part.copy()
    neg_label[3] = -1
    one_short = np.where(c.part == 2, 0, c.part).astype(np.int32)      # labels 0, 1 with nparts 3: part 2 is empty
    outside = c.adj.copy()
    outside[0] = c.n
    for what, match in ((dict(adj=asym), "symmetric"), (dict(adj=outside), "outside"), (dict(xadj=c.xadj[::-1].copy()), "xadj"),
                        (dict(part=bad_label), "label"), (dict(part=neg_label), "label"), (dict(part=one_short), "empty"),
                        (dict(rounds=-1), "rounds"), (dict(max_size=-1), "max_size"), (dict(min_size=-2), "min_size"),
                        (dict(renumber=2), "renumber"), (dict(renumber=-1), "renumber"), (dict(nparts=0), "nparts"),
                        (dict(nparts=c.n + 1), "nparts")):
        kw = dict(good)
        kw.update(what)
        for on_device in (False, True):
            before = np.ascontiguousarray(kw["part"], np.int32).copy()
            part = _dev(before) if on_device else before.copy()
            with pytest.raises(RuntimeError, match=match):
                capi.partition_refine(kw["n"], kw["xadj"], kw["adj"], kw["nparts"], part, kw["rounds"], kw["max_size"],
                                      kw["min_size"], 0, renumber=kw["renumber"])
            after = part.cpu().numpy() if on_device else part
            assert np.array_equal(after, before), what
    # the mesh entry: bad rounds leave the handle alone
    mesh, _ = pc.mesh_cases(4)["mixed"]
    h = C.c_void_p(7)
    epa, rr = (C.c_int * 1)(8), (C.c_int * 1)(-1)
    o = capi.partition_options(growth=0)
    rc_ = lib.saamge_amd_partition_mesh_refined(C.c_int(len(mesh[0]) - 1), C.c_int(0), mesh[0].ctypes.data_as(C.c_void_p),
                                                mesh[1].ctypes.data_as(C.c_void_p), C.c_int(mesh[2]), C.c_int(1), epa, C.byref(o), rr,
                                                None, C.byref(h))
    assert rc_ != 0 and h.value == 7
    with pytest.raises(ValueError):
        capi.partition_mesh(mesh[1], mesh[2], [8], elem_ptr=mesh[0], refine_rounds=[1, 1])


def test_nothing_outlives_the_calls():
    capi = _capi()
    c = rc.get("hex12_vertex")
    live0, _ = capi.memory_stats(reset_peak=True)
    capi.partition_refine(c.n, c.xadj, c.adj, c.nparts, c.part.copy(), 8, c.max_size, c.min_size, renumber=True)
    live1, peak1 = capi.memory_stats()
    assert live1 == live0 and peak1 > live0
    capi.partition_refine(c.n, c.xadj, c.adj, c.nparts, c.part.copy(), 0, c.max_size, c.min_size)       # nothing to do
    capi.partition_refine(0, np.zeros(1, np.int64), np.zeros(0, np.int32), 0, np.zeros(0, np.int32), 4)  # an empty graph
    assert capi.memory_stats()[0] == live0


def _true_rel_res(prob, x):
    return np.linalg.norm(prob.A @ x - prob.b) / np.linalg.norm(prob.b)


def test_poisson32_three_levels_from_refined_partitions():
    """The bounds of test_gpu_partition_growth.py::test_poisson32_three_levels_from_balanced_growth, against the same box
    hierarchy, for partitions refined with 32 rounds per level.  The printed lines hold the figures recorded in DESIGN.md
    section 4.5 beside the unrefined ones."""
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
    for rounds in ([0, 0], [32, 32]):
        P = capi.partition_mesh(e2d, prob.ND, [256, 8], refine_rounds=rounds)
        h = capi.Hierarchy.from_partitioning(prob, params, P)
        x, it, conv, _ = h.pcg(prob.b, rel_tol=1e-8)
        r = _true_rel_res(prob, x)
        print("refine_rounds %s: parts %s it %d res %.2e %s" % (rounds, P.nparts, it, r, figures(h)))
        h.close()
        P.close()
        if rounds[0]:
            assert conv
            assert r <= 1e-6 and r <= 10.0 * max(rb, 1e-16)
            assert it <= math.ceil(1.5 * itb), (it, itb)
