"""GPU tests of the device partitioner (csrc/partition.hip): exact integer agreement with the CPU model
(saamge_amd/partition_model.py), the enforced properties at a larger size, hierarchies built from its partitions, and its
use of device memory."""
import math

import numpy as np
import pytest

from saamge_amd import partition_model as pm
from saamge_amd import problems as pr

import partition_cases as pc

pytestmark = pytest.mark.gpu


def _capi():
    from saamge_amd import capi
    capi.load()
    return capi


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


CASES24 = None
CASES64 = None


def _cases24():
    global CASES24
    if CASES24 is None:
        CASES24 = pc.mesh_cases(24)
    return CASES24


# ---------------------------------------------------------------------------------------------------------------------
# 1. device = model, integer for integer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hex_vertex", "hex_face", "mixed", "hex_vertex_perm", "hex_face_perm", "mixed_perm"])
def test_partition_mesh_equals_the_model(name):
    capi = _capi()
    mesh, ms = _cases24()[name]
    ep, e2d, ND = mesh
    epa = [48, 6]
    for seed, lloyd, device_in in ((0, 0, False), (0, 0, True), (3, 0, True), (3, 2, False), (3, 2, True)):
        parts, nparts, graphs = pm.partition_mesh(ep, e2d, ND, epa, min_shared=ms, seed=seed, lloyd_iters=lloyd)
        if device_in:
            dep, de2d = _dev(ep), _dev(e2d)
            P = capi.partition_mesh(de2d, ND, epa, elem_ptr=dep, min_shared=ms, seed=seed, lloyd_iters=lloyd)
        elif name.startswith("hex") and not name.endswith("perm"):
            P = capi.partition_mesh(e2d.reshape(-1, 8), ND, epa, min_shared=ms, seed=seed, lloyd_iters=lloyd)   # uniform nde
        else:
            P = capi.partition_mesh(e2d, ND, epa, elem_ptr=ep, min_shared=ms, seed=seed, lloyd_iters=lloyd)
        assert P.nparts == nparts, (P.nparts, nparts)
        for k in range(3):
            xadj, adj = P.graph(k)
            assert np.array_equal(xadj, graphs[k][0]) and np.array_equal(adj, graphs[k][1]), "graph %d" % k
        for k in range(2):
            assert np.array_equal(P.part(k), parts[k]), "partition %d" % k
        # one level through partition_graph, host and device pointers
        xadj, adj = graphs[0]
        n = len(ep) - 1
        part, npt = capi.partition_graph(n, xadj, adj, epa[0], seed=seed, lloyd_iters=lloyd)
        assert npt == nparts[0] and np.array_equal(part, parts[0])
        import torch
        dpart = torch.empty(n, dtype=torch.int32, device="cuda")
        _, npt = capi.partition_graph(n, _dev(xadj), _dev(adj), epa[0], part=dpart, seed=seed, lloyd_iters=lloyd)
        assert npt == nparts[0] and np.array_equal(dpart.cpu().numpy(), parts[0])
        P.close()


@pytest.mark.parametrize("epa", [1, 10 ** 6])
@pytest.mark.parametrize("name", ["hex_vertex", "mixed_perm"])
def test_degenerate_sizes_equal_the_model(name, epa):
    capi = _capi()
    mesh, ms = pc.mesh_cases(12)[name]
    ep, e2d, ND = mesh
    for seed in (0, 3):
        parts, nparts, graphs = pm.partition_mesh(ep, e2d, ND, [epa], min_shared=ms, seed=seed)
        for dev in (False, True):
            a, b = (_dev(e2d), _dev(ep)) if dev else (e2d, ep)
            P = capi.partition_mesh(a, ND, [epa], elem_ptr=b, min_shared=ms, seed=seed)
            assert P.nparts == nparts and np.array_equal(P.part(0), parts[0])
            xq, aq = P.graph(1)
            assert np.array_equal(xq, graphs[1][0]) and np.array_equal(aq, graphs[1][1])
            P.close()
            n = len(ep) - 1
            x, j = (_dev(graphs[0][0]), _dev(graphs[0][1])) if dev else graphs[0]
            part, npt = capi.partition_graph(n, x, j, epa, seed=seed)
            assert npt == nparts[0] and np.array_equal(part, parts[0])


@pytest.mark.parametrize("epa", [1, 4, 100])
def test_three_components_equal_the_model(epa):
    capi = _capi()
    n, xadj, adj = pc.three_components()
    for seed in (0, 3):
        for lloyd in (0, 1):
            ref, nref = pm.partition_graph(n, xadj, adj, epa, seed=seed, lloyd_iters=lloyd)
            part, npt = capi.partition_graph(n, xadj, adj, epa, seed=seed, lloyd_iters=lloyd)
            assert npt == nref and np.array_equal(part, ref)
            pc.check_partition(n, xadj, adj, part, npt, 2 * epa)
            import torch
            dpart = torch.empty(n, dtype=torch.int32, device="cuda")
            _, npt = capi.partition_graph(n, _dev(xadj), _dev(adj), epa, part=dpart, seed=seed, lloyd_iters=lloyd)
            assert npt == nref and np.array_equal(dpart.cpu().numpy(), ref)


def test_small_caps_equal_the_model():
    """A tight cap and a large minimum: many repair and merge rounds."""
    capi = _capi()
    mesh, ms = pc.mesh_cases(12)["mixed_perm"]
    xadj, adj = pm.build_element_graph(mesh[0], mesh[1], mesh[2], ms)
    n = len(mesh[0]) - 1
    for kw in (dict(max_size=40, min_size=20), dict(max_size=0, min_size=30), dict(max_size=33, min_size=0)):
        ref, nref = pm.partition_graph(n, xadj, adj, 32, **kw)
        part, npt = capi.partition_graph(n, xadj, adj, 32, **kw)
        assert npt == nref and np.array_equal(part, ref), kw
        pc.check_partition(n, xadj, adj, part, npt, kw["max_size"])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the enforced properties at 64^3 (checked with scipy, not with the model)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hex_vertex", "hex_face", "mixed", "hex_vertex_perm", "hex_face_perm", "mixed_perm"])
def test_properties_at_64(name):
    capi = _capi()
    global CASES64
    if CASES64 is None:
        CASES64 = pc.mesh_cases(64)
    mesh, ms = CASES64[name]
    ep, e2d, ND = mesh
    epa = [256, 8]
    P = capi.partition_mesh(e2d, ND, epa, elem_ptr=ep, min_shared=ms)
    P2 = capi.partition_mesh(e2d, ND, epa, elem_ptr=ep, min_shared=ms)
    for k in range(2):
        xadj, adj = P.graph(k)
        pc.check_partition(P.n_elem[k], xadj, adj, P.part(k), P.nparts[k], 2 * epa[k])
        assert np.array_equal(P.part(k), P2.part(k))
    P.close()
    P2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. hierarchies from the device partitions
# ---------------------------------------------------------------------------------------------------------------------
def _true_rel_res(prob, x):
    return np.linalg.norm(prob.A @ x - prob.b) / np.linalg.norm(prob.b)


def test_poisson32_three_levels_from_device_partitions():
    """Measured on one MI355X (recorded in DESIGN.md section 4.5): see the printed line."""
    capi = _capi()
    prob = pr.poisson3d_problem(32, blk=(8, 8, 4), coarse_blk=[(2, 2, 2)])
    params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3, coarse_rtol=1e-28)
    hb = capi.Hierarchy.from_problem(prob, params)
    xb, itb, convb, _ = hb.pcg(prob.b, rel_tol=1e-8)
    info_b = [hb.level_info(l) for l in range(hb.num_levels - 1)]
    hb.close()
    # the boxes hold 256 elements, the coarse boxes 8 agglomerates
    P = capi.partition_mesh(np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32), prob.ND, [256, 8])
    for on_host in (False, True):
        h = capi.Hierarchy.from_partitioning(prob, params, P, on_host=on_host)
        x, it, conv, _ = h.pcg(prob.b, rel_tol=1e-8)
        info = [h.level_info(l) for l in range(h.num_levels - 1)]
        h.close()
        rb, r = _true_rel_res(prob, xb), _true_rel_res(prob, x)
        print("box: it %d res %.2e levels %s | device partitions %s (host arrays %s): it %d res %.2e levels %s"
              % (itb, rb, info_b, P.nparts, on_host, it, r, info))
        assert convb and conv
        assert r <= 1e-6 and r <= 10.0 * max(rb, 1e-16)
        assert it <= math.ceil(1.5 * itb), (it, itb)
    P.close()


def test_mixed_mesh_three_levels_from_device_partitions():
    capi = _capi()
    prob = pr.poisson3d_mixed_problem((16, 16, 8), (4, 4, 2), coarse_blk=[(2, 2, 2)], wedges="half")
    params = capi.default_params(num_coarsenings=2, theta=0.003, nu_relax=3, coarse_rtol=1e-28)
    epa0 = int(round(prob.NE / (int(np.max(prob.partitions[0])) + 1)))
    P = capi.partition_mesh(np.ascontiguousarray(prob.elem_to_dof, dtype=np.int32), prob.ND, [epa0, 8],
                            elem_ptr=np.ascontiguousarray(prob.elem_ptr, dtype=np.int32))
    h = capi.Hierarchy.from_partitioning(prob, params, P)
    x, it, conv, _ = h.pcg(prob.b, rel_tol=1e-8)          # max_iter: the default of the existing mixed-element tests
    print("mixed: parts %s, it %d, res %.2e" % (P.nparts, it, _true_rel_res(prob, x)))
    assert conv and _true_rel_res(prob, x) <= 1e-6
    h.close()
    P.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. memory and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_nothing_outlives_the_calls():
    capi = _capi()
    mesh, ms = pc.mesh_cases(12)["mixed"]
    ep, e2d, ND = mesh
    xadj, adj = pm.build_element_graph(ep, e2d, ND, ms)
    n = len(ep) - 1
    live0, _ = capi.memory_stats(reset_peak=True)
    capi.partition_graph(n, xadj, adj, 32, lloyd_iters=1)
    live1, peak1 = capi.memory_stats()
    assert live1 == live0 and peak1 > live0
    P = capi.partition_mesh(e2d, ND, [32, 4], elem_ptr=ep)
    assert capi.memory_stats()[0] > live0
    P.close()
    assert capi.memory_stats()[0] == live0


def test_bad_input_is_refused():
    capi = _capi()
    n, xadj, adj = pc.three_components()
    with pytest.raises(RuntimeError, match="elems_per_agg"):
        capi.partition_graph(n, xadj, adj, 0)
    with pytest.raises(RuntimeError, match="n < 0"):
        capi.partition_graph(-1, xadj, adj, 4)
    bad = adj.copy()
    bad[0] = n
    with pytest.raises(RuntimeError, match="outside"):
        capi.partition_graph(n, xadj, bad, 4)
    v = int(np.flatnonzero(np.diff(xadj) > 0)[0])
    u = int(adj[xadj[v]])
    w = next(w for w in range(n) if w != v and w != u and w not in adj[xadj[v]:xadj[v + 1]])
    asym = adj.copy()
    asym[xadj[v]] = w
    with pytest.raises(RuntimeError, match="symmetric"):
        capi.partition_graph(n, xadj, asym, 4)
    xbad = xadj.copy()
    xbad[3] = xbad[4] + 1
    with pytest.raises(RuntimeError, match="xadj"):
        capi.partition_graph(n, xbad, adj, 4)
    mesh, _ = pc.mesh_cases(4)["mixed"]
    e2d = mesh[1].copy()
    e2d[5] = mesh[2]
    with pytest.raises(RuntimeError, match="out of range"):
        capi.partition_mesh(e2d, mesh[2], [8], elem_ptr=mesh[0])
    e2d = mesh[1].copy()
    e2d[1] = e2d[0]
    with pytest.raises(RuntimeError, match="twice"):
        capi.partition_mesh(e2d, mesh[2], [8], elem_ptr=mesh[0])
    with pytest.raises(ValueError, match="twice"):
        pm.build_element_graph(mesh[0], e2d, mesh[2])
    with pytest.raises(RuntimeError, match="xadj on the device"):
        capi.partition_graph(n, _dev(xadj), adj, 4)


def test_degenerate_and_three_component_cases_at_64_scale_properties():
    """The degenerate sizes on the device output alone, checked with scipy."""
    capi = _capi()
    mesh, ms = pc.mesh_cases(12)["mixed_perm"]
    ep, e2d, ND = mesh
    for epa in (1, 10 ** 6):
        P = capi.partition_mesh(e2d, ND, [epa], elem_ptr=ep, min_shared=ms)
        xadj, adj = P.graph(0)
        pc.check_partition(P.n_elem[0], xadj, adj, P.part(0), P.nparts[0], 2 * epa)
        P.close()
