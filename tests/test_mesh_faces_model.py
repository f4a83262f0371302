"""saamge_amd/mesh_model.py held to what is known without it: problems.boundary_faces, partition_model.build_element_graph,
the counts of a box, the invariants of a face table, and the integers of the small cases written out here."""
import numpy as np
import pytest

from saamge_amd import elmat_model as em
from saamge_amd import mesh_model as mm
from saamge_amd import partition_model as pm
from saamge_amd import problems as pr

import bdr_forms_cases as bc
import mesh_faces_cases as mc

EXISTING = [n for _, n in mc.EXISTING]


def test_there_are_22_existing_meshes():
    assert len(EXISTING) == 22 and len(set(EXISTING)) == 22


@pytest.mark.parametrize("name", EXISTING)
def test_boundary_list_is_problems_boundary_faces(name):
    NV, dim, e2v, ep = mc.case(name)
    T = mc.table(name)
    fe, fl = pr.boundary_faces(dim, e2v, ep)
    assert np.array_equal(T.bdr_elem, fe) and np.array_equal(T.bdr_local, fl)
    assert T.bdr_elem.dtype == np.int32 and T.bdr_local.dtype == np.int32
    assert T.info[4] == 0 and T.info[6] == -1      # no mixed-order pair, no non-manifold face on these meshes


@pytest.mark.parametrize("name", sorted(mc.PURE_MIN_SHARED))
def test_graph_is_the_partitioner_graph_with_the_face_count(name):
    NV, dim, e2v, ep = mc.case(name)
    T = mc.table(name)
    nd = mc.node_counts(e2v, ep)
    xadj, adj = pm.build_element_graph(np.concatenate([[0], np.cumsum(nd)]), e2v.ravel(), NV, min_shared=mc.PURE_MIN_SHARED[name])
    assert np.array_equal(T.xadj, xadj) and np.array_equal(T.adj, adj)
    assert T.xadj.dtype == np.int64 and T.adj.dtype == np.int32


@pytest.mark.parametrize("name,n", [("hex_3x2x2", (3, 2, 2)), ("hex_5x4x3", (5, 4, 3)), ("hex_9x8x7", (9, 8, 7)),
                                    ("hex27_5x4x3", (5, 4, 3))])
def test_box_counts(name, n):
    nx, ny, nz = n
    sides = nx * ny + ny * nz + nx * nz
    T = mc.table(name)
    assert T.info[0] == 6 * nx * ny * nz
    assert T.info[2] == 2 * sides and T.info[1] == 3 * nx * ny * nz - sides
    assert T.info[3] == 2 * T.info[1] and T.info[5] == 8 and T.info[7] == 0


@pytest.mark.parametrize("name", mc.NAMES)
def test_invariants(name):
    NV, dim, e2v, ep = mc.case(name)
    T = mc.table(name)
    S = int(T.slot_ptr[-1])
    nd = mc.node_counts(e2v, ep)
    assert T.slot_ptr.dtype == np.int64 and len(T.slot_ptr) == len(nd) + 1
    assert np.array_equal(np.diff(T.slot_ptr), [len(em.FACE_NODES[(dim, int(c))]) for c in nd])
    assert T.info[0] == S == 2 * T.info[1] + T.info[2]
    inner = np.flatnonzero(T.nbr_elem >= 0)
    assert np.array_equal(T.nbr_local < 0, T.nbr_elem < 0)
    across = T.slot_ptr[T.nbr_elem[inner]] + T.nbr_local[inner]
    assert np.array_equal(T.slot_ptr[T.nbr_elem[across]] + T.nbr_local[across], inner)      # the slot across the slot across s is s
    selem = np.repeat(np.arange(len(nd)), np.diff(T.slot_ptr))
    assert (T.nbr_elem[inner] != selem[inner]).all()
    rows = np.repeat(np.arange(len(nd)), np.diff(T.xadj))
    assert T.info[3] == len(T.adj) == T.xadj[-1]
    assert set(zip(rows.tolist(), T.adj.tolist())) == set(zip(T.adj.tolist(), rows.tolist()))      # symmetric
    assert (rows != T.adj).all()
    for e in range(len(nd)):
        r = T.adj[T.xadj[e]:T.xadj[e + 1]]
        assert (np.diff(r) > 0).all()
    assert T.info[7] == int((np.diff(T.xadj) == 0).sum())
    assert T.info[5] == (int(np.bincount(e2v.ravel()).max()) if e2v.size else 0)


# ---- the integers of the added cases, written out --------------------------------------------------------------------------------
INFO = {
    "pair_rotated_hex": [12, 1, 10, 2, 0, 2, -1, 0],
    "pair_rotated_tet": [8, 1, 6, 2, 0, 2, -1, 0],
    "pair_wedge_hex": [11, 1, 9, 2, 0, 2, -1, 0],
    "pair_wedge_tet": [9, 1, 7, 2, 0, 2, -1, 0],
    "hex8_on_hex27": [12, 1, 10, 2, 1, 2, -1, 0],
    "double_contact": [8, 2, 4, 2, 0, 2, -1, 0],
    "fan_70": [210, 70, 70, 140, 0, 70, -1, 0],
    "renumbered_hex_5x4x3": [360, 133, 94, 266, 0, 8, -1, 0],
    "hole": [324, 104, 116, 208, 0, 7, -1, 0],
    "two_blocks": [144, 40, 64, 80, 0, 8, -1, 0],
    "empty": [0, 0, 0, 0, 0, 0, -1, 0],
    "isolated": [8, 0, 8, 0, 0, 2, -1, 2],
}
# the only interior slots: (element, local face) -> (element, local face) across
PAIRS = {
    "pair_rotated_hex": {(0, 2): (1, 3)},
    "pair_rotated_tet": {(0, 0): (1, 1)},
    "pair_wedge_hex": {(0, 2): (1, 5)},
    "pair_wedge_tet": {(0, 1): (1, 0)},
    "hex8_on_hex27": {(0, 5): (1, 0)},
    "double_contact": {(0, 0): (1, 0), (0, 1): (1, 1)},
}


@pytest.mark.parametrize("name", sorted(INFO))
def test_added_case_info(name):
    assert mc.table(name).info == INFO[name]


@pytest.mark.parametrize("name", ["single_%d_%d" % t for t in mc.TYPES])
def test_single_element(name):
    NV, dim, e2v, ep = mc.case(name)
    T = mc.table(name)
    nf = len(em.FACE_NODES[(dim, e2v.shape[1])])
    assert T.info == [nf, 0, nf, 0, 0, 1, -1, 1]
    assert np.array_equal(T.nbr_elem, -np.ones(nf)) and np.array_equal(T.nbr_local, -np.ones(nf))
    assert np.array_equal(T.bdr_elem, np.zeros(nf)) and np.array_equal(T.bdr_local, np.arange(nf))
    assert np.array_equal(T.xadj, [0, 0]) and len(T.adj) == 0


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_pairs_written_out(name):
    T = mc.table(name)
    want_e, want_l = -np.ones(T.info[0], np.int64), -np.ones(T.info[0], np.int64)
    for (e, l), (f, m) in PAIRS[name].items():
        want_e[T.slot_ptr[e] + l], want_l[T.slot_ptr[e] + l] = f, m
        want_e[T.slot_ptr[f] + m], want_l[T.slot_ptr[f] + m] = e, l
    assert np.array_equal(T.nbr_elem, want_e) and np.array_equal(T.nbr_local, want_l)
    assert np.array_equal(T.xadj, [0, 1, 2]) and np.array_equal(T.adj, [1, 0])


def test_fan():
    T = mc.table("fan_70")
    k = np.arange(70)
    # triangle k = (0, 1 + k, 1 + (k + 1) % 70): face 0 meets face 2 of triangle k - 1, face 1 is the rim
    assert np.array_equal(T.nbr_elem.reshape(70, 3), np.stack([(k - 1) % 70, -1 + 0 * k, (k + 1) % 70], axis=1))
    assert np.array_equal(T.nbr_local.reshape(70, 3), np.stack([2 + 0 * k, -1 + 0 * k, 0 * k], axis=1))
    assert np.array_equal(T.bdr_elem, k) and np.array_equal(T.bdr_local, 1 + 0 * k)


def test_renumbered_is_the_relabelled_table():
    T0, T1 = mc.table("hex_5x4x3"), mc.table("renumbered_hex_5x4x3")
    pe, _ = mc.renumbering()
    inv = np.empty_like(pe)
    inv[pe] = np.arange(len(pe))
    old = T0.nbr_elem.reshape(-1, 6)[pe]                      # new element k is old element pe[k]; the local faces keep their index
    assert np.array_equal(T1.nbr_elem.reshape(-1, 6), np.where(old < 0, -1, inv[np.maximum(old, 0)]))
    assert np.array_equal(T1.nbr_local.reshape(-1, 6), T0.nbr_local.reshape(-1, 6)[pe])


def test_hole_has_boundary_faces_inside():
    NV, dim, e2v, ep = mc.case("hole")
    T = mc.table("hole")
    X = mc.coords("hex_5x4x3")
    _, nodes = mm.face_nodes(dim, e2v, ep, T.bdr_elem, T.bdr_local)
    centre = X[nodes.reshape(-1, 4)].mean(axis=1)
    inside = ((centre > 0.0) & (centre < 1.0)).all(axis=1)
    assert inside.sum() == 22 and len(inside) == 116


def test_two_blocks_is_disconnected():
    T = mc.table("two_blocks")
    rows = np.repeat(np.arange(24), np.diff(T.xadj))
    assert ((rows < 12) == (T.adj < 12)).all()
    half = mc.table("hex_3x2x2")
    assert np.array_equal(T.adj[:len(half.adj)], half.adj) and np.array_equal(T.adj[len(half.adj):], half.adj + 12)


@pytest.mark.parametrize("name", sorted(mc.NONMANIFOLD))
def test_nonmanifold_is_refused(name):
    NV, dim, e2v, ep = mc.case(name)
    with pytest.raises(mm.MeshError) as r:
        mm.FaceTable(NV, dim, e2v, ep)
    assert r.value.element == 0 and r.value.info[6] == 0


def test_nonmanifold_names_the_lowest_element():
    # a tetrahedron in front that has no part in it: the three on one face are elements 1, 2, 3
    e2v = np.array([[6, 7, 8, 9], [0, 1, 2, 3], [4, 1, 2, 3], [5, 1, 2, 3]], np.int32)
    with pytest.raises(mm.MeshError) as r:
        mm.FaceTable(10, 3, e2v)
    assert r.value.element == 1


@pytest.mark.parametrize("name", sorted(mc.REFUSED_MESHES))
def test_mesh_refusals(name):
    NV, dim, e2v, ep, word = mc.REFUSED_MESHES[name]
    with pytest.raises(ValueError, match=word):
        mm.FaceTable(NV, dim, e2v, ep)
    with pytest.raises(ValueError, match=word):
        mm.face_nodes(dim, e2v, ep, np.zeros(1, np.int32), np.zeros(1, np.int32), NV=NV)


# ---- the face-list calls ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXISTING)
def test_face_nodes_are_the_face_vertices(name):
    NV, dim, e2v, ep = mc.case(name)
    for variant, (fe, fl) in mc.face_variants(name).items():
        ptr, nodes = mm.face_nodes(dim, e2v, ep, fe, fl)
        want = bc.face_vertices(dim, e2v, ep, fe, fl)
        assert ptr.dtype == np.int32 and nodes.dtype == np.int32
        assert np.array_equal(ptr, np.concatenate([[0], np.cumsum([len(v) for v in want])]))
        assert np.array_equal(nodes, np.concatenate(want))


@pytest.mark.parametrize("name", ["hex_5x4x3", "mixed_4", "quads_4x3", "quad9_4x3", "tet10_3x2x2", "mixed_tet4_tet10_hex27"])
def test_face_dofs_against_a_loop(name):
    NV, dim, e2v, ep = mc.case(name)
    nd = mc.node_counts(e2v, ep)
    off = np.concatenate([[0], np.cumsum(nd)])
    flat = e2v.ravel()
    for variant, (fe, fl) in mc.face_variants(name).items():
        for vdim in (1, dim):
            for mask in sorted({1, 2, 2 ** dim - 1}):
                if mask >= 2 ** vdim:
                    with pytest.raises(ValueError, match="comp_mask"):
                        mm.face_dofs(dim, e2v, ep, fe, fl, vdim, mask, 0x02, np.zeros(vdim * NV, np.int8))
                    continue
                for flag in (0x02, 0x05):
                    before = np.random.default_rng(19).integers(0, 8, vdim * NV).astype(np.int8)      # bits set beforehand
                    want, touched = before.copy(), set()
                    for e, l in zip(fe, fl):
                        for a in em.FACE_NODES[(dim, int(nd[e]))][l]:
                            touched.add(int(flat[off[e] + a]))
                            for i in range(vdim):
                                if (mask >> i) & 1:
                                    want[vdim * flat[off[e] + a] + i] |= flag
                    got = before.copy()
                    info = mm.face_dofs(dim, e2v, ep, fe, fl, vdim, mask, flag, got)
                    assert np.array_equal(got, want)
                    assert info == [len(fe), len(touched), int((want != before).sum()), -1]


def test_face_dofs_on_all_boundary_faces_marks_the_boundary_of_the_box():
    NV, dim, e2v, ep = mc.case("hex_5x4x3")
    T = mc.table("hex_5x4x3")
    X = mc.coords("hex_5x4x3")
    flags = np.zeros(NV, np.int8)
    mm.face_dofs(dim, e2v, ep, T.bdr_elem, T.bdr_local, 1, 1, 0x02, flags)
    on = ((X == 0.0) | (X == 1.0)).any(axis=1)
    assert np.array_equal(flags != 0, on)


def test_face_list_refusals():
    NV, dim, e2v, ep = mc.case("mixed_4")
    nd = mc.node_counts(e2v, ep)
    wedge = int(np.flatnonzero(nd == 6)[0])
    ok_e, ok_l = np.array([0, 1, 2, 3], np.int32), np.array([0, 0, 0, 0], np.int32)
    cases = [(np.array([0, 1, len(nd), -1]), ok_l, 2, "face_elem"),
             (np.array([0, -3, 2, len(nd)]), ok_l, 1, "face_elem"),
             (np.array([0, wedge, wedge]), np.array([0, 5, 7]), 1, "face_local"),
             (np.array([0, 1, 2]), np.array([0, -1, 0]), 1, "face_local"),
             (np.array([3, 0, 1, 0, 1]), np.array([0, 2, 1, 2, 1]), 1, "twice")]
    for fe, fl, index, word in cases:
        for call in (lambda: mm.face_nodes(dim, e2v, ep, fe, fl),
                     lambda: mm.face_dofs(dim, e2v, ep, fe, fl, 1, 1, 2, np.zeros(NV, np.int8))):
            with pytest.raises(em.FaceError, match=word) as r:
                call()
            assert r.value.face == index
    flags = np.zeros(NV, np.int8)
    for vdim, mask, flag, word in [(2, 1, 2, "vdim"), (1, 0, 2, "comp_mask"), (1, 2, 2, "comp_mask"), (3, 8, 2, "comp_mask"),
                                   (1, 1, 0, "flag"), (1, 1, 128, "flag")]:
        with pytest.raises(ValueError, match=word):
            mm.face_dofs(dim, e2v, ep, ok_e, ok_l, vdim, mask, flag, np.zeros(vdim * NV, np.int8) if vdim in (1, 3) else flags)
    assert not flags.any()
    assert mm.face_nodes(dim, e2v, ep, np.zeros(0, np.int32), np.zeros(0, np.int32))[0].tolist() == [0]      # NF = 0 is legal
