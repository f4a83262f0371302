"""Meshes shared by the tests of the data at quadrature points (test_elmat_points_model.py, test_gpu_elmat_points.py): one small
mesh per element type from the existing case modules, each undeformed ("box": affine elements on the unit square / cube) and
jittered, the mixed lists, and the grids of the convergence check."""
import numpy as np

from saamge_amd import elmat_model as em
from saamge_amd import mesh_lift_model as lm
from saamge_amd import mesh_refine_model as rm
from saamge_amd import problems as pr

import elmat_cases as ec
import elmat_p2_cases as pc
import elmat_q2_cases as qc

U = 2.0 ** -53

# type -> (case module, name of its smallest mesh, the module's jitter of the moved variant)
TYPES = {
    "tri3": (ec, "tris_4x3", True), "quad4": (ec, "quads_4x3", True), "tet4": (ec, "tets_3x2x2", True),
    "hex8": (ec, "hex_3x2x2", True), "wedge6": (None, "wedges_2", True),
    "quad9": (qc, "quad9_4x3", "curved"), "hex27": (qc, "hex27_3x2x2", "curved"),
    "tri6": (pc, "tri6_5x3", "curved"), "tet10": (pc, "tet10_3x2x2", "curved"),
}
ORDER = {"tri3": 1, "quad4": 1, "tet4": 1, "hex8": 1, "wedge6": 1, "quad9": 2, "hex27": 2, "tri6": 2, "tet10": 2}
_meshes = {}


def _wedges(n):
    p = pr.poisson3d_mixed_problem(n, (2, 2, 2), wedges="all")
    return pr.grid_coords(n), np.ascontiguousarray(p.elem_to_dof.astype(np.int32).reshape(-1, 6))


def mesh(kind, moved=False):
    """(coords, elem_to_vertex, elem_ptr) of the type's mesh; moved: jittered (order 1) / curved (order 2)"""
    key = (kind, moved)
    if key not in _meshes:
        mod, name, jit = TYPES[kind]
        if mod is None:
            X, e2v = _wedges(2)
            _meshes[key] = (pr.jitter(X, (2, 2, 2), ec.JITTER, seed=7) if moved else X, e2v, None)
        elif mod is ec:
            _meshes[key] = mod.mesh(name, moved)
        else:
            _meshes[key] = mod.mesh(name, jit if moved else "box")
    return _meshes[key]


def mixed(name):
    """the mixed lists: "3d" hexes and wedges, then tetrahedra on their own vertices (all three 3-D order-1 types); "2d" the
    triangles, 6-node triangles and 9-node quadrilaterals of elmat_p2_cases"""
    if name not in _meshes:
        if name == "2d":
            _meshes[name] = pc.mesh("mixed_tri3_tri6_quad9", "curved")
        else:
            X, e2v, ep = ec.mesh("mixed_4", True)
            Xt, t2v, _ = ec.mesh("tets_3x2x2", True)
            lists = np.concatenate([e2v, (t2v[:20] + len(X)).ravel()]).astype(np.int32)
            ptr = np.concatenate([ep, ep[-1] + 4 * np.arange(1, 21)]).astype(np.int32)
            _meshes[name] = (np.ascontiguousarray(np.concatenate([X, Xt])), lists, ptr)
    return _meshes[name]


def nodal(X, vdim, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (len(X), vdim))


def rule_constants(dim, nd):
    """(L, G) of a type's mass rule from the model's tables: L = max over the points of sum_a |N_a|, G = max over the points of
    sum_a max_k |dN_a[k]| -- the condition numbers of the sums over the nodes (L = 1 for the order-1 types: N_a >= 0)."""
    nq = em.MASS_NPOINTS[(dim, nd)]
    L = max(sum(abs(v) for v in em.shape_values(dim, nd, q)) for q in range(nq))
    G = max(sum(max(abs(c) for c in d) for d in em.mass_reference_gradients(dim, nd, q)) for q in range(nq))
    return L, G


def convergence_grids(kind):
    """three meshes (coords, lists) of the type with the mesh widths 1/4, 1/8, 1/16 on the unit square / cube: the 4^2 / 4^3
    grid refined with mesh_refine_model one and two levels and, for order 2, lifted with mesh_lift_model afterwards.  The
    refinement refuses wedges: their three grids are built directly."""
    if kind == "wedge6":
        return [_wedges(n) for n in (4, 8, 16)]
    dim = 2 if kind in ("tri3", "quad4", "tri6", "quad9") else 3
    if kind in ("tri3", "tri6"):
        X, e2v = pr.grid_coords((4, 4)), pr.quads_to_tris(4, 4)
    elif kind in ("quad4", "quad9"):
        p = pr.quad_mesh_problem(4, 4, coef=1.0)
        X, e2v = np.ascontiguousarray(p.coords), p.elem_to_dof.astype(np.int32)
    elif kind in ("tet4", "tet10"):
        X, e2v = pr.grid_coords(4), pr.hex_to_tets(4)
    else:
        X, e2v = pr.grid_coords(4), ec.hex_vertices((4, 4, 4))
    out = [(X, e2v)]
    for levels in (1, 2):
        R = rm.refine(len(X), dim, X, e2v, None, levels)
        out.append((R.coords, R.lists()))
    if ORDER[kind] == 2:
        lifted = []
        for Xl, vl in out:
            L = lm.lift_order2(len(Xl), dim, Xl, vl)
            lifted.append((L.coords2, L.lists()))
        out = lifted
    return out
