"""Meshes and coefficients shared by the element-matrix tests (test_elmat_model.py, test_gpu_elmat.py): the smallest meshes that
reach every type, a partial wavefront, several workgroups and a mesh of two types."""
import numpy as np

from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

EPS = 2.220446049250313e-16
JITTER = 0.2


def hex_vertices(n):
    """element -> vertex lists of the hex grid of problems.poisson3d_problem, without building the problem"""
    nx, ny, nz = n
    nvx, nvy = nx + 1, ny + 1
    ez, ey, ex = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ex, ey, ez = ex.ravel(), ey.ravel(), ez.ravel()
    return np.stack([((ez + c) * nvy + ey + b) * nvx + ex + a for (a, b, c) in pr._HEX_LOC], axis=1).astype(np.int32)


def _mixed():
    p = pr.poisson3d_mixed_problem(4, (2, 2, 2), wedges="half")
    return pr.grid_coords(4), p.elem_to_dof.astype(np.int32), p.elem_ptr.astype(np.int32), (4, 4, 4)


def _quads():
    p = pr.mltest_problem()
    return np.ascontiguousarray(p.coords), p.elem_to_dof.astype(np.int32), None, (4, 3)


# name -> (coords, elem_to_vertex, elem_ptr, dims)
MESHES = {
    "hex_3x2x2": lambda: (pr.grid_coords((3, 2, 2)), hex_vertices((3, 2, 2)), None, (3, 2, 2)),      # 12 elements: a partial wavefront
    "hex_5x4x3": lambda: (pr.grid_coords((5, 4, 3)), hex_vertices((5, 4, 3)), None, (5, 4, 3)),      # 60 elements
    "hex_9x8x7": lambda: (pr.grid_coords((9, 8, 7)), hex_vertices((9, 8, 7)), None, (9, 8, 7)),      # several workgroups
    "mixed_4": _mixed,                                                                              # hexes and wedges: two lists
    "tets_3x2x2": lambda: (pr.grid_coords((3, 2, 2)), pr.hex_to_tets((3, 2, 2)), None, (3, 2, 2)),
    "quads_4x3": _quads,
    "tris_4x3": lambda: (_quads()[0], pr.quads_to_tris(4, 3), None, (4, 3)),
}
_meshes = {}


def mesh(name, jittered=False):
    """(coords, elem_to_vertex, elem_ptr); jittered: every vertex moved by up to 0.2 mesh widths"""
    if name not in _meshes:
        _meshes[name] = MESHES[name]()
    X, e2v, ep, dims = _meshes[name]
    if jittered:
        X = pr.jitter(X, dims, JITTER, seed=7)
    return X, e2v, ep


def num_elements(e2v, ep):
    return len(ep) - 1 if ep is not None else e2v.shape[0]


def coefficients(NE, dim, kind, ncoef, seed=5):
    """Per-element coefficients in [0.5, 2), so that a matrix written to the wrong element shows; the off-diagonal entries of a
    full tensor in [-0.2, 0.2] (the tensor stays positive definite)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.5, 2.0, (NE, ncoef))
    if kind == 0 and ncoef > dim:
        c[:, dim:] = rng.uniform(-0.2, 0.2, (NE, ncoef - dim))
    return c


def per_element(elmat, e2v, ep, comp):
    """the packed or (NE, size, size) matrices as a list of 2-D arrays"""
    if ep is None:
        return list(elmat)
    nd = np.diff(ep).astype(np.int64) * comp
    off = np.concatenate([[0], np.cumsum(nd * nd)])
    return [elmat[off[e]:off[e + 1]].reshape(nd[e], nd[e]) for e in range(len(nd))]


_model = {}


def model(name, jittered, kind, ncoef, seed=5):
    """The model's matrices of a case and its coefficients, computed once and left unchanged."""
    key = (name, jittered, kind, ncoef, seed)
    if key not in _model:
        X, e2v, ep = mesh(name, jittered)
        coef = coefficients(num_elements(e2v, ep), X.shape[1], kind, ncoef, seed)
        K = em.element_matrices(X, e2v, kind, coef, elem_ptr=ep)
        K.setflags(write=False)
        _model[key] = (K, coef)
    return _model[key]
