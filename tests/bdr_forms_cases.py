"""Face lists, coefficients and nodal data shared by the boundary-form tests (test_bdr_forms_model.py, test_gpu_bdr_forms.py):
every mesh of elmat_cases.MESHES and elmat_q2_cases.MESHES -- already the smallest that reach a partial wavefront (12
elements), several workgroups (hex_9x8x7: 382 boundary faces; quad9_9x8), corner elements with 3 or more faces, triangle and
quadrilateral faces side by side (mixed_4) and two face types in one list (mixed_hex8_hex27) -- with four face lists each:

  all        the boundary faces, ascending by (element, local face) (problems.boundary_faces)
  shuffled   the same list permuted (seed 3)
  side       the boundary faces on the side x = 0 of the box
  interior   the boundary faces and a few interior ones (every fifth, at most seven)

A face's coefficient depends on (element, local face) alone, so that a permuted list describes the same problem."""
import numpy as np

from saamge_amd import elmat_model as em
from saamge_amd import problems as pr

import elmat_cases as ec
import elmat_q2_cases as qc

VARIANTS = ("all", "shuffled", "side", "interior")
CASES = [("q1", name, jit) for name in ec.MESHES for jit in (False, True)] + \
        [("q2", name, jit) for name in qc.MESHES for jit in qc.JITTERS]
IDS = ["%s-%s" % (c[1], c[2]) for c in CASES]


def mesh(family, name, jitter):
    return ec.mesh(name, jitter) if family == "q1" else qc.mesh(name, jitter)


def box_mesh(family, name):
    return ec.mesh(name, False) if family == "q1" else qc.mesh(name, "box")


def node_counts(e2v, ep):
    return np.diff(ep).astype(np.int64) if ep is not None else np.full(e2v.shape[0], e2v.shape[1], np.int64)


def face_vertices(dim, e2v, ep, fe, fl):
    """the vertex ids of every listed face, a list of arrays"""
    nd = node_counts(e2v, ep)
    off = np.concatenate([[0], np.cumsum(nd)])
    flat = np.asarray(e2v).ravel()
    return [flat[off[e] + np.array(em.FACE_NODES[(dim, int(nd[e]))][l])] for e, l in zip(fe, fl)]


def on_side(family, name, fe, fl, axis, value):
    """which of the listed faces lie on the side coordinate[axis] == value of the undeformed box"""
    X, e2v, ep = box_mesh(family, name)
    return np.array([bool(np.all(X[v, axis] == value)) for v in face_vertices(X.shape[1], e2v, ep, fe, fl)], bool)


_faces = {}


def faces(family, name, variant):
    """(face_elem, face_local), int32, of a mesh and a variant; computed once"""
    key = (family, name, variant)
    if key not in _faces:
        X, e2v, ep = box_mesh(family, name)
        dim = X.shape[1]
        fe, fl = pr.boundary_faces(dim, e2v, ep)
        if variant == "shuffled":
            p = np.random.default_rng(3).permutation(len(fe))
            fe, fl = fe[p], fl[p]
        elif variant == "side":
            sel = on_side(family, name, fe, fl, 0, 0.0)
            fe, fl = fe[sel], fl[sel]
        elif variant == "interior":
            nd = node_counts(e2v, ep)
            every = [(e, l) for e in range(len(nd)) for l in range(len(em.FACE_NODES[(dim, int(nd[e]))]))]
            inner = sorted(set(every) - set(zip(fe.tolist(), fl.tolist())))[::5][:7]
            fe = np.concatenate([fe, np.array([e for e, _ in inner], np.int32)])
            fl = np.concatenate([fl, np.array([l for _, l in inner], np.int32)])
        else:
            assert variant == "all"
        _faces[key] = (np.ascontiguousarray(fe, np.int32), np.ascontiguousarray(fl, np.int32))
    return _faces[key]


def face_coefficients(NE, fe, fl, seed=13):
    """per-face coefficients in [0.5, 2) that depend on (element, local face) alone"""
    table = np.random.default_rng(seed).uniform(0.5, 2.0, (NE, em.MAX_FACES))
    return np.ascontiguousarray(table[fe, fl])


def nodal_data(NV, dim, seed=17):
    """(g (NV,), g (NV, dim)) in [-1, 1)"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, NV), rng.uniform(-1.0, 1.0, (NV, dim))


def zeros(e2v, ep, vdim, square):
    nd = node_counts(e2v, ep) * vdim
    return np.zeros(int((nd ** 2).sum() if square else nd.sum()))
