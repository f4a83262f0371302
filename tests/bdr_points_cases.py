"""Meshes, face lists and point data shared by the tests of the boundary data at the face points (test_bdr_points_model.py,
test_gpu_bdr_points.py): every mesh of bdr_forms_cases (elmat_cases.MESHES, elmat_q2_cases.MESHES) and of elmat_p2_cases.MESHES --
all nine element types, the box / straight / curved jitters, at most 504 elements, face counts that are no multiple of the 5 / 16 /
32 faces a workgroup takes, triangles and quadrilaterals in one list (mixed_4: hexahedra and wedges), 4-node and 9-node faces in
one list (mixed_hex8_hex27) -- with the four face lists "all", "shuffled", "side" and "interior" of bdr_forms_cases.

Data at a face point depends on (element, local face, point) alone, so that a permuted list describes the same problem."""
import numpy as np

from saamge_amd import elmat_model as em

import bdr_forms_cases as bc
import elmat_cases as ec
import elmat_p2_cases as pc

VARIANTS = bc.VARIANTS
CASES = list(bc.CASES) + [("p2", name, jit) for name in pc.MESHES for jit in pc.JITTERS]
IDS = ["%s-%s" % (c[1], c[2]) for c in CASES]
MAX_POINTS = 9      # of a face rule


def mesh(family, name, jitter):
    return pc.mesh(name, jitter) if family == "p2" else bc.mesh(family, name, jitter)


def faces(family, name, variant):
    return pc.faces(name, variant) if family == "p2" else bc.faces(family, name, variant)


def is_box(family, jitter):
    """every element is an axis-parallel image of its reference element"""
    return jitter is False or jitter == "box"


def is_straight(family, jitter):
    """no face is bent by a midside node (the faces of jittered hexahedra are bilinear, which the outward test allows for)"""
    return family == "q1" or jitter in ("box", "straight")


def offsets(dim, e2v, ep, fe, fl):
    """fp_ptr of a face list, from the model's tables alone"""
    nd = bc.node_counts(e2v, ep)
    n = [em.FACE_NPOINTS[(dim, len(em.FACE_NODES[(dim, int(nd[e]))][l]))] for e, l in zip(fe, fl)]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def _at_points(table, fe, fl, fp):
    f = np.repeat(np.arange(len(fe)), np.diff(fp))
    q = np.arange(fp[-1]) - fp[f]
    return np.ascontiguousarray(table[fe[f], fl[f], q])


def point_coefficients(NE, fe, fl, fp, seed=31):
    """(NFQ,) in [0.5, 2)"""
    return _at_points(np.random.default_rng(seed).uniform(0.5, 2.0, (NE, em.MAX_FACES, MAX_POINTS)), fe, fl, fp)


def point_data(NE, fe, fl, fp, vdim, seed=37):
    """(NFQ, vdim) in [-1, 1)"""
    return _at_points(np.random.default_rng(seed).uniform(-1.0, 1.0, (NE, em.MAX_FACES, MAX_POINTS, vdim)), fe, fl, fp)


def whole_faces(fe, fl, fp, other_fe, other_fl, other_fp):
    """the point indices of the list (fe, fl) that hold, face by face, the points of the list (other_fe, other_fl) of the same faces"""
    at = {(int(e), int(l)): f for f, (e, l) in enumerate(zip(fe, fl))}
    src = [at[(int(e), int(l))] for e, l in zip(other_fe, other_fl)]
    return np.concatenate([np.arange(fp[f], fp[f + 1]) for f in src]) if src else np.zeros(0, np.int64)


_model = {}


def model(family, name, jitter, variant):
    """what the model gives for a case and a face list, computed once and left unchanged: fp, xq, wmeas, normal; uq1, gradq1 and
    uqd, gradqd of bdr_forms_cases.nodal_data; the point data cq, gq1, gqd"""
    key = (family, name, jitter, variant)
    if key not in _model:
        X, e2v, ep = mesh(family, name, jitter)
        dim, NE = X.shape[1], ec.num_elements(e2v, ep)
        fe, fl = faces(family, name, variant)
        u1, ud = bc.nodal_data(len(X), dim)
        fp, xq, wmeas, normal = em.boundary_points(X, e2v, fe, fl, elem_ptr=ep)
        w = {"fp": fp, "xq": xq, "wmeas": wmeas, "normal": normal}
        w["uq1"], w["gradq1"] = em.boundary_eval(X, e2v, fe, fl, u1, elem_ptr=ep)
        w["uqd"], w["gradqd"] = em.boundary_eval(X, e2v, fe, fl, ud, vdim=dim, elem_ptr=ep)
        w["cq"] = point_coefficients(NE, fe, fl, fp)
        w["gq1"], w["gqd"] = point_data(NE, fe, fl, fp, 1), point_data(NE, fe, fl, fp, dim)
        for v in w.values():
            v.setflags(write=False)
        _model[key] = w
    return _model[key]
