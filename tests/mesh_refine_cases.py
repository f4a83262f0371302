"""Meshes shared by the refinement tests (test_mesh_refine_model.py, test_gpu_mesh_refine.py): the liftable cases of
mesh_lift_cases.NAMES with its coords(), and the numbers of levels each is refined by.  Every case is refined once; the small
ones (at most 72 elements) two and three times as well, the others twice -- the largest is hex_9x8x7 at two levels with 32 256
elements.

model(name, levels) is the definition's result with the interpolations kept, computed once and left unchanged."""
import numpy as np

from saamge_amd import mesh_refine_model as rm

import mesh_lift_cases as lc

NAMES = list(lc.NAMES)
GEOMETRIC = list(lc.GEOMETRIC)
SMALL = ["hex_3x2x2", "tets_3x2x2", "quads_4x3", "tris_4x3", "pair_rotated_hex", "pair_rotated_tet", "double_contact", "empty",
         "isolated", "single_2_3", "single_2_4", "single_3_4", "single_3_8", "tris_and_quads", "tet_beside_hex"]
LEVELS = {n: (1, 2, 3) if n in SMALL else (1, 2) for n in NAMES}
CASES = [(n, r) for n in NAMES for r in LEVELS[n]]
AFFINE = ["tris_4x3", "tets_3x2x2", "quads_4x3", "hex_3x2x2"]      # undeformed: every element is an affine image of its reference
_models = {}

case = lc.case
coords = lc.coords


def model(name, levels):
    if (name, levels) not in _models:
        NV, dim, e2v, ep = case(name)
        R = rm.MeshRefine(NV, dim, coords(name), e2v, ep, levels=levels, want_interp=True)
        for a in R.arrays() + tuple(a for P in R.P for a in P.arrays()):
            a.setflags(write=False)
        _models[(name, levels)] = R
    return _models[(name, levels)]


def dyadic_coords(name):
    """coordinates that are multiples of 1/16 below 4 in size: every sum and halving of a few refinements is exact"""
    NV, dim, _, _ = case(name)
    return np.random.default_rng(41).integers(-64, 64, (NV, dim)) / 16.0
