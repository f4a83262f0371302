"""Every level of the library's hierarchy against the oracle at the level-0 tolerances, given the library's own basis
(tests/conditional_cases.py): the oracle is rebuilt with the library's eigenvectors and MIS bases injected on every level, so
the freedom that keeps tests/test_gpu_parity.py loose below level 0 is gone and what the library derived from its bases --
the weighted-l1 diagonal, eigenvalues, singular values, the coarse element matrices P_loc^T A_e P_loc with several coarse
dofs per MIS, the level-1 agglomerate assembly, the second Galerkin product, the level-1 smoother -- is held to round-off.
The cases at larger theta (cc.LARGE_THETA) put 4-44 vectors on a fine agglomerate and up to 180 on a level-1 one: wide MIS
gathers (more candidate columns than dofs) of up to 225 rows, cuts that drop up to 15 directions of a rank-deficient gather,
up to 225 coarse dofs per MIS in the coarse element matrices, level-1 blocks of the product that take rap_numeric_kernel's
multi-pass path.

A failure localises itself: Ds or the residual against the oracle's agglomerate matrix -> csrc/assemble.hip / the coarse
element matrices; eigenvalues or projectors with a clean residual -> csrc/eig*.hip; singular values or the column space ->
csrc/mis.hip; Ac -> the Galerkin product; the V-cycle alone -> the level-1 smoother or the coarsest solve.
Run with `pytest -m gpu` on an MI355X."""
import ctypes

import pytest

import conditional_cases as cc

pytestmark = pytest.mark.gpu

# The elasticity cases also through the dense eigensolver and with the identical-agglomerate search off (the switches of
# tests/test_gpu_scale.py::test_every_remaining_option_flipped_gives_the_golden), so that the check does not depend on
# which path produced the basis.
VARIANTS = [(name, "default") for name in cc.CASES] + [(name, v) for name in cc.ELASTICITY for v in ("dense", "no_dedupe")]
# The cases at larger theta through both eigensolvers, the elasticity ones with the search off as well.  (Not under
# eig_strict: on pskew_t012 and on level 1 of el_t005 the few-eigenpairs path hands matrices it claims to the dense one,
# DESIGN.md section 2.1 "Open limits".)
VARIANTS += [(name, "dense") for name in cc.LARGE_THETA] + [(name, "no_dedupe") for name in cc.LARGE_THETA if name.startswith("el_")]


@pytest.mark.parametrize("name,variant", VARIANTS)
def test_every_level_matches_the_oracle_given_the_librarys_basis(name, variant):
    from saamge_amd import capi
    prob, testmesh = cc.problem(name), cc.uses_testmesh(name)
    old = capi.get_options()
    if variant == "no_dedupe":
        capi.set_options(eig_dedupe=0)
    try:
        params = capi.default_params(num_coarsenings=cc.NCOARS, theta=cc.theta_of(name), nu_relax=3, testmesh=testmesh,
                                     keep_debug=True, coarse_rtol=1e-28, eigensolver="dense" if variant == "dense" else "subspace")
        h = capi.Hierarchy.from_problem(prob, params)
    finally:
        capi.load().saamge_amd_set_options(ctypes.byref(old))
    try:
        view = cc.capi_view(h)
        H_cond, recorded = cc.conditional_oracle(prob, cc.NCOARS, view, theta=cc.theta_of(name), testmesh=testmesh)
        levels, solves = cc.measure_conditional(prob, view, H_cond, recorded)
        print(cc.format_measured("%s/%s" % (name, variant), levels, solves))
        bad = cc.failures_of(levels, solves)
        if bad:
            raise cc.ConditionalMismatch(bad)
    finally:
        h.close()
